#!/usr/bin/env python3
"""Tensor output against sample output on one 4096x3072 4:2:0 image solved jointly:
  kernels  k_to_tensor<3, dtype, layout> for u8 / f16 / bf16 / f32 in chw (planar stores) and hwc (interleaved stores), and
           k_to_samples<3> at 8 bits, all from ONE `rocprofv3 --kernel-trace` run of this script's --kernels mode (a child
           process of its own): median device time per launch, and the fraction of the 6.2 TB/s this part delivers that the
           algorithmic bytes — 12 read + 3 x element size written per pixel — in that time are;
  batch    images per second through Batch (three slots, outputs reused), f16 chw tensor jobs that stay on the GPU against
           bits=8 jobs that come down to the host, alternated in one process.
Appends one JSON line per measurement to OUT (default profiles/tensor_probe.jsonl) and prints them.
    python tools/tensor_probe.py [ITERATIONS] [ROUNDS] [OUT]"""
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
HBM_TBS = 6.2
DTYPES = {"u8": (0, 1), "f16": (1, 2), "bf16": (2, 2), "f32": (3, 4)}      # name -> (J2P_DTYPE_*, bytes per element)
LAYOUTS = {"chw": 1, "hwc": 2}                                             # name -> k_to_tensor's LAYOUT (planar, interleaved)


def kernels_mode(launches):
    """what the profiler wraps: every tensor kernel and the sample kernel, `launches` + 1 times each, from one solver"""
    import torch
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    rgb = np.empty((H, W, 3), np.uint8)
    with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1) as s:
        s.run(1)
        for name in DTYPES:
            td = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]
            for layout in LAYOUTS:
                t = torch.empty((3, H, W) if layout == "chw" else (H, W, 3), dtype=td, device="cuda:0")
                for _ in range(launches + 1):
                    s.to_tensor(W, H, layout=layout, out=t)
                    torch.cuda.synchronize()
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])
        s._lib.j2p_planes_to_rgb.argtypes = [ctypes.POINTER(j._CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
        for _ in range(launches + 1):
            if s._lib.j2p_planes_to_rgb(refs, W, H, 8, rgb.ctypes.data) != 0:
                sys.exit("j2p_planes_to_rgb failed")


if "--kernels" in sys.argv:
    kernels_mode(int(sys.argv[2]))
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "tensor_probe.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
if os.path.exists(rocprof):
    launches = 10
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                              os.path.abspath(__file__), "--kernels", str(launches)], capture_output=True, text=True, timeout=900, cwd=tmp)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        durations = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].split("(")[0].replace(" ", "")
                    durations.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)

    def kernel(name, element_bytes, **what):
        d = [x for k, vs in durations.items() if k.endswith(name.replace(" ", "")) for x in vs][1:]        # (the first launch loads the code)
        if not d:
            sys.exit(f"no launch of {name} in the kernel trace")
        us, nbytes = statistics.median(d), (12 + 3 * element_bytes) * W * H
        emit({"what": "kernel", "kernel": name, **what, "image": f"{W}x{H}", "launches": len(d), "us_median": round(us, 2),
              "us_min": round(min(d), 2), "us_max": round(max(d), 2), "bytes_per_pixel": 12 + 3 * element_bytes,
              "TB_per_s": round(nbytes / us / 1e6, 3), "fraction_of_6.2_TB_per_s": round(nbytes / us / 1e6 / HBM_TBS, 3)})
        return us

    for dtype, (code, nbytes) in DTYPES.items():
        for layout, path in LAYOUTS.items():
            us = kernel(f"k_to_tensor<3, {code}, {path}>", nbytes, dtype=dtype, layout=layout)
            if (dtype, layout) == ("u8", "hwc"):
                u8_hwc = us
    samples_us = kernel("k_to_samples<3>", 1, dtype="u8", layout="hwc (8-bit samples, then downloaded)")
    emit({"what": "same bytes", "k_to_tensor<3, 0, 2>_us": round(u8_hwc, 2), "k_to_samples<3>_us": round(samples_us, 2),
          "tensor_kernel_is_at_least_as_fast": bool(u8_hwc <= samples_us)})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

# ---- batch: images per second, tensors that stay against samples that come down ----
import torch  # noqa: E402

planes = synth.make_planes(W, H, "420", 50, seed=1240)
IN_FLIGHT, IMAGES = 3, 12
rgb = [np.empty((H, W, 3), np.uint8) for _ in range(IN_FLIGHT)]
slots = torch.empty((IN_FLIGHT, 3, H, W), dtype=torch.float16, device="cuda:0")
scale = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)]
bias = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
with j.Batch(devices=(0,), slots_per_device=IN_FLIGHT) as b:
    def run(kind, n):
        def submit(i):
            if kind == "f16 chw tensor":
                return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, tensor=slots[i % IN_FLIGHT], scale=scale, bias=bias)
            return b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, bits=8, out=rgb[i % IN_FLIGHT])
        t0 = time.perf_counter()
        tickets = [submit(i) for i in range(min(IN_FLIGHT, n))]
        for i in range(n):
            b.wait(tickets[i])
            if i + IN_FLIGHT < n:
                tickets.append(submit(i + IN_FLIGHT))
        return n / (time.perf_counter() - t0)

    kinds = ["f16 chw tensor", "RGB8 to the host"]
    for kind in kinds:
        run(kind, IN_FLIGHT)
    rates = {k: [] for k in kinds}
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            rates[kind].append(run(kind, IMAGES))
    for kind in kinds:
        emit({"what": "batch", "image": f"{W}x{H} 4:2:0 joint", "output": kind, "iterations": its, "rounds": rounds, "images_per_round": IMAGES,
              "slots": IN_FLIGHT, "images_per_s_median": round(statistics.median(rates[kind]), 2), "images_per_s_best": round(max(rates[kind]), 2),
              "images_per_s_worst": round(min(rates[kind]), 2)})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
