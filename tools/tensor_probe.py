#!/usr/bin/env python3
"""Tensor output against sample output on one 4096x3072 4:2:0 image solved jointly:
  kernels  k_to_tensor<3, dtype, layout> for u8 / f16 / bf16 / f32 in chw (planar stores) and hwc (interleaved stores), the
           u8 hwc tensor at width 4095 (row stride 12285: the generic stores), and the kernel behind the SAMPLE calls —
           j2p_planes_to_rgb at 8 bits (widths 4096 and 4095) and 16 bits, j2p_planes_to_grey of a one-plane solver at 8 bits.
           Two `rocprofv3 --kernel-trace` runs of this script, child processes of their own: --kernels (the tensor calls,
           found by kernel name) and --samples (the sample calls and no other conversion, found by CALL: they are the last
           launches of that process, in the order made — whatever the kernel behind them is called).  Median device time
           per launch, and the fraction of the 6.2 TB/s this part delivers that the algorithmic bytes — 4 read per plane +
           element size written per sample — in that time are;
  batch    images per second through Batch (three slots, outputs reused), f16 chw tensor jobs that stay on the GPU against
           bits=8 jobs that come down to the host, alternated in one process.
Public API only, so the same file runs against any build that has tensor output.  Appends one JSON line per measurement to
OUT (default profiles/tensor_probe.jsonl) and prints them; COMMIT, when given, goes into every line as "commit".
    python tools/tensor_probe.py [ITERATIONS] [ROUNDS] [OUT] [COMMIT]"""
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


# the sample calls of --samples, in the order made: (name, planes, width, bits)
SAMPLE_CALLS = [("j2p_planes_to_rgb", 3, W, 8), ("j2p_planes_to_rgb", 3, W - 1, 8), ("j2p_planes_to_rgb", 3, W, 16),
                ("j2p_planes_to_grey", 1, W, 8)]


def kernels_mode(launches):
    """what the profiler wraps: every tensor kernel, `launches` + 1 times each, from one solver"""
    import torch
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1) as s:
        s.run(1)
        for name in DTYPES:
            td = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]
            for layout in LAYOUTS:
                t = torch.empty((3, H, W) if layout == "chw" else (H, W, 3), dtype=td, device="cuda:0")
                for _ in range(launches + 1):
                    s.to_tensor(W, H, layout=layout, out=t)
                    torch.cuda.synchronize()
        t = torch.empty((H, W - 1, 3), dtype=torch.uint8, device="cuda:0")
        for _ in range(launches + 1):
            s.to_tensor(W - 1, H, layout="hwc", out=t)
            torch.cuda.synchronize()


def samples_mode(launches):
    """what the profiler wraps: SAMPLE_CALLS, `launches` + 1 times each, after both solvers have run"""
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    lib = j.load_library()
    for name in ("j2p_planes_to_rgb", "j2p_planes_to_grey"):
        getattr(lib, name).argtypes = [ctypes.POINTER(j._CPlaneRef), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, 1) as s, j.Solver(planes[:1], WEIGHT, [PWEIGHT], 1) as g:
        s.run(1)
        g.run(1)
        s.sync()
        g.sync()
        for name, nplane, w, bits in SAMPLE_CALLS:
            solver = s if nplane == 3 else g
            refs = (j._CPlaneRef * nplane)(*[j._CPlaneRef(solver._h, c) for c in range(nplane)])
            out = np.empty((H, w, nplane * bits // 8), np.uint8)
            for _ in range(launches + 1):
                if getattr(lib, name)(refs, w, H, bits, out.ctypes.data) != 0:
                    sys.exit(f"{name} failed")


for flag, mode in (("--kernels", kernels_mode), ("--samples", samples_mode)):
    if flag in sys.argv:
        mode(int(sys.argv[2]))
        sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "tensor_probe.jsonl")
commit = {"commit": args[3]} if len(args) > 3 else {}
lines = []


def emit(rec):
    rec = {**commit, **rec}
    lines.append(rec)
    print(json.dumps(rec), flush=True)


# ---- kernels: two profiled child processes ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
if os.path.exists(rocprof):
    launches = 10

    def trace(flag):
        """(name, microseconds) of every kernel launch of the child process, in the order they started; the runtime's own
        kernels (copies and fills) left out"""
        with tempfile.TemporaryDirectory() as tmp:
            res = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                                  os.path.abspath(__file__), flag, str(launches)], capture_output=True, text=True, timeout=900, cwd=tmp)
            if res.returncode != 0:
                sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
                with open(path, newline="") as f:
                    for row in csv.DictReader(f):
                        name = row["Kernel_Name"].split("(")[0].replace(" ", "")
                        if not name.startswith("__amd_rocclr"):
                            rows.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        return [(name, us) for _, name, us in sorted(rows)]

    def kernel(name, d, nplane, w, element_bytes, **what):
        us, per_pixel = statistics.median(d), nplane * (4 + element_bytes)
        nbytes = per_pixel * w * H
        emit({"what": "kernel", "kernel": name, **what, "image": f"{w}x{H}", "launches": len(d), "us_median": round(us, 2),
              "us_min": round(min(d), 2), "us_max": round(max(d), 2), "bytes_per_pixel": per_pixel,
              "TB_per_s": round(nbytes / us / 1e6, 3), "fraction_of_6.2_TB_per_s": round(nbytes / us / 1e6 / HBM_TBS, 3)})
        return us

    tensor_launches = trace("--kernels")

    def tensor_kernel(name, w, element_bytes, **what):
        d = [us for k, us in tensor_launches if k.endswith(name.replace(" ", ""))][1:]     # (the first launch loads the code)
        if not d:
            sys.exit(f"no launch of {name} in the kernel trace")
        return kernel(name, d, 3, w, element_bytes, **what)

    tensor_us = {}
    for dtype, (code, nbytes) in DTYPES.items():
        for layout, path in LAYOUTS.items():
            tensor_us[dtype, layout, W] = tensor_kernel(f"k_to_tensor<3, {code}, {path}>", W, nbytes, dtype=dtype, layout=layout)
    tensor_us["u8", "hwc", W - 1] = tensor_kernel("k_to_tensor<3, 0, 0>", W - 1, 1, dtype="u8", layout="hwc (generic stores)")

    sample_launches = trace("--samples")[-len(SAMPLE_CALLS) * (launches + 1):]
    if len(sample_launches) != len(SAMPLE_CALLS) * (launches + 1):
        sys.exit("fewer kernel launches in the sample trace than sample calls")
    sample_us = {}
    for i, (call, nplane, w, bits) in enumerate(SAMPLE_CALLS):
        group = sample_launches[i * (launches + 1):(i + 1) * (launches + 1)]
        names = sorted({k for k, _ in group})
        if len(names) != 1:
            sys.exit(f"{call}: its launches are not of one kernel: {names}")
        sample_us[nplane, w, bits] = kernel(names[0], [us for _, us in group][1:], nplane, w, bits // 8, call=f"{call}(w={w}, bits={bits})",
                                            then="downloaded")
    for w in (W, W - 1):
        t, s = tensor_us["u8", "hwc", w], sample_us[3, w, 8]
        emit({"what": "same bytes", "image": f"{w}x{H}", "u8_hwc_tensor_us": round(t, 2), "rgb8_samples_us": round(s, 2),
              "tensor_kernel_is_at_least_as_fast": bool(t <= s)})
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
