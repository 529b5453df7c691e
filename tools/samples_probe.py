#!/usr/bin/env python3
"""Sample input (Solver.from_samples, Batch.submit(samples=...)) against coefficient input, one process, alternated runs, medians:
  kernel   k_samples_to_coefficients on the luma plane (4096x3072) and on a 4:2:0 chroma plane (2048x1536) of one image — with the
           8-byte loads of aligned rows and with the byte loads of any other input —, next to k_quantise_blocks<1, 1> on the same
           luma plane, from one `rocprofv3 --kernel-trace --stats` run of this script's --kernels
           mode (a child process of its own): microseconds, bytes moved per sample, the fraction of 6.2 TB/s that is;
  create   wall time of solver creation for one 4:2:0 image at 4096x3072 and at 1920x1080: j2p_solver_create from host coefficient
           arrays (2 B per coefficient up), from_samples from tensors on the GPU (nothing up), from_samples from host arrays (1 B
           per sample up); the three taken in turn, the order reversed every other round;
  batch    images per second through Batch (three slots) for 1080p 4:2:0 jobs into f16 224x224 slots: device-sample jobs against
           coefficient jobs.
Appends one JSON line per measurement to OUT (default profiles/sample_input.jsonl) and prints them.
    python tools/samples_probe.py [ITERATIONS = 50] [ROUNDS = 9] [OUT]"""
import csv
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
from jpeg2png_amd.synth import Plane  # noqa: E402

WEIGHT, PWEIGHT = 0.3, 0.001
PEAK = 6.2e12          # bytes per second: what the projection kernel reaches


def image(w, h, seed):
    """(planes with coefficients, bare planes, uint8 samples per plane) of a synthetic 4:2:0 image at quality 50"""
    planes = synth.make_planes(w, h, "420", 50, seed=seed)
    samples = [np.clip(np.rint(j.decode_plane(p) + np.float32(128)), 0, 255).astype(np.uint8) for p in planes]
    bare = [Plane(p.w, p.h, p.w_samp, p.h_samp, None, p.quant_table) for p in planes]
    return planes, bare, samples


def kernels_mode(rounds):
    """what the profiler wraps: per round one solver from device samples (three launches of k_samples_to_coefficients: Y, Cb, Cr),
    one k_quantise_blocks<1, 1> of its luma plane, and one solver from the same samples at an odd address and a row stride of
    w + 5 bytes, whose three launches load byte by byte"""
    import torch
    planes, bare, samples = image(4096, 3072, 1240)
    dev = [torch.from_numpy(a).cuda() for a in samples]
    odd = []
    for a in samples:
        h, w = a.shape
        buf = torch.zeros(h * (w + 5) + 8, dtype=torch.uint8, device="cuda")
        view = buf[1:1 + h * (w + 5)].view(h, w + 5)[:, :w]
        view.copy_(torch.from_numpy(a))
        odd.append(view)
    torch.cuda.synchronize()
    for _ in range(rounds + 1):
        with j.Solver.from_samples(dev, bare, WEIGHT, [PWEIGHT] * 3, 1) as s:
            s.coefficients(0, planes[0].quant_table)
        with j.Solver.from_samples(odd, bare, WEIGHT, [PWEIGHT] * 3, 1) as s:
            pass


if "--kernels" in sys.argv:
    kernels_mode(int(sys.argv[2]))
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 9
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "sample_input.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
if os.path.exists(rocprof):
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                              os.path.abspath(__file__), "--kernels", str(rounds)], capture_output=True, text=True, timeout=900, cwd=tmp)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        launches = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].replace(" ", "")
                    kind = "samples" if "k_samples_to_coefficients" in name else ("quantise" if "k_quantise_blocks<1,1>" in name else None)
                    if kind:
                        launches.append((int(row["Start_Timestamp"]), kind, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    launches.sort()
    kinds = [k for _, k, _ in launches]
    if len(launches) % 7 or kinds != ["samples", "samples", "samples", "quantise", "samples", "samples", "samples"] * (len(launches) // 7):
        sys.exit(f"unexpected launch order in the kernel trace: {kinds[:14]}")
    launches = launches[7:]                                  # the first round: code objects load
    groups = {"k_samples_to_coefficients, luma 4096x3072": ([d for i, (_, _, d) in enumerate(launches) if i % 7 == 0], 4096 * 3072, 3),
              "k_samples_to_coefficients, 4:2:0 chroma 2048x1536": ([d for i, (_, _, d) in enumerate(launches) if i % 7 in (1, 2)], 2048 * 1536, 3),
              "k_quantise_blocks<1, 1>, luma 4096x3072": ([d for i, (_, _, d) in enumerate(launches) if i % 7 == 3], 4096 * 3072, 6),
              "k_samples_to_coefficients, byte loads (odd address, row stride w + 5), luma 4096x3072": ([d for i, (_, _, d) in enumerate(launches) if i % 7 == 4], 4096 * 3072, 3),
              "k_samples_to_coefficients, byte loads, 4:2:0 chroma 2048x1536": ([d for i, (_, _, d) in enumerate(launches) if i % 7 in (5, 6)], 2048 * 1536, 3)}
    for name, (d, n, per) in groups.items():
        us = statistics.median(d)
        emit({"what": "kernel", "kernel": name, "launches": len(d), "us": spread(d), "bytes_per_sample": per,
              "TB_per_s": round(n * per / us / 1e6, 3), "fraction_of_6.2_TB_per_s": round(n * per / (us * 1e-6) / PEAK, 3)})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

import torch  # noqa: E402

# ---- create: coefficient path against the sample paths ----
for w, h in ((4096, 3072), (1920, 1080)):
    planes, bare, samples = image(w, h, 1240)
    for p in planes:
        p.data = np.ascontiguousarray(p.data, np.int16)       # (the arrays the library copies from, made once)
    dev = [torch.from_numpy(a).cuda() for a in samples]
    torch.cuda.synchronize()
    pw = [PWEIGHT] * 3

    def once(kind):
        t0 = time.perf_counter()
        if kind == "coefficients, host arrays":
            s = j.Solver(planes, WEIGHT, pw, its)
        elif kind == "samples, device tensors":
            s = j.Solver.from_samples(dev, bare, WEIGHT, pw, its)
        else:
            s = j.Solver.from_samples(samples, bare, WEIGHT, pw, its)
        dt = (time.perf_counter() - t0) * 1e3
        s.close()
        return dt

    kinds = ["coefficients, host arrays", "samples, device tensors", "samples, host arrays"]
    for kind in kinds:
        once(kind)
        once(kind)
    t = {k: [] for k in kinds}
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            t[kind].append(once(kind))
    up = {"coefficients, host arrays": sum(2 * p.w * p.h for p in planes), "samples, device tensors": 0, "samples, host arrays": sum(a.size for a in samples)}
    for kind in kinds:
        emit({"what": "create", "image": f"{w}x{h} 4:2:0", "input": kind, "rounds": rounds, "ms": spread(t[kind]), "upload_bytes": up[kind]})

# ---- batch: 1080p jobs into 224x224 f16 slots ----
planes, bare, samples = image(1920, 1080, 1241)
dev = [torch.from_numpy(a).cuda() for a in samples]
njob = 24
slots = torch.empty((njob, 3, 224, 224), dtype=torch.float16, device="cuda")
torch.cuda.synchronize()
with j.Batch(devices=(0,), slots_per_device=3) as b:
    def run(kind):
        t0 = time.perf_counter()
        tickets = []
        for i in range(njob):
            out = [{"tensor": slots[i], "out_width": 224, "out_height": 224, "filter": "triangle"}]
            if kind == "device samples":
                tickets.append(b.submit(bare, WEIGHT, [PWEIGHT] * 3, its, width=1920, height=1080, outputs=out, samples=dev))
            else:
                tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=1920, height=1080, outputs=out))
        for tk in tickets:
            b.wait(tk)
        return njob / (time.perf_counter() - t0)

    kinds = ["coefficients", "device samples"]
    for kind in kinds:
        run(kind)
    rate = {k: [] for k in kinds}
    for r in range(max(3, rounds // 2)):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            rate[kind].append(run(kind))
    for kind in kinds:
        emit({"what": "batch", "image": "1920x1080 4:2:0", "input": kind, "output": "f16 chw 224x224, triangle", "iterations": its, "jobs_per_run": njob,
              "slots": 3, "images_per_s": spread(rate[kind])})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
