#!/usr/bin/env python3
"""Estimated tables (samples_histogram, Solver.from_samples(quant="estimate"), Batch.submit(quant="estimate")) against the plain
sample path, one process, alternated runs, medians:
  kernel   k_samples_dct_histogram on a 4096x3072 luma plane next to k_samples_to_coefficients on the same plane, from one
           `rocprofv3 --kernel-trace --stats` run of this script's --kernels mode (a child process of its own): microseconds and
           their ratio.  The histogram kernel reads the same byte per sample and writes next to nothing, where the sample kernel
           writes two bytes per sample: the sample kernel's time is the yardstick, not a gate;
  call     wall time of samples_histogram for that plane from a device tensor and from a host array, and of estimate_quant_table;
  create   wall time of solver creation for one 4:2:0 image at 4096x3072 and at 1920x1080 from device tensors: from_samples with
           the tables given against from_samples(quant="estimate"); taken in turn, the order reversed every other round;
  batch    images per second through Batch (three slots) for 1080p 4:2:0 device-sample jobs into f16 224x224 slots, with and
           without quant="estimate".
Appends one JSON line per measurement to OUT (default profiles/quant_estimate.jsonl) and prints them.
    python tools/estimate_probe.py [ITERATIONS = 50] [ROUNDS = 9] [OUT]"""
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


def image(w, h, seed):
    """(bare planes with the tables, bare planes without, uint8 samples per plane) of a synthetic 4:2:0 image at quality 50"""
    planes = synth.make_planes(w, h, "420", 50, seed=seed)
    samples = [np.clip(np.rint(j.decode_plane(p) + np.float32(128)), 0, 255).astype(np.uint8) for p in planes]
    given = [Plane(p.w, p.h, p.w_samp, p.h_samp, None, p.quant_table) for p in planes]
    none = [Plane(p.w, p.h, p.w_samp, p.h_samp, None, None) for p in planes]
    return given, none, samples


def kernels_mode(rounds):
    """what the profiler wraps: per round one solver from device samples (three launches of k_samples_to_coefficients: Y, Cb, Cr)
    and one histogram of the luma plane"""
    import torch
    given, _, samples = image(4096, 3072, 1240)
    dev = [torch.from_numpy(a).cuda() for a in samples]
    torch.cuda.synchronize()
    for _ in range(rounds + 1):
        with j.Solver.from_samples(dev, given, WEIGHT, [PWEIGHT] * 3, 1):
            pass
        j.samples_histogram(dev[0])


if "--kernels" in sys.argv:
    kernels_mode(int(sys.argv[2]))
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 9
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "quant_estimate.jsonl")
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
                    kind = "samples" if "k_samples_to_coefficients" in name else ("histogram" if "k_samples_dct_histogram" in name else None)
                    if kind:
                        launches.append((int(row["Start_Timestamp"]), kind, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    launches.sort()
    kinds = [k for _, k, _ in launches]
    if len(launches) % 4 or kinds != ["samples", "samples", "samples", "histogram"] * (len(launches) // 4):
        sys.exit(f"unexpected launch order in the kernel trace: {kinds[:12]}")
    launches = launches[4:]                                  # the first round: code objects load
    sample_us = [d for i, (_, _, d) in enumerate(launches) if i % 4 == 0]
    hist_us = [d for i, (_, _, d) in enumerate(launches) if i % 4 == 3]
    emit({"what": "kernel", "kernel": "k_samples_to_coefficients, luma 4096x3072", "launches": len(sample_us), "us": spread(sample_us)})
    emit({"what": "kernel", "kernel": "k_samples_dct_histogram, luma 4096x3072", "launches": len(hist_us), "us": spread(hist_us),
          "ratio_to_k_samples_to_coefficients": round(statistics.median(hist_us) / statistics.median(sample_us), 3)})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

import torch  # noqa: E402

# ---- call: the histogram and the rule ----
given, none, samples = image(4096, 3072, 1240)
dev = [torch.from_numpy(a).cuda() for a in samples]
torch.cuda.synchronize()
for what, arg in (("device tensor", dev[0]), ("host array", samples[0])):
    t = []
    for _ in range(rounds + 2):
        t0 = time.perf_counter()
        hist, blocks, excluded = j.samples_histogram(arg)
        t.append((time.perf_counter() - t0) * 1e3)
    emit({"what": "call", "call": "samples_histogram, luma 4096x3072", "input": what, "ms": spread(t[2:]), "blocks": blocks, "excluded": excluded})
t = []
for _ in range(rounds):
    t0 = time.perf_counter()
    table, det, quality = j.estimate_quant_table(hist)
    t.append((time.perf_counter() - t0) * 1e3)
emit({"what": "call", "call": "estimate_quant_table", "ms": spread(t), "determined": int(det.sum()), "equal_to_the_images_table": int((table[det] == given[0].quant_table[det]).sum()),
      "quality": quality})

# ---- create: tables given against tables estimated ----
for w, h in ((4096, 3072), (1920, 1080)):
    given, none, samples = image(w, h, 1240)
    dev = [torch.from_numpy(a).cuda() for a in samples]
    torch.cuda.synchronize()
    pw = [PWEIGHT] * 3

    def once(kind):
        t0 = time.perf_counter()
        s = j.Solver.from_samples(dev, given, WEIGHT, pw, its) if kind == "given" else j.Solver.from_samples(dev, none, WEIGHT, pw, its, quant="estimate")
        dt = (time.perf_counter() - t0) * 1e3
        s.close()
        return dt

    kinds = ["given", "estimate"]
    for kind in kinds:
        once(kind)
        once(kind)
    t = {k: [] for k in kinds}
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            t[kind].append(once(kind))
    for kind in kinds:
        emit({"what": "create", "image": f"{w}x{h} 4:2:0", "input": "samples, device tensors", "tables": kind, "rounds": rounds, "ms": spread(t[kind])})

# ---- batch: 1080p jobs into 224x224 f16 slots ----
given, none, samples = image(1920, 1080, 1241)
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
            if kind == "estimate":
                tickets.append(b.submit(none, WEIGHT, [PWEIGHT] * 3, its, width=1920, height=1080, outputs=out, samples=dev, quant="estimate"))
            else:
                tickets.append(b.submit(given, WEIGHT, [PWEIGHT] * 3, its, width=1920, height=1080, outputs=out, samples=dev))
        for tk in tickets:
            b.wait(tk)
            if kind == "estimate":
                b.estimated_tables(tk)
        return njob / (time.perf_counter() - t0)

    kinds = ["given", "estimate"]
    for kind in kinds:
        run(kind)
    rate = {k: [] for k in kinds}
    for r in range(max(3, rounds // 2)):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            rate[kind].append(run(kind))
    for kind in kinds:
        emit({"what": "batch", "image": "1920x1080 4:2:0", "input": "device samples", "tables": kind, "output": "f16 chw 224x224, triangle", "iterations": its,
              "jobs_per_run": njob, "slots": 3, "images_per_s": spread(rate[kind])})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
