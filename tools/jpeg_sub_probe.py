#!/usr/bin/env python3
"""Subsampled JPEG output (-j Q -S 420) against 4:4:4 JPEG output and RGB8 on one 4096x3072 4:2:0 image, default 50
iterations, alternated runs, medians (the sibling of tools/jpeg_probe.py):
  kernels  k_quantise_blocks<2, 2> per chroma plane next to k_quantise_blocks<1, 1> on the same two planes, from one
           `rocprofv3 --kernel-trace --stats` run of this script's --kernels mode (a child process of its own) in which
           every round holds one 4:4:4 and one 4:2:0 coefficient job: launches in time order are Y, Cb, Cr of the first
           and Y, Cb, Cr of the second;
  batch    wall time per image through Batch (submit + wait, one slot, output arrays reused): RGB8 samples (3 B/pixel
           down), 4:4:4 coefficients (6 B/pixel), 4:2:0 coefficients (3 B/pixel), alternated in one process;
  cli      the command-line driver end to end, `-j 95` with and without `-S 420`: wall time, output bytes.
Appends one JSON line per measurement to OUT (default profiles/jpeg_sub_probe.jsonl) and prints them.
    python tools/jpeg_sub_probe.py [ITERATIONS] [ROUNDS] [OUT] [SAMPLING = 420]"""
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

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
QUALITY = 95
FACTORS = {"422": (2, 1), "420": (2, 2), "440": (1, 2)}


def tables(quality):
    return [synth.quant_table("luma", quality), synth.quant_table("chroma", quality), synth.quant_table("chroma", quality)]


def coef_arrays(subs):
    return [np.empty((-(-(H // 8) // sy), -(-(W // 8) // sx), 64), np.int16) for sx, sy in subs]


def kernels_mode(its, rounds, subs):
    """what the profiler wraps: one 4:4:4 and one subsampled coefficient job per round"""
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    full, sub = coef_arrays([(1, 1)] * 3), coef_arrays(subs)
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        for _ in range(rounds + 1):
            b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, quant_tables=tables(QUALITY), out=full))
            b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, quant_tables=tables(QUALITY), out=sub,
                            subsampling=subs))


if "--kernels" in sys.argv:
    sx, sy = FACTORS[sys.argv[4]]
    kernels_mode(int(sys.argv[2]), int(sys.argv[3]), [(1, 1), (sx, sy), (sx, sy)])
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "jpeg_sub_probe.jsonl")
sampling = args[3] if len(args) > 3 else "420"
subs = [(1, 1), FACTORS[sampling], FACTORS[sampling]]
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
if os.path.exists(rocprof):
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                              os.path.abspath(__file__), "--kernels", str(its), str(rounds), sampling], capture_output=True, text=True,
                             timeout=900, cwd=tmp)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        launches = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_quantise_blocks" in row["Kernel_Name"]:
                        start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                        full = "k_quantise_blocks<1,1>" in row["Kernel_Name"].replace(" ", "")
                        launches.append((start, "full" if full else "sub", (end - start) / 1e3))
    launches.sort()
    # every round: full Y, full Cb, full Cr | full Y, sub Cb, sub Cr
    kinds = [k for _, k, _ in launches]
    if len(launches) % 6 or kinds != ["full", "full", "full", "full", "sub", "sub"] * (len(launches) // 6):
        sys.exit(f"unexpected launch order in the kernel trace: {kinds[:12]}")
    groups = {"k_quantise_blocks<1, 1>, chroma planes of the 4:4:4 job": [d for i, (_, _, d) in enumerate(launches) if i % 6 in (1, 2)],
              f"k_quantise_blocks<{subs[1][0]}, {subs[1][1]}>, chroma planes of the {sampling} job": [d for _, k, d in launches if k == "sub"],
              "k_quantise_blocks<1, 1>, luma planes of both jobs": [d for i, (_, _, d) in enumerate(launches) if i % 6 in (0, 3)]}
    for name, d in groups.items():
        emit({"what": "kernel", "kernel": name, "image": f"{W}x{H}", "launches": len(d), "us_median": round(statistics.median(d), 2),
              "us_min": round(min(d), 2), "us_max": round(max(d), 2), "per": "plane"})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

# ---- batch: per image ----
planes = synth.make_planes(W, H, "420", 50, seed=1240)
rgb = np.empty((H, W, 3), np.uint8)
full, sub = coef_arrays([(1, 1)] * 3), coef_arrays(subs)
qt = tables(QUALITY)
kinds = ["RGB8", "coefficients 444", f"coefficients {sampling}"]
with j.Batch(devices=(0,), slots_per_device=1) as b:
    for n_it in (its, 0):
        def once(kind):
            t0 = time.perf_counter()
            if kind == "RGB8":
                b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, n_it, width=W, height=H, bits=8, out=rgb))
            elif kind == "coefficients 444":
                b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, n_it, width=W, height=H, quant_tables=qt, out=full))
            else:
                b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, n_it, width=W, height=H, quant_tables=qt, out=sub, subsampling=subs))
            return (time.perf_counter() - t0) * 1e3

        for kind in kinds:
            once(kind)
        samples = {k: [] for k in kinds}
        for r in range(rounds):
            for kind in (kinds if r % 2 == 0 else kinds[::-1]):
                samples[kind].append(once(kind))
        nbytes = {"RGB8": rgb.nbytes, "coefficients 444": sum(c.nbytes for c in full), f"coefficients {sampling}": sum(c.nbytes for c in sub)}
        for kind in kinds:
            emit({"what": "batch", "image": f"{W}x{H} 4:2:0", "output": kind, "iterations": n_it, "rounds": rounds,
                  "ms_per_image_median": round(statistics.median(samples[kind]), 2), "ms_per_image_best": round(min(samples[kind]), 2), "ms_per_image_worst": round(max(samples[kind]), 2),
                  "download_bytes": nbytes[kind], "download_bytes_per_pixel": round(nbytes[kind] / (W * H), 2)})

# ---- the driver end to end: a process per run, as a user runs it ----
from jpeg2png_amd.buildlib import build_cli  # noqa: E402
from PIL import Image  # noqa: E402

exe = build_cli()
with tempfile.TemporaryDirectory() as tmp:
    jpg = os.path.join(tmp, "in.jpg")
    Image.fromarray(synth.synth_rgb(W, H, 1241).astype(np.uint8), "RGB").save(jpg, "JPEG", quality=50, subsampling=2)
    runs = {f"-j {QUALITY}": ("out444.jpg", ["-j", str(QUALITY)]),
            f"-j {QUALITY} -S {sampling}": ("outsub.jpg", ["-j", str(QUALITY), "-S", sampling])}
    samples = {k: [] for k in runs}
    sizes = {}
    for r in range(rounds + 1):
        for kind in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            out = os.path.join(tmp, runs[kind][0])
            t0 = time.perf_counter()
            res = subprocess.run([exe, jpg, "-o", out, "-q", "-i", str(its), *runs[kind][1]], capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            if res.returncode != 0:
                sys.exit(f"{kind}: {res.stderr}")
            sizes[kind] = os.path.getsize(out)
            if r:                                       # round 0: warm-up (page cache, code objects)
                samples[kind].append(dt * 1e3)
    for kind in runs:
        emit({"what": "cli", "image": f"{W}x{H} 4:2:0 q50", "input_bytes": os.path.getsize(jpg), "run": kind, "iterations": its,
              "rounds": rounds, "ms_median": round(statistics.median(samples[kind]), 1), "ms_best": round(min(samples[kind]), 1),
              "output_bytes": sizes[kind]})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
