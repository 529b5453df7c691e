#!/usr/bin/env python3
"""JPEG output (-j) against PNG output on one 4096x3072 4:2:0 image, default 50 iterations, three runs each:
  kernels  k_quantise_blocks<1, 1> (one launch per plane) against k_to_samples<3> (one launch per image) from a
           `rocprofv3 --kernel-trace --stats` run of this script's --kernels mode (a child process of its own), with the
           fraction of the 6.2 TB/s this part delivers that 6 B/sample (4 read, 2 written) in the measured time is;
  batch    wall time per image through Batch (submit + wait, one slot, output arrays reused), RGB8 samples (3 B/pixel down)
           against int16 coefficients (6 B/pixel down), alternated in one process; also with 0 iterations, where upload,
           conversion and download are all there is;
  cli      the command-line driver end to end, `-j 95` against the same command writing the PNG: wall time, output bytes.
Appends one JSON line per measurement to OUT (default profiles/jpeg_probe.jsonl) and prints them.
    python tools/jpeg_probe.py [ITERATIONS] [ROUNDS] [OUT]"""
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
HBM_TBS = 6.2
QUALITY = 95


def tables(quality):
    """libjpeg's tables for `quality` as jpeg_set_quality(Q, TRUE) scales Annex K (the rule synth.quant_table restates)"""
    return [synth.quant_table("luma", quality), synth.quant_table("chroma", quality), synth.quant_table("chroma", quality)]


def kernels_mode(its, rounds):
    """what the profiler wraps: one RGB job and one coefficient job per round"""
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    rgb = np.empty((H, W, 3), np.uint8)
    coef = [np.empty((H // 8, W // 8, 64), np.int16) for _ in range(3)]
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        for _ in range(rounds + 1):
            b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, bits=8, out=rgb))
            b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, quant_tables=tables(QUALITY), out=coef))


if "--kernels" in sys.argv:
    kernels_mode(int(sys.argv[2]), int(sys.argv[3]))
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 3
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "jpeg_probe.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
if os.path.exists(rocprof):
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                              os.path.abspath(__file__), "--kernels", str(its), str(rounds)], capture_output=True, text=True,
                             timeout=900, cwd=tmp)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        durations = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].split("(")[0]
                    durations.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name, bytes_per_sample, samples in (("k_quantise_blocks<1, 1>", 6, W * H), ("k_to_samples<3>", 15, W * H)):
        d = [x for k, vs in durations.items() if k.replace(" ", "").endswith(name.replace(" ", "")) for x in vs]
        if not d:
            sys.exit(f"no launch of {name} in the kernel trace")
        us = statistics.median(d)
        emit({"what": "kernel", "kernel": name, "image": f"{W}x{H}", "launches": len(d), "us_median": round(us, 2),
              "us_min": round(min(d), 2), "us_max": round(max(d), 2),
              "per": "plane" if name.startswith("k_quantise_blocks") else "image (three planes in, RGB8 out)",
              "bytes_per_sample": bytes_per_sample, "TB_per_s": round(bytes_per_sample * samples / us / 1e6, 3),
              "fraction_of_6.2_TB_per_s": round(bytes_per_sample * samples / us / 1e6 / HBM_TBS, 3)})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

# ---- batch: per image, RGB8 against coefficients ----
planes = synth.make_planes(W, H, "420", 50, seed=1240)
rgb = np.empty((H, W, 3), np.uint8)
coef = [np.empty((H // 8, W // 8, 64), np.int16) for _ in range(3)]
qt = tables(QUALITY)
with j.Batch(devices=(0,), slots_per_device=1) as b:
    for n_it in (its, 0):
        def once(kind):
            t0 = time.perf_counter()
            if kind == "RGB8":
                b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, n_it, width=W, height=H, bits=8, out=rgb))
            else:
                b.wait(b.submit(planes, WEIGHT, [PWEIGHT] * 3, n_it, width=W, height=H, quant_tables=qt, out=coef))
            return (time.perf_counter() - t0) * 1e3

        kinds = ["RGB8", "coefficients"]
        for kind in kinds:
            once(kind)
        samples = {k: [] for k in kinds}
        for r in range(rounds):
            for kind in (kinds if r % 2 == 0 else kinds[::-1]):
                samples[kind].append(once(kind))
        for kind in kinds:
            emit({"what": "batch", "image": f"{W}x{H} 4:2:0", "output": kind, "iterations": n_it, "rounds": rounds,
                  "ms_per_image_median": round(statistics.median(samples[kind]), 2), "ms_per_image_best": round(min(samples[kind]), 2), "ms_per_image_worst": round(max(samples[kind]), 2),
                  "download_bytes": rgb.nbytes if kind == "RGB8" else sum(c.nbytes for c in coef),
                  "download_bytes_per_pixel": 3 if kind == "RGB8" else 6})

# ---- the driver end to end: a process per run, as a user runs it ----
from jpeg2png_amd.buildlib import build_cli  # noqa: E402
from PIL import Image  # noqa: E402

exe = build_cli()
with tempfile.TemporaryDirectory() as tmp:
    jpg = os.path.join(tmp, "in.jpg")
    Image.fromarray(synth.synth_rgb(W, H, 1241).astype(np.uint8), "RGB").save(jpg, "JPEG", quality=50, subsampling=2)
    runs = {"PNG": ("out.png", []), f"-j {QUALITY}": ("out.jpg", ["-j", str(QUALITY)])}
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
