#!/usr/bin/env python3
"""Greyscale output against colour: wall time per image through Batch (submit + wait, one slot, output arrays reused)
for the default joint RGB job and the luma-only one-plane job of `-g` on the same 4:2:0 image, alternated in the same
process; then the command-line driver end to end (JPEG read, solve, PNG deflate and write) on one 12-Mpixel JPEG, default
against -g.  Appends one JSON line per measurement to OUT (default profiles/grey_probe.jsonl) and prints them.
    python tools/grey_probe.py [ITERATIONS] [ROUNDS] [OUT]"""
import json
import os
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

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "grey_probe.jsonl")
WEIGHT, PWEIGHT = 0.3, 0.001
SIZES = [(1920, 1080), (4096, 3072)]
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


with j.Batch(devices=(0,), slots_per_device=1) as b:
    for w, h in SIZES:
        planes = synth.make_planes(w, h, "420", 50, seed=1240)
        rgb = np.empty((h, w, 3), np.uint8)
        grey = np.empty((h, w), np.uint8)
        jobs = {"joint RGB": (planes, rgb), "grey (-g)": (planes[:1], grey)}

        def once(kind):
            p, out = jobs[kind]
            t0 = time.perf_counter()
            b.wait(b.submit(p, WEIGHT, [PWEIGHT] * len(p), its, width=w, height=h, bits=8, out=out))
            return (time.perf_counter() - t0) * 1e3

        for kind in jobs:                               # warm-up: arenas in the pool, code objects loaded
            once(kind)
        samples = {k: [] for k in jobs}
        for r in range(rounds):                         # alternated, the order flipped every round
            for kind in (list(jobs) if r % 2 == 0 else list(jobs)[::-1]):
                samples[kind].append(once(kind))
        for kind in jobs:
            emit({"what": "batch", "image": f"{w}x{h} 4:2:0", "job": kind, "iterations": its, "rounds": rounds,
                  "ms_per_image_median": round(statistics.median(samples[kind]), 2),
                  "ms_per_image_best": round(min(samples[kind]), 2), "ms_per_image_worst": round(max(samples[kind]), 2), "output_bytes": jobs[kind][1].nbytes})
        rg = statistics.median(samples["grey (-g)"]) / statistics.median(samples["joint RGB"])
        emit({"what": "batch", "image": f"{w}x{h} 4:2:0", "summary": True, "grey_over_joint_rgb": round(rg, 3)})

# the driver end to end on one 12-Mpixel JPEG: a process per run, as a user runs it
from jpeg2png_amd.buildlib import build_cli  # noqa: E402
from PIL import Image  # noqa: E402

exe = build_cli()
w, h = 4096, 3072
with tempfile.TemporaryDirectory() as tmp:
    jpg = os.path.join(tmp, "in.jpg")
    Image.fromarray(synth.synth_rgb(w, h, 1241).astype(np.uint8), "RGB").save(jpg, "JPEG", quality=50, subsampling=2)
    runs = {"default (joint RGB)": [], "-g": ["-g"]}
    samples = {k: [] for k in runs}
    sizes = {}
    for r in range(rounds + 1):
        for kind in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            png = os.path.join(tmp, "out.png")
            t0 = time.perf_counter()
            res = subprocess.run([exe, jpg, "-o", png, "-q", "-i", str(its), *runs[kind]], capture_output=True, text=True,
                                 timeout=600)
            dt = time.perf_counter() - t0
            if res.returncode != 0:
                sys.exit(f"{kind}: {res.stderr}")
            sizes[kind] = os.path.getsize(png)
            if r:                                       # round 0: warm-up (page cache, code objects)
                samples[kind].append(dt * 1e3)
    for kind in runs:
        emit({"what": "cli", "image": f"{w}x{h} 4:2:0 q50", "run": kind, "iterations": its, "rounds": rounds,
              "ms_median": round(statistics.median(samples[kind]), 1), "ms_best": round(min(samples[kind]), 1),
              "png_bytes": sizes[kind]})
    rg = statistics.median(samples["-g"]) / statistics.median(samples["default (joint RGB)"])
    emit({"what": "cli", "image": f"{w}x{h} 4:2:0 q50", "summary": True, "grey_over_default": round(rg, 3)})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
