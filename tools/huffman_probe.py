#!/usr/bin/env python3
"""Optimised Huffman tables on the GPU (J2P_JPEG_OPTIMIZE: k_entropy_histogram, the tables on the host, a third wait) against the
plain file, with the method of tools/entropy_probe.py, on one 4096x3072 4:2:0 image at Q 75 and Q 95, alternated runs, medians:
  kernels  k_entropy_histogram next to k_entropy_lengths (the same walk) and the other kernels of Solver.to_jpeg(optimize=True),
           from one `rocprofv3 --kernel-trace` run of this script's --kernels mode (a child process of its own), per call; once
           more per library named in VARIANTS (name=path,...: other builds of the histogram kernel);
  call     wall time of Solver.to_jpeg with and without optimize in one process, and the two files' sizes;
  parent   Solver.to_jpeg WITHOUT optimize under this library and under the parent commit's (PARENT=path), a process each,
           alternated: the plain path must not have moved;
  batch    images per second through Batch (three slots) for jpeg= jobs with and without "optimize".
Appends one JSON line per measurement to OUT (default profiles/huffman_gpu.jsonl) and prints them.
    [PARENT=lib.so] [VARIANTS=name=lib.so,...] python tools/huffman_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
import csv
import glob
import json
import os
import pickle
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
QUALITIES = (75, 95)
SUB = (2, 2)
IMAGE = f"{W}x{H} 4:2:0"


def solved(planes, its):
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return s


def timed(s, q, optimize):
    t0 = time.perf_counter()
    data = s.to_jpeg(W, H, quality=q, subsampling=SUB, optimize=True) if optimize else s.to_jpeg(W, H, quality=q, subsampling=SUB)
    return (time.perf_counter() - t0) * 1e3, data


if len(sys.argv) > 1 and sys.argv[1] in ("--kernels", "--plain"):
    # the child processes: planes from the pickle the parent left, so that every child solves the same image
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    if sys.argv[1] == "--kernels":
        for q in QUALITIES:
            for _ in range(rounds + 1):
                s.to_jpeg(W, H, quality=q, subsampling=SUB, optimize=True)
    else:
        for q in QUALITIES:
            timed(s, q, False)
            ms = [timed(s, q, False)[0] for _ in range(rounds)]
            print(json.dumps({"quality": q, "ms": ms}), flush=True)
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "huffman_gpu.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


work = tempfile.mkdtemp()
planes = synth.make_planes(W, H, "420", 50, seed=1240)
pickled = os.path.join(work, "planes.pickle")
with open(pickled, "wb") as f:
    pickle.dump(planes, f)


def child(mode, library, n):
    env = dict(os.environ)
    if library:
        env["J2P_LIBRARY"] = os.path.abspath(library)
    return [sys.executable, os.path.abspath(__file__), mode, pickled, str(its), str(n)], env


# ---- kernels: a profiled child process per build of the histogram kernel ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
NAMES = ("k_quantise_blocks", "k_entropy_histogram", "k_entropy_lengths", "k_scan_sums", "k_scan_tiles", "k_scan_apply", "k_entropy_pack",
         "k_stuff_count", "k_stuff_copy")
builds = [("release", None)] + [tuple(v.split("=", 1)) for v in os.environ.get("VARIANTS", "").split(",") if "=" in v]
for build, library in builds:
    if not os.path.exists(rocprof):
        emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})
        break
    with tempfile.TemporaryDirectory() as tmp:
        cmd, env = child("--kernels", library, rounds)
        res = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", *cmd], capture_output=True, text=True, timeout=900,
                             cwd=tmp, env=env)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        launches = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = next((n for n in NAMES if n in row["Kernel_Name"]), None)
                    if name:
                        launches.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    launches.sort()
    calls, cur = [], {}
    for _, name, us in launches:
        cur.setdefault(name, []).append(us)
        if name == "k_stuff_copy":                      # (ends a call)
            calls.append(cur)
            cur = {}
    if len(calls) != len(QUALITIES) * (rounds + 1):
        sys.exit(f"unexpected number of calls in the kernel trace: {len(calls)}")
    for qi, q in enumerate(QUALITIES):
        mine = calls[qi * (rounds + 1) + 1:(qi + 1) * (rounds + 1)]
        for name in NAMES if build == "release" else ("k_entropy_histogram", "k_entropy_lengths"):
            per_call = [sum(c.get(name, [])) for c in mine]
            emit({"what": "kernel", "build": build, "quality": q, "image": IMAGE, "kernel": name, "launches_per_call": len(mine[0].get(name, [])),
                  "us_per_call_median": round(statistics.median(per_call), 2), "us_per_call_min": round(min(per_call), 2),
                  "us_per_call_max": round(max(per_call), 2), "calls": len(mine)})
        total = [sum(sum(v) for v in c.values()) for c in mine]
        emit({"what": "kernels of a call", "build": build, "quality": q, "image": IMAGE, "us_median": round(statistics.median(total), 2), "calls": len(mine)})

# ---- one call, with and without the tables, in one process ----
s = solved(planes, its)
for q in QUALITIES:
    timed(s, q, False)
    timed(s, q, True)
    t = {False: [], True: []}
    size = {}
    for r in range(rounds):
        for optimize in ((False, True) if r % 2 == 0 else (True, False)):
            ms, data = timed(s, q, optimize)
            t[optimize].append(ms)
            size[optimize] = len(data)
    emit({"what": "call", "quality": q, "image": IMAGE, "rounds": rounds,
          "plain_ms_median": round(statistics.median(t[False]), 3), "plain_ms_min": round(min(t[False]), 3), "plain_ms_max": round(max(t[False]), 3),
          "optimize_ms_median": round(statistics.median(t[True]), 3), "optimize_ms_min": round(min(t[True]), 3), "optimize_ms_max": round(max(t[True]), 3),
          "plain_bytes": size[False], "optimize_bytes": size[True], "saved_percent": round(100.0 * (size[False] - size[True]) / size[False], 2)})
s.close()

# ---- the plain path under this library and the parent commit's: a process each, alternated ----
parent = os.environ.get("PARENT")
if parent and os.path.exists(parent):
    ms = {"this": {q: [] for q in QUALITIES}, "parent": {q: [] for q in QUALITIES}}
    medians = {"this": {q: [] for q in QUALITIES}, "parent": {q: [] for q in QUALITIES}}
    for r in range(3):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            cmd, env = child("--plain", parent if which == "parent" else None, rounds)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
            if res.returncode != 0:
                sys.exit(f"{which}: {res.stderr[-2000:]}")
            for line in res.stdout.splitlines():
                rec = json.loads(line)
                ms[which][rec["quality"]] += rec["ms"]
                medians[which][rec["quality"]].append(statistics.median(rec["ms"]))
    for q in QUALITIES:
        emit({"what": "plain to_jpeg against the parent", "quality": q, "image": IMAGE, "runs": 3, "calls_per_run": rounds,
              "this_ms_median_of_runs": round(statistics.median(medians["this"][q]), 3), "this_ms_runs": [round(v, 3) for v in medians["this"][q]],
              "parent_ms_median_of_runs": round(statistics.median(medians["parent"][q]), 3), "parent_ms_runs": [round(v, 3) for v in medians["parent"][q]],
              "this_ms_min": round(min(ms["this"][q]), 3), "parent_ms_min": round(min(ms["parent"][q]), 3)})
else:
    emit({"what": "plain to_jpeg against the parent", "unmeasured": "no PARENT library given"})

# ---- batch: images per second, three slots ----
IMAGES = 12
with j.Batch(devices=(0,), slots_per_device=3) as b:
    for q in QUALITIES:
        def burst(optimize):
            t0 = time.perf_counter()
            tickets = []
            for i in range(IMAGES):
                if len(tickets) == 3:
                    b.wait(tickets.pop(0))
                tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, jpeg={"quality": q, "subsampling": SUB, "optimize": optimize}))
            for t in tickets:
                b.wait(t)
            return IMAGES / (time.perf_counter() - t0)

        burst(False)
        burst(True)
        rates = {False: [], True: []}
        for r in range(rounds):
            for optimize in ((False, True) if r % 2 == 0 else (True, False)):
                rates[optimize].append(burst(optimize))
        emit({"what": "batch", "quality": q, "image": IMAGE, "iterations": its, "slots": 3, "images_per_burst": IMAGES, "rounds": rounds,
              "plain_images_per_s_median": round(statistics.median(rates[False]), 2), "plain_images_per_s_min": round(min(rates[False]), 2),
              "plain_images_per_s_max": round(max(rates[False]), 2),
              "optimize_images_per_s_median": round(statistics.median(rates[True]), 2), "optimize_images_per_s_min": round(min(rates[True]), 2),
              "optimize_images_per_s_max": round(max(rates[True]), 2)})

shutil.rmtree(work, ignore_errors=True)
with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
