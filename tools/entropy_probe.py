#!/usr/bin/env python3
"""The JPEG file made on the GPU (j2p_planes_to_jpeg, Batch jpeg= jobs, `-j Q -e`) against what it replaces — the coefficients
brought down and entropy-coded by libjpeg on one core — on one 4096x3072 4:2:0 image at Q 75 and Q 95, alternated runs, medians:
  kernels  every kernel of Solver.to_jpeg from one `rocprofv3 --kernel-trace` run of this script's --kernels mode (a child
           process of its own), per call;
  call     wall time of Solver.to_jpeg (the file comes down) against Solver.coefficients() of the three components (the
           coefficients come down) plus libjpeg's coding of them — the helper tests/c/write_coefficients.c with -t, which times
           jpeg_finish_compress alone, on one core — with the bytes each brings down;
  batch    images per second through Batch (three slots) for jpeg= jobs against quant_tables= jobs (which leave the coding to
           the caller: it is NOT in their time);
  cli      the command-line driver end to end, `-j Q -S 420` with and without `-e`.
Appends one JSON line per measurement to OUT (default profiles/entropy_gpu.jsonl) and prints them.
    python tools/entropy_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
import csv
import glob
import json
import os
import shutil
import statistics
import struct
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
QUALITIES = (75, 95)
SUB = (2, 2)
SUBS = [(1, 1), SUB, SUB]
PREFIX = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")


def solved(its):
    planes = synth.make_planes(W, H, "420", 50, seed=1240)
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return planes, s


if "--kernels" in sys.argv:
    # what the profiler wraps: per quality one warm-up call and `rounds` calls
    _, s = solved(int(sys.argv[2]))
    for q in QUALITIES:
        for _ in range(int(sys.argv[3]) + 1):
            s.to_jpeg(W, H, quality=q, subsampling=SUB)
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "entropy_gpu.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
NAMES = ("k_quantise_blocks", "k_entropy_lengths", "k_scan_sums", "k_scan_tiles", "k_scan_apply", "k_entropy_pack", "k_stuff_count", "k_stuff_copy")
if os.path.exists(rocprof):
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                              "--kernels", str(its), str(rounds)], capture_output=True, text=True, timeout=900, cwd=tmp)
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
    # a call: 3 k_quantise_blocks ... 1 k_stuff_copy, which ends it; calls in time order: per quality a warm-up and `rounds`
    calls, cur = [], {}
    for _, name, us in launches:
        cur.setdefault(name, []).append(us)
        if name == "k_stuff_copy":
            calls.append(cur)
            cur = {}
    if len(calls) != len(QUALITIES) * (rounds + 1):
        sys.exit(f"unexpected number of calls in the kernel trace: {len(calls)}")
    for qi, q in enumerate(QUALITIES):
        mine = calls[qi * (rounds + 1) + 1:(qi + 1) * (rounds + 1)]
        total = []
        for name in NAMES:
            per_call = [sum(c.get(name, [])) for c in mine]
            emit({"what": "kernel", "quality": q, "image": f"{W}x{H} 4:2:0", "kernel": name, "launches_per_call": len(mine[0].get(name, [])),
                  "us_per_call_median": round(statistics.median(per_call), 2), "us_per_call_min": round(min(per_call), 2),
                  "us_per_call_max": round(max(per_call), 2), "calls": len(mine)})
        total = [sum(sum(v) for v in c.values()) for c in mine]
        emit({"what": "kernels of a call", "quality": q, "image": f"{W}x{H} 4:2:0", "us_median": round(statistics.median(total), 2), "calls": len(mine)})
else:
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})

# ---- one call: the file against the coefficients and libjpeg ----
helper = None
if os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
    helper = os.path.join(tempfile.mkdtemp(), "write_coefficients")
    subprocess.run(["gcc", "-O2", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "write_coefficients.c"), "-o", helper,
                    os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)


def libjpeg_ms(coefficients, quality):
    """(milliseconds of jpeg_finish_compress on one core, the file) for these coefficients"""
    raw = struct.pack("<6I", W, H, 3, quality, *SUB) + b"".join(a.tobytes() for a in coefficients)
    res = subprocess.run(["taskset", "-c", "0", helper, "-t"] if shutil.which("taskset") else [helper, "-t"], input=raw, capture_output=True, check=True)
    return float(res.stderr.decode().strip()), res.stdout


planes, s = solved(its)
for q in QUALITIES:
    tables = j.quality_tables(q, 3)

    def gpu_file():
        t0 = time.perf_counter()
        data = s.to_jpeg(W, H, quality=q, subsampling=SUB)
        return (time.perf_counter() - t0) * 1e3, data

    def coefficients_down():
        t0 = time.perf_counter()
        arrays = [s.coefficients(c, tables[c], subsampling=SUBS[c]) for c in range(3)]
        return (time.perf_counter() - t0) * 1e3, arrays

    gpu_file()
    coefficients_down()
    t_file, t_coef, t_host = [], [], []
    for r in range(rounds):
        for kind in (("file", "coef") if r % 2 == 0 else ("coef", "file")):
            if kind == "file":
                ms, data = gpu_file()
                t_file.append(ms)
            else:
                ms, arrays = coefficients_down()
                t_coef.append(ms)
                if helper:
                    host_ms, host_file = libjpeg_ms(arrays, q)
                    t_host.append(host_ms)
                    if host_file != data:
                        sys.exit(f"Q {q}: the GPU's file is not libjpeg's")
    emit({"what": "call", "quality": q, "image": f"{W}x{H} 4:2:0", "rounds": rounds, "file_bytes": len(data),
          "to_jpeg_ms_median": round(statistics.median(t_file), 3), "to_jpeg_ms_min": round(min(t_file), 3), "to_jpeg_ms_max": round(max(t_file), 3),
          "to_jpeg_bytes_down": len(data) + 16,
          "coefficients_ms_median": round(statistics.median(t_coef), 3), "coefficients_ms_min": round(min(t_coef), 3),
          "coefficients_ms_max": round(max(t_coef), 3), "coefficients_bytes_down": sum(a.nbytes for a in arrays),
          "libjpeg_one_core_ms_median": round(statistics.median(t_host), 3) if t_host else None,
          "libjpeg_one_core_ms_min": round(min(t_host), 3) if t_host else None, "same_bytes": bool(t_host)})
s.close()

# ---- batch: images per second, three slots ----
IMAGES = 12
with j.Batch(devices=(0,), slots_per_device=3) as b:
    for q in QUALITIES:
        tables = j.quality_tables(q, 3)
        outs = [[np.empty((-(-(H // 8) // sy), -(-(W // 8) // sx), 64), np.int16) for sx, sy in SUBS] for _ in range(3)]

        def burst(kind):
            t0 = time.perf_counter()
            tickets = []
            for i in range(IMAGES):
                if len(tickets) == 3:                   # three in flight: an output array set per slot
                    b.wait(tickets.pop(0))
                if kind == "jpeg":
                    tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, jpeg={"quality": q, "subsampling": SUB}))
                else:
                    tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, quant_tables=tables, subsampling=SUBS, out=outs[i % 3]))
            for t in tickets:
                b.wait(t)
            return IMAGES / (time.perf_counter() - t0)

        burst("jpeg")
        burst("coefficients")
        rates = {"jpeg": [], "coefficients": []}
        for r in range(rounds):
            for kind in (("jpeg", "coefficients") if r % 2 == 0 else ("coefficients", "jpeg")):
                rates[kind].append(burst(kind))
        emit({"what": "batch", "quality": q, "image": f"{W}x{H} 4:2:0", "iterations": its, "slots": 3, "images_per_burst": IMAGES, "rounds": rounds,
              "jpeg_images_per_s_median": round(statistics.median(rates["jpeg"]), 2), "jpeg_images_per_s_min": round(min(rates["jpeg"]), 2),
              "jpeg_images_per_s_max": round(max(rates["jpeg"]), 2),
              "coefficients_images_per_s_median": round(statistics.median(rates["coefficients"]), 2),
              "coefficients_images_per_s_min": round(min(rates["coefficients"]), 2), "coefficients_images_per_s_max": round(max(rates["coefficients"]), 2),
              "note": "the coefficient jobs' files are still to be coded by the caller"})

# ---- the driver end to end: a process per run, as a user runs it ----
from jpeg2png_amd.buildlib import build_cli  # noqa: E402
from PIL import Image  # noqa: E402

exe = build_cli()
if exe:
    with tempfile.TemporaryDirectory() as tmp:
        jpg = os.path.join(tmp, "in.jpg")
        Image.fromarray(synth.synth_rgb(W, H, 1241).astype(np.uint8), "RGB").save(jpg, "JPEG", quality=50, subsampling=2)
        for q in QUALITIES:
            runs = {f"-j {q} -S 420": ("host.jpg", []), f"-j {q} -S 420 -e": ("gpu.jpg", ["-e"])}
            samples = {k: [] for k in runs}
            for r in range(rounds + 1):
                for kind in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                    out = os.path.join(tmp, runs[kind][0])
                    t0 = time.perf_counter()
                    res = subprocess.run([exe, jpg, "-o", out, "-q", "-i", str(its), "-j", str(q), "-S", "420", *runs[kind][1]], capture_output=True,
                                         text=True, timeout=600)
                    dt = time.perf_counter() - t0
                    if res.returncode != 0:
                        sys.exit(f"{kind}: {res.stderr}")
                    if r:                               # round 0: warm-up (page cache, code objects)
                        samples[kind].append(dt * 1e3)
            same = open(os.path.join(tmp, "host.jpg"), "rb").read() == open(os.path.join(tmp, "gpu.jpg"), "rb").read()
            for kind in runs:
                emit({"what": "cli", "image": f"{W}x{H} 4:2:0 q50", "run": kind, "iterations": its, "rounds": rounds,
                      "ms_median": round(statistics.median(samples[kind]), 1), "ms_min": round(min(samples[kind]), 1), "ms_max": round(max(samples[kind]), 1),
                      "output_bytes": os.path.getsize(os.path.join(tmp, runs[kind][0])), "same_bytes": same})

with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
