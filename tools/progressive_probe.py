#!/usr/bin/env python3
"""The progressive JPEG file on the GPU (k_prog_*; Solver.to_jpeg(progressive=True)) against the optimised and the plain file and
against the CPU path it replaces, with the method of tools/huffman_probe.py, on one 4096x3072 4:2:0 image at Q 75 and Q 95,
alternated runs, medians:
  kernels  every kernel of Solver.to_jpeg(progressive=True), per call, and the host's waits (hipStreamSynchronize) per call of the
           progressive and of the optimised form, from one `rocprofv3 --kernel-trace --hip-trace` run of this script's --kernels mode
           (a child process of its own); the same run codes the two pathological images of DESIGN.md section 25 — AC scans that are
           ONE segment, which one lane of k_prog_runs walks — through entropy_encode(progressive=True);
  call     wall time of Solver.to_jpeg progressive, optimised and plain in one process, and the three files' sizes;
  cpu      the path the call replaces: Solver.coefficients x 3 and libjpeg's progressive coding of them on one core
           (tests/c/write_coefficients_progressive.c -t: jpeg_finish_compress alone), where libjpeg's headers are installed;
  parent   Solver.to_jpeg plain and optimised under this library and under the parent commit's (PARENT=path), a process each,
           alternated, medians of three runs: the existing paths must not have moved;
  batch    images per second through Batch (three slots) for jpeg= jobs progressive and optimised.
Appends one JSON line per measurement to OUT (default profiles/progressive_gpu.jsonl) and prints them.
    [PARENT=lib.so] python tools/progressive_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
import csv
import glob
import json
import os
import pickle
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
IMAGE = f"{W}x{H} 4:2:0"
FORMS = ("progressive", "optimize", "plain")


def solved(planes, its):
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return s


def timed(s, q, form):
    t0 = time.perf_counter()
    data = s.to_jpeg(W, H, quality=q, subsampling=SUB, progressive=form == "progressive", optimize=form == "optimize")
    return (time.perf_counter() - t0) * 1e3, data


def flat_image(ac):
    """every block alike: DC 0 and `ac` at all 63 AC positions"""
    bw, bh = W // 8, H // 8
    luma, chroma = np.full((bh, bw, 64), ac, np.int16), np.full((bh // 2, bw // 2, 64), ac, np.int16)
    luma[:, :, 0] = chroma[:, :, 0] = 0
    return [luma, chroma, chroma]


# the images of DESIGN.md section 25 whose AC scans are ONE segment each, walked by one lane of k_prog_runs: all zero — every scan,
# runs of 32767 blocks — and 4 everywhere — the refinement scans, no new coefficient and 63 correction bits a block: a run every 15
PATHOLOGICAL = (("every coefficient zero", 0), ("every AC coefficient 4", 4))


if len(sys.argv) > 1 and sys.argv[1] in ("--kernels", "--existing"):
    # the child processes: planes from the pickle the parent left, so that every child solves the same image
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    if sys.argv[1] == "--kernels":
        for form in ("progressive", "optimize"):
            for q in QUALITIES:
                for _ in range(rounds + 1):
                    timed(s, q, form)
        tables = j.quality_tables(75, 3)
        for _name, ac in PATHOLOGICAL:
            image = flat_image(ac)
            for _ in range(3):
                j.entropy_encode(image, W, H, tables, SUB, progressive=True)
    else:
        for form in ("plain", "optimize"):
            for q in QUALITIES:
                timed(s, q, form)
                ms = [timed(s, q, form)[0] for _ in range(rounds)]
                print(json.dumps({"form": form, "quality": q, "ms": ms}), flush=True)
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "progressive_gpu.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def spread(prefix, values, digits=3):
    return {prefix + "_median": round(statistics.median(values), digits), prefix + "_min": round(min(values), digits), prefix + "_max": round(max(values), digits)}


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


# ---- kernels and waits: one profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
NEW = ("k_prog_classify", "k_prog_runs", "k_prog_ac<0>", "k_prog_ac<1>", "k_prog_ac<2>", "k_prog_dc<0>", "k_prog_dc<1>", "k_prog_dc<2>")
NAMES = ("k_quantise_blocks",) + NEW + ("k_entropy_histogram", "k_entropy_lengths", "k_entropy_pack", "k_scan_sums", "k_scan_tiles", "k_scan_apply",
                                        "k_stuff_count", "k_stuff_copy")
if not os.path.exists(rocprof):
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})
else:
    with tempfile.TemporaryDirectory() as tmp:
        cmd, env = child("--kernels", None, rounds)
        res = subprocess.run([rocprof, "--kernel-trace", "--hip-trace", "--output-format", "csv", "-d", tmp, "--", *cmd], capture_output=True, text=True,
                             timeout=900, cwd=tmp, env=env)
        if res.returncode != 0:
            sys.exit("profiled run failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
        launches, waits = [], []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = next((n for n in NAMES if n in row["Kernel_Name"]), None)
                    if name:
                        launches.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        for path in glob.glob(os.path.join(tmp, "**", "*hip_api_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if row["Function"] == "hipStreamSynchronize":
                        waits.append(int(row["Start_Timestamp"]))
    launches.sort()
    # a call: from its first kernel (k_quantise_blocks of a solver's call, k_prog_classify of the zero image's) to its last k_stuff_copy
    calls, cur, begun, copies = [], {}, None, 0
    ncalls = 2 * len(QUALITIES) * (rounds + 1)
    for at, name, us in launches:
        progressive = len(calls) < ncalls // 2 or len(calls) >= ncalls
        if begun is None:
            begun = at
        cur.setdefault(name, []).append(us)
        if name == "k_stuff_copy":
            copies += 1
            if copies == (10 if progressive else 1):       # (ends a call: a copy per scan)
                calls.append((begun, at, cur))
                cur, begun, copies = {}, None, 0
    if len(calls) != ncalls + 3 * len(PATHOLOGICAL):
        sys.exit(f"unexpected number of calls in the kernel trace: {len(calls)}")

    def waits_of(k):
        """the host's waits between the call's first kernel and the next call's (the last wait follows the last kernel)"""
        end = calls[k + 1][0] if k + 1 < len(calls) else float("inf")
        return sum(1 for w in waits if calls[k][0] <= w < end)

    for fi, form in enumerate(("progressive", "optimize")):
        for qi, q in enumerate(QUALITIES):
            k0 = (fi * len(QUALITIES) + qi) * (rounds + 1)
            mine = calls[k0 + 1:k0 + rounds + 1]
            if form == "progressive":
                for name in NAMES:
                    per_call = [sum(c[2].get(name, [])) for c in mine]
                    if max(per_call) == 0:
                        continue
                    emit({"what": "kernel", "quality": q, "image": IMAGE, "kernel": name, "new": name in NEW, "launches_per_call": len(mine[0][2].get(name, [])),
                          "calls": len(mine), **spread("us_per_call", per_call, 2)})
                new = [sum(sum(v) for n, v in c[2].items() if n in NEW) for c in mine]
                emit({"what": "new kernels of a call", "quality": q, "image": IMAGE, "calls": len(mine), **spread("us", new, 2)})
            total = [sum(sum(v) for v in c[2].values()) for c in mine]
            counted = ([waits_of(k) for k in range(k0 + 1, k0 + rounds + 1)] if waits else None)
            emit({"what": "kernels and waits of a call", "form": form, "quality": q, "image": IMAGE, "calls": len(mine), **spread("kernels_us", total, 2),
                  "launches": sum(len(v) for v in mine[0][2].values()),
                  "host_waits_per_call": counted if counted else "unmeasured: no hip api trace found"})
    for k, (name, _ac) in enumerate(PATHOLOGICAL):
        mine = calls[ncalls + 3 * k + 1:ncalls + 3 * k + 3]
        # (a call whose first buffer was too small, or whose block moved, walks the scans again: per pass over the 8 AC scans)
        passes = [len(c[2].get("k_prog_runs", [])) / 8 for c in mine]
        emit({"what": "pathological image", "image": f"{IMAGE}, {name}", "calls": len(mine), "passes_per_call": passes,
              **spread("k_prog_runs_us_per_pass", [sum(c[2].get("k_prog_runs", [])) / n for c, n in zip(mine, passes)], 2),
              "k_prog_runs_us_longest_launch": round(max(max(c[2].get("k_prog_runs", [0])) for c in mine), 2),
              **spread("kernels_us_per_call", [sum(sum(v) for v in c[2].values()) for c in mine], 2)})

# ---- one call of each form, in one process ----
s = solved(planes, its)
files = {}
for q in QUALITIES:
    for form in FORMS:
        timed(s, q, form)
    t = {form: [] for form in FORMS}
    for r in range(rounds):
        for form in (FORMS if r % 2 == 0 else FORMS[::-1]):
            ms, data = timed(s, q, form)
            t[form].append(ms)
            files[q, form] = data
    size = {form: len(files[q, form]) for form in FORMS}
    rec = {"what": "call", "quality": q, "image": IMAGE, "rounds": rounds}
    for form in FORMS:
        rec.update(spread(form + "_ms", t[form]))
        rec[form + "_bytes"] = size[form]
    rec["progressive_against_optimize_percent"] = round(100.0 * (size["progressive"] - size["optimize"]) / size["optimize"], 2)
    rec["progressive_against_plain_percent"] = round(100.0 * (size["progressive"] - size["plain"]) / size["plain"], 2)
    emit(rec)

# ---- the path the call replaces: the coefficients down, libjpeg's progressive coding on one core ----
prefix = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")
helper = os.path.join(work, "write_coefficients_progressive")
built = os.path.exists(os.path.join(prefix, "include", "jpeglib.h")) and subprocess.run(
    ["gcc", "-O2", "-I", os.path.join(prefix, "include"), os.path.join(ROOT, "tests", "c", "write_coefficients_progressive.c"), "-o", helper,
     os.path.join(prefix, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(prefix, "lib")]).returncode == 0
for q in QUALITIES:
    if not built:
        emit({"what": "cpu path", "quality": q, "unmeasured": "libjpeg's headers are not installed"})
        continue
    tables = j.quality_tables(q, 3)
    bw, bh = W // 8, H // 8
    down, code = [], []
    for r in range(rounds):
        t0 = time.perf_counter()
        coef = [s.coefficients(c, tables[c], blocks_w=bw // (2 if c else 1), blocks_h=bh // (2 if c else 1), subsampling=SUB if c else (1, 1)) for c in range(3)]
        down.append((time.perf_counter() - t0) * 1e3)
        raw = struct.pack("<6I", W, H, 3, q, *SUB) + b"".join(np.ascontiguousarray(a, dtype=np.int16).tobytes() for a in coef)
        res = subprocess.run([helper, "-t"], input=raw, capture_output=True, check=True)
        code.append(float(res.stderr.decode().split()[-1]))
        same = res.stdout == files[q, "progressive"]
    emit({"what": "cpu path", "quality": q, "image": IMAGE, "rounds": rounds, **spread("coefficients_x3_ms", down), **spread("libjpeg_progressive_ms", code),
          "sum_of_medians_ms": round(statistics.median(down) + statistics.median(code), 3), "same_bytes_as_the_gpu": same})
s.close()

# ---- the existing forms under this library and the parent commit's: a process each, alternated ----
parent = os.environ.get("PARENT")
if parent and os.path.exists(parent):
    medians = {(which, form, q): [] for which in ("this", "parent") for form in ("plain", "optimize") for q in QUALITIES}
    for r in range(3):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            cmd, env = child("--existing", parent if which == "parent" else None, rounds)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
            if res.returncode != 0:
                sys.exit(f"{which}: {res.stderr[-2000:]}")
            for line in res.stdout.splitlines():
                rec = json.loads(line)
                medians[which, rec["form"], rec["quality"]].append(statistics.median(rec["ms"]))
    for form in ("plain", "optimize"):
        for q in QUALITIES:
            mine, theirs = medians["this", form, q], medians["parent", form, q]
            emit({"what": "existing to_jpeg against the parent", "form": form, "quality": q, "image": IMAGE, "runs": 3, "calls_per_run": rounds,
                  "this_ms_median_of_runs": round(statistics.median(mine), 3), "this_ms_runs": [round(v, 3) for v in mine],
                  "parent_ms_median_of_runs": round(statistics.median(theirs), 3), "parent_ms_runs": [round(v, 3) for v in theirs],
                  "parent_spread_percent": round(100.0 * (max(theirs) - min(theirs)) / statistics.median(theirs), 2)})
else:
    emit({"what": "existing to_jpeg against the parent", "unmeasured": "no PARENT library given"})

# ---- batch: images per second, three slots ----
IMAGES = 12
with j.Batch(devices=(0,), slots_per_device=3) as b:
    for q in QUALITIES:
        def burst(form):
            t0 = time.perf_counter()
            tickets = []
            for i in range(IMAGES):
                if len(tickets) == 3:
                    b.wait(tickets.pop(0))
                tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, jpeg={"quality": q, "subsampling": SUB, form: True}))
            for t in tickets:
                b.wait(t)
            return IMAGES / (time.perf_counter() - t0)

        forms = ("progressive", "optimize")
        for form in forms:
            burst(form)
        rates = {form: [] for form in forms}
        for r in range(rounds):
            for form in (forms if r % 2 == 0 else forms[::-1]):
                rates[form].append(burst(form))
        emit({"what": "batch", "quality": q, "image": IMAGE, "iterations": its, "slots": 3, "images_per_burst": IMAGES, "rounds": rounds,
              **spread("progressive_images_per_s", rates["progressive"], 2), **spread("optimize_images_per_s", rates["optimize"], 2)})

shutil.rmtree(work, ignore_errors=True)
with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
