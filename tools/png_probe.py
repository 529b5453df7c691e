#!/usr/bin/env python3
"""The PNG coder on the GPU (Solver.to_png: k_to_samples, k_png_filter, k_png_count, the tables on the host, k_png_pack, k_png_chunks,
k_png_crc) on one 4096x3072 4:2:0 image, 8 and 16 bits, with the method of tools/huffman_probe.py, alternated runs, medians:
  kernels  every kernel of a to_png call from one `rocprofv3 --kernel-trace` run of this script's --kernels mode (a child process of
           its own), per call;
  call     wall time of Solver.to_png, the file's size, and the size of zlib's own file of the same filtered stream (level 6, what
           libpng deflates with) and of PIL's file of the same pixels;
  sizes    the same for other block_bytes and idat_bytes: what the defaults were chosen from;
  batch    images per second through Batch (three slots) for png= jobs against bits=8 jobs (samples down, no file);
  cli      the command-line driver end to end with -P against without it (PARENT_CLI=path: the parent commit's binary without it),
           five alternated runs, on a quality-95 file of the image.
Appends one JSON line per measurement to OUT (default profiles/png_gpu.jsonl) and prints them.
    [PARENT_CLI=jpeg2png_gpu] python tools/png_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
import csv
import glob
import io
import json
import os
import pickle
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
IMAGE = f"{W}x{H} 4:2:0"
BITS = (8, 16)


def solved(planes, its):
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return s


def timed(s, bits, **kw):
    t0 = time.perf_counter()
    data = s.to_png(W, H, bits=bits, **kw)
    return (time.perf_counter() - t0) * 1e3, data


if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    for bits in BITS:
        for _ in range(rounds + 1):
            s.to_png(W, H, bits=bits)
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "png_gpu.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def spread(prefix, values, digits=3):
    return {prefix + "_median": round(statistics.median(values), digits), prefix + "_min": round(min(values), digits),
            prefix + "_max": round(max(values), digits)}


work = tempfile.mkdtemp()
planes = synth.make_planes(W, H, "420", 95, seed=1240)
pickled = os.path.join(work, "planes.pickle")
with open(pickled, "wb") as f:
    pickle.dump(planes, f)

# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
NAMES = ("k_to_samples", "k_png_filter", "k_png_count", "k_png_pack", "k_png_chunks", "k_png_crc")
if not os.path.exists(rocprof):
    emit({"what": "kernel", "unmeasured": "rocprofv3 not found"})
else:
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [sys.executable, os.path.abspath(__file__), "--kernels", pickled, str(its), str(rounds)]
        res = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", *cmd], capture_output=True, text=True, timeout=900,
                             cwd=tmp)
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
        if name == "k_png_crc":                         # (ends a call)
            calls.append(cur)
            cur = {}
    if len(calls) != len(BITS) * (rounds + 1):
        sys.exit(f"unexpected number of calls in the kernel trace: {len(calls)}")
    for bi, bits in enumerate(BITS):
        mine = calls[bi * (rounds + 1) + 1:(bi + 1) * (rounds + 1)]
        for name in NAMES:
            per_call = [sum(c.get(name, [])) for c in mine]
            emit(dict({"what": "kernel", "bits": bits, "image": IMAGE, "kernel": name, "launches_per_call": len(mine[0].get(name, [])), "calls": len(mine)},
                      **spread("us_per_call", per_call, 2)))
        total = [sum(sum(v) for v in c.values()) for c in mine]
        emit({"what": "kernels of a call", "bits": bits, "image": IMAGE, "us_median": round(statistics.median(total), 2), "calls": len(mine)})

# ---- one call; the file against zlib's and PIL's of the same pixels ----
import numpy as np  # noqa: E402
import png_cases as pc  # noqa: E402
from PIL import Image  # noqa: E402

s = solved(planes, its)
for bits in BITS:
    timed(s, bits)
    ms, data = [], b""
    for _ in range(rounds):
        t, data = timed(s, bits)
        ms.append(t)
    stream = zlib.decompress(pc.idat_data(data)[0])
    rle = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    rec = dict({"what": "call", "bits": bits, "image": IMAGE, "rounds": rounds, "bytes": len(data), "sample_bytes": W * H * 3 * bits // 8,
                "zlib_level_6_bytes_of_the_same_filtered_stream": len(zlib.compress(stream, 6)),
                "zlib_rle_bytes_of_the_same_filtered_stream": len(rle.compress(stream)) + len(rle.flush())},
               **spread("ms", ms))
    if bits == 8:
        # (PIL's file of the same pixels: its own filter choice and zlib at its default level)
        pixels = np.asarray(Image.open(io.BytesIO(data)))
        out = io.BytesIO()
        Image.fromarray(pixels).save(out, "PNG")
        rec["pil_bytes_of_the_same_pixels"] = len(out.getvalue())
    emit(rec)

# ---- other block and chunk sizes ----
for block_bytes, idat_bytes in ((4096, 8192), (8192, 8192), (16384, 8192), (32768, 8192), (65536, 8192), (262144, 8192), (1 << 20, 8192),
                                (32768, 2048), (32768, 32768), (32768, 1 << 20)):
    timed(s, 8, block_bytes=block_bytes, idat_bytes=idat_bytes)
    ms, data = [], b""
    for _ in range(rounds):
        t, data = timed(s, 8, block_bytes=block_bytes, idat_bytes=idat_bytes)
        ms.append(t)
    emit(dict({"what": "sizes", "bits": 8, "image": IMAGE, "block_bytes": block_bytes, "idat_bytes": idat_bytes, "bytes": len(data), "rounds": rounds},
              **spread("ms", ms)))
s.close()

# ---- batch: images per second, three slots ----
IMAGES = 12
with j.Batch(devices=(0,), slots_per_device=3) as b:
    outs = [np.empty((H, W, 3), np.uint8) for _ in range(3)]

    def burst(png):
        t0 = time.perf_counter()
        tickets = []
        for i in range(IMAGES):
            if len(tickets) == 3:
                b.wait(tickets.pop(0))
            kw = {"png": {"bits": 8}} if png else {"bits": 8, "out": outs[i % 3]}
            tickets.append(b.submit(planes, WEIGHT, [PWEIGHT] * 3, its, width=W, height=H, **kw))
        for t in tickets:
            b.wait(t)
        return IMAGES / (time.perf_counter() - t0)

    burst(False)
    burst(True)
    rates = {False: [], True: []}
    for r in range(rounds):
        for png in ((False, True) if r % 2 == 0 else (True, False)):
            rates[png].append(burst(png))
    emit(dict({"what": "batch", "image": IMAGE, "iterations": its, "slots": 3, "images_per_burst": IMAGES, "rounds": rounds},
              **spread("samples_images_per_s", rates[False], 2), **spread("png_images_per_s", rates[True], 2)))

# ---- the command line, end to end ----
from jpeg2png_amd.buildlib import build_cli  # noqa: E402
cli = build_cli()
parent_cli = os.environ.get("PARENT_CLI")
if cli is None:
    emit({"what": "cli", "unmeasured": "the driver was not built (no libjpeg / libpng headers)"})
else:
    jpg = os.path.join(work, "in.jpg")
    Image.fromarray(synth.synth_rgb(W, H, 1240).astype(np.uint8), "RGB").save(jpg, "JPEG", quality=95, subsampling=2)
    runs = {"with -P": [cli, jpg, "-q", "-P", "-o", os.path.join(work, "gpu.png")],
            "without": [parent_cli if parent_cli and os.path.exists(parent_cli) else cli, jpg, "-q", "-o", os.path.join(work, "libpng.png")]}
    secs = {k: [] for k in runs}
    for r in range(5):
        for k in (("with -P", "without") if r % 2 == 0 else ("without", "with -P")):
            t0 = time.perf_counter()
            res = subprocess.run(runs[k], capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.exit(f"{k}: {res.stderr[-2000:]}")
            secs[k].append(time.perf_counter() - t0)
    a, bb = Image.open(os.path.join(work, "gpu.png")), Image.open(os.path.join(work, "libpng.png"))
    emit(dict({"what": "cli", "image": IMAGE + " quality 95", "iterations": 50, "runs": 5, "without_is_the_parent_binary": bool(parent_cli and os.path.exists(parent_cli)),
               "same_pixels": bool(np.array_equal(np.asarray(a), np.asarray(bb))),
               "with_P_bytes": os.path.getsize(os.path.join(work, "gpu.png")), "without_bytes": os.path.getsize(os.path.join(work, "libpng.png"))},
              **spread("with_P_s", secs["with -P"]), **spread("without_s", secs["without"])))

shutil.rmtree(work, ignore_errors=True)
with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
