#!/usr/bin/env python3
"""Upright output (k_upright_rows, k_upright_transpose) on one 4096x3072 4:2:0 image, with the method of tools/png_probe.py,
alternated runs, medians:
  kernels  the permutation kernels of an oriented Solver.to_tensor (f32) for orientation 3 (row-wise) and 6 (transposing), next to
           k_to_tensor of the same calls and of the unoriented call, from one `rocprofv3 --kernel-trace` run of this script's
           --kernels mode (a child process of its own); a launch permutes the three planes, so per plane is a third;
  tensor   wall time of the oriented Solver.to_tensor (f16 CHW) against the caller's own way on the parent path: the unoriented
           to_tensor followed by torch's rot90 / flip and .contiguous();
  files    wall time of to_png and to_jpeg, oriented (6) against unoriented;
  batch    images per second through Batch (three slots) for tag-6 file jobs with orientation="exif" into 224x224 f16 slots,
           against the same file without the tag;
  parent   (PARENT=path of the parent commit's library) the UNORIENTED to_tensor, to_png and to_jpeg under this library and the
           parent's, a process each (this script's --unoriented mode), alternated, three each.
Appends one JSON line per measurement to OUT (default profiles/upright.jsonl) and prints them.
    [PARENT=libjpeg2png_amd.so] python tools/upright_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

W, H = 4096, 3072
WEIGHT, PWEIGHT = 0.3, 0.001
IMAGE = f"{W}x{H} 4:2:0"


def solved(planes, its):
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return s


def size(o):
    return (H, W) if o >= 5 else (W, H)


def spread(prefix, values, digits=3):
    return {prefix + "_median": round(statistics.median(values), digits), prefix + "_min": round(min(values), digits),
            prefix + "_max": round(max(values), digits)}


def wall(call, rounds):
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
    import torch
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    for o in (1, 3, 6):
        s.set_orientation(o, W, H)
        out = torch.empty((3, size(o)[1], size(o)[0]), dtype=torch.float32, device="cuda")
        for _ in range(rounds + 1):
            s.to_tensor(*size(o), out=out)
            torch.cuda.synchronize()
    s.close()
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--unoriented":
    import torch
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    out = torch.empty((3, H, W), dtype=torch.float16, device="cuda")
    print(json.dumps({"to_tensor_f16_ms": statistics.median(wall(lambda: s.to_tensor(W, H, out=out), rounds)),
                      "to_png_ms": statistics.median(wall(lambda: s.to_png(W, H), rounds)),
                      "to_jpeg_ms": statistics.median(wall(lambda: s.to_jpeg(W, H, quality=90, subsampling=(2, 2)), rounds))}))
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "upright.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


work = tempfile.mkdtemp()
planes = synth.make_planes(W, H, "420", 95, seed=1240)
pickled = os.path.join(work, "planes.pickle")
with open(pickled, "wb") as f:
    pickle.dump(planes, f)

# ---- kernels: a profiled child process ----
rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
NAMES = ("k_upright_rows", "k_upright_transpose", "k_to_tensor")
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
    tensor = [us for _, name, us in launches if name == "k_to_tensor"]
    if len(tensor) != 3 * (rounds + 1):
        sys.exit(f"unexpected number of k_to_tensor launches in the kernel trace: {len(tensor)}")
    plane_bytes = W * H * 4
    for i, o in enumerate((1, 3, 6)):
        mine = tensor[i * (rounds + 1) + 1:(i + 1) * (rounds + 1)]
        # k_to_tensor f32: reads three planes, writes three
        emit(dict({"what": "kernel", "image": IMAGE, "orientation": o, "kernel": "k_to_tensor f32", "calls": len(mine),
                   "tb_per_s_at_median": round(6 * plane_bytes / statistics.median(mine) / 1e6, 3)}, **spread("us", mine, 2)))
    for o, name in ((3, "k_upright_rows"), (6, "k_upright_transpose")):
        mine = [us for _, n, us in launches if n == name][1:]
        emit(dict({"what": "kernel", "image": IMAGE, "orientation": o, "kernel": name, "planes_per_launch": 3, "calls": len(mine),
                   "us_per_plane_median": round(statistics.median(mine) / 3, 2),
                   "tb_per_s_at_median": round(6 * plane_bytes / statistics.median(mine) / 1e6, 3)}, **spread("us", mine, 2)))

# ---- the caller's alternative, and the files ----
import numpy as np  # noqa: E402
import torch  # noqa: E402
import upright_cases as uc  # noqa: E402

s = solved(planes, its)
TORCH = {3: lambda t: torch.flip(t, (1, 2)), 6: lambda t: torch.rot90(t, -1, (1, 2))}
for o in (3, 6):
    uw, uh = size(o)
    out = torch.empty((3, uh, uw), dtype=torch.float16, device="cuda")
    plain = torch.empty((3, H, W), dtype=torch.float16, device="cuda")
    s.set_orientation(o, W, H)
    ours = wall(lambda: s.to_tensor(uw, uh, out=out), rounds)
    s.set_orientation(1, W, H)
    theirs = wall(lambda: TORCH[o](s.to_tensor(W, H, out=plain)).contiguous(), rounds)
    same = bool(torch.equal(out, TORCH[o](plain).contiguous()))
    emit(dict({"what": "tensor", "image": IMAGE, "dtype": "f16 chw", "orientation": o, "rounds": rounds, "same_elements": same},
              **spread("oriented_ms", ours), **spread("unoriented_then_torch_ms", theirs)))
for name, call in (("to_png", lambda w, h: s.to_png(w, h)), ("to_jpeg 4:2:0 Q90", lambda w, h: s.to_jpeg(w, h, quality=90, subsampling=(2, 2)))):
    s.set_orientation(6, W, H)
    turned = wall(lambda: call(H, W), rounds)
    s.set_orientation(1, W, H)
    plain = wall(lambda: call(W, H), rounds)
    emit(dict({"what": "file", "image": IMAGE, "form": name, "orientation": 6, "rounds": rounds}, **spread("oriented_ms", turned),
              **spread("unoriented_ms", plain)))
emit({"what": "memory", "image": IMAGE, "upright_bytes": s.upright_bytes(), "output_scratch_bytes": s.output_scratch_bytes()})
s.close()

# ---- batch: tag-6 file jobs into 224 x 224 slots ----
from PIL import Image  # noqa: E402

buf = io.BytesIO()
exif = Image.Exif()
exif[uc.TAG] = 6
Image.fromarray(synth.synth_rgb(W, H, 1240).astype(np.uint8), "RGB").save(buf, "JPEG", quality=95, subsampling=2, exif=exif.tobytes())
tagged = buf.getvalue()
untagged = uc.strip_app_segments(tagged)
IMAGES = 12
with j.Batch(devices=(0,), slots_per_device=3) as b:
    slots = [torch.empty((3, 224, 224), dtype=torch.float16, device="cuda") for _ in range(3)]

    def burst(file):
        t0 = time.perf_counter()
        tickets = []
        for i in range(IMAGES):
            if len(tickets) == 3:
                b.wait(tickets.pop(0))
            tickets.append(b.submit(None, WEIGHT, [PWEIGHT] * 3, its, file=file, orientation="exif",
                                    outputs=[{"tensor": slots[i % 3], "out_width": 224, "out_height": 224, "filter": "triangle"}]))
        for t in tickets:
            b.wait(t)
        return IMAGES / (time.perf_counter() - t0)

    burst(untagged)
    burst(tagged)
    rates = {False: [], True: []}
    for r in range(rounds):
        for tag in ((False, True) if r % 2 == 0 else (True, False)):
            rates[tag].append(burst(tagged if tag else untagged))
    emit(dict({"what": "batch", "image": IMAGE + " quality 95", "iterations": its, "slots": 3, "images_per_burst": IMAGES, "rounds": rounds,
               "slot": "224x224 f16 triangle"}, **spread("untagged_images_per_s", rates[False], 2), **spread("tag_6_images_per_s", rates[True], 2)))

# ---- unoriented calls against the parent commit's library ----
parent = os.environ.get("PARENT")
if not parent or not os.path.exists(parent):
    emit({"what": "unoriented calls against the parent", "unmeasured": "PARENT names no library"})
else:
    got = {"change": [], "parent": []}
    for r in range(3):
        for k in (("change", "parent") if r % 2 == 0 else ("parent", "change")):
            env = dict(os.environ, **({"J2P_LIBRARY": parent} if k == "parent" else {}))
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--unoriented", pickled, str(its), str(max(rounds, 9))], capture_output=True,
                                 text=True, timeout=900, env=env)
            if res.returncode != 0:
                sys.exit(f"{k}: {res.stderr[-2000:]}")
            got[k].append(json.loads(res.stdout.strip().splitlines()[-1]))
    for key in ("to_tensor_f16_ms", "to_png_ms", "to_jpeg_ms"):
        emit(dict({"what": "unoriented call against the parent", "image": IMAGE, "call": key, "processes_each": 3},
                  **spread("change", [g[key] for g in got["change"]]), **spread("parent", [g[key] for g in got["parent"]])))

shutil.rmtree(work, ignore_errors=True)
with open(out_path, "a") as f:
    for r in lines:
        f.write(json.dumps(r) + "\n")
