#!/usr/bin/env python3
"""Restart intervals in the JPEG files the GPU writes (restart_rows=, restart_interval=), with the method of
tools/progressive_probe.py, on one 4096x3072 4:2:0 image at Q 75 and Q 95, medians of alternated runs:
  call     file size and wall time of Solver.to_jpeg for the three coders with restart_rows=1 against the same call without restarts
           in the same process;
  decode   entropy_decode(progressive=True, stats=True) — decode_ms, rounds, host waits, the share of AC refinement — of the
           library's own progressive file written with restart_rows=1 against the same image written without restarts: the payoff
           ("files with restart intervals, which this form already spreads over wavefronts");
  parent   Solver.to_jpeg plain, optimised and progressive WITHOUT restarts under this library and under the parent commit's
           (PARENT=path), a process each, three alternated runs: the existing paths must not have moved.  The parent's own
           run-to-run spread is reported next to the difference.
Appends one JSON line per measurement to OUT (default profiles/restart_markers.jsonl) and prints them.
    [PARENT=lib.so] python tools/restart_probe.py [ITERATIONS = 50] [ROUNDS = 5] [OUT]"""
import json
import os
import pickle
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
FORMS = ("plain", "optimize", "progressive")


def solved(planes, its):
    s = j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its)
    s.run(its)
    s.sync()
    return s


def timed(s, q, form, **restart):
    t0 = time.perf_counter()
    data = s.to_jpeg(W, H, quality=q, subsampling=SUB, progressive=form == "progressive", optimize=form == "optimize", **restart)
    return (time.perf_counter() - t0) * 1e3, data


if len(sys.argv) > 1 and sys.argv[1] == "--existing":
    # a child process: planes from the pickle the parent left, so that every child solves the same image; no restart keyword, so
    # that the parent commit's library serves too
    with open(sys.argv[2], "rb") as f:
        planes = pickle.load(f)
    its, rounds = int(sys.argv[3]), int(sys.argv[4])
    s = solved(planes, its)
    for form in FORMS:
        for q in QUALITIES:
            timed(s, q, form)
            ms = [timed(s, q, form)[0] for _ in range(rounds)]
            print(json.dumps({"form": form, "quality": q, "ms": ms}), flush=True)
    s.close()
    sys.exit(0)

args = sys.argv[1:]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "restart_markers.jsonl")
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def spread(prefix, values, digits=3):
    return {prefix + "_median": round(statistics.median(values), digits), prefix + "_min": round(min(values), digits), prefix + "_max": round(max(values), digits)}


planes = synth.make_planes(W, H, "420", 50, seed=1240)
s = solved(planes, its)

# ---- call: the three coders with and without restart_rows=1, alternated ----
files = {}
for q in QUALITIES:
    for form in FORMS:
        timed(s, q, form)
        timed(s, q, form, restart_rows=1)
        without, with_rows = [], []
        for _ in range(rounds):
            ms, plain = timed(s, q, form)
            without.append(ms)
            ms, rows = timed(s, q, form, restart_rows=1)
            with_rows.append(ms)
        files[(q, form)] = (plain, rows)
        rec = {"what": "call", "image": IMAGE, "quality": q, "form": form, "restart_rows": 1, "rounds": rounds, "bytes": len(plain), "bytes_rows": len(rows),
               "markers": sum(rows.count(bytes([0xff, 0xd0 + k])) for k in range(8))}
        rec.update(spread("ms", without))
        rec.update(spread("ms_rows", with_rows))
        emit(rec)
s.close()

# ---- decode: the library's own progressive file, with and without restarts ----
for q in QUALITIES:
    plain, rows = files[(q, "progressive")]
    want = j.entropy_decode(plain, progressive=True)
    got = j.entropy_decode(rows, progressive=True)
    same = all((a == b).all() for a, b in zip(want, got))
    for name, data in (("none", plain), ("rows_1", rows)):
        j.entropy_decode(data, progressive=True)
        stats = [j.entropy_decode(data, progressive=True, stats=True)[1] for _ in range(rounds)]
        rec = {"what": "decode", "image": IMAGE, "quality": q, "restart": name, "bytes": len(data), "rounds_run": rounds, "same_coefficients": bool(same)}
        rec.update(spread("decode_ms", [st["decode_ms"] for st in stats]))
        for key in ("rounds", "host_waits", "subsequences", "ac_refine_share"):
            if key in stats[-1]:
                rec[key] = stats[-1][key]
        emit(rec)

# ---- parent: the paths without restarts, this library against the parent commit's ----
parent = os.environ.get("PARENT")
if parent:
    work = tempfile.mkdtemp()
    pickled = os.path.join(work, "planes.pickle")
    with open(pickled, "wb") as f:
        pickle.dump(planes, f)
    runs = {"this": [], "parent": []}
    for _ in range(3):
        for name, library in (("this", None), ("parent", parent)):
            env = dict(os.environ)
            if library:
                env["J2P_LIBRARY"] = os.path.abspath(library)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing", pickled, str(its), str(rounds)], env=env, capture_output=True,
                                 text=True, check=True, timeout=600).stdout
            runs[name].append({(r["form"], r["quality"]): statistics.median(r["ms"]) for r in map(json.loads, out.splitlines())})
    for form in FORMS:
        for q in QUALITIES:
            this, old = [r[(form, q)] for r in runs["this"]], [r[(form, q)] for r in runs["parent"]]
            rec = {"what": "parent", "image": IMAGE, "quality": q, "form": form, "processes": 3}
            rec.update(spread("ms", this))
            rec.update(spread("parent_ms", old))
            rec["difference_of_medians_ms"] = round(statistics.median(this) - statistics.median(old), 3)
            rec["parent_spread_ms"] = round(max(old) - min(old), 3)
            emit(rec)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    for rec in lines:
        f.write(json.dumps(rec) + "\n")
