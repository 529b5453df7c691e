#!/usr/bin/env python3
"""Zoomed joint solves, resident on one GPU: time per iteration after warm-up (synchronised host clock over whole
runs) and the phase kernels' device times (HIP events, Solver.enable_timing), for the wide-footprint projection path
(J2P_OPT_WIDE_FOOTPRINT 1) and the generic one (0) alternated in the same process, beside the same-canvas 4:4:4 joint
solve.  Appends one JSON line per workload and path to OUT (default profiles/zoom_by_size.jsonl) and prints them.
    python tools/zoom_probe.py [ITERATIONS] [ROUNDS] [OUT] [--quick]
(--quick: one round of 10 iterations, nothing written — what a rocprofv3 --kernel-trace --stats run wraps; J2P_LIBRARY
picks the build, the digest tells same bits)"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j  # noqa: E402
from jpeg2png_amd import synth  # noqa: E402

quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if a != "--quick"]
its = int(args[0]) if args else 50
rounds = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "zoom_by_size.jsonl")
if quick:
    its, rounds = 10, 1
tag = os.path.basename(os.environ.get("J2P_LIBRARY", "release"))
WEIGHT, PWEIGHT = 0.3, 0.001
# (name, image w, h, subsampling, zoom): three zoomed 4:2:0 images and the 4:4:4 canvas of the same size
WORKLOADS = [("2048^2 4:2:0 x2", 2048, 2048, "420", 2), ("1024^2 4:2:0 x4", 1024, 1024, "420", 4),
             ("1360^2 4:2:0 x3", 1360, 1360, "420", 3), ("4096^2 4:4:4 x1", 4096, 4096, "444", 1)]


def digest(s, n):
    h = hashlib.blake2b(digest_size=8)
    for c in range(n):
        h.update(s.download(c).tobytes())
    return h.hexdigest()


def timed(s):
    s.reset()
    s.sync()
    t0 = time.perf_counter()
    s.run(its)
    s.sync()
    return (time.perf_counter() - t0) / its * 1e6


lines = []
for name, w, h, sub, zoom in WORKLOADS:
    planes = j.zoomed(synth.make_planes(w, h, sub, 50, seed=1238), zoom)
    variants = [1, 0] if zoom > 1 else [1]
    with j.Solver(planes, WEIGHT, [PWEIGHT] * 3, its) as s:
        samples = {v: [] for v in variants}
        digests, paths = {}, {}
        for v in variants:                       # warm-up of both paths
            s.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, v)
            timed(s)
            digests[v] = digest(s, 3)
            paths[v] = "".join("w" if s.wide_footprint(c) else "-" for c in range(3))
        for r in range(rounds):                  # alternated, the order flipped every round
            for v in (variants if r % 2 == 0 else variants[::-1]):
                s.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, v)
                samples[v].append(timed(s))
        kern = {}
        for v in variants:                       # device times of the two phases, in a pass of their own
            s.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, v)
            s.reset()
            s.enable_timing(1)
            s.run(its)
            s.sync()
            g, p, n = s.kernel_times()
            s.enable_timing(0)
            kern[v] = (g * 1e3, p * 1e3)
        for v in variants:
            rec = {"workload": name, "canvas": f"{s.W}x{s.H}", "sampling": [[p.w_samp, p.h_samp] for p in planes],
                   "path": "wide" if v else "generic", "channels_on_wide_path": paths[v], "library": tag, "iterations": its,
                   "us_per_iteration_median": round(statistics.median(samples[v]), 2),
                   "us_per_iteration_best": round(min(samples[v]), 2), "gradient_kernel_us": round(kern[v][0], 2),
                   "project_kernel_us": round(kern[v][1], 2), "digest": digests[v]}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        if len(variants) == 2 and digests[0] != digests[1]:
            print(f"DIGESTS DIFFER: {name}", flush=True)
            sys.exit(1)

ref = next(r for r in lines if r["workload"].startswith("4096^2 4:4:4"))
summary = []
for r in lines:
    if r["path"] != "wide" or r is ref:
        continue
    g = next(x for x in lines if x["workload"] == r["workload"] and x["path"] == "generic")
    summary.append({"workload": r["workload"], "library": tag, "summary": True,
                    "wide_over_generic_iteration": round(r["us_per_iteration_median"] / g["us_per_iteration_median"], 3),
                    "wide_over_generic_project_kernel": round(r["project_kernel_us"] / g["project_kernel_us"], 3),
                    "wide_over_444_iteration": round(r["us_per_iteration_median"] / ref["us_per_iteration_median"], 3),
                    "generic_over_444_iteration": round(g["us_per_iteration_median"] / ref["us_per_iteration_median"], 3)})
    print(json.dumps(summary[-1]), flush=True)
if not quick:
    with open(out_path, "a") as f:
        for r in lines + summary:
            f.write(json.dumps(r) + "\n")
