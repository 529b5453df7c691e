"""A/B of two builds of the library on the SAME planes in ONE process, runs alternated: us per iteration (wall clock
over reset + run + sync), the HIP-event figures of the two phase kernels, the non-temporal level the policy chose and the
digest of every solved plane.  Written for the shared gradient / prob-state buffer (profiles/r07_shared_state_ab.jsonl): `--a` is
the parent commit's library, `--b` the tree's.  Each plane is synthesised once; per pair the solver of A, then the solver of B
is created, warmed, timed and destroyed (one solver alive at a time: the non-temporal policy sees its bytes alone).
usage: python tools/share_state_ab.py --a PARENT.so [--b LIB.so] [--pairs 3] [--its 100] [--reps 3] [--only NAME,...] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpeg2png_amd as j                  # noqa: E402
from jpeg2png_amd import synth            # noqa: E402

WEIGHT, PWEIGHT = 0.3, 0.001
# name: (W, H, subsampling, quality, Y only)
PLANES = {
    "1080p Y": (1920, 1080, "444", 10, True),
    "2048^2": (2048, 2048, "444", 10, True),
    "4096x3584": (4096, 3584, "444", 10, True),
    "4096^2": (4096, 4096, "444", 10, True),
    "4096x4608": (4096, 4608, "444", 10, True),
    "4096x5120": (4096, 5120, "444", 10, True),
    "8192x4096": (8192, 4096, "444", 10, True),
    "16384x2048": (16384, 2048, "444", 10, True),
    "8192^2": (8192, 8192, "444", 10, True),
    "4096^2 4:4:4 joint": (4096, 4096, "444", 10, False),
    "configs[4] slice (1080p 4:2:0 Q50 joint)": (1920, 1080, "420", 50, False),
}


def make(name):
    W, H, sub, q, y_only = PLANES[name]
    if y_only and W * H > (1 << 25):
        return [synth.make_y_plane_banded(W, H, q, seed=1237, band_rows=1024, workers=16)]
    return synth.make_planes(W, H, sub, q, seed=1237 if y_only else 1238, y_only=y_only)


def one(path, planes, its, reps):
    with j.library(path) as lib:
        s = j.Solver(planes, WEIGHT, [PWEIGHT] * len(planes), its)
        try:
            def run():
                s.reset()
                s.run(its)
                s.sync()
            run()
            s.enable_timing(16)
            t0 = time.perf_counter()
            for _ in range(reps):
                run()
            dt = (time.perf_counter() - t0) / reps
            g_ms, p_ms, n = s.kernel_times()
            s.enable_timing(0)
            digest = hashlib.blake2b(digest_size=16)
            for c in range(s.nch):
                digest.update(np.ascontiguousarray(s.download(c)))
            shared = None
            if hasattr(lib, "j2p_solver_shares_state"):
                shared = [s.shares_state(c) for c in range(s.nch)]
            return {"us_per_iteration": round(dt / its * 1e6, 2), "k_gradient_us": round(g_ms * 1e3, 2), "k_project_us": round(p_ms * 1e3, 2),
                    "event_samples": n, "shares_state": shared, "digest": digest.hexdigest()}
        finally:
            s.close()
            lib.j2p_pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="library A (the parent commit's)")
    ap.add_argument("--b", default=j.LIB_PATH, help="library B (default: the tree's)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--its", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated plane names (default: all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    names = [n for n in PLANES if not a.only or n in a.only.split(",")]
    out = open(a.out, "a") if a.out else None
    for name in names:
        planes = make(name)
        runs = {"a": [], "b": []}
        for _ in range(a.pairs):
            runs["a"].append(one(a.a, planes, a.its, a.reps))
            runs["b"].append(one(a.b, planes, a.its, a.reps))
        us = {k: [r["us_per_iteration"] for r in v] for k, v in runs.items()}
        digests = {k: sorted({r["digest"] for r in v}) for k, v in runs.items()}
        line = {"plane": name + f" Q{PLANES[name][3]} -i {a.its}", "pairs": a.pairs, "reps_per_run": a.reps,
                "a_us_per_iteration": us["a"], "b_us_per_iteration": us["b"],
                "a_mean": round(float(np.mean(us["a"])), 2), "b_mean": round(float(np.mean(us["b"])), 2),
                "a_spread": round(max(us["a"]) - min(us["a"]), 2), "b_minus_a": round(float(np.mean(us["b"]) - np.mean(us["a"])), 2),
                "a_k_gradient_us": [r["k_gradient_us"] for r in runs["a"]], "b_k_gradient_us": [r["k_gradient_us"] for r in runs["b"]],
                "a_k_project_us": [r["k_project_us"] for r in runs["a"]], "b_k_project_us": [r["k_project_us"] for r in runs["b"]],
                "b_shares_state": runs["b"][0]["shares_state"],
                "digests_equal": digests["a"] == digests["b"] and len(digests["a"]) == 1, "digest": digests["b"][0]}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        del planes


if __name__ == "__main__":
    main()
