"""Phase orders against each other and against the parent commit's library, on the SAME planes in ONE process, runs alternated
(tools/share_state_ab.py extended by the order override): us per iteration (wall clock over reset + run + sync), the HIP-event
figures of the two phase kernels and the digest of every solved plane.  Per pair the parent's solver, then one solver of the
tree's library per order is created, warmed, timed and destroyed (one solver alive at a time); who goes first rotates from
pair to pair (the first solver of a pair ran up to 1 us per iteration slower than the same schedule later in it).  Orders are
"GP" pairs of J2P_ORDER_* digits, gradient then projection: 00 forward / forward, 10 the gradient phase bottom-up per XCD,
01 the projection, 11 both; "policy" = what the library chooses itself.
usage: python tools/phase_order_ab.py --a PARENT.so [--b LIB.so] [--orders policy,00,10,01,11] [--pairs 3] [--its 100] [--reps 3]
       [--only NAME,...] [--out FILE]"""
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
    "4096x2048": (4096, 2048, "444", 10, True),
    "4096^2": (4096, 4096, "444", 10, True),
    "4096x4608": (4096, 4608, "444", 10, True),
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


def one(path, order, planes, its, reps):
    """order: None (the library as it is: the parent, or the policy) or a "GP" string"""
    with j.library(path) as lib:
        s = j.Solver(planes, WEIGHT, [PWEIGHT] * len(planes), its)
        try:
            if order is not None:
                s.debug_option(j.J2P_OPT_PHASE_ORDER, j.phase_order(int(order[0]), int(order[1])))
            took = s.phase_order() if hasattr(lib, "j2p_solver_phase_order") else None

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
            return {"us_per_iteration": round(dt / its * 1e6, 2), "k_gradient_us": round(g_ms * 1e3, 2), "k_project_us": round(p_ms * 1e3, 2),
                    "order": took, "digest": digest.hexdigest()}
        finally:
            s.close()
            lib.j2p_pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="library A (the parent commit's)")
    ap.add_argument("--b", default=j.LIB_PATH, help="library B (default: the tree's)")
    ap.add_argument("--orders", default="policy,00,10,01,11")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--its", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated plane names (default: all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    names = [n for n in PLANES if not a.only or n in a.only.split(",")]
    orders = a.orders.split(",")
    out = open(a.out, "a") if a.out else None
    for name in names:
        planes = make(name)
        runs = {k: [] for k in ["parent"] + orders}
        for pair in range(a.pairs):
            seq = ["parent"] + orders
            for o in seq[pair % len(seq):] + seq[:pair % len(seq)]:
                if o == "parent":
                    runs[o].append(one(a.a, None, planes, a.its, a.reps))
                else:
                    runs[o].append(one(a.b, None if o == "policy" else o, planes, a.its, a.reps))
        us = {k: [r["us_per_iteration"] for r in v] for k, v in runs.items()}
        digests = sorted({r["digest"] for v in runs.values() for r in v})
        parent_span = round(max(us["parent"]) - min(us["parent"]), 2)
        line = {"plane": name + f" Q{PLANES[name][3]} -i {a.its}", "pairs": a.pairs, "reps_per_run": a.reps,
                "us_per_iteration": us, "parent_span": parent_span,
                "median_minus_parent": {k: round(float(np.median(v) - np.median(us["parent"])), 2) for k, v in us.items() if k != "parent"},
                # the project's rule for a gain: every run faster than every parent run AND the median difference beyond the parent's own span
                "gain": {k: bool(max(v) < min(us["parent"]) and np.median(us["parent"]) - np.median(v) > parent_span) for k, v in us.items() if k != "parent"},
                "slower": {k: bool(min(v) > max(us["parent"]) and np.median(v) - np.median(us["parent"]) > parent_span) for k, v in us.items() if k != "parent"},
                "k_gradient_us": {k: [r["k_gradient_us"] for r in v] for k, v in runs.items()},
                "k_project_us": {k: [r["k_project_us"] for r in v] for k, v in runs.items()},
                "policy_order": runs["policy"][0]["order"] if "policy" in runs else None,
                "digests_equal": len(digests) == 1, "digest": digests[0]}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        del planes


if __name__ == "__main__":
    main()
