"""randomised sweep of zooming: cases of the shared stream (tests/sweep_cases.py) zoomed 2, 3 or 4 times
(jpeg2png_amd.zoomed), sizes scaled down so that the canvas stays near 0.5 Mpixel, with the wide-footprint path and the
one-launch projection of small canvases each switched on or off at random — every solve bit-identical to the
UNMODIFIED reference's compute() on the same planes (log rows too, where the case logs).
usage: python tools/sweep_zoom.py [ncases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg2png_amd as j  # noqa: E402
from oracle import bindings  # noqa: E402
from sweep_cases import cases  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng([seed, 0x200])
bad = 0
for cs in cases(seed, n):
    s = int(rng.integers(2, 5))
    shrink = max(1.0, (cs.W * cs.H * s * s / 5e5) ** 0.5)
    cs.W, cs.H = max(1, int(cs.W / shrink)), max(1, int(cs.H / shrink))
    cs.iterations = min(cs.iterations, 10)
    wide, mixed = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    planes = cs.planes()
    for p in planes:
        p.fdata = bindings.decode_plane(p)
    z = j.zoomed(planes, s)
    want, want_log, _ = bindings.ref_compute(z, cs.weight, cs.pweights, cs.iterations, log=cs.log)
    with j.Solver(z, cs.weight, cs.pweights, cs.iterations) as sv:
        sv.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, wide)
        sv.debug_option(j.J2P_OPT_MIXED_PROJECT, mixed)
        rows = sv.run(cs.iterations, log=cs.log)
        paths = "".join("w" if sv.wide_footprint(c) else "-" for c in range(len(z)))
        got = [sv.download(c) for c in range(len(z))]
    same = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
    if same and cs.log and cs.iterations:
        same = bool(np.allclose(rows[:, 1:], want_log[:, 1:], rtol=1e-9, atol=2e-6))
    bad += not same
    print(("ok   " if same else "DIFF ") + cs.describe() + f"  zoom {s} wide {wide} mixed {mixed} paths {paths}", flush=True)
print(f"{n - bad}/{n} zoomed cases bit-identical to the reference")
sys.exit(1 if bad else 0)
