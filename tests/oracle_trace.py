"""The per-iteration comparison of a whole-canvas Solver with the CPU oracle: the gradient after phase_gradient() and the
iterate after phase_project() of EVERY iteration against the buffers oracle_set_trace fills, bitwise (so also the sign of
zero).  Shared by tests/test_screens_gpu.py and tools/trace_vs_oracle.py; no pytest here."""
import ctypes
from dataclasses import dataclass

import numpy as np

from oracle import bindings


def oracle_trace(planes, weight, pweights, iterations):
    """(trace, final planes): trace[it, c, 0] is the oracle's gradient of iteration it, trace[it, c, 1] its new iterate"""
    CW, CH = bindings.canvas_size(planes)
    trace = np.zeros((max(iterations, 1), len(planes), 2, CH, CW), dtype=np.float32)
    lib = bindings.oracle_lib()
    lib.oracle_set_trace.argtypes = [ctypes.c_void_p]
    lib.oracle_set_trace.restype = None
    lib.oracle_set_trace(trace.ctypes.data)
    try:
        want, _ = bindings.oracle_compute(planes, weight, pweights, iterations)
    finally:
        lib.oracle_set_trace(None)
    return trace[:iterations], want


@dataclass
class Difference:
    iteration: int
    what: str                # "gradient" or "iterate"
    channel: int
    count: int               # differing pixels of this plane
    x: int                   # the first of them in raster order
    y: int
    got: np.ndarray          # the GPU's plane
    want: np.ndarray         # the oracle's

    def __str__(self):
        g, w = self.got[self.y, self.x], self.want[self.y, self.x]
        return (f"iteration {self.iteration} {self.what} channel {self.channel}: {self.count} differ; first ({self.x},{self.y}) "
                f"gpu {g!r} {int(g.view(np.uint32)):#x} oracle {w!r} {int(w.view(np.uint32)):#x}")


def differing(got, want):
    """[(x, y)] of the pixels whose bits differ, raster order"""
    ys, xs = np.nonzero(np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32))
    return list(zip(xs.tolist(), ys.tolist()))


def first_difference(planes, weight, pweights, iterations, trace, device=0):
    """drive a whole-canvas Solver phase by phase; the first plane that differs from the trace as a Difference, or None"""
    import jpeg2png_amd as j
    with j.Solver(planes, weight, pweights, iterations, device=device) as s:
        for it in range(iterations):
            s.phase_gradient()
            for idx, what in enumerate(("gradient", "iterate")):
                if what == "iterate":
                    s.phase_project()
                for c in range(len(planes)):
                    got = s.download_gradient(c) if what == "gradient" else s.download(c)
                    bad = differing(got, trace[it, c, idx])
                    if bad:
                        return Difference(it, what, c, len(bad), bad[0][0], bad[0][1], got, trace[it, c, idx])
    return None
