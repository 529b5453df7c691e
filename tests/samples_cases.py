"""Sample input (j2p_solver_create_from_samples): the cases the CPU and GPU tests share, and the header's definition restated
with numpy and the CPU oracle's dct8x8s.

The definition: sample (X, Y) of a coefficient plane is the given sample at (min(X, w - 1), min(Y, h - 1)); v = (float32)s - 128;
every 8x8 block of v through dct8x8s (oracle.bindings.dct_blocks); each coefficient divided by (float32)step in float32; np.rint
(ties to even); int16, block-major [h / 8][w / 8][64].

The cases: the seven solver fixtures of tests/golden/ and four synthetic images, each turned into the 8-bit planes a decoder would
hand over — the oracle's decode of the coefficients + 128, rounded and clipped to uint8.  All steps are 5 or more and no sample
clips, so the restatement recovers the cases' own coefficients exactly (tests/test_samples_cpu.py shows it), which is what lets the
GPU tests compare with the fixtures' `data`."""
import functools
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")) if not f.endswith("dct_blocks.npz"))
SYNTH = {  # name: (W, H, subsampling, quality, seed)
    "synth_420_72x40_q30": (72, 40, "420", 30, 3),
    "synth_444_40x24_q75": (40, 24, "444", 75, 5),
    "synth_422_136x24_q20": (136, 24, "422", 20, 9),
    "synth_440_24x72_q50": (24, 72, "440", 50, 11),
}
NAMES = FIXTURES + sorted(SYNTH)
# the fixtures whose solves the GPU tests repeat: joint, subsampled, padded, TGV
SOLVED = ("rgb420_padded_40x20", "rgb422_48x32", "rgb444_48x32_q50", "y_48x40_tgv")


class Case:
    def __init__(self, name, planes, weight, pweight, iterations):
        self.name, self.planes, self.weight, self.pweight, self.iterations = name, planes, weight, pweight, iterations

    def bare_planes(self):
        """the planes as from_samples takes them: geometry and table, no arrays"""
        from jpeg2png_amd.synth import Plane
        return [Plane(p.w, p.h, p.w_samp, p.h_samp, None, p.quant_table) for p in self.planes]

    def coefficient_planes(self):
        """the planes as Solver takes them when the library is to decode them itself"""
        from jpeg2png_amd.synth import Plane
        return [Plane(p.w, p.h, p.w_samp, p.h_samp, p.data, p.quant_table) for p in self.planes]

    @functools.cached_property
    def samples(self):
        """per plane the uint8 [h, w] samples a decoder would deliver (read-only: shared between tests)"""
        out = [plane_samples(p) for p in self.planes]
        for a in out:
            a.setflags(write=False)
        return out


def plane_samples(p):
    """a plane's coefficients as decoded 8-bit samples: oracle decode + 128, rounded, clipped to uint8"""
    from oracle import bindings
    return np.clip(np.rint(bindings.decode_plane(p) + np.float32(128)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    from jpeg2png_amd import synth
    from jpeg2png_amd.synth import Plane
    if name in SYNTH:
        W, H, sub, q, seed = SYNTH[name]
        return Case(name, synth.make_planes(W, H, sub, q, seed=seed), 0.3, [0.001] * 3, 6)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    planes, c = [], 0
    while f"geom{c}" in z:
        w, h, ws, hs = (int(v) for v in z[f"geom{c}"])
        planes.append(Plane(w, h, ws, hs, z[f"data{c}"], z[f"quant{c}"]))
        c += 1
    return Case(name, planes, float(z["weight"]), [float(v) for v in z["pweight"]], int(z["iterations"]))


def replicate(samples, plane_w, plane_h):
    """the samples present, padded to the coefficient plane's size with their last column and row"""
    h, w = samples.shape
    assert 0 < h <= plane_h and 0 < w <= plane_w
    return np.pad(samples, ((0, plane_h - h), (0, plane_w - w)), mode="edge")


def expected_coefficients(samples, plane_w, plane_h, quant_table):
    """the header's definition on the CPU -> int16 [plane_h / 8, plane_w / 8, 64]"""
    from oracle import bindings
    v = replicate(np.asarray(samples, np.uint8), plane_w, plane_h).astype(np.float32) - np.float32(128)
    bh, bw = plane_h // 8, plane_w // 8
    blocks = v.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    d = bindings.dct_blocks(blocks)
    assert d.dtype == np.float32
    t = d / np.asarray(quant_table, np.uint16).astype(np.float32)[None, :]
    assert t.dtype == np.float32
    r = np.rint(t)
    assert r.min() >= -1024 and r.max() <= 1016
    return r.astype(np.int16).reshape(bh, bw, 64)


def clipped(samples):
    s = np.asarray(samples)
    return int(((s == 0) | (s == 255)).sum())
