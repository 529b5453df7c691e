"""Flat and uniformly coloured inputs: builders only (no GPU, no pytest), shared by test_degenerate_cpu.py and
test_degenerate_gpu.py.

The parity suite's planes are all `synth` texture, whose per-channel gradient norm ||g|| is of the order of sqrt(pixels).
Two regimes the kernels branch on are only reached by content like this:

  ||g|| == 0 for a whole channel   the `norm != 0` test of compute.c:212, restated on every projection path, and every
                                    norm reduction delivering an exact 0.0
  0 < ||g|| < 2^-20                den_ok(norm) switches phase B's short division off (j2p_kernels.hip.h)

Kinds, applied to the planes of synth.make_planes (coefficients rewritten, fdata decoded by the oracle):

  K0   every coefficient 0 in every channel
  K1   DC only, the DCT round trip of the decoded value exact, dc != 0: ||g|| = 0 in every iteration, plane not 0
  K2   DC only, the round trip off by an ulp: ||g|| = 0 in iteration 0, tiny from iteration 1 on
  K3a  live luma + K0 chroma (a grey photograph stored as a 3-component JPEG)
  K3b  live luma + K2 chroma of different signs (a tinted image)
  K3c  K0 luma + live chroma
  K4   a live image whose upper block rows are zeroed in all channels: tile rows and bands whose partials are all
       exactly 0 beside live ones
"""
import copy
import math

import numpy as np

from jpeg2png_amd import synth
from oracle import bindings

KINDS = ("K0", "K1", "K2", "K3a", "K3b", "K3c", "K4")
Y_ONLY_KINDS = ("K0", "K1", "K2", "K4")
DEN_OK_MIN = 2.0 ** -20                 # den_ok()'s lower bound, j2p_kernels.hip.h
DC_RANGE = 1023                         # baseline JPEG: |dc| <= 1023 before the level shift's 11 bits run out


def _one_block(plane, dc):
    """the decoded 8x8 block of a DC-only block with coefficient dc, and the DCT of that block (float32, the oracle's)"""
    one = synth.Plane(8, 8, 1, 1, np.zeros(64, np.int16), plane.quant_table)
    one.data[0] = dc
    pix = bindings.decode_plane(one)
    return pix, bindings.dct_blocks(pix.reshape(1, 64))[0]


def round_trip_is_exact(plane, dc):
    """dct(decode(dc)) == dc * q bitwise in all 64 positions: the projection then finds cos == d * q for ever"""
    _, coef = _one_block(plane, dc)
    want = np.zeros(64, np.float32)
    want[0] = np.float32(dc) * np.float32(plane.quant_table[0])
    return np.array_equal(coef.view(np.uint32), want.view(np.uint32))


def find_dc(plane, exact, sign=1):
    """the first dc of sign * (1 .. 1023) whose round trip through the plane's own table is exact / inexact — a
    deterministic search; raises when there is none"""
    for k in range(1, DC_RANGE + 1):
        if round_trip_is_exact(plane, sign * k) == exact:
            return sign * k
    raise LookupError(f"no dc in {sign} * 1..{DC_RANGE} with an {'exact' if exact else 'inexact'} round trip for this table")


def set_zero(plane):
    plane.data = np.zeros_like(np.asarray(plane.data, np.int16))


def set_dc(plane, dc):
    d = np.zeros_like(np.asarray(plane.data, np.int16))
    d[0::64] = dc
    plane.data = d


def upper_rows(planes):
    """K4: the canvas rows [0, n) that are zeroed — about half the canvas, a multiple of the band alignment (lcm of 16 and
    every channel's 8 * h_samp), so that a band can be cut to hold nothing else"""
    align = 16
    for p in planes:
        align = math.lcm(align, 8 * p.h_samp)
    H = max(p.h * p.h_samp for p in planes)
    n = (H // 2) // align * align
    if n == 0:
        raise ValueError(f"a canvas of {H} rows has no aligned upper half (alignment {align})")
    return n


def zero_upper_rows(planes):
    n = upper_rows(planes)
    for p in planes:
        d = np.array(p.data, np.int16).reshape(p.h // 8, p.w // 8, 64)
        d[: n // (8 * p.h_samp)] = 0
        p.data = d.reshape(-1)
    return n


def k4_cuts(planes, nband):
    """band boundaries for K4: the first band is exactly the zeroed rows, the rest is cut into near-equal aligned bands"""
    align = 16
    for p in planes:
        align = math.lcm(align, 8 * p.h_samp)
    H = max(p.h * p.h_samp for p in planes)
    n = upper_rows(planes)
    units = -(-(H - n) // align)
    if units < nband - 1:
        raise ValueError(f"{H - n} live rows do not make {nband - 1} bands of {align} rows")
    cuts = [0, n]
    for b in range(1, nband - 1):
        cuts.append(n + (units * b // (nband - 1)) * align)
    return cuts + [H]


def apply_kind(planes, kind):
    """rewrite the coefficients of `planes` (a synth.make_planes list, changed in place) to the kind and decode fdata
    with the oracle.  Returns the planes"""
    if kind not in KINDS:
        raise ValueError(kind)
    if len(planes) == 1 and kind not in Y_ONLY_KINDS:
        raise ValueError(f"{kind} needs three channels")
    if kind == "K0":
        for p in planes:
            set_zero(p)
    elif kind == "K1":
        for c, p in enumerate(planes):
            set_dc(p, find_dc(p, exact=True, sign=-1 if c == 2 else 1))
    elif kind == "K2":
        for c, p in enumerate(planes):
            set_dc(p, find_dc(p, exact=False, sign=-1 if c == 2 else 1))
    elif kind == "K3a":
        for p in planes[1:]:
            set_zero(p)
    elif kind == "K3b":
        for c, p in enumerate(planes[1:]):
            set_dc(p, find_dc(p, exact=False, sign=1 if c == 0 else -1))
    elif kind == "K3c":
        set_zero(planes[0])
    elif kind == "K4":
        zero_upper_rows(planes)
    for p in planes:
        p.fdata = bindings.decode_plane(p)
    return planes


def make(kind, W, H, sub="444", quality=10, seed=1, y_only=False, zoom=1):
    """the planes of a W x H image of the kind, fdata decoded; zoom: every sampling factor times zoom (jpeg2png_amd.zoomed)"""
    planes = apply_kind(synth.make_planes(W, H, sub, quality, seed=seed, y_only=y_only), kind)
    if zoom != 1:
        planes = [copy.copy(p) for p in planes]
        for p in planes:
            p.w_samp, p.h_samp = p.w_samp * zoom, p.h_samp * zoom
    return planes


def uniform_channels(planes, kind):
    """the channels whose decoded plane is one value AND which cover the whole canvas (a plane smaller than the canvas
    leaves pixels that get no probability gradient: they stay behind when the rest moves, and the channel is no longer
    uniform — in the reference as well)"""
    W, H = bindings.canvas_size(planes)
    which = {"K0": range(len(planes)), "K1": range(len(planes)), "K2": range(len(planes)), "K3a": (1, 2), "K3b": (1, 2),
             "K3c": (0,), "K4": ()}[kind]
    return [c for c in which if planes[c].w * planes[c].w_samp == W and planes[c].h * planes[c].h_samp == H]


def upsampled(planes):
    """the canvas planes compute() starts from: replicate up-sampling with edge clamp (compute.c:295-303)"""
    W, H = bindings.canvas_size(planes)
    out = []
    for p in planes:
        cy = np.minimum(np.arange(H) // p.h_samp, p.h - 1)
        cx = np.minimum(np.arange(W) // p.w_samp, p.w - 1)
        out.append(np.ascontiguousarray(p.fdata[np.ix_(cy, cx)], np.float32))
    return out


def one_value(a):
    """the float32 array holds one bit pattern"""
    return len(np.unique(np.ascontiguousarray(a, np.float32).view(np.uint32))) == 1


def minus_zeros(a):
    """how many elements are -0.0"""
    a = np.asarray(a)
    return int(((a == 0) & np.signbit(a)).sum())


def clean(a):
    """no -0.0 and no NaN"""
    return not np.isnan(np.asarray(a)).any() and minus_zeros(a) == 0


def restated_norm(plane, pweight):
    """float64 norm over the channel's footprint in the canvas of p_alpha * idct((dct(decode) - d * q) / q^2) (compute.c:41-51,
    245), the plane's own samples each counted w_samp * h_samp times (compute.c:53-66).  For a uniform plane that is the
    whole gradient — TV and TGV contribute nothing — and so what den_ok() sees from iteration 1 on.  The transforms are
    the oracle's float32 ones (the residual IS their rounding), the quotient and the product float32 as in the solver"""
    bh, bw = plane.h // 8, plane.w // 8
    pix = np.asarray(plane.fdata, np.float32).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    q = np.asarray(plane.quant_table, np.uint16).astype(np.float32)
    d = np.asarray(plane.data, np.int16).reshape(-1, 64).astype(np.float32)
    # every distinct (block pixels, coefficients) pair once: uniform planes have one
    key = np.concatenate([pix.view(np.uint32), d.view(np.uint32)], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    upix, ud = uniq[:, :64].copy().view(np.float32), uniq[:, 64:].copy().view(np.float32)
    cos = bindings.dct_blocks(upix)
    e = ((cos - ud * q).astype(np.float32) / (q * q).astype(np.float32)).astype(np.float32)
    p_alpha = np.float32(np.float32(pweight) * np.float32(2) * np.float32(255) * np.sqrt(np.float32(2)))
    g = (p_alpha * bindings.dct_blocks(e, inverse=True)).astype(np.float32)
    per_block = (g.astype(np.float64) ** 2).sum(axis=1)
    total = per_block[np.asarray(inverse).reshape(-1)].sum()
    return float(np.sqrt(total * plane.w_samp * plane.h_samp))


# ---- the cases both test modules run: the smallest shapes that still reach each projection / reduction path ----
WEIGHT, PWEIGHT, ITERATIONS = 0.3, 0.001, 6
SHAPES = {
    # 1x1 register strips plus the ragged direct / generic remainder
    "y_200x136": dict(W=200, H=136, sub="444", y_only=True),
    # 2x2 SubTile strips, padded chroma, luma pixels the luma plane does not cover (canvas 160x80, luma 160x72)
    "420_154x69": dict(W=154, H=69, sub="420"),
    # 2x1 and 1x2 (the chroma planes pad beyond the luma plane here as well)
    "422_152x72": dict(W=152, H=72, sub="422"),
    "440_152x72": dict(W=152, H=72, sub="440"),
    # wide footprints: 3x3 luma, 6x6 chroma
    "420_157x101_x3": dict(W=157, H=101, sub="420", zoom=3),
    # 1032 tile rows of 4 rows: tickets, then a k_norm_finish launch
    "y_64x4128": dict(W=64, H=4128, sub="444", y_only=True),
}
SHAPE_KINDS = {name: (("K0", "K4") if name == "y_64x4128" else Y_ONLY_KINDS if kw.get("y_only") else KINDS)
               for name, kw in SHAPES.items()}
CASES = [(shape, kind) for shape in SHAPES for kind in SHAPE_KINDS[shape]]
_cache = {}


def case(shape, kind):
    """(planes, expectation) of one case, built once per process and to be left unchanged.  The expectation holds the
    oracle's canvas planes after 1, 2 and ITERATIONS iterations ("o1", "o2", "want"), its log rows ("rows"), the
    up-sampled input ("input") and, where the compiled reference is there, its planes and CSV rows ("ref", "ref_rows")"""
    key = (shape, kind)
    if key not in _cache:
        planes = make(kind, seed=7, **SHAPES[shape])
        pw = [PWEIGHT] * len(planes)
        e = {"input": upsampled(planes)}
        e["o1"], _ = bindings.oracle_compute(planes, WEIGHT, pw, 1)
        e["o2"], _ = bindings.oracle_compute(planes, WEIGHT, pw, 2)
        e["want"], e["rows"] = bindings.oracle_compute(planes, WEIGHT, pw, ITERATIONS, log=True)
        e["ref"] = e["ref_rows"] = None
        if bindings.have_ref():
            e["ref"], e["ref_rows"], _ = bindings.ref_compute(planes, WEIGHT, pw, ITERATIONS, log=True)
        _cache[key] = (planes, e)
    return _cache[key]
