"""Operands aimed at the two fast-path screens of k_gradient's march: builders only (no GPU, no pytest), shared by
test_screen_cases_cpu.py and test_screens_gpu.py.  Everything is numpy float32, evaluated in the operation order of the
kernel and the oracle (compute.c:73-197), so that a radicand computed here IS the radicand a lane holds.

The march is bit-identical to the reference because two kinds of row take the plain IEEE path:

  the operand screen    a row that loaded a pixel that is neither 0 nor in 2^-20 <= |y| < 2^41
  the mantissa screen   a row trip in which a lane holds a radicand whose low 16 bits are >= 0xfffe (allones_candidate):
                        the twice-refined reciprocal of a norm with an all-ones mantissa is not RN(1 / n), and the
                        one-correction quotient is then wrong for the numerators 2^j (division_exhaustive pass 2:
                        radicands 0x407ffffe / 0x407fffff, times powers of 4, numerator 0x3f800000)

Random texture never meets the second (2 radicands per binade pair x 1 of 2^23 numerator mantissas), and the suite's
planes stay far inside or far outside the first.  Here:

  site planes       textured planes into which a few pixel values are implanted so that ONE pixel (the site, itself 0) has
                    an offending radicand AND a numerator that the short division gets wrong there; kinds:
                      tv1    1 channel, TV radicand            tgv1   1 channel, TGV2 radicand
                      tv3    3 channels, joint TV radicand     tgv3   3 channels, joint TGV2 radicand
                    at columns of both parities in edge, free and narrow strips, on the seam between two strips, on the
                    rows around a tile-row boundary, on row 1 and in the short last tile row; no two sites of a plane share
                    a row trip of one wavefront (one slow site would cover for a screen that missed the other)
  boundary planes   textured planes with patches of values at the edges of the accepted range, just inside and just outside
  table planes      a quantisation table with steps around 8192 (k_project's table path needs q * q <= 2^26)
"""
import copy
from dataclasses import dataclass, field

import numpy as np

from conftest import make_case
from oracle import bindings

F = np.float32
W, H = 400, 56                      # strips of columns 0-125, 126-249, 250-373, 374-399; tile rows of 16 rows, the last of 8
SCREEN_LO, SCREEN_HI = F(2.0 ** -20), F(2.0 ** 41)       # the operand screen: 0 or SCREEN_LO <= |y| < SCREEN_HI
MANTISSAS = (0x7ffffe, 0x7fffff)


def bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def f32(b):
    return np.array([b], np.uint32).view(F)[0]


def is_offending(radicand):
    """0x407ffffe or 0x407fffff times a power of 4: the radicands whose root has an all-ones mantissa"""
    b = bits(radicand)
    exp, man = (b >> 23) & 0xff, b & 0x7fffff
    return b >> 31 == 0 and 0 < exp < 255 and exp % 2 == 0 and man in MANTISSAS


def is_missed_numerator(v):
    """+-2^j: the numerators whose one-correction quotient is wrong at an offending radicand.  (2^j (1 + 2^-23) was
    believed to be another while the exhaustive kernel compared only the even numerator of each pair and counted it
    twice; compared properly its quotient is right, so a site must not rely on it)"""
    b = bits(v) & 0x7fffffff
    return 0 < (b >> 23) < 255 and (b & 0x7fffff) == 0


def passes_operand_screen(a):
    a = np.abs(np.asarray(a, F))
    return (a == 0) | ((a >= SCREEN_LO) & (a < SCREEN_HI))


def canvases(planes):
    """the canvas planes iteration 0 differentiates: replicate up-sampling with edge clamp (compute.c:295-303); the FISTA
    factor of iteration 0 is 0, so the point IS the input"""
    CW, CH = bindings.canvas_size(planes)
    out = []
    for p in planes:
        cy = np.minimum(np.arange(CH) // p.h_samp, p.h - 1)
        cx = np.minimum(np.arange(CW) // p.w_samp, p.w - 1)
        out.append(np.ascontiguousarray(np.asarray(p.fdata, F)[np.ix_(cy, cx)]))
    return out


def tv_scale(nch):
    return F(1.0 / float(np.sqrt(F(nch))))                      # compute.c:90, the division in double


def tgv_scale(nch, weight):
    alpha = F(weight) / np.sqrt(F(2))                           # compute.c:258
    return F(float(alpha) * 1.0 / float(np.sqrt(F(nch))))       # compute.c:154


# ---- one pixel, scalar float32 ----
def _dx(f, x, y):
    return F(0) if x >= f.shape[1] - 1 else f[y, x + 1] - f[y, x]


def _dy(f, x, y):
    return F(0) if y >= f.shape[0] - 1 else f[y + 1, x] - f[y, x]


def _hessian(f, x, y):
    gx, gy = _dx(f, x, y), _dy(f, x, y)
    xx = F(0) if x == 0 else gx - _dx(f, x - 1, y)
    gyx = F(0) if x == 0 else gy - _dy(f, x - 1, y)
    gxy = F(0) if y == 0 else gx - _dx(f, x, y - 1)
    yy = F(0) if y == 0 else gy - _dy(f, x, y - 1)
    return xx, F(gxy + gyx) * F(0.5), yy                        # ((g_xy + g_yx) / 2., exact halving)


@dataclass
class Operands:
    tv: np.float32                   # TV radicand ((gx0^2 + gy0^2) + gx1^2) + ..., compute.c:84-89
    tgv: np.float32                  # TGV2 radicand, sum over the channels of (xx^2 + 2 sy^2) + yy^2, compute.c:148-152
    tv_numerators: list              # per channel (a gx, a gy, a -(gx + gy)), a = 1 / sqrtf(nchannel)
    tgv_numerators: list             # per channel (sy + xx, yy + sy, sy, (xx + sy) + yy)


def site_operands(planes, x, y):
    """the two radicands and the seven numerators per channel of canvas pixel (x, y) at iteration 0"""
    a = tv_scale(len(planes))
    tv, tgv = F(0), F(0)
    tv_num, tgv_num = [], []
    with np.errstate(over="ignore"):
        for f in canvases(planes):
            gx, gy = _dx(f, x, y), _dy(f, x, y)
            tv = F(tv + gx * gx)
            tv = F(tv + gy * gy)
            xx, sy, yy = _hessian(f, x, y)
            tgv = F(tgv + F(F(xx * xx + F(2) * F(sy * sy)) + yy * yy))
            tv_num.append((a * gx, a * gy, a * -F(gx + gy)))
            tgv_num.append((sy + xx, yy + sy, sy, F(xx + sy) + yy))
    return Operands(tv, tgv, tv_num, tgv_num)


# ---- the whole canvas, vectorised float32 ----
def _differences(f):
    gx, gy = np.zeros_like(f), np.zeros_like(f)
    gx[:, :-1] = f[:, 1:] - f[:, :-1]
    gy[:-1] = f[1:] - f[:-1]
    xx, gyx, gxy, yy = (np.zeros_like(f) for _ in range(4))
    xx[:, 1:] = gx[:, 1:] - gx[:, :-1]
    gyx[:, 1:] = gy[:, 1:] - gy[:, :-1]
    gxy[1:] = gx[1:] - gx[:-1]
    yy[1:] = gy[1:] - gy[:-1]
    return gx, gy, xx, (gxy + gyx) * F(0.5), yy


def radicand_planes(planes):
    """(TV radicand, TGV2 radicand) of every canvas pixel, as site_operands makes them"""
    r1 = r2 = None
    with np.errstate(over="ignore"):
        for f in canvases(planes):
            gx, gy, xx, sy, yy = _differences(f)
            r1 = gx * gx if r1 is None else r1 + gx * gx
            r1 = r1 + gy * gy
            t = (xx * xx + F(2) * (sy * sy)) + yy * yy
            r2 = t if r2 is None else r2 + t
    return r1, r2


def restated_gradient(planes, weight):
    """the objective gradient of iteration 0 per channel, TV and TGV2 terms gathered in the raster order of the reference's
    scatter (compute.c:91-123, :156-195; the prob term is +0 in iteration 0): an independent float32 restatement that
    tests compare with the oracle's trace.  Every quotient is IEEE (numpy's)"""
    chans = canvases(planes)
    n = len(chans)
    a1, a2 = tv_scale(n), tgv_scale(n, weight)
    r1, r2 = radicand_planes(planes)
    n1, n2 = np.sqrt(r1), np.sqrt(r2)

    def shifted(a, dx, dy):
        """b[y, x] = a[y + dy, x + dx], and whether that source pixel exists"""
        b, ok = np.zeros_like(a), np.zeros(a.shape, bool)
        ys = slice(max(0, -dy), a.shape[0] - max(0, dy))
        xs = slice(max(0, -dx), a.shape[1] - max(0, dx))
        yt = slice(max(0, -dy) + dy, a.shape[0] - max(0, dy) + dy)
        xt = slice(max(0, -dx) + dx, a.shape[1] - max(0, dx) + dx)
        b[ys, xs] = a[yt, xt]
        ok[ys, xs] = True
        return b, ok

    out = []
    with np.errstate(all="ignore"):
        for f in chans:
            gx, gy, xx, sy, yy = _differences(f)
            g = np.zeros_like(f)

            def add(g, scaled_quotient, norm, dx, dy):
                q, ok = shifted(scaled_quotient, dx, dy)
                nn, _ = shifted(norm, dx, dy)
                return np.where(ok & (nn != 0), g + q, g)
            g = add(g, (a1 * gy) / n1, n1, 0, -1)
            g = add(g, (a1 * gx) / n1, n1, -1, 0)
            g = add(g, (a1 * -(gx + gy)) / n1, n1, 0, 0)
            if weight != 0:
                down = a2 * ((yy + sy) / n2)
                diag = a2 * ((-sy) / n2)
                side = a2 * ((sy + xx) / n2)
                own = a2 * (-((F(2) * xx + F(2) * sy) + F(2) * yy) / n2)
                g = add(g, down, n2, 0, -1)
                g = add(g, diag, n2, 1, -1)
                g = add(g, side, n2, -1, 0)
                g = add(g, own, n2, 0, 0)
                g = add(g, side, n2, 1, 0)
                g = add(g, diag, n2, -1, 1)
                g = add(g, down, n2, 0, 1)
            out.append(g)
    return out


def candidate_rows(planes):
    """per canvas row: the columns whose TV or TGV2 radicand has low 16 bits >= 0xfffe (what allones_candidate flags)"""
    r1, r2 = radicand_planes(planes)
    hit = ((r1.view(np.uint32) & 0xffff) >= 0xfffe) | ((r2.view(np.uint32) & 0xffff) >= 0xfffe)
    return [np.nonzero(row)[0].tolist() for row in hit]


def screened_rows(planes):
    """per canvas row: every channel's pixels of rows r-1, r, r+1 pass the operand screen"""
    ok = np.logical_and.reduce([passes_operand_screen(f).all(axis=1) for f in canvases(planes)])
    pad = np.concatenate([[True], ok, [True]])
    return pad[:-2] & pad[1:-1] & pad[2:]


# ---- the operand values of the sites ----
TV1_PAIRS = ((0x3f800000, 0x3fddb3d6), (0x3f000000, 0x3ff7def5))         # (gx, gy): radicands 0x407ffffe, 0x407fffff
TV1_SCALES = (0, -6, 9)
TV3_GX0, TV3_GY0, TV3_GX1 = 0x3fddb3d8, 0x3e800000, (0x3f77deef, 0x3f77def1)   # a gx0 == 1.0f; radicands 0x407ffffe, 0x407fffff


def _tgv_radicand(u, v):
    sy = F(u + v) * F(0.5)
    return F(F(u * u + F(2) * F(sy * sy)) + v * v), (sy + u, v + sy, sy, F(u + sy) + v)


def find_tgv_pair(mantissa, reach=8, targets=(16.0, 64.0, 256.0, 1024.0, 4096.0)):
    """(u, v): with the site 0, its right neighbour u, its lower neighbour v and everything else in reach 0, the second
    differences are xx = u, yy = v, sy = (u + v) / 2 and the TGV2 radicand is (u^2 + 2 sy^2) + v^2.  u = 1 + t, v = 1 - t
    makes sy = 1 and the radicand 4 + 2 t^2, which is the power of four R at t = sqrt((R - 4) / 2).  For each R in turn all
    pairs within `reach` ulps of that real root are tried, nearest first, for a radicand just below R with the wanted
    mantissa and a numerator the short form misses (sy stays 1 only where u + v is exactly 2, so a step of t moves the
    radicand by more than an ulp and a given R may have no pair: hence several).  Deterministic; raises if there is none"""
    order = sorted(((du, dv) for du in range(-reach, reach + 1) for dv in range(-reach, reach + 1)),
                   key=lambda d: (max(abs(d[0]), abs(d[1])), d))
    for R in targets:
        t = np.sqrt((np.float64(R) - 4) / 2)
        u0, v0 = F(1 + t), F(1 - t)
        for du, dv in order:
            u, v = f32(bits(u0) + du), f32(bits(v0) + dv)
            rad, nums = _tgv_radicand(u, v)
            if is_offending(rad) and bits(rad) & 0x7fffff == mantissa and any(is_missed_numerator(n) for n in nums):
                return bits(u), bits(v)
    raise LookupError(f"no (u, v) within {reach} ulps of the roots for R in {targets} gives a TGV2 radicand ending in {mantissa:#x}")


_tgv_pairs = {}


def tgv_pair(mantissa):
    if mantissa not in _tgv_pairs:
        _tgv_pairs[mantissa] = find_tgv_pair(mantissa)
    return _tgv_pairs[mantissa]


# ---- site planes ----
@dataclass
class Site:
    kind: str                # tv1, tgv1, tv3, tgv3
    x: int
    y: int
    variant: int             # index into the kind's operand variants
    radicand: int = 0        # bits, filled in by the builder's own check
    numerator: int = 0       # bits of the missed numerator found

    @property
    def id(self):
        return f"{self.kind}-{self.x},{self.y}"

    def reached(self):
        """the canvas pixels the site's terms under the offending norm are added to (the reference's scatter)"""
        x, y = self.x, self.y
        if self.kind.startswith("tv"):
            return {(x, y), (x + 1, y), (x, y + 1)}
        return {(x, y), (x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1), (x - 1, y + 1), (x + 1, y - 1)}


@dataclass
class Case:
    name: str
    planes: list
    weight: float
    sites: list = field(default_factory=list)
    patches: list = field(default_factory=list)      # boundary planes: (x0, y0, w, h)
    iterations: int = 3
    _expect: dict = field(default_factory=dict, repr=False)

    @property
    def pweights(self):
        return [0.001] * len(self.planes)


VARIANTS = {"tv1": len(TV1_PAIRS) * len(TV1_SCALES), "tgv1": 2, "tv3": 2, "tgv3": 2}
# positions (x, y) of the sites of one plane; consecutive sites take consecutive operand variants
GROUPS = {
    # even and odd columns in an edge strip (rows 5, 9: first tile row, first strip), in a free strip (rows 21, 25: second
    # tile row, second strip), in the narrow last strip; row 1; the short last tile row
    "cols": ((40, 5), (180, 21), (41, 9), (181, 25), (390, 37), (391, 41), (201, 1), (300, 51)),
    # the seam between the first two strips: the source terms of these columns are computed by both
    "seam": ((124, 19), (125, 23), (126, 27), (127, 35)),
    # around the boundary of the first two tile rows (and the cut of a two-band run at row 16), one strip each
    "rows": ((60, 14), (200, 15), (330, 16)),
    # 4:2:0: odd columns and even rows, so that the step to the right crosses a chroma sample and the step down does not
    "luma420": ((181, 24), (41, 6), (125, 14), (391, 40)),
}
SITE_PLANES = ([(kind, "y" if kind.endswith("1") else "444", group) for kind in ("tv1", "tgv1", "tv3", "tgv3")
                for group in ("cols", "seam", "rows")] + [("tv3", "420", "luma420")])
SITES = [(kind, layout, group, i) for kind, layout, group in SITE_PLANES for i in range(len(GROUPS[group]))]


QUALITY = 90                        # at the suite's usual quality 10 four pixels in five lie in flat runs (radicand 0); here under 1 %


def _texture(layout, seed):
    return make_case(W, H, "420" if layout == "420" else "444", QUALITY, seed=seed, y_only=layout == "y")


def _put(plane, x, y, value):
    """canvas pixel (x, y) of the plane's channel: the sample under it"""
    plane.fdata[y // plane.h_samp, x // plane.w_samp] = value


def implant(planes, site):
    """write the site's operands into the planes (changed in place)"""
    x, y, k = site.x, site.y, site.variant
    if site.kind == "tv1":
        gx, gy = TV1_PAIRS[k % len(TV1_PAIRS)]
        s = F(2.0 ** TV1_SCALES[k // len(TV1_PAIRS)])
        for (px, py, v) in ((x, y, F(0)), (x + 1, y, f32(gx) * s), (x, y + 1, f32(gy) * s)):
            _put(planes[0], px, py, v)
    elif site.kind == "tv3":
        for (c, px, py, v) in ((0, x, y, F(0)), (0, x + 1, y, f32(TV3_GX0)), (0, x, y + 1, f32(TV3_GY0)),
                               (1, x, y, F(0)), (1, x + 1, y, f32(TV3_GX1[k])), (1, x, y + 1, F(0)),
                               (2, x, y, F(0)), (2, x + 1, y, F(0)), (2, x, y + 1, F(0))):
            _put(planes[c], px, py, v)
    else:
        u, v = tgv_pair(MANTISSAS[k])
        for c in range(len(planes)):
            for (dx, dy) in ((0, 0), (-1, 0), (0, -1), (-1, 1), (1, -1), (1, 0), (0, 1)):
                _put(planes[c], x + dx, y + dy, F(0))
        _put(planes[0], x + 1, y, f32(u))
        _put(planes[0], x, y + 1, f32(v))


def check_site(planes, site):
    """the builder's own assertion: radicand offending, a numerator under it missed by the short form, every implanted value
    inside the operand screen.  Raises LookupError otherwise; fills in site.radicand / site.numerator"""
    ops = site_operands(planes, site.x, site.y)
    if site.kind.startswith("tv"):
        rad, nums = ops.tv, [n for ch in ops.tv_numerators for n in ch]
    else:
        rad, nums = ops.tgv, [n for ch in ops.tgv_numerators for n in ch]
    missed = [n for n in nums if is_missed_numerator(n)]
    if not is_offending(rad) or not missed:
        raise LookupError(f"site {site.id}: radicand {bits(rad):#x}, numerators {[hex(bits(n)) for n in nums]}")
    for f in canvases(planes):
        patch = f[max(0, site.y - 1):site.y + 2, max(0, site.x - 1):site.x + 2]
        if not passes_operand_screen(patch).all():
            raise LookupError(f"site {site.id}: an implanted value fails the operand screen")
    site.radicand, site.numerator = bits(rad), bits(missed[0])


def build_site_plane(kind, layout, group, seed=300):
    """a textured plane set with the group's sites of the kind implanted.  The texture's seed is the first of seed, seed + 1,
    ... for which the rows of every site are ordinary rows of the screened path apart from the site: rows y-1 .. y+1 pass
    the operand screen and no other pixel of row y is a candidate of the mantissa screen (either would send the site's row
    trip down the IEEE path whatever the screen made of the site).  Raises if a site is not found or no seed does"""
    for s in range(seed, seed + 16):
        planes = _texture(layout, s)
        sites = [Site(kind, x, y, i % VARIANTS[kind]) for i, (x, y) in enumerate(GROUPS[group])]
        for site in sites:
            implant(planes, site)
        for site in sites:
            check_site(planes, site)
        cand, ok = candidate_rows(planes), screened_rows(planes)
        if all(ok[site.y] and cand[site.y] == [site.x] for site in sites):
            return Case(f"{kind}-{layout}-{group}", planes, 0.3, sites=sites)
    raise LookupError(f"{kind}-{layout}-{group}: no texture seed in {seed}..{seed + 15} leaves the sites' rows ordinary")


# ---- boundary planes ----
SMALL = [F(0)] + [F(s * m * 2.0 ** -20) for s in (1, -1) for m in (1.0, 1.0 + 2.0 ** -23, 1.5)]
LARGE = F(2.0 ** 41 - 2.0 ** 17)                     # the largest float below 2^41; its mantissa is all ones
LARGE_PLAIN = F(1.375 * 2.0 ** 40)                   # second differences of 5.5 * 2^40, radicands with short mantissas
OUTSIDE = [F(s) * v for s in (1, -1) for v in (f32(bits(SCREEN_LO) - 1), SCREEN_HI)]
# (x0, y0) of the 6 x 5 patches: edge strip, the seam, a free strip across the rows 14-18, a free strip, the narrow strip,
# the last tile row
PATCHES = ((38, 2), (122, 22), (183, 14), (300, 36), (384, 27), (210, 49))
PATCH_W, PATCH_H = 6, 5
STRIPS = ((0, 125), (126, 249), (250, 373), (374, 399))      # output columns of the wavefronts' strips at W = 400
# "large" is the value the range ends with.  Squares of an all-ones mantissa end in ...fffe, so every radicand of such a
# patch is a candidate of the mantissa screen and its rows take the IEEE path with 2^43-sized operands in them;
# "large_plain" and "mixed" hold large values whose radicands are no candidates and so stay on the screened path.
BOUNDARY_GROUPS = ("small", "large", "large_plain", "mixed", "outside")
BOUNDARY_CASES = [(group, layout, weight) for group in BOUNDARY_GROUPS for layout in ("y", "444") for weight in (0.3, 0.0)]


def _patch_values(group, rng, c):
    yy, xx = np.mgrid[0:PATCH_H, 0:PATCH_W]
    sign = np.where((xx + yy + c) % 2 == 0, F(1), F(-1)).astype(F)     # alternating in both directions
    small = np.array(SMALL, F)[rng.integers(0, len(SMALL), (PATCH_H, PATCH_W))]
    if group == "small":
        return small
    if group == "large":
        return sign * LARGE
    if group == "large_plain":
        return sign * LARGE_PLAIN
    if group == "mixed":
        return np.where((xx // 2 + yy) % 2 == 0, sign * LARGE_PLAIN, small).astype(F)
    return np.where((xx + 2 * yy) % 3 == 0, np.array(OUTSIDE, F)[rng.integers(0, len(OUTSIDE), (PATCH_H, PATCH_W))],
                    np.where((xx + yy) % 2 == 0, sign * LARGE_PLAIN, small)).astype(F)


def predicted_fast_rows(planes, x0, y0):
    """how many of the patch's rows are predicted to stay on the screened path in the strips that load the patch: rows
    r-1 .. r+1 pass the operand screen and no column of those strips (two halo columns included) holds a candidate of the
    mantissa screen in row r"""
    ok, cand = screened_rows(planes), candidate_rows(planes)
    spans = [(a - 2, b + 2) for a, b in STRIPS if x0 - 2 <= b and x0 + PATCH_W + len(planes) + 1 >= a]
    return sum(1 for r in range(y0, y0 + PATCH_H) if ok[r] and not any(a <= col <= b for col in cand[r] for a, b in spans))


def build_boundary_plane(group, layout, weight, seed=500):
    """a textured plane set with patches of the group's values in every channel (shifted by a column per channel).  The
    seed is the first of seed, seed + 1, ... whose texture passes the operand screen everywhere and for which the patches
    are on the path they are meant for: in small / large_plain / mixed every patch has a row that is predicted to stay
    on the screened path and at least half of all patch rows are; in large every patch row holds a candidate of the
    mantissa screen; in outside every patch row fails the operand screen.  Raises if no seed does"""
    for s in range(seed, seed + 16):
        planes = _texture(layout, s)
        if not all(passes_operand_screen(f).all() for f in canvases(planes)):
            continue
        rng = np.random.default_rng(s)
        for c, p in enumerate(planes):
            for (x0, y0) in PATCHES:
                p.fdata[y0:y0 + PATCH_H, x0 + c:x0 + c + PATCH_W] = _patch_values(group, rng, c)
        ok, cand = screened_rows(planes), candidate_rows(planes)
        fast = [predicted_fast_rows(planes, x0, y0) for (x0, y0) in PATCHES]
        rows = [r for (_, y0) in PATCHES for r in range(y0, y0 + PATCH_H)]
        if group == "outside":
            good = not any(ok[r] for r in rows)
        elif group == "large":
            good = all(ok[r] and cand[r] for r in rows)
        else:
            good = min(fast) >= 1 and 2 * sum(fast) >= len(rows)
        if good:
            return Case(f"{group}-{layout}-w{weight}", planes, weight, patches=[(x0, y0, PATCH_W, PATCH_H) for x0, y0 in PATCHES])
    raise LookupError(f"{group}-{layout}: no texture seed in {seed}..{seed + 15} puts the patch rows on the path they are meant for")


# ---- quantisation table ----
TABLES = {"8191_8192_8193": (8191, 8192, 8193),      # one step past 2^13: q * q > 2^26, the table path must switch off
          "8191_8192": (8191, 8192)}                 # q * q == 2^26 exactly: the table path at its last accepted step


def build_table_plane(name):
    """Y-only 72 x 40 whose quantisation table holds the steps at its first AC positions (where quality-10 texture has
    non-zero coefficients), decoded with that table; 6 iterations.  Every step is below 32768"""
    planes = make_case(72, 40, "444", 10, seed=611, y_only=True)
    q = np.array(planes[0].quant_table, np.uint16).copy()
    for pos, step in zip((1, 8, 2), TABLES[name]):
        q[pos] = step
    assert q.max() < 32768
    planes[0].quant_table = q
    planes[0].fdata = bindings.decode_plane(planes[0])
    return Case(f"table-{name}", planes, 0.3, iterations=6)


# ---- the cases, built once per process and left unchanged ----
_cache = {}


def site_case(kind, layout, group):
    key = ("site", kind, layout, group)
    if key not in _cache:
        _cache[key] = build_site_plane(kind, layout, group)
    return _cache[key]


def boundary_case(group, layout, weight):
    key = ("boundary", group, layout, weight)
    if key not in _cache:
        _cache[key] = build_boundary_plane(group, layout, weight)
    return _cache[key]


def table_case(name):
    key = ("table", name)
    if key not in _cache:
        _cache[key] = build_table_plane(name)
    return _cache[key]


def plain_case():
    """a plane without sites: the texture alone"""
    key = ("plain",)
    if key not in _cache:
        _cache[key] = Case("plain-y", _texture("y", 300), 0.3)
    return _cache[key]


# every case as a key for get_case, with its test id
ALL_CASES = ([("site",) + p for p in SITE_PLANES] + [("boundary",) + b for b in BOUNDARY_CASES]
             + [("table", name) for name in TABLES] + [("plain",)])
ALL_IDS = ([f"{kind}-{layout}-{group}" for kind, layout, group in SITE_PLANES]
           + [f"{group}-{layout}-w{weight}" for group, layout, weight in BOUNDARY_CASES]
           + [f"table-{name}" for name in TABLES] + ["plain"])


def get_case(key):
    return {"site": site_case, "boundary": boundary_case, "table": table_case, "plain": plain_case}[key[0]](*key[1:])


def expectation(case):
    """the oracle's truth for a case, computed once: "trace" [iteration, channel, 0 gradient / 1 iterate, H, W], the final
    planes "want" and the log rows "rows\""""
    if not case._expect:
        from oracle_trace import oracle_trace
        trace, want = oracle_trace(case.planes, case.weight, case.pweights, case.iterations)
        _, rows = bindings.oracle_compute(case.planes, case.weight, case.pweights, case.iterations, log=True)
        case._expect.update(trace=trace, want=want, rows=rows)
    return case._expect


def fresh(case):
    """a copy of the case's planes for a run that rewrites them (jpeg2png_amd.compute)"""
    return copy.deepcopy(case.planes)
