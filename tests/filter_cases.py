"""Filtered tensor output (j2p_planes_to_tensor_resampled): the definition of include/jpeg2png_amd.h restated, and the cases both
test files go through.  No tests here.

`taps` are the taps of one axis in Python floats — IEEE doubles, every operation rounded on its own, which is what the header
asks for — with the weights narrowed to np.float32 at the end.  `resample` is the definition step by step in np.float32, every
product and every sum an operation of its own in the header's order, vectorised over the outputs by stepping through the tap
index: an output with fewer taps than its neighbour gets padded taps of weight +0.f AFTER its own, whose products are zeros and
whose additions change no bit (a sum that starts at +0.f is never -0.f, and x + (+-0) is x).  `evaluate64` is the same
definition with double weights and double sums, for the error bound of the CPU tests."""
import numpy as np

from resize_cases import clamped, elements, unclamped          # the source and the elements: restated there  # noqa: F401

TRIANGLE, CUBIC = 1, 2                                          # J2P_FILTER_*
FILTERS = {"triangle": TRIANGLE, "cubic": CUBIC}
KERNEL_CHUNK = 512                                              # kResizeChunk: source columns a wavefront stages at a time


def weight(filter, a):
    """w(a), a = |u|"""
    if filter == TRIANGLE:
        return 1. - a if a < 1. else 0.
    if a < 1.:
        return ((1.5 * a - 2.5) * a) * a + 1.
    if a < 2.:
        return (((a - 5.) * a + 8.) * a - 4.) * -0.5
    return 0.


def taps64(filter, box, out):
    """per output index X of an axis: (first source index, [w_i / S as doubles])"""
    assert box >= 1 and out >= 1
    if out == box:
        return [(X, [1.]) for X in range(out)]
    R = 2. if filter == CUBIC else 1.
    scale = float(box) / float(out)
    fs = scale if scale > 1. else 1.
    sup = R * fs
    res = []
    for X in range(out):
        c = (float(X) + 0.5) * scale
        first = max(0, int(c - sup + 0.5))                      # int() truncates
        end = min(box, int(c + sup + 0.5))
        assert first < end
        ws = [weight(filter, abs(((float(i) - c) + 0.5) / fs)) for i in range(first, end)]
        S = 0.
        for w in ws:
            S = S + w
        assert S > 0.5, (filter, box, out, X, S)
        res.append((first, [w / S for w in ws]))
    return res


def taps(filter, box, out):
    """the same with the weights as the definition has them: f_i = (float)(w_i / S)"""
    return [(first, [np.float32(f) for f in fs]) for first, fs in taps64(filter, box, out)]


def tap_arrays(t, dtype):
    """taps as arrays [out, n] with n the largest tap count: source indices (padded ones repeat the last) and weights (padded
    ones +0)"""
    n = max(len(ws) for _, ws in t)
    idx = np.zeros((len(t), n), np.int64)
    wts = np.zeros((len(t), n), dtype)
    for X, (first, ws) in enumerate(t):
        idx[X, :len(ws)] = np.arange(first, first + len(ws))
        idx[X, len(ws):] = first + len(ws) - 1
        wts[X, :len(ws)] = ws
    return idx, wts


def accumulate(v, box, out_w, out_h, filter):
    """acc of the definition, BEFORE the clamp, of one channel: v the clamped float32 image [h, w], box (x, y, w, h)"""
    f32 = np.float32
    bx, by, bw, bh = box
    sub = np.ascontiguousarray(v[by:by + bh, bx:bx + bw], f32)
    ix, wx = tap_arrays(taps(filter, bw, out_w), f32)
    iy, wy = tap_arrays(taps(filter, bh, out_h), f32)
    r = np.zeros((bh, out_w), f32)                              # r_j for every row of the box and every output column
    for t in range(ix.shape[1]):
        prod = (wx[:, t][None, :] * sub[:, ix[:, t]]).astype(f32)
        r = (r + prod).astype(f32)
    acc = np.zeros((out_h, out_w), f32)
    for t in range(iy.shape[1]):
        prod = (wy[:, t][:, None] * r[iy[:, t], :]).astype(f32)
        acc = (acc + prod).astype(f32)
    return acc


def resample(v, box, out_w, out_h, filter):
    """m = min(max(acc, 0.f), 255.f)"""
    return np.minimum(np.maximum(accumulate(v, box, out_w, out_h, filter), np.float32(0)), np.float32(255)).astype(np.float32)


def evaluate64(v, box, out_w, out_h, filter):
    """the same definition with double weights, products and sums"""
    bx, by, bw, bh = box
    sub = v[by:by + bh, bx:bx + bw].astype(np.float64)
    ix, wx = tap_arrays(taps64(filter, bw, out_w), np.float64)
    iy, wy = tap_arrays(taps64(filter, bh, out_h), np.float64)
    r = np.zeros((bh, out_w))
    for t in range(ix.shape[1]):
        r += wx[:, t][None, :] * sub[:, ix[:, t]]
    acc = np.zeros((out_h, out_w))
    for t in range(iy.shape[1]):
        acc += wy[:, t][:, None] * r[iy[:, t], :]
    return np.minimum(np.maximum(acc, 0.), 255.)


def bound(box, out_w, out_h, filter):
    """|resample - evaluate64| at most.  With u = 2^-24 and values of at most 255: a weight's narrowing to f32 costs u of it;
    a tap's product one rounding, and its term then passes through at most n - 1 additions, each a rounding of a partial sum
    that is at most 255 * L (L the largest sum of |f_i| of the axis) — so r_j is off by at most (n_x + 1) * u * 255 * L_x, which
    the second pass scales by at most L_y and to which it adds its own (n_y + 1) * u * (255 * L_x) * L_y.  Two more units and
    1 % cover the second-order terms and the double evaluation's own rounding; the clamp moves two values no further apart."""
    def axis(b, o):
        t = taps(filter, b, o)
        return max(len(ws) for _, ws in t), max(float(np.sum(np.abs(np.array(ws, np.float64)))) for _, ws in t)
    (n_x, l_x), (n_y, l_y) = axis(box[2], out_w), axis(box[3], out_h)
    return (n_x + n_y + 4) * 2.0 ** -24 * 255. * l_x * l_y * 1.01


def expected(planes, w, h, box, out_w, out_h, filter, dtype, layout, scale=None, bias=None):
    """the resampled tensor's bit patterns from the downloaded planes of a w x h image"""
    return elements([resample(v, box, out_w, out_h, filter) for v in clamped(planes, w, h)], dtype, layout, scale, bias)


def step_plane(w=48, h=40, at=24):
    """0 left of column `at`, 255 from it on: what makes a cubic overshoot at both ends"""
    v = np.zeros((h, w), np.float32)
    v[:, at:] = 255.
    return v


# ---- the cases: image -> (width, height); then (image, box or None for the whole image, out_w, out_h), each under both filters ----
IMAGES = {"clamping_444": (48, 40), "padded_420": (45, 37), "grey": (45, 37), "wide": (1040, 24), "large_grey": (2048, 1040), "step": (48, 40)}
SMALL_CASES = [
    ("padded_420", None, 7, 5),                 # shrinking, no integer ratio on either axis
    ("clamping_444", None, 24, 20),             # integer ratio 2 x 2
    ("clamping_444", None, 12, 10),             # integer ratio 4 x 4
    ("padded_420", None, 45, 5),                # x not resized
    ("padded_420", None, 7, 37),                # y not resized
    ("padded_420", None, 45, 37),               # neither
    ("padded_420", None, 20, 50),               # shrinks x, enlarges y
    ("padded_420", None, 61, 11),               # enlarges x, shrinks y
    ("padded_420", (5, 3, 16, 16), 37, 41),     # enlarging, no integer ratio
    ("padded_420", (7, 9, 5, 3), 64, 40),
    ("padded_420", (10, 10, 1, 1), 5, 3),       # a box of one pixel
    ("padded_420", None, 1, 1),
    ("padded_420", None, 44, 36),               # ratios just above 1
    ("padded_420", None, 46, 38),               # ... and just below
    ("padded_420", (13, 9, 32, 28), 5, 4),      # touches the image's right and bottom edge, inside the 48 x 48 canvas: the
    ("padded_420", (13, 9, 32, 28), 40, 33),    # windows are clipped there and the padding is never read
    ("grey", None, 7, 5),
    ("grey", (3, 1, 40, 30), 10, 30),
    ("grey", (3, 1, 40, 30), 70, 33),
    ("step", None, 19, 40),                     # the clamp at both ends (cubic), above 255 from rounding alone (triangle, 77)
    ("step", None, 77, 40),
    ("padded_420", None, 33, 5),                # tiles of 32 columns: one column in the last
    ("padded_420", None, 65, 37),
] + [("padded_420", (bx, 2, 40, 30), 17, 13) for bx in (1, 2, 3, 5)] + [   # every column alignment of the 16-byte loads
    ("padded_420", (bx, 2, 40, 30), 40, 30) for bx in (1, 2, 3, 5)]
WIDE_CASES = [("wide", None, ow, 5) for ow in (1, 3, 64, 65, 1039, 1041)] + [   # rows of two chunks and a tail
    ("wide", (517, 3, 520, 20), 519, 31), ("wide", (2, 0, 1038, 24), 2000, 3)]
# The tile rule (filter_tile in j2p_output.hip): 256 columns x 4 rows per wavefront; while that gives fewer than 2048 wavefronts
# the columns are halved down to 64, then the rows down to 1, and last the tile is 32 columns — which is how every small and
# wide case above runs.
LARGE_CASES = [
    ("large_grey", None, 2047, 1039),               # tiles of 256 columns, four output rows per wavefront that share source rows
    ("large_grey", (3, 5, 700, 500), 2047, 2100),   # ... enlarging: the source segment is shorter than the tile
    ("large_grey", None, 2049, 1040),               # y not resized; one column in the last tile of 256
    ("large_grey", None, 1024, 768),                # tiles of 64 columns x 4 rows
    ("large_grey", (0, 0, 640, 480), 700, 520),     # tiles of 64 columns x 2 rows, the last of 60
    ("large_grey", None, 300, 3),                   # an output row of about 700 (triangle) or 1040 (cubic) source rows
]
CASES = SMALL_CASES + WIDE_CASES + LARGE_CASES
# (box, out) pairs of one axis beyond the cases', for the hook
AXIS_PAIRS = [(65500, 1), (65500, 65499), (1, 5), (5, 64), (7, 7)]


def case_box(image, box):
    w, h = IMAGES[image]
    return (0, 0, w, h) if box is None else box
