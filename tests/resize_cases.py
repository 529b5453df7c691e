"""Resized tensor output (j2p_planes_to_tensor_resized): the definition of include/jpeg2png_amd.h restated in numpy, and the
cases both test files go through.  No tests here.

`taps` are the integer taps of one axis; `resample` is the definition step by step in np.float32 — every product and every
sum an operation of its own, in the order the header gives — vectorised over the outputs by stepping through the tap index:
an output with fewer taps than its neighbour gets a padded tap of weight 0, whose product is +0.f (the values are finite
and never negative) and whose addition changes no bit, since a sum that starts at +0.f is never -0.f.  `integral` is the
same area integral in float64, for the error bound of the CPU tests."""
import numpy as np

# source columns a wavefront of k_to_tensor_resized stages at a time (kResizeChunk in j2p_output_kernels.hip.h): the wide case below
# is 1040 columns so that its rows span three chunks.  The tile rule (resize_tile in j2p_output.hip): 256 output columns per
# wavefront, halved down to 32 while there are fewer than 2048 wavefronts — the small cases run with tiles of 32, the wide ones
# at widths 64, 65 and 1039 with tails of one column — and 2, 4 or 8 output rows per wavefront while 4096 wavefronts remain
KERNEL_CHUNK = 512


def taps(box, out):
    """per output index X of an axis: (first source index, [weights]) — lo = X * box, hi = lo + box, sources lo // out ..
    (hi - 1) // out, weight min(hi, (i + 1) * out) - max(lo, i * out); an axis that is not resized: one tap of weight 1"""
    assert 1 <= out <= box
    if out == box:
        return [(X, [1]) for X in range(out)]
    res = []
    for X in range(out):
        lo, hi = X * box, (X + 1) * box
        i0, i1 = lo // out, (hi - 1) // out
        res.append((i0, [min(hi, (i + 1) * out) - max(lo, i * out) for i in range(i0, i1 + 1)]))
    return res


def tap_arrays(box, out):
    """the same as arrays [out, n] with n the largest tap count: source indices (padded ones repeat the last) and weights
    (padded ones 0)"""
    t = taps(box, out)
    n = max(len(ws) for _, ws in t)
    idx = np.zeros((out, n), np.int64)
    wts = np.zeros((out, n), np.int64)
    for X, (first, ws) in enumerate(t):
        for k in range(n):
            idx[X, k] = first + min(k, len(ws) - 1)
            wts[X, k] = ws[k] if k < len(ws) else 0
    return idx, wts


def resample(v, box, out_w, out_h):
    """the mean m (before the element is made of it) of one channel: v the clamped float32 image [h, w], box (x, y, w, h)"""
    f32 = np.float32
    bx, by, bw, bh = box
    sub = np.ascontiguousarray(v[by:by + bh, bx:bx + bw], f32)
    ix, wx = tap_arrays(bw, out_w)
    iy, wy = tap_arrays(bh, out_h)
    r = np.zeros((bh, out_w), f32)                          # r_j for every row of the box and every output column
    for t in range(ix.shape[1]):
        prod = (wx[:, t].astype(f32)[None, :] * sub[:, ix[:, t]]).astype(f32)
        r = (r + prod).astype(f32)
    acc = np.zeros((out_h, out_w), f32)
    for t in range(iy.shape[1]):
        prod = (wy[:, t].astype(f32)[:, None] * r[iy[:, t], :]).astype(f32)
        acc = (acc + prod).astype(f32)
    m = acc
    if out_w != bw:
        m = (m / f32(bw)).astype(f32)
    if out_h != bh:
        m = (m / f32(bh)).astype(f32)
    return np.minimum(m, f32(255)).astype(f32)


def integral(v, box, out_w, out_h):
    """the area integral in float64: exact integer weights, one division"""
    bx, by, bw, bh = box
    sub = v[by:by + bh, bx:bx + bw].astype(np.float64)
    ix, wx = tap_arrays(bw, out_w)
    iy, wy = tap_arrays(bh, out_h)
    r = np.zeros((bh, out_w))
    for t in range(ix.shape[1]):
        r += wx[:, t].astype(np.float64)[None, :] * sub[:, ix[:, t]]
    acc = np.zeros((out_h, out_w))
    for t in range(iy.shape[1]):
        acc += wy[:, t].astype(np.float64)[:, None] * r[iy[:, t], :]
    return np.minimum(acc / float(int(wx[0].sum()) * int(wy[0].sum())), 255.)


def bound(box, out_w, out_h):
    """|resample - integral| at most: one rounding per product and per addition of the two passes plus two divisions, each at
    most 2^-24 of a value that is at most 255 after normalisation; 1 % for the second-order terms"""
    n_x = tap_arrays(box[2], out_w)[0].shape[1]
    n_y = tap_arrays(box[3], out_h)[0].shape[1]
    return (n_x + n_y + 4) * 2.0 ** -24 * 255. * 1.01


# ---- the source, as tests/test_tensor_gpu.py restates it ----

def unclamped(planes, w, h):
    """the float32 values the clamp sees (png.c:37-45 after jpeg2png.c:156-159): one array per output channel"""
    yi = (planes[0][:h, :w].astype(np.float64) + 128.).astype(np.float32)
    if len(planes) == 1:
        return [yi]
    y, cb, cr = yi.astype(np.float64), planes[1][:h, :w].astype(np.float64), planes[2][:h, :w].astype(np.float64)
    return [(y + 1.402 * cr).astype(np.float32), (y - 0.34414 * cb - 0.71414 * cr).astype(np.float32), (y + 1.772 * cb).astype(np.float32)]


def clamped(planes, w, h):
    """the float32 values after the clamp (png.c:15-17), one array per output channel"""
    return [np.where(v.astype(np.float64) > 255., np.float32(255), np.where(v.astype(np.float64) < 0., np.float32(0), v)).astype(np.float32)
            for v in unclamped(planes, w, h)]


def bf16_bits(t):
    u = np.ascontiguousarray(t, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def elements(means, dtype, layout, scale=None, bias=None):
    """the tensor's bit patterns (uint8 / uint16 / uint32) from the per-channel means: TensorElement, restated"""
    out = []
    for k, m in enumerate(means):
        if dtype == "u8":
            out.append(m.astype(np.uint32).astype(np.uint8))
            continue
        t = (m * np.float32(1.0 if scale is None else scale[k])).astype(np.float32)
        t = (t + np.float32(0.0 if bias is None else bias[k])).astype(np.float32)
        out.append({"f32": lambda: t.view(np.uint32), "f16": lambda: t.astype(np.float16).view(np.uint16), "bf16": lambda: bf16_bits(t)}[dtype]())
    return np.stack(out, axis=0 if layout == "chw" else 2)


def expected(planes, w, h, box, out_w, out_h, dtype, layout, scale=None, bias=None):
    """the resized tensor's bit patterns from the downloaded planes of a w x h image"""
    return elements([resample(v, box, out_w, out_h) for v in clamped(planes, w, h)], dtype, layout, scale, bias)


# ---- the cases: image -> (width, height); then (image, box or None for the whole image, out_w, out_h) ----
IMAGES = {"clamping_444": (48, 40), "padded_420": (45, 37), "grey": (45, 37), "wide": (1040, 24), "large_grey": (2048, 1040)}
CASES = [
    ("padded_420", None, 7, 5),                 # no integer ratio on either axis
    ("clamping_444", None, 12, 10),             # integer ratios 4 x 4
    ("clamping_444", None, 7, 5),
    ("padded_420", None, 45, 5),                # x not resized
    ("padded_420", None, 7, 37),                # y not resized
    ("padded_420", (13, 9, 32, 28), 5, 4),      # touches the image's right and bottom edge, inside the 48 x 48 canvas
    ("padded_420", (13, 9, 32, 28), 32, 28),
    ("padded_420", None, 1, 1),
    ("padded_420", None, 44, 36),               # ratios just above 1
    ("grey", None, 7, 5),
    ("grey", (3, 1, 40, 30), 10, 30),
] + [("padded_420", (bx, 2, 40, 30), 40, 30) for bx in (1, 2, 3, 5)] + [   # pure crops from every column alignment
    ("wide", None, ow, 5) for ow in (1, 3, 64, 65, 1039)                    # rows of three chunks; tiles with tails of one
] + [("wide", (517, 3, 520, 20), 519, 20), ("wide", (2, 0, 1038, 24), 1038, 24)] + [
    # large enough (8 tiles of 256 columns x more than 1024 rows) for wavefronts that own two output rows each: rows that share
    # a source row with the next (ratio just above 1), and rows that do not (y not resized)
    ("large_grey", None, 2047, 1039), ("large_grey", None, 2047, 1040)]


def case_box(image, box):
    w, h = IMAGES[image]
    return (0, 0, w, h) if box is None else box
