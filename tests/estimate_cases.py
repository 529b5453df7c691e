"""Estimated tables (include/jpeg2png_amd.h, "Estimated tables"): the histogram and the rule restated with numpy, and the corpus the
CPU and GPU tests share.

histogram(samples): every complete 8x8 block without a sample of 0 or 255, v = float32(s) - 128, dct8x8s (the oracle's, through
tests/samples_cases.py's way: oracle.bindings.dct_blocks), m = |rint|, counted per natural-order frequency.
estimate(hist, chroma): the rule, integers only, with the distance table d(m, q) written out once.

The corpus: PIL-written JPEGs of one synthetic image (smooth waves, noise, an edge, a patch clipped to 255 and a band clipped to 0)
at 512x384 and 200x120, qualities 50..98, 4:4:4 and 4:2:0.  The samples are what a decoder hands over: PIL's draft("YCbCr") decode
— all three channels of a 4:4:4 file, the luma of a 4:2:0 file (PIL upsamples its chroma) — and, for the chroma of the small
4:2:0 files at the file's own sampling, the decode restatement of tests/decode_cases.py, the oracle's decode and rounding to bytes."""
import functools
import io

import numpy as np

import samples_cases as sc

BINS = 1024
SIZES = ((512, 384), (200, 120))
QUALITIES = (50, 75, 85, 90, 95, 98)
SUBSAMPLINGS = ("444", "420")
CORPUS = [(w, h, q, s) for (w, h) in SIZES for q in QUALITIES for s in SUBSAMPLINGS]


# ---- the histogram ----
def histogram(samples):
    """-> (hist uint32 [64, 1024], blocks counted, blocks excluded)"""
    from oracle import bindings
    s = np.asarray(samples, np.uint8)
    h, w = s.shape
    bh, bw = h // 8, w // 8
    hist = np.zeros((64, BINS), np.uint32)
    if bh == 0 or bw == 0:
        return hist, 0, 0
    blocks = s[:bh * 8, :bw * 8].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    keep = ~((blocks == 0) | (blocks == 255)).any(axis=1)
    counted = blocks[keep]
    if len(counted):
        # (equal blocks are transformed once: a flat plane is one block)
        uniq, times = np.unique(counted, axis=0, return_counts=True)
        d = bindings.dct_blocks(uniq.astype(np.float32) - np.float32(128))
        assert d.dtype == np.float32
        m = np.abs(np.rint(d).astype(np.int64))
        assert m.max() <= 1016
        for j in range(64):
            hist[j] = np.bincount(m[:, j], weights=times, minlength=BINS).astype(np.uint32)
    return hist, int(keep.sum()), int((~keep).sum())


# ---- the rule ----
QMIN, QMAX, SLACK_PERCENT, MIN_VALUES, SMALL_DIVISOR = 4, 255, 5, 12, 4


@functools.lru_cache(maxsize=None)
def _distance():
    """d[q, m]: the distance of m to the nearest multiple of q (row 0 unused)"""
    m = np.arange(BINS, dtype=np.int64)
    d = np.zeros((QMAX + 1, BINS), np.int64)
    for q in range(1, QMAX + 1):
        r = m % q
        d[q] = np.minimum(r, q - r)
    return d


def ijg_table(quality, chroma):
    from jpeg2png_amd.synth import quant_table
    return quant_table("chroma" if chroma else "luma", quality).astype(np.int64)


def step_of(h):
    """one frequency -> (step or 0, nz)"""
    d = _distance()
    h = np.asarray(h, np.int64)
    nz = int(h[2:].sum())

    def search(lo):
        part = h.copy()
        part[:lo] = 0
        allowed = SLACK_PERCENT * int(part.sum()) // 100
        for q in range(QMAX, QMIN - 1, -1):
            if int(part[d[q] > 1].sum()) <= allowed:
                return q
        return 0
    qmax = search(2)
    if not qmax:
        if search(4):
            return 0, nz
        s = 1
        for q in (3, 2):
            if int(h[2:][np.arange(2, BINS) % q != 0].sum()) <= nz // SMALL_DIVISOR:
                s = q
                break
        overlap = int(np.minimum(h[2:BINS - s], h[2 + s:]).sum())
        return (s if 2 * overlap >= nz else 0), nz
    best, best_cost = 0, None
    for q in range(qmax, max(QMIN - 1, qmax - 3), -1):
        cost = int((h[2:] * np.minimum(d[q, 2:], 2) ** 2).sum())
        if best_cost is None or cost < best_cost:
            best, best_cost = q, cost
    return best, nz


def estimate(hist, chroma=False):
    """-> (table uint16 [64], determined bool [64], quality)"""
    hist = np.asarray(hist)
    assert hist.shape == (64, BINS)
    steps, determined = np.zeros(64, np.int64), np.zeros(64, bool)
    for j in range(64):
        steps[j], nz = step_of(hist[j])
        determined[j] = steps[j] > 0 and nz >= MIN_VALUES
    quality = 100
    if determined.any():
        best = None
        for q in range(100, 0, -1):
            total = int(np.abs(ijg_table(q, chroma) - steps)[determined].sum())
            if best is None or total < best:
                best, quality = total, q
    fill = ijg_table(quality, chroma)
    table = np.zeros(64, np.int64)
    for j in range(64):
        if determined[j]:
            table[j] = steps[j]
        else:
            seen = np.nonzero(hist[j])[0]
            mmax = int(seen[-1]) if len(seen) else 0
            table[j] = max(int(fill[j]), 2 * (mmax - 1))
    return np.clip(table, 1, 255).astype(np.uint16), determined, quality


# ---- the corpus ----
@functools.lru_cache(maxsize=None)
def image(w, h):
    """RGB uint8 [h, w, 3]: smooth parts, noise, an edge, clipped patches"""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = 128 + 60 * np.sin(x / 37) + 40 * np.cos(y / 23) + 30 * np.sin((x + y) / 11)
    a = np.stack([a, 128 + 50 * np.sin(x / 50 + 1) + 20 * np.cos(y / 9), 128 + 60 * np.cos((x - y) / 31)], -1)
    a += rng.normal(0, 6, a.shape)
    a[h // 3:h // 2, w // 4:w // 2] += 70
    a[10:40, 10:min(200, w - 10)] = 255
    a[50:60, :] = 0
    return np.clip(a, 0, 255).astype(np.uint8)


def jpeg_bytes(rgb, quality, subsampling):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(f, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[subsampling])
    return f.getvalue()


def pil_ycc(data):
    """a file decoded by libjpeg without colour conversion -> uint8 [h, w, 3] (the chroma of a subsampled file upsampled)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    return np.asarray(im)


def own_sampling_planes(data):
    """every component at the file's own sampling: the decode restatement's coefficients, the oracle's decode, + 128, rounded and
    clipped to bytes (samples_cases.plane_samples), cut to the component's samples"""
    import decode_cases as dc
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    arrays, _ = dc.decode(data)
    head = j.jpeg_header(data)
    out = []
    for a, k in zip(arrays, head["components"]):
        p = Plane(k["w"], k["h"], k["w_samp"], k["h_samp"], np.ascontiguousarray(a).reshape(-1), k["quant_table"])
        out.append(sc.plane_samples(p)[:k["samples_h"], :k["samples_w"]])
    return out


class Channel:
    """one channel of one corpus file: its samples (read-only), the file's table, whether it is chroma"""
    def __init__(self, name, samples, table, chroma):
        self.name, self.samples, self.table, self.chroma = name, samples, np.asarray(table, np.uint16), chroma
        self.samples.setflags(write=False)

    @functools.cached_property
    def hist(self):
        out = histogram(self.samples)
        out[0].setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def corpus_file(w, h, quality, subsampling):
    """-> (the file's bytes, [Channel])"""
    import jpeg2png_amd as j
    data = jpeg_bytes(image(w, h), quality, subsampling)
    tables = [p.quant_table for p in j.jpeg_header(data)["planes"]]
    ycc = pil_ycc(data)
    name = f"{w}x{h}_q{quality}_{subsampling}"
    channels = [Channel(name + "_y", np.array(ycc[:, :, 0]), tables[0], False)]
    if subsampling == "444":
        channels += [Channel(name + "_" + n, np.array(ycc[:, :, c]), tables[c], True) for c, n in ((1, "cb"), (2, "cr"))]
    elif (w, h) == SIZES[-1]:
        own = own_sampling_planes(data)
        channels += [Channel(name + "_" + n + "_own", np.array(own[c]), tables[c], True) for c, n in ((1, "cb"), (2, "cr"))]
    return data, channels


def corpus_channels():
    return [ch for key in CORPUS for ch in corpus_file(*key)[1]]


def recompressed(quality_first=50, quality_second=95, size=SIZES[0]):
    """the double-compression case: a quality_first file decoded to RGB, saved again at quality_second, decoded to YCbCr
    -> (luma samples, the first file's luma table, the second file's)"""
    from PIL import Image
    import jpeg2png_amd as j
    first = jpeg_bytes(image(*size), quality_first, "444")
    rgb = np.asarray(Image.open(io.BytesIO(first)).convert("RGB"))
    second = jpeg_bytes(rgb, quality_second, "444")
    return (np.array(pil_ycc(second)[:, :, 0]), j.jpeg_header(first)["planes"][0].quant_table, j.jpeg_header(second)["planes"][0].quant_table)


# ---- directed histograms for the rule ----
def _hist(rows):
    """{frequency: {m: count}} -> hist"""
    h = np.zeros((64, BINS), np.uint32)
    for j, counts in rows.items():
        for m, n in counts.items():
            h[j, m] = n
    return h


def directed_histograms():
    """name -> hist.  Frequency 0 carries the case; the others stay empty unless said"""
    out = {"all_zero": _hist({})}
    out["single_value"] = _hist({0: {40: 1}})
    out["values_only_at_q"] = _hist({0: {0: 500, 10: 40}, 9: {0: 100, 37: 16}})
    out["q4"] = _hist({0: {0: 100, 4: 30, 8: 20, 12: 5, 3: 3, 5: 2}})
    # the small steps: only +-3 seen (4 explains them within 1 and the cost does not go below 4: one multiple alone is not enough to
    # name 3), exact multiples of 3, of 2, and neither
    out["only_3"] = _hist({0: {0: 100, 3: 20}})
    out["q3"] = _hist({0: {0: 100, 3: 30, 6: 20, 9: 10, 12: 5, 2: 2, 4: 3, 7: 2}})
    out["q2"] = _hist({0: {0: 100, 2: 30, 4: 20, 6: 10, 8: 5, 3: 3, 5: 2, 7: 2}})
    # clusters around the multiples of 17, four wide (a flat block's DC is rounded as one): no step within 1, and no small step either
    out["clusters"] = _hist({0: {0: 100, 13: 10, 17: 30, 21: 10, 30: 8, 34: 20, 38: 8}})
    # a step of 24 whose zeros' noise reaches 2 and 3: the values of 4 and more have a step, so none is named
    out["noisy_zeros"] = _hist({0: {0: 900, 1: 60, 2: 5, 3: 1, 24: 8, 48: 3}})
    out["q1"] = _hist({0: {0: 100, 2: 20, 3: 18, 4: 15, 5: 12, 6: 9, 7: 7}})
    out["q255"] = _hist({0: {0: 100, 255: 20, 510: 3, 254: 2, 765: 1}})
    # 204 values of 2 and more: 10 may lie off the multiples of 20; with 11 of 205 the step 20 fails and a smaller one has to
    # explain them
    base = {0: 300, 20: 100, 40: 60, 60: 30, 19: 2, 21: 2}
    out["outliers_at_allowance"] = _hist({0: {**base, 30: 10}})
    out["outliers_above_allowance"] = _hist({0: {**base, 30: 11}})
    # at the least number of values a determined entry needs, one below it, and the 15 and 16 of the rule this one started from
    out["nz_11"] = _hist({0: {0: 900, 1: 50, 16: 8, 32: 3}})
    out["nz_12"] = _hist({0: {0: 900, 1: 50, 16: 8, 32: 4}})
    out["nz_15"] = _hist({0: {0: 900, 1: 50, 16: 10, 32: 5}})
    out["nz_16"] = _hist({0: {0: 900, 1: 50, 16: 10, 32: 6}})
    # every frequency determined, as a quality-50 chroma table; and a row whose largest value lifts the fill
    t = ijg_table(50, True)
    out["quality_50_chroma"] = _hist({j: {0: 50, int(t[j]): 20, 2 * int(t[j]): 4} for j in range(64)})
    out["fill_lifted_by_mmax"] = _hist({0: {0: 50, 16: 20, 32: 4}, 63: {0: 70, 200: 4}})
    return out
