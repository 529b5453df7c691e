"""The baseline JPEG file of include/jpeg2png_amd.h ("The JPEG file") restated in plain Python, and the cases the entropy
coder's tests share (tests/test_entropy_cpu.py checks the restatement against libjpeg, tests/test_entropy_gpu.py the device's
coder against the restatement).

encode(...) returns the file; encode_report(...) also how many FF bytes of the entropy-coded data were stuffed and how many
bits the last byte was short (the 1-bits added), which the case preconditions are about."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K.3: BITS and HUFFVAL of DC0, AC0, DC1, AC1
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = list(range(12))
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]
AC_VALS = [bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")]


def _codes(bits, vals):
    """{symbol: (code, length)}: in order of length, consecutive within a length, doubled from one length to the next"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[t], DC_VALS) for t in range(2)]
AC_CODES = [_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def grids(width, height, ncomp, sub):
    """[(blocks_h, blocks_w)] per component"""
    bw, bh = -(-width // 8), -(-height // 8)
    sx, sy = sub if ncomp == 3 else (1, 1)
    return [(bh, bw)] + [(-(-bh // sy), -(-bw // sx))] * (ncomp - 1)


def _segment(marker, payload):
    return bytes([0xff, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def header(width, height, ncomp, sub, quant):
    sx, sy = sub if ncomp == 3 else (1, 1)
    out = b"\xff\xd8" + _segment(0xe0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if ncomp == 3 else 1):
        out += _segment(0xdb, bytes([t]) + bytes(int(quant[t][ZIGZAG[k]]) for k in range(64)))
    sof = bytes([8, height >> 8, height & 255, width >> 8, width & 255, ncomp])
    for c in range(ncomp):
        sof += bytes([c + 1, (sx << 4) | sy if c == 0 else 0x11, 0 if c == 0 else 1])
    out += _segment(0xc0, sof)
    for t in range(2 if ncomp == 3 else 1):
        out += _segment(0xc4, bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS))
        out += _segment(0xc4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    sos = bytes([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + _segment(0xda, sos + bytes([0, 0x3f, 0]))


class _Bits:
    """bits into bytes, highest bit first; n: bits written, acc: the `pending` bits no whole byte has taken yet"""

    def __init__(self):
        self.acc, self.pending, self.n, self.data = 0, 0, 0, bytearray()

    def put(self, value, length):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.pending += length
        self.n += length
        while self.pending >= 8:
            self.pending -= 8
            self.data.append(self.acc >> self.pending)
            self.acc &= (1 << self.pending) - 1


def _value(bits, table, symbol, v, s):
    code, length = table[symbol]
    bits.put(code, length)
    if s:
        bits.put(v if v >= 0 else v - 1, s)


def _block(bits, t, block, pred):
    """one block (64 ints, natural order) against the DC predictor; returns its DC"""
    d = int(block[0]) - pred
    _value(bits, DC_CODES[t], abs(d).bit_length(), d, abs(d).bit_length())
    r = 0
    for k in range(1, 64):
        v = int(block[ZIGZAG[k]])
        if v == 0:
            r += 1
            continue
        while r > 15:
            bits.put(*AC_CODES[t][0xf0])
            r -= 16
        s = abs(v).bit_length()
        _value(bits, AC_CODES[t], (r << 4) | s, v, s)
        r = 0
    if r > 0:
        bits.put(*AC_CODES[t][0x00])
    return int(block[0])


def scan_order(width, height, ncomp, sub):
    """[(component, block row, block column) or (component, None, None) for a dummy block] in scan order"""
    g = grids(width, height, ncomp, sub)
    if ncomp == 1:
        return [(0, y, x) for y in range(g[0][0]) for x in range(g[0][1])]
    sx, sy = sub
    out = []
    for my in range(g[1][0]):
        for mx in range(g[1][1]):
            for ry in range(sy):
                for rx in range(sx):
                    y, x = my * sy + ry, mx * sx + rx
                    out.append((0, y, x) if y < g[0][0] and x < g[0][1] else (0, None, None))
            out += [(1, my, mx), (2, my, mx)]
    return out


def encode_report(coefficients, width, height, quant, sub=(1, 1)):
    """(file, stuffed FF bytes, 1-bits that completed the last byte)"""
    ncomp = len(coefficients)
    coefficients = [np.asarray(a).reshape(gh, gw, 64) for a, (gh, gw) in zip(coefficients, grids(width, height, ncomp, sub))]
    bits = _Bits()
    pred = [0, 0, 0]
    zero = np.zeros(64, dtype=np.int64)
    for c, y, x in scan_order(width, height, ncomp, sub):
        if y is None:
            dummy = zero.copy()
            dummy[0] = pred[c]
            pred[c] = _block(bits, 0, dummy, pred[c])
        else:
            pred[c] = _block(bits, 0 if c == 0 else 1, coefficients[c][y, x], pred[c])
    short = -bits.n % 8
    bits.put((1 << short) - 1, short)
    data = bytes(bits.data)
    stuffed = data.count(b"\xff")
    return header(width, height, ncomp, sub, quant) + data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9", stuffed, short


def encode(coefficients, width, height, quant, sub=(1, 1)):
    return encode_report(coefficients, width, height, quant, sub)[0]


# ---- the cases ----
def quant_tables(quality, ncomp):
    from jpeg2png_amd import quality_tables
    return quality_tables(quality, ncomp)


def _blocks(rng, shape, kind):
    gh, gw = shape
    if kind == "zero":
        return np.zeros((gh, gw, 64), dtype=np.int16)
    if kind == "dense":
        return rng.integers(-1023, 1024, size=(gh, gw, 64)).astype(np.int16)
    if kind == "last":                  # only coefficient 63 (zigzag and natural alike) set: three ZRL codes and no EOB
        a = np.zeros((gh, gw, 64), dtype=np.int16)
        a[:, :, 63] = rng.integers(1, 1024, size=(gh, gw))
        return a
    # sparse: what a quantised photograph looks like — a DC that wanders, a few small low-frequency ACs
    a = np.zeros((gh, gw, 64), dtype=np.int16)
    a[:, :, 0] = rng.integers(-200, 201, size=(gh, gw))
    for k in range(1, 12):
        keep = rng.random((gh, gw)) < 0.5 / k
        a[:, :, ZIGZAG[k]] = np.where(keep, rng.integers(-40 // k - 1, 40 // k + 2, size=(gh, gw)), 0)
    return a


def make(width, height, ncomp, sub, kind, seed=1, quality=75):
    """a case: dict(width, height, sub, quant, coefficients)"""
    rng = np.random.default_rng(seed)
    sub = sub if ncomp == 3 else (1, 1)
    return {"width": width, "height": height, "sub": sub, "quality": quality, "quant": quant_tables(quality, ncomp),
            "coefficients": [_blocks(rng, g, kind) for g in grids(width, height, ncomp, sub)]}


def run_lengths_case():
    """grey blocks whose only non-zero AC sits behind exactly 14, 15, 16, 31, 32, 47 and 62 zeros (zigzag positions 15, 16, 17,
    32, 33, 48 and 63): zero to three ZRL codes, and no EOB behind position 63"""
    runs = [14, 15, 16, 31, 32, 47, 62]
    case = make(8 * len(runs), 8, 1, (1, 1), "zero")
    for i, r in enumerate(runs):
        case["coefficients"][0][0, i, ZIGZAG[r + 1]] = (-1) ** i * (3 + 100 * i)
    return case


def dc_swing_case():
    """neighbouring DCs of -1023 and +1023 in every component: differences of category 11 in both directions"""
    case = make(32, 16, 3, (1, 1), "zero")
    for a in case["coefficients"]:
        flat = a.reshape(-1, 64)
        flat[:, 0] = np.where(np.arange(flat.shape[0]) % 2 == 0, -1023, 1023)
    return case


def _search(want, last=0):
    """the first seed (of a fixed sequence) whose 16x8 grey sparse case, coefficient 63 of its last block set to `last`, ends as
    `want` says"""
    for seed in range(1, 4000):
        case = make(16, 8, 1, (1, 1), "sparse", seed=seed)
        case["coefficients"][0][0, 1, 63] = last
        data, _stuffed, short = encode_report(case["coefficients"], 16, 8, case["quant"])
        if want(data, short):
            return case
    raise AssertionError("no seed gives the directed ending")


def aligned_end_case():
    """the entropy-coded data ends on a byte boundary: no padding bits"""
    return _search(lambda data, short: short == 0)


def stuffed_end_case():
    """the last byte, completed with 1-bits, is FF and gets its 00: the data ends with the eight 1-bits of a coefficient 63 of
    +255 (no EOB behind position 63), of which the last byte holds some"""
    return _search(lambda data, short: short > 0 and data.endswith(b"\xff\x00\xff\xd9"), last=255)


def directed_cases():
    """{name: case}: what tests/test_entropy_gpu.py sends through j2p_entropy_encode"""
    cases = {
        "grey_8x8_zero": make(8, 8, 1, (1, 1), "zero"),
        "colour_1x1_420": make(1, 1, 3, (2, 2), "sparse", seed=2),
        "colour_16x16_420": make(16, 16, 3, (2, 2), "sparse", seed=3),
        "dense_24x40_444": make(24, 40, 3, (1, 1), "dense", seed=4, quality=95),
        "grey_17x9_dense": make(17, 9, 1, (1, 1), "dense", seed=5),
        "last_only_40x24_420": make(40, 24, 3, (2, 2), "last", seed=6),
        "dc_swing": dc_swing_case(),
        "run_lengths": run_lengths_case(),
        "aligned_end": aligned_end_case(),
        "stuffed_end": stuffed_end_case(),
        "dense_368x368_420": make(368, 368, 3, (2, 2), "dense", seed=7, quality=95),
        "sparse_368x368_420": make(368, 368, 3, (2, 2), "sparse", seed=8),
    }
    for (w, h) in ((40, 24), (41, 23)):
        for name, sub in (("420", (2, 2)), ("422", (2, 1)), ("440", (1, 2))):
            cases[f"sparse_{w}x{h}_{name}"] = make(w, h, 3, sub, "sparse", seed=w + h + sub[0] * 2 + sub[1])
    return cases
