"""The JPEG file with optimised Huffman tables (include/jpeg2png_amd.h: "Optimised Huffman tables") restated in plain Python on
top of tests/entropy_cases.py, and the cases its tests share (tests/test_huffman_cpu.py checks the restatement against libjpeg's
optimize_coding and the C table builder against the restatement, tests/test_huffman_gpu.py the device's histogram and files
against the restatement).

walk(...) is the scan as it is coded, symbol by symbol; counts(...) and encode_report(...) both read it, so what is counted is
what is coded.  table(count) is one table's BITS and HUFFVAL; Refused is the count above COUNT_LIMIT."""
import numpy as np

import entropy_cases as ec

COUNT_LIMIT = 1_000_000_000
TABLE_NAMES = ("dc0", "ac0", "dc1", "ac1")


class Refused(Exception):
    pass


def walk(coefficients, width, height, sub):
    """per scan position, dummy blocks included: (table, DC difference, [(AC symbol, value, size)]) — a ZRL is (0xF0, 0, 0), the
    EOB (0x00, 0, 0)"""
    ncomp = len(coefficients)
    zz = [np.asarray(a).reshape(gh, gw, 64)[:, :, ec.ZIGZAG].tolist() for a, (gh, gw) in zip(coefficients, ec.grids(width, height, ncomp, sub))]
    pred = [0, 0, 0]
    for c, y, x in ec.scan_order(width, height, ncomp, sub):
        if y is None:
            yield 0, 0, [(0x00, 0, 0)]
            continue
        block = zz[c][y][x]
        d, pred[c] = block[0] - pred[c], block[0]
        ac, r = [], 0
        for k in range(1, 64):
            v = block[k]
            if v == 0:
                r += 1
                continue
            for _ in range(r >> 4):
                ac.append((0xf0, 0, 0))
            s = abs(v).bit_length()
            ac.append((((r & 15) << 4) | s, v, s))
            r = 0
        if r > 0:
            ac.append((0x00, 0, 0))
        yield (0 if c == 0 else 1), d, ac


def counts(coefficients, width, height, sub=(1, 1)):
    """[DC0, AC0, DC1, AC1]: 256 counts each (DC1 and AC1 all zero for one component)"""
    out = [[0] * 256 for _ in range(4)]
    for t, d, ac in walk(coefficients, width, height, sub):
        out[2 * t][abs(d).bit_length()] += 1
        for symbol, _v, _s in ac:
            out[2 * t + 1][symbol] += 1
    return out


def code_lengths(count):
    """(BITS[1..16] as a list of 16, the longest length before limiting) of one table's 256 counts"""
    if max(count) > COUNT_LIMIT:
        raise Refused(f"a count of {max(count)}")
    freq = list(count) + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        for i in range(257):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    if longest > 32:
        raise Refused(f"a code of {longest} bits before limiting")
    bits = [0] * 33
    for n in codesize:
        if n:
            bits[n] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = max(n for n in range(1, 17) if bits[n] > 0)
    bits[i] -= 1
    return bits[1:17], longest


def table(count):
    """(BITS, HUFFVAL, the longest length before limiting)"""
    bits, longest = code_lengths(count)
    vals = sorted((s for s in range(256) if count[s]), key=lambda s: (-count[s], s))
    assert sum(bits) == len(vals)
    return bits, vals, longest


def header(width, height, ncomp, sub, quant, tables):
    """entropy_cases.header with the DHT segments of tables = [(BITS, HUFFVAL)] for DC0, AC0, DC1, AC1"""
    plain = ec.header(width, height, ncomp, sub, quant)
    first = plain.index(b"\xff\xc4")
    sos = plain.index(b"\xff\xda", first)
    dht = b""
    for t in range(2 if ncomp == 3 else 1):
        for cls in (0, 1):
            bits, vals = tables[2 * t + cls][:2]
            dht += ec._segment(0xc4, bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals))
    return plain[:first] + dht + plain[sos:]


def encode_report(coefficients, width, height, quant, sub=(1, 1)):
    """(file, dict of counts, tables [(BITS, HUFFVAL, longest)] x 4, bits of the scan, stuffed FF bytes)"""
    ncomp = len(coefficients)
    count = counts(coefficients, width, height, sub)
    tables = [table(count[k]) if k < 2 or ncomp == 3 else ([0] * 16, [], 0) for k in range(4)]
    codes = [ec._codes(b, v) for b, v, _ in tables]
    bits = ec._Bits()
    for t, d, ac in walk(coefficients, width, height, sub):
        s = abs(d).bit_length()
        ec._value(bits, codes[2 * t], s, d, s)
        for symbol, v, s in ac:
            ec._value(bits, codes[2 * t + 1], symbol, v, s)
    scan_bits = bits.n
    short = -bits.n % 8
    bits.put((1 << short) - 1, short)
    data = bytes(bits.data)
    file = header(width, height, ncomp, sub, quant, tables) + data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    return file, {"counts": count, "tables": tables, "bits": scan_bits, "stuffed": data.count(b"\xff")}


def encode(coefficients, width, height, quant, sub=(1, 1)):
    return encode_report(coefficients, width, height, quant, sub)[0]


def encode_case(case):
    return encode_report(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])


# ---- the cases ----
def _one_ac(width, height, placed):
    """a grey case whose block i holds the single AC coefficient placed[i] = (zigzag position, value); blocks beyond are zero"""
    case = ec.make(width, height, 1, (1, 1), "zero")
    flat = case["coefficients"][0].reshape(-1, 64)
    assert len(placed) <= flat.shape[0]
    rows = np.arange(len(placed))
    flat[rows, [ec.ZIGZAG[k] for k, _ in placed]] = [v for _, v in placed]
    return case


LIMITED_COUNTS = [1, 1, 2, 2, 3] + [-int(-(1.7 ** i) // 1) for i in range(3, 20)]


def limited_case():
    """1928x1928 grey, 58081 blocks: 22 (run, size) symbols whose counts grow like 1.7^i, one coefficient per block, so that the
    Huffman tree is deeper than 16 and the lengths are limited"""
    symbols = [(r, s) for s in (1, 2) for r in range(11)]
    rng = np.random.default_rng(22)
    placed = []
    for (r, s), n in zip(symbols, rng.permutation(LIMITED_COUNTS)):
        placed += [(r + 1, (1 << (s - 1)) * (-1) ** (r + s))] * int(n)
    order = rng.permutation(len(placed))
    return _one_ac(1928, 1928, [placed[i] for i in order])


def zrl_heavy_case():
    """grey blocks whose only coefficient is at zigzag 63, 47, 31 and 17: runs of 62, 46, 30 and 16, so 0xF0 is counted 3, 2, 1, 1
    times, and only the first has no EOB"""
    return _one_ac(32, 8, [(63, -5), (47, 300), (31, 1), (17, -1023)])


def ties_case():
    """grey 80x48, 60 blocks: 20 (run, size) symbols three times each, in an order that is not the symbols'"""
    symbols = [(r, s) for r in (0, 3, 7, 15) for s in (1, 2, 4, 7, 10)]
    rng = np.random.default_rng(5)
    placed = [(r + 1, (1 << (s - 1)) + (s > 1)) for r, s in symbols] * 3
    return _one_ac(80, 48, [placed[i] for i in rng.permutation(len(placed))])


def extra_cases():
    return {
        "limited": limited_case(),
        "single_symbol": ec.make(16, 16, 3, (2, 2), "zero"),
        "zrl_heavy": zrl_heavy_case(),
        "two_tiles": ec.make(72, 72, 1, (1, 1), "sparse", seed=72),
        "dummies_41x23_420": ec.make(41, 23, 3, (2, 2), "sparse", seed=4123),
        "ties": ties_case(),
    }


def directed_cases():
    """{name: case}: entropy_cases' directed cases and the ones above — what tests/test_huffman_gpu.py sends through the device"""
    cases = ec.directed_cases()
    cases.update(extra_cases())
    return cases


SUBS = {"444": (1, 1), "420": (2, 2), "422": (2, 1), "440": (1, 2)}
SIZES = [(1, 1), (8, 8), (16, 16), (40, 24), (41, 23), (24, 40), (17, 9), (200, 136)]


def sweep():
    """every size x component count and sampling x content, at Q 50 and 95 alternately"""
    k = 0
    for w, h in SIZES:
        for ncomp, sub in [(1, "444")] + [(3, s) for s in SUBS]:
            for kind in ("zero", "dense", "last", "sparse"):
                k += 1
                yield f"{w}x{h}_{ncomp}_{sub}_{kind}", ec.make(w, h, ncomp, SUBS[sub], kind, seed=k, quality=(50, 95)[k % 2])
