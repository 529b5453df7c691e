"""The progressive JPEG file of include/jpeg2png_amd.h ("The progressive JPEG file") restated in plain Python on top of
tests/entropy_cases.py (header pieces, scan order, bit writer) and tests/huffman_cases.py (the tables), and the cases its tests
share (tests/test_progressive_cpu.py checks the restatement against libjpeg's jpeg_simple_progression,
tests/test_progressive_gpu.py the device's coder against the restatement).

A scan is first walked into its operations — ("s", table, symbol) and ("b", value, length) — with no table in hand; the counts
and the coded bits both read that list, so what is counted is what is coded.  encode_report(...) returns the file and, per scan,
its parameters, the counts of each table it used, its bits before padding, its stuffed FF bytes, how many EOB runs it flushed and
why, and how many ZRLs it emitted."""
import numpy as np

import entropy_cases as ec
import huffman_cases as hc

# (components; Ss, Se; Ah, Al) — jpeg_simple_progression() of IJG libjpeg
SCANS = {
    3: [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
        ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)],
    1: [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)],
}
EOBRUN_LIMIT = 0x7fff
CORRECTION_LIMIT = 937          # libjpeg's MAX_CORR_BITS - DCTSIZE2 + 1: a run is flushed once it holds MORE bits than this
WHY = ("limit_7fff", "limit_937", "next_block", "end_of_scan")


class Refused(Exception):
    pass


def _magnitude(ops, v, s):
    if s:
        ops.append(("b", (v if v >= 0 else v - 1) & ((1 << s) - 1), s))


def _dc_values(zz, width, height, sub, al):
    """(table, DC >> al) per position of the interleaved scan; a dummy block repeats its predecessor"""
    ncomp = len(zz)
    last = [0, 0, 0]
    for c, y, x in ec.scan_order(width, height, ncomp, sub):
        if y is not None:
            last[c] = zz[c][y][x][0]
        yield c, last[c] >> al


def _dc_first(zz, width, height, sub, al, ops):
    pred = [0, 0, 0]
    for c, v in _dc_values(zz, width, height, sub, al):
        d, pred[c] = v - pred[c], v
        s = abs(d).bit_length()
        ops.append(("s", ("dc", 0 if c == 0 else 1), s))
        _magnitude(ops, d, s)


def _dc_refine(zz, width, height, sub, al, ops):
    for _c, v in _dc_values(zz, width, height, sub, al):
        ops.append(("b", v & 1, 1))


class _Run:
    """the pending EOB run of an AC scan: its length and, in refinement scans, the correction bits that wait with it"""

    def __init__(self, ops, table, flushes):
        self.ops, self.table, self.flushes, self.n, self.bits = ops, table, flushes, 0, []

    def flush(self, why):
        if self.n == 0:
            return
        extra = self.n.bit_length() - 1
        self.ops.append(("s", self.table, extra << 4))
        if extra:
            self.ops.append(("b", self.n & ((1 << extra) - 1), extra))
        self.ops += [("b", b, 1) for b in self.bits]
        self.n, self.bits = 0, []
        self.flushes[why] += 1


def _ac_first(blocks, table, ss, se, al, ops, flushes):
    run = _Run(ops, table, flushes)
    for block in blocks:
        r = 0
        for k in (range(ss, se + 1) if any(block[ss:se + 1]) else ()):
            v = block[k]
            t = abs(v) >> al
            if t == 0:
                r += 1
                continue
            run.flush("next_block")
            while r > 15:
                ops.append(("s", table, 0xf0))
                r -= 16
            s = t.bit_length()
            if s > 10:
                raise Refused(f"a coefficient of {v} at Al = {al}")
            ops.append(("s", table, (r << 4) | s))
            ops.append(("b", (t if v >= 0 else ~t) & ((1 << s) - 1), s))
            r = 0
        if r > 0 or not any(block[ss:se + 1]):           # (a band of zeros: walked at once)
            run.n += 1
            if run.n == EOBRUN_LIMIT:
                run.flush("limit_7fff")
    run.flush("end_of_scan")


def _ac_refine(blocks, table, ss, se, al, ops, flushes):
    """returns the number of ZRLs"""
    run = _Run(ops, table, flushes)
    zrls = 0
    for block in blocks:
        if not any(block[ss:se + 1]):                   # (a band of zeros, walked at once: it joins the run with no correction bit)
            run.n += 1
            if run.n == EOBRUN_LIMIT:
                run.flush("limit_7fff")
            continue
        t = [abs(v) >> al for v in block]
        eob = max((k for k in range(ss, se + 1) if t[k] == 1), default=0)
        r, waiting = 0, []
        for k in range(ss, se + 1):
            if t[k] == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                run.flush("next_block")
                ops.append(("s", table, 0xf0))
                zrls += 1
                r -= 16
                ops += [("b", b, 1) for b in waiting]
                waiting = []
            if t[k] > 1:
                waiting.append(t[k] & 1)
                continue
            run.flush("next_block")
            ops.append(("s", table, (r << 4) | 1))
            ops.append(("b", 0 if block[k] < 0 else 1, 1))
            ops += [("b", b, 1) for b in waiting]
            waiting = []
            r = 0
        if r > 0 or waiting:
            run.n += 1
            run.bits += waiting
            if run.n == EOBRUN_LIMIT:
                run.flush("limit_7fff")
            elif len(run.bits) > CORRECTION_LIMIT:
                run.flush("limit_937")
    run.flush("end_of_scan")
    return zrls


def scan_operations(zz, width, height, sub, scan):
    """(operations, flushes by reason, ZRLs of a refinement scan) of one scan; zz: per component [row][column][zigzag position]"""
    comps, ss, se, ah, al = scan
    ops, flushes, zrls = [], dict.fromkeys(WHY, 0), 0
    if ss == 0:
        (_dc_refine if ah else _dc_first)(zz, width, height, sub, al, ops)
    else:
        c = comps[0]
        blocks = [b for row in zz[c] for b in row]
        table = ("ac", 0 if c == 0 else 1)
        if ah:
            zrls = _ac_refine(blocks, table, ss, se, al, ops, flushes)
        else:
            _ac_first(blocks, table, ss, se, al, ops, flushes)
    return ops, flushes, zrls


def scan_tables(ncomp, scan):
    """the tables a scan's DHT segments carry, in their order: ("dc" or "ac", slot)"""
    comps, ss, se, ah, _al = scan
    out = []
    for c in comps:
        if ss == 0 and ah == 0 and ("dc", min(c, 1)) not in out:
            out.append(("dc", min(c, 1)))
        if se and ("ac", min(c, 1)) not in out:
            out.append(("ac", min(c, 1)))
    return out


def _sos(scan):
    comps, ss, se, ah, al = scan
    sos = bytes([len(comps)])
    for c in comps:
        td = min(c, 1) if ss == 0 and ah == 0 else 0
        ta = min(c, 1) if se else 0
        sos += bytes([c + 1, (td << 4) | ta])
    return ec._segment(0xda, sos + bytes([ss, se, (ah << 4) | al]))


def encode_report(coefficients, width, height, quant, sub=(1, 1)):
    """(file, [per scan: dict(scan, counts {table: 256 counts}, tables {table: (BITS, HUFFVAL, longest)}, bits, stuffed, flushes,
    zrls)])"""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    zz = [np.asarray(a).reshape(gh, gw, 64)[:, :, ec.ZIGZAG].tolist() for a, (gh, gw) in zip(coefficients, ec.grids(width, height, ncomp, sub))]
    plain = ec.header(width, height, ncomp, sub, quant)
    sof, dht = plain.index(b"\xff\xc0"), plain.index(b"\xff\xc4")
    file = bytearray(plain[:sof] + b"\xff\xc2" + plain[sof + 2:dht])
    report = []
    for scan in SCANS[ncomp]:
        ops, flushes, zrls = scan_operations(zz, width, height, sub, scan)
        counts = {t: [0] * 256 for t in scan_tables(ncomp, scan)}
        for op in ops:
            if op[0] == "s":
                counts[op[1]][op[2]] += 1
        tables = {}
        for t, count in counts.items():
            try:
                tables[t] = hc.table(count)
            except hc.Refused as e:
                raise Refused(str(e))
            bits, vals, _longest = tables[t]
            file += ec._segment(0xc4, bytes([((t[0] == "ac") << 4) | t[1]]) + bytes(bits) + bytes(vals))
        codes = {t: ec._codes(b, v) for t, (b, v, _) in tables.items()}
        bits = ec._Bits()
        for op in ops:
            if op[0] == "s":
                bits.put(*codes[op[1]][op[2]])
            else:
                bits.put(op[1], op[2])
        nbits = bits.n
        short = -bits.n % 8
        bits.put((1 << short) - 1, short)
        data = bytes(bits.data)
        file += _sos(scan) + data.replace(b"\xff", b"\xff\x00")
        report.append({"scan": scan, "counts": counts, "tables": tables, "bits": nbits, "stuffed": data.count(b"\xff"),
                       "flushes": flushes, "zrls": zrls})
    return bytes(file + b"\xff\xd9"), report


def encode(coefficients, width, height, quant, sub=(1, 1)):
    return encode_report(coefficients, width, height, quant, sub)[0]


def encode_case(case):
    return encode_report(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])


# ---- the cases ----
def eobrun_limit_case():
    """grey 1456x1456, all zero: 182 x 182 = 33124 blocks, every AC scan one run that is flushed at 32767 and again at 357"""
    return ec.make(1456, 1456, 1, (1, 1), "zero")


def correction_limit_case():
    """grey 64x64: block b holds a seeded random number 0..63 of coefficients from {4, -4, -5, 6} at random AC positions and
    nothing else — no refinement scan meets a new coefficient, each is one run, and the 937-bit rule cuts it at uneven places"""
    case = ec.make(64, 64, 1, (1, 1), "zero")
    rng = np.random.default_rng(937)
    flat = case["coefficients"][0].reshape(-1, 64)
    for b in range(flat.shape[0]):
        n = int(rng.integers(0, 64))
        where = 1 + rng.permutation(63)[:n]
        flat[b, [ec.ZIGZAG[k] for k in where]] = rng.choice([4, -4, -5, 6], size=n)
    return case


def refine_zrl_case():
    """grey 48x8, six blocks built by hand (zigzag positions):
    0: +1, -1, +1 at 20, 40 and 60 with -4 at 1..5 and +4 at 22, 39 and 50: the 17 zeros between 20 and 39 give a ZRL at 39, a
       position that was non-zero before, and the correction bit of 22 follows that ZRL
    1: -1 at 3, twenty zeros, then +4 at 24: the zeros behind the last +-1 give no ZRL
    2: +-2 and +-3 only: new in scan (2, 1), corrections in (1, 0)
    3: +-1 everywhere
    4: +1 at 63 alone: three ZRLs in the last scan
    5: zero"""
    case = ec.make(48, 8, 1, (1, 1), "zero")
    blocks = case["coefficients"][0].reshape(-1, 64)

    def put(b, k, v):
        blocks[b, ec.ZIGZAG[k]] = v
    for k, v in ((20, 1), (40, -1), (60, 1), (22, 4), (39, 4), (50, 4)):
        put(0, k, v)
    for k in range(1, 6):
        put(0, k, -4)
    put(1, 3, -1)
    put(1, 24, 4)
    for i, k in enumerate((2, 9, 17, 18, 40, 63)):
        put(2, k, (2, -3, 3, -2)[i % 4])
    for k in range(1, 64):
        put(3, k, (-1) ** k)
    put(4, 63, 1)
    return case


EXISTING = ["grey_8x8_zero", "colour_1x1_420", "sparse_41x23_420", "sparse_40x24_422", "sparse_41x23_440", "dc_swing", "run_lengths",
            "stuffed_end", "dense_368x368_420", "sparse_368x368_420"]


def new_cases():
    return {"eobrun_limit": eobrun_limit_case(), "correction_limit": correction_limit_case(), "refine_zrl": refine_zrl_case()}


def gpu_cases():
    """{name: case}: what tests/test_progressive_gpu.py sends through j2p_entropy_encode_progressive"""
    directed = ec.directed_cases()
    cases = {name: directed[name] for name in EXISTING}
    cases.update(new_cases())
    return cases
