"""The progressive JPEG file of include/jpeg2png_amd.h ("The progressive JPEG file") restated in plain Python on top of
tests/entropy_cases.py (header pieces, scan order, bit writer) and tests/huffman_cases.py (the tables), and the cases its tests
share (tests/test_progressive_cpu.py checks the restatement against libjpeg's jpeg_simple_progression,
tests/test_progressive_gpu.py the device's coder against the restatement).

A scan is first walked into its operations — ("s", table, symbol) and ("b", value, length) — with no table in hand; the counts
and the coded bits both read that list, so what is counted is what is coded.  encode_report(...) returns the file and, per scan,
its parameters, the counts of each table it used, its bits before padding, its stuffed FF bytes, how many EOB runs it flushed and
why, and how many ZRLs it emitted — and what the directed cases are searched and asserted by: every EOB run it flushed (its first
block, its length, why), the 1-bits that completed the scan's last byte and that byte before stuffing."""
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


def dc_slice(values, ah, ops):
    """one restart interval of a DC scan (tests/scan_decode_cases.py writes files with restarts): values, [(component, DC >> Al)]
    of its positions in scan order, coded as _dc_first and _dc_refine code a whole scan; the predictors start at 0"""
    pred = [0, 0, 0]
    for c, v in values:
        if ah:
            ops.append(("b", v & 1, 1))
        else:
            d, pred[c] = v - pred[c], v
            s = abs(d).bit_length()
            ops.append(("s", ("dc", 0 if c == 0 else 1), s))
            _magnitude(ops, d, s)


class _Run:
    """the pending EOB run of an AC scan: its length and, in refinement scans, the correction bits that wait with it"""

    def __init__(self, ops, table, runs):
        self.ops, self.table, self.runs, self.n, self.bits, self.first = ops, table, runs, 0, [], 0

    def join(self, b):
        """block b joins the run"""
        if self.n == 0:
            self.first = b
        self.n += 1

    def flush(self, why):
        if self.n == 0:
            return
        extra = self.n.bit_length() - 1
        self.ops.append(("s", self.table, extra << 4))
        if extra:
            self.ops.append(("b", self.n & ((1 << extra) - 1), extra))
        self.ops += [("b", b, 1) for b in self.bits]
        self.runs.append((self.first, self.n, why))
        self.n, self.bits = 0, []


def _ac_first(blocks, table, ss, se, al, ops, runs):
    run = _Run(ops, table, runs)
    for b, block in enumerate(blocks):
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
            run.join(b)
            if run.n == EOBRUN_LIMIT:
                run.flush("limit_7fff")
    run.flush("end_of_scan")


def _ac_refine(blocks, table, ss, se, al, ops, runs):
    """returns the number of ZRLs"""
    run = _Run(ops, table, runs)
    zrls = 0
    for b, block in enumerate(blocks):
        if not any(block[ss:se + 1]):                   # (a band of zeros, walked at once: it joins the run with no correction bit)
            run.join(b)
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
            run.join(b)
            run.bits += waiting
            if run.n == EOBRUN_LIMIT:
                run.flush("limit_7fff")
            elif len(run.bits) > CORRECTION_LIMIT:
                run.flush("limit_937")
    run.flush("end_of_scan")
    return zrls


def scan_walk(zz, width, height, sub, scan):
    """(operations, EOB runs as (first block, length, why) in the order they were flushed, ZRLs of a refinement scan) of one scan;
    zz: per component [row][column][zigzag position]"""
    comps, ss, se, ah, al = scan
    ops, runs, zrls = [], [], 0
    if ss == 0:
        (_dc_refine if ah else _dc_first)(zz, width, height, sub, al, ops)
    else:
        c = comps[0]
        blocks = [b for row in zz[c] for b in row]
        table = ("ac", 0 if c == 0 else 1)
        if ah:
            zrls = _ac_refine(blocks, table, ss, se, al, ops, runs)
        else:
            _ac_first(blocks, table, ss, se, al, ops, runs)
    return ops, runs, zrls


def count_by_why(runs):
    flushes = dict.fromkeys(WHY, 0)
    for _first, _length, why in runs:
        flushes[why] += 1
    return flushes


def scan_operations(zz, width, height, sub, scan):
    """(operations, flushes by reason, ZRLs of a refinement scan) of one scan"""
    ops, runs, zrls = scan_walk(zz, width, height, sub, scan)
    return ops, count_by_why(runs), zrls


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
    zrls, runs [(first block, length, why)], short: the 1-bits that completed the last byte, last: that byte before stuffing, None
    where the scan has no data)])"""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    zz = [np.asarray(a).reshape(gh, gw, 64)[:, :, ec.ZIGZAG].tolist() for a, (gh, gw) in zip(coefficients, ec.grids(width, height, ncomp, sub))]
    plain = ec.header(width, height, ncomp, sub, quant)
    sof, dht = plain.index(b"\xff\xc0"), plain.index(b"\xff\xc4")
    file = bytearray(plain[:sof] + b"\xff\xc2" + plain[sof + 2:dht])
    report = []
    for scan in SCANS[ncomp]:
        ops, runs, zrls = scan_walk(zz, width, height, sub, scan)
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
                       "flushes": count_by_why(runs), "zrls": zrls, "runs": runs, "short": short, "last": data[-1] if data else None})
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


def _put(case, b, values):
    """block b of a grey case: {zigzag position: value}"""
    flat = case["coefficients"][0].reshape(-1, 64)
    for k, v in values.items():
        flat[b, ec.ZIGZAG[k]] = v


def cut_from_block_case(b):
    """grey 1456x1456 (33124 blocks), all zero but block b, which is new in every AC scan and ends in a tail in each — 4 at 1 (scan
    1-5), -4 at 6 (6-63), 2 at 7 (2, 1), -1 at 8 (1, 0): the run that starts AT block b is cut at 32767 blocks.  With b = 1 (mod 4) the
    walking lane of k_prog_runs reaches its 16-byte alignment with a length of 3 (mod 4), the only residue from which four blocks at
    once could step onto 32767 (32763 + 4): the guard of that fast path decides.  b = 1: the lane of block 1 walks, fifteen single
    steps first; b = 17: another workgroup lane than that of block 0, which walks the seventeen blocks in front"""
    case = ec.make(1456, 1456, 1, (1, 1), "zero")
    _put(case, b, {1: 4, 6: -4, 7: 2, 8: -1})
    return case


BOTH_LIMITS = {"dense": range(0, 15), "sixty": range(1015, 1015 + 10 * 3001, 3001), "fifty": range(32787, 32787 + 8 * 7, 7)}


def both_limits_case():
    """grey 1456x1456: blocks 0..14 hold 2 and -3 at every AC position (945 correction bits in the last scan: the 937-bit rule cuts
    behind block 14); ten blocks hold 3 at 1..60 (600 correction bits) inside the run that starts at block 15 and is cut at 32767
    blocks, eight blocks hold -2 at 1..50 (400) in the run behind it.  600 + 400 > 937: a cutter that keeps the flushed run's
    waiting bits cuts the last run where libjpeg does not"""
    case = ec.make(1456, 1456, 1, (1, 1), "zero")
    for b in BOTH_LIMITS["dense"]:
        _put(case, b, {k: 2 if k % 2 else -3 for k in range(1, 64)})
    for b in BOTH_LIMITS["sixty"]:
        _put(case, b, {k: 3 for k in range(1, 61)})
    for b in BOTH_LIMITS["fifty"]:
        _put(case, b, {k: -2 for k in range(1, 51)})
    return case


# a base seed at which row_1's one block is a late block with a coefficient at position 63 (a refinement scan with no run at all);
# the densities below were chosen so that the family then shows every run tests/test_progressive_cpu.py asserts of it
ROW_SEED = 52
ROW_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def row_case(n):
    """grey 8n x 8, one row of n blocks from one seeded generator: quiet blocks (zero, 55 %), CARRIERS (43 %: 1 to 24 coefficients
    of magnitude 4..7: new in the first scans, corrections in both refinement scans — some five waiting bits a block, so that
    the 937-bit rule cuts runs of the long rows) and LATE blocks (2 %: one to three of +-1, +-2 or +-3: new only in a refinement
    scan, one in four at position 63, where no tail follows); from 17 blocks on, blocks 15, 16, 17 and n - 1 are late blocks.
    The sizes are those around the 16 flag bytes a load of k_prog_runs, the 64 blocks a workgroup of k_prog_classify and the 1024
    items a tile of k_scan_* (over the items of all scans)"""
    case = ec.make(8 * n, 8, 1, (1, 1), "zero")
    rng = np.random.default_rng(ROW_SEED + n)
    forced = (15, 16, 17, n - 1) if n >= 17 else ()
    for b in range(n):
        kind = rng.random()
        if b in forced or kind < 0.02:
            where = 1 + rng.permutation(63)[:int(rng.integers(1, 4))]
            if rng.random() < 0.25:
                where[0] = 63
            _put(case, b, {int(k): int(rng.choice([1, -1, 2, -2, 3, -3])) for k in where})
        elif kind < 0.45:
            where = 1 + rng.permutation(63)[:int(rng.integers(1, 25))]
            _put(case, b, {int(k): int(rng.choice([4, -5, 6, -7, -4, 5, -6, 7])) for k in where})
    return case


# ---- how a scan's stream ends ----
KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")
STREAM_ENDS = tuple(f"{kind}_{end}" for kind in KINDS for end in ("whole_bytes", "ff_end")) + ("whole_words",)
END_SHAPES = ((16, 8, 1, (1, 1)), (24, 16, 3, (2, 2)))


def scan_kind(scan):
    _comps, ss, _se, ah, _al = scan
    return ("dc" if ss == 0 else "ac") + ("_refine" if ah else "_first")


def stream_ends(report):
    """which of STREAM_ENDS a file's report shows.  <kind>_whole_bytes: a scan of that kind that is not the file's last ends with no
    padding bit; <kind>_ff_end: one that is not the last is completed with 1-bits to a last byte of FF, so its stuffed 00 is the
    scan's final byte, in front of the next scan's DHT; whole_words: some scan's bits are a multiple of 32"""
    out = set()
    for r in report[:-1]:
        if r["short"] == 0:
            out.add(scan_kind(r["scan"]) + "_whole_bytes")
        elif r["last"] == 0xff:
            out.add(scan_kind(r["scan"]) + "_ff_end")
    if any(r["bits"] % 32 == 0 for r in report):
        out.add("whole_words")
    return out


_END_SEEDS = {}


def _stream_end_seeds():
    """{one of STREAM_ENDS: (shape, seed)}: per property the first seed (of a fixed sequence, as entropy_cases._search) whose sparse
    16x8 grey or 24x16 4:2:0 case shows it — found in one pass, once.  dc_refine_whole_bytes is not searched: a DC refinement scan
    is one bit per position, 2 and 12 at these sizes, never a multiple of 8 (dc_refine_whole_bytes_case is built by hand)"""
    wanted = set(STREAM_ENDS) - {"dc_refine_whole_bytes"}
    if not _END_SEEDS:
        found = {}
        for seed in range(1, 4000):
            for shape in END_SHAPES:
                for end in stream_ends(encode_case(ec.make(*shape, "sparse", seed=seed))[1]):
                    found.setdefault(end, (shape, seed))
            if wanted <= set(found):
                break
        else:
            raise AssertionError(f"no seed gives the directed endings {sorted(wanted - set(found))}")
        _END_SEEDS.update({end: found[end] for end in wanted})
    return _END_SEEDS


def dc_refine_whole_bytes_case():
    """grey 64x8: eight positions, eight bits of DC refinement and no padding"""
    return ec.make(64, 8, 1, (1, 1), "sparse", seed=1)


def stream_end_cases():
    """{"end_" + one of STREAM_ENDS: a case that shows it}"""
    cases = {"end_" + end: ec.make(*shape, "sparse", seed=seed) for end, (shape, seed) in sorted(_stream_end_seeds().items())}
    cases["end_dc_refine_whole_bytes"] = dc_refine_whole_bytes_case()
    return cases


EXISTING = ["grey_8x8_zero", "colour_1x1_420", "sparse_41x23_420", "sparse_40x24_422", "sparse_41x23_440", "dc_swing", "run_lengths",
            "stuffed_end", "dense_368x368_420", "sparse_368x368_420"]
STREAM_END_NAMES = ["end_" + end for end in STREAM_ENDS]


def new_cases():
    cases = {"eobrun_limit": eobrun_limit_case(), "correction_limit": correction_limit_case(), "refine_zrl": refine_zrl_case(),
             "cut_from_block_1": cut_from_block_case(1), "cut_from_block_17": cut_from_block_case(17), "both_limits": both_limits_case()}
    cases.update({f"row_{n}": row_case(n) for n in ROW_SIZES})
    cases.update(stream_end_cases())
    return cases


def gpu_cases():
    """{name: case}: what tests/test_progressive_gpu.py sends through j2p_entropy_encode_progressive"""
    directed = ec.directed_cases()
    cases = {name: directed[name] for name in EXISTING}
    cases.update(new_cases())
    return cases
