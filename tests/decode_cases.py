"""Reading a baseline JPEG file (include/jpeg2png_amd.h: "Reading a JPEG file") restated in plain Python, and a file writer for the
cases the decoder's tests share (tests/test_decode_cpu.py holds the restatement against libjpeg and the C parser against
jpeg_header(); tests/test_decode_gpu.py holds the device's decoder against the restatement).

decode(data) -> (arrays, info): per component an int16 array [blocks_h, blocks_w, 64] in natural order.  Refused files raise
Refused with .code EFORMAT or ENOTSUP and .why, a word for what was wrong.

write(...) builds on tests/entropy_cases.py — its scan order, its _block and its four kinds of content, imported and not edited —
and adds restart intervals, sampling factors beyond 2, Huffman tables other than Annex K's, fill bytes and bytes behind EOI.

framing_cases() was chosen for what a JPEG file may contain; boundary_cases(), place_markers() and periodic_case() for where the
device's kernels divide their work (restart markers on lane, chunk and workgroup edges, more intervals than a workgroup or a
scan tile holds, more scan tiles than k_scan_tiles takes in one trip); damaged_cases() are the files to refuse."""
import contextlib

import numpy as np

import entropy_cases as ec

EFORMAT, ENOTSUP = -6, -7


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(f"{'EFORMAT' if code == EFORMAT else 'ENOTSUP'}: {why}")
        self.code, self.why = code, why


# ---- the restated decoder ----
def _tables_from(bits, vals):
    """{(length, code): symbol} of one DHT table"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= 1 << length:
                raise Refused(EFORMAT, "table")
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def parse(data):
    """the marker segments: dict of width, height, components [(id, h, v, tq, td, ta)], quant {slot: uint16[64] natural}, dc / ac
    {slot: {(length, code): symbol}}, restart_interval, scan_begin, scan_end"""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Refused(EFORMAT, "soi")
    quant, dc, ac, frame, ri, pos = {}, {}, {}, None, 0, 2
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise Refused(EFORMAT, "marker")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m == 0xD9:
            raise Refused(EFORMAT, "eoi")
        if pos + 2 > len(data):
            raise Refused(EFORMAT, "segment")
        n = int.from_bytes(data[pos:pos + 2], "big")
        if n < 2 or pos + n > len(data):
            raise Refused(EFORMAT, "segment")
        body = data[pos + 2:pos + n]
        pos += n
        if m == 0xDB:
            at = 0
            while at < len(body):
                precision, slot = body[at] >> 4, body[at] & 15
                at += 1
                size = 128 if precision else 64
                if precision > 1 or slot > 3 or at + size > len(body):
                    raise Refused(EFORMAT, "dqt")
                raw = np.frombuffer(body, ">u2" if precision else np.uint8, 64, at).astype(np.uint16)
                at += size
                q = np.zeros(64, np.uint16)
                q[ec.ZIGZAG] = raw
                quant[slot] = q
        elif m == 0xC4:
            at = 0
            while at < len(body):
                cls, slot = body[at] >> 4, body[at] & 15
                at += 1
                if cls > 1 or slot > 3 or at + 16 > len(body):
                    raise Refused(EFORMAT, "dht")
                bits = list(body[at:at + 16])
                if sum(bits) > 256 or at + 16 + sum(bits) > len(body):
                    raise Refused(EFORMAT, "dht")
                vals = list(body[at + 16:at + 16 + sum(bits)])
                at += 16 + sum(bits)
                if cls == 0 and any(v > 15 for v in vals):
                    raise Refused(EFORMAT, "dht")
                (ac if cls else dc)[slot] = _tables_from(bits, vals)
        elif m in (0xC0, 0xC1):
            if frame is not None or len(body) < 6:
                raise Refused(EFORMAT, "sof")
            if body[0] in (12, 16):
                raise Refused(ENOTSUP, "precision")
            if body[0] != 8:
                raise Refused(EFORMAT, "sof")
            nc = body[5]
            if nc == 0 or len(body) != 6 + 3 * nc:
                raise Refused(EFORMAT, "sof")
            if nc not in (1, 3):
                raise Refused(ENOTSUP, "components")
            height, width = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            if width == 0:
                raise Refused(EFORMAT, "sof")
            if height == 0:
                raise Refused(ENOTSUP, "dnl")
            comps = [[body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]] for i in range(nc)]
            if any(not 1 <= h <= 4 or not 1 <= v <= 4 or tq > 3 for _, h, v, tq in comps):
                raise Refused(EFORMAT, "sof")
            frame = {"width": width, "height": height, "components": comps}
        elif 0xC0 <= m <= 0xCF:
            raise Refused(ENOTSUP, "process")
        elif m == 0xDD:
            if len(body) != 2:
                raise Refused(EFORMAT, "dri")
            ri = int.from_bytes(body, "big")
        elif m in (0xDC, 0xDE, 0xDF):
            raise Refused(ENOTSUP, "dnl" if m == 0xDC else "process")
        elif m == 0xDA:
            if frame is None or len(body) < 1 or len(body) != 4 + 2 * body[0] or body[0] == 0 or body[0] > len(frame["components"]):
                raise Refused(EFORMAT, "sos")
            if body[0] != len(frame["components"]):
                raise Refused(ENOTSUP, "scans")
            ids = [c[0] for c in frame["components"]]
            for i, comp in enumerate(frame["components"]):
                if body[1 + 2 * i] not in ids:
                    raise Refused(EFORMAT, "sos")
                if body[1 + 2 * i] != comp[0]:
                    raise Refused(ENOTSUP, "order")
                comp += [body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15]
                if comp[4] > 3 or comp[5] > 3:
                    raise Refused(EFORMAT, "sos")
            if bytes(body[-3:]) != b"\x00\x3f\x00":
                raise Refused(EFORMAT, "sos")
            break
    for _, _, _, tq, td, ta in frame["components"]:
        if tq not in quant or td not in dc or ta not in ac:
            raise Refused(EFORMAT, "missing table")
    if len(frame["components"]) == 3 and sum(h * v for _, h, v, *_ in frame["components"]) > 10:
        raise Refused(EFORMAT, "mcu")
    end = pos
    while True:
        end = data.find(b"\xff", end)
        if end < 0 or end + 1 >= len(data):
            raise Refused(EFORMAT, "truncated")
        nxt = data[end + 1]
        if nxt == 0 or 0xD0 <= nxt <= 0xD7:
            end += 2
        elif nxt == 0xFF:
            end += 1
        else:
            break
    at = end
    while True:
        if at + 2 > len(data) or data[at] != 0xFF:
            raise Refused(EFORMAT, "truncated")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        at += 2
        if m == 0xD9:
            break
        if m == 0xDC:
            raise Refused(ENOTSUP, "dnl")
        if m == 0xDA:
            raise Refused(ENOTSUP, "scans")
        if m == 0x01 or 0xD0 <= m <= 0xD8 or at + 2 > len(data):
            raise Refused(EFORMAT, "marker")
        n = int.from_bytes(data[at:at + 2], "big")
        if n < 2 or at + n > len(data):
            raise Refused(EFORMAT, "segment")
        at += n
    frame.update(quant=quant, dc=dc, ac=ac, restart_interval=ri, scan_begin=pos, scan_end=end)
    # a block is at least two symbols (two bits), a restart marker two bytes: less data than that is a truncated scan
    comps, mcus_w, mcus_h = geometry(frame)
    blocks = mcus_w * mcus_h * sum(h * v for _, _, h, v in comps)
    if (end - pos) * 8 < 2 * blocks or -(-mcus_w * mcus_h // (ri or mcus_w * mcus_h)) - 1 > (end - pos) // 2:
        raise Refused(EFORMAT, "truncated")
    return frame


def geometry(frame):
    """per component (blocks_h, blocks_w, h, v) with h = v = 1 for a single component; MCUs across, down"""
    comps = frame["components"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    width, height = frame["width"], frame["height"]
    grids = [(-(-(-(-height * c[2] // vmax)) // 8), -(-(-(-width * c[1] // hmax)) // 8)) for c in comps]
    if len(comps) == 1:
        return [(grids[0][0], grids[0][1], 1, 1)], grids[0][1], grids[0][0]
    return [(g[0], g[1], c[1], c[2]) for g, c in zip(grids, comps)], -(-width // (8 * hmax)), -(-height // (8 * vmax))


class _Reader:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8)).tolist()
        self.pos, self.n = 0, 8 * len(data)

    def bit(self):
        if self.pos >= self.n:
            raise Refused(EFORMAT, "truncated")
        b = self.bits[self.pos]
        self.pos += 1
        return b

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Refused(EFORMAT, "code")

    def value(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def _intervals(ecs):
    """the entropy-coded data cut at its RSTn markers and unstuffed: [bytes]; the markers' numbers"""
    out, numbers, cur, i = [], [], bytearray(), 0
    while i < len(ecs):
        b = ecs[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif i + 1 < len(ecs) and ecs[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif i + 1 < len(ecs) and 0xD0 <= ecs[i + 1] <= 0xD7:
            out.append(bytes(cur))
            numbers.append(ecs[i + 1] & 7)
            cur = bytearray()
            i += 2
        else:
            i += 1                       # a fill byte
    out.append(bytes(cur))
    return out, numbers


def decode(data):
    data = bytes(data)
    frame = parse(data)
    comps, mcus_w, mcus_h = geometry(frame)
    arrays = [np.zeros((gh, gw, 64), dtype=np.int16) for gh, gw, _, _ in comps]
    nmcu, ri = mcus_w * mcus_h, frame["restart_interval"] or mcus_w * mcus_h
    chunks, numbers = _intervals(data[frame["scan_begin"]:frame["scan_end"]])
    if len(chunks) != -(-nmcu // ri) or numbers != [k % 8 for k in range(len(numbers))]:
        raise Refused(EFORMAT, "restart")
    for k, chunk in enumerate(chunks):
        rd, pred = _Reader(chunk), [0] * len(comps)
        for mcu in range(k * ri, min((k + 1) * ri, nmcu)):
            my, mx = divmod(mcu, mcus_w)
            for c, (gh, gw, h, v) in enumerate(comps):
                _, _, _, _, td, ta = frame["components"][c]
                for j in range(h * v):
                    by, bx = my * v + j // h, mx * h + j % h
                    block = np.zeros(64, dtype=np.int64)
                    pred[c] += rd.value(rd.symbol(frame["dc"][td]))
                    if not -32768 <= pred[c] <= 32767:
                        raise Refused(EFORMAT, "dc")
                    block[0] = pred[c]
                    pos = 1
                    while pos < 64:
                        rs = rd.symbol(frame["ac"][ta])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            pos += 16
                            if pos > 64:
                                raise Refused(EFORMAT, "run")
                            continue
                        pos += r
                        v_ = rd.value(s)
                        if pos > 63:
                            raise Refused(EFORMAT, "run")
                        block[ec.ZIGZAG[pos]] = v_
                        pos += 1
                    if by < gh and bx < gw:
                        arrays[c][by, bx] = block
        if rd.pos > rd.n or rd.n - rd.pos >= 8:
            raise Refused(EFORMAT, "leftover")
    return arrays, frame


# ---- the writer ----
ANNEX_K = {"dc": [(ec.DC_BITS[t], list(ec.DC_VALS)) for t in range(2)], "ac": [(ec.AC_BITS[t], list(ec.AC_VALS[t])) for t in range(2)]}


def _codes(bits, vals):
    return ec._codes(bits, vals)


def optimal_table(counts):
    """(BITS, HUFFVAL) from symbol counts the way Annex K.2 builds them: Huffman lengths with one reserved code point so that no code
    is all ones, lengths above 16 folded back"""
    freq = {s: n for s, n in counts.items() if n > 0}
    freq[256] = 1
    size = {s: 0 for s in freq}
    others = {s: None for s in freq}
    live = dict(freq)
    while len(live) > 1:
        a = min(live, key=lambda s: (live[s], -s))
        fa = live.pop(a)
        b = min(live, key=lambda s: (live[s], -s))
        live[b] += fa
        for head in (b, a):
            s = head
            while True:
                size[s] += 1
                if others[s] is None:
                    break
                s = others[s]
            if head == b:
                others[s] = a
    bits = [0] * 33
    for s in size:
        bits[size[s]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                        # the reserved code point
    vals = [s for length in range(1, 33) for s in sorted(freq) if s != 256 and size[s] == length]
    return bits[1:17], vals


@contextlib.contextmanager
def _coding_with(dc_pairs, ac_pairs):
    """entropy_cases._block codes with its module's DC_CODES / AC_CODES [0] and [1]: these, for the time being.  The swap is of
    module globals: anything else that codes with entropy_cases while the block is open would code with these tables too, so it is
    only safe in a single-threaded suite (as this one is) and the block holds nothing but the writer's own coding loop."""
    saved = ec.DC_CODES, ec.AC_CODES
    ec.DC_CODES, ec.AC_CODES = [dc if isinstance(dc, dict) else _codes(*dc) for dc in dc_pairs], [ac if isinstance(ac, dict) else _codes(*ac) for ac in ac_pairs]
    try:
        yield
    finally:
        ec.DC_CODES, ec.AC_CODES = saved


class _Counting(dict):
    """a code table that counts what is looked up and codes nothing"""

    def __init__(self):
        super().__init__()
        self.counts = {}

    def __getitem__(self, symbol):
        self.counts[symbol] = self.counts.get(symbol, 0) + 1
        return (0, 1)


def _segment(marker, payload, fill):
    return (b"\xff" * (2 if fill else 0)) + ec._segment(marker, payload)


def _code_scan(coefficients, order, per_mcu, nmcu, ri, swapped):
    """the stuffed entropy-coded data of every restart interval, coded with entropy_cases' current tables: [bytes]"""
    chunks = []
    zero = np.zeros(64, dtype=np.int64)
    for first in range(0, nmcu, ri):
        bits, pred = ec._Bits(), [0, 0, 0]
        for c, y, x in order[first * per_mcu:min(first + ri, nmcu) * per_mcu]:
            t = (0 if c == 0 else 1) if not swapped else (1 if c == 0 else 0)
            if y is None:
                dummy = zero.copy()
                dummy[0] = pred[c]
                pred[c] = ec._block(bits, t, dummy, pred[c])
            else:
                pred[c] = ec._block(bits, t, coefficients[c][y, x], pred[c])
        short = -bits.n % 8
        bits.put((1 << short) - 1, short)
        chunks.append(bytes(bits.data).replace(b"\xff", b"\xff\x00"))
    return chunks


def _layout(coefficients, width, height, sub):
    """what the writer codes: (coefficients as grids, sub, scan order, blocks per MCU, MCUs)"""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    grids = ec.grids(width, height, ncomp, sub)
    coefficients = [np.asarray(a).reshape(gh, gw, 64) for a, (gh, gw) in zip(coefficients, grids)]
    order = ec.scan_order(width, height, ncomp, sub)
    per_mcu = sub[0] * sub[1] + 2 if ncomp == 3 else 1
    return coefficients, sub, order, per_mcu, len(order) // per_mcu


def symbol_counts(coefficients, width, height, sub=(1, 1), restart=0):
    """{"dc": [{symbol: count}, {symbol: count}], "ac": [...]}: what a file of these coefficients codes with table pair 0
    (component 0) and pair 1 (the others)"""
    coefficients, sub, order, per_mcu, nmcu = _layout(coefficients, width, height, sub)
    counting = [_Counting(), _Counting()], [_Counting(), _Counting()]
    with _coding_with(*counting):
        _code_scan(coefficients, order, per_mcu, nmcu, restart or nmcu, False)
    return {"dc": [t.counts for t in counting[0]], "ac": [t.counts for t in counting[1]]}


def write(coefficients, width, height, quant, sub=(1, 1), restart=0, tables="annex_k", fill=False, trailing=b"", dqt16=False, sof=0xC0, report=None):
    """a baseline JPEG file of the coefficients (entropy_cases' grids for sub = (sx, sy), chroma 1x1).
    restart: MCUs per restart interval (0: none).  tables: "annex_k" (slots 0 / 1 as libjpeg writes them), "swapped" (component 0 codes
    with Annex K's chroma pair from slot 2, components 1 and 2 with the luma pair from slot 3), "own" (tables built from this
    file's own symbol counts, component 0's in slot 0, the others' in slot 1) or explicit ones, {"dc": [(BITS, HUFFVAL), (BITS,
    HUFFVAL)], "ac": [...]}, written to slots 0 and 1 as "own" does.  fill: two FF fill bytes in front of every marker
    from DQT on, the RSTn included.  trailing: bytes behind EOI.  dqt16: 16-bit DQT entries, both tables in one segment.
    report (a dict): receives 'stuffed_before_rst', how many restart markers follow a stuffed FF 00 directly."""
    ncomp = len(coefficients)
    coefficients, sub, order, per_mcu, nmcu = _layout(coefficients, width, height, sub)
    ri = restart or nmcu
    swapped = isinstance(tables, str) and tables == "swapped"

    if isinstance(tables, dict):
        pairs = tables
    elif tables == "own":
        counts = symbol_counts(coefficients, width, height, sub, restart)
        pairs = {kind: [optimal_table(n) if n else ANNEX_K[kind][i] for i, n in enumerate(counts[kind])] for kind in ("dc", "ac")}
    else:
        pairs = ANNEX_K
    with _coding_with(pairs["dc"], pairs["ac"]):
        chunks = _code_scan(coefficients, order, per_mcu, nmcu, ri, swapped)

    slots = (3, 2) if swapped else (0, 1)                                      # the slot of pair 0 (luma's, or the first own), of pair 1
    ntab = 2 if ncomp == 3 else 1
    out = b"\xff\xd8" + ec._segment(0xe0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    dqt = [bytes([(16 if dqt16 else 0) | t]) + b"".join(int(quant[t][ec.ZIGZAG[k]]).to_bytes(2 if dqt16 else 1, "big") for k in range(64)) for t in range(ntab)]
    out += _segment(0xdb, b"".join(dqt), fill) if dqt16 else b"".join(_segment(0xdb, d, fill) for d in dqt)
    body = bytes([8, height >> 8, height & 255, width >> 8, width & 255, ncomp])
    for c in range(ncomp):
        body += bytes([c + 1, (sub[0] << 4) | sub[1] if c == 0 else 0x11, 0 if c == 0 else 1])
    out += _segment(sof, body, fill)
    used = (0, 1) if ncomp == 3 else ((1,) if swapped else (0,))
    for t in used:
        out += _segment(0xc4, bytes([slots[t]]) + bytes(pairs["dc"][t][0]) + bytes(pairs["dc"][t][1]), fill)
        out += _segment(0xc4, bytes([0x10 | slots[t]]) + bytes(pairs["ac"][t][0]) + bytes(pairs["ac"][t][1]), fill)
    if restart:
        out += _segment(0xdd, bytes([restart >> 8, restart & 255]), fill)
    body = bytes([ncomp])
    for c in range(ncomp):
        t = (0 if c == 0 else 1) if not swapped else (1 if c == 0 else 0)
        body += bytes([c + 1, (slots[t] << 4) | slots[t]])
    out += _segment(0xda, body + bytes([0, 0x3f, 0]), fill)
    stuffed_before = 0
    for k, chunk in enumerate(chunks):
        if k:
            stuffed_before += chunks[k - 1].endswith(b"\xff\x00")
            out += (b"\xff\xff" if fill else b"") + bytes([0xff, 0xd0 + (k - 1) % 8])
        out += chunk
    if report is not None:
        report["stuffed_before_rst"] = stuffed_before
    return out + (b"\xff\xff" if fill else b"") + b"\xff\xd9" + bytes(trailing)


def write_case(case, **kw):
    return write(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], **kw)


# ---- the cases ----
def _stuffed_before_rst_case():
    """a 4:4:4 file with a restart interval of one MCU in which a stuffed FF stands directly in front of a restart marker"""
    for seed in range(1, 400):
        case = ec.make(24, 16, 3, (1, 1), "dense", seed=seed, quality=95)
        report = {}
        data = write_case(case, restart=1, report=report)
        if report["stuffed_before_rst"]:
            return case, data
    raise AssertionError("no seed puts a stuffed FF in front of a restart marker")


def framing_cases():
    """{name: (case, file)}: sampling, tables and framing beyond what entropy_cases.encode writes"""
    out = {}
    for name, sub in (("422", (2, 1)), ("440", (1, 2)), ("411", (4, 1))):
        case = ec.make(41, 23, 3, sub, "sparse", seed=11 + sub[0] + 3 * sub[1])
        out[f"sparse_41x23_{name}"] = (case, write_case(case))
    case = ec.make(41, 23, 3, (2, 2), "sparse", seed=21)
    out["swapped_tables"] = (case, write_case(case, tables="swapped"))
    out["own_tables"] = (case, write_case(case, tables="own"))
    dense = ec.make(24, 40, 3, (1, 1), "dense", seed=22, quality=95)
    out["own_tables_dense"] = (dense, write_case(dense, tables="own"))
    grey = ec.make(17, 9, 1, (1, 1), "sparse", seed=23)
    out["grey_swapped"] = (grey, write_case(grey, tables="swapped"))
    out["restart_1"] = (case, write_case(case, restart=1))
    out["restart_3"] = (case, write_case(case, restart=3))                  # 3 MCUs across: 41 / 16
    four = ec.make(41, 23, 3, (1, 1), "sparse", seed=24)                   # 6 x 3 MCUs
    out["restart_4_of_6"] = (four, write_case(four, restart=4))            # does not divide the MCU row
    out["restart_row"] = (four, write_case(four, restart=6))
    out["restart_wraps"] = (four, write_case(four, restart=1))             # 17 markers: RST numbers go round twice
    out["restart_grey"] = (grey, write_case(grey, restart=2))
    out["stuffed_before_rst"] = _stuffed_before_rst_case()
    out["fill_bytes"] = (four, write_case(four, restart=5, fill=True))
    out["trailing_bytes"] = (case, write_case(case, trailing=b"\xff\xd9\x00\xff\xda garbage \xff"))
    out["dqt16_sof1"] = (case, write_case(case, dqt16=True, sof=0xC1))
    return out


def _cut(data, frame, keep):
    """the file with only the first `keep` bytes of its entropy-coded data, EOI behind them"""
    return data[:frame["scan_begin"] + keep] + b"\xff\xd9"


def damaged_cases():
    """{name: (file, why)}: files the decoder must refuse with EFORMAT; `why` is what the restated decoder says"""
    out = {}
    case = ec.make(32, 16, 1, (1, 1), "sparse", seed=31)
    good = write_case(case)
    frame = parse(good)
    n = frame["scan_end"] - frame["scan_begin"]
    out["cut_mid_block"] = _cut(good, frame, n // 2)
    # a cut on a byte boundary between two blocks: a seed whose first block codes to whole bytes, none of them FF
    for seed in range(1, 4000):
        c = ec.make(32, 8, 1, (1, 1), "sparse", seed=seed)
        one = [c["coefficients"][0][:, :1]]
        _, stuffed, short = ec.encode_report(one, 8, 8, c["quant"])
        if short == 0 and stuffed == 0:
            f = write_case(c)
            first = parse(ec.encode(one, 8, 8, c["quant"]))
            out["cut_between_blocks"] = _cut(f, parse(f), first["scan_end"] - first["scan_begin"])
            break
    rst = ec.make(41, 23, 3, (1, 1), "sparse", seed=24)
    f = write_case(rst, restart=2)
    at = f.index(b"\xff\xd3", parse(f)["scan_begin"])
    out["rst_number_changed"] = f[:at + 1] + b"\xd5" + f[at + 2:]
    out["rst_removed"] = f[:at] + f[at + 2:]
    # a bit flip that leads to a code in no table, found by search against the restated decoder
    dense = ec.make(16, 8, 1, (1, 1), "dense", seed=32)
    f = write_case(dense)
    fr = parse(f)
    for bit in range(8 * (fr["scan_end"] - fr["scan_begin"])):
        i = fr["scan_begin"] + bit // 8
        flipped = f[:i] + bytes([f[i] ^ (0x80 >> (bit % 8))]) + f[i + 1:]
        if flipped[i] == 0xFF or f[i] == 0xFF or (i > 0 and f[i - 1] == 0xFF):
            continue
        try:
            decode(flipped)
        except Refused as e:
            if e.why == "code":
                out["code_in_no_table"] = flipped
                break
    # a run past coefficient 63: four times (run 15, size 1) from position 1 lands on 16, 32, 48 and then 64
    bits = ec._Bits()
    bits.put(*ec.DC_CODES[0][0])
    for _ in range(4):
        bits.put(*ec.AC_CODES[0][0xF1])
        bits.put(1, 1)
    short = -bits.n % 8
    bits.put((1 << short) - 1, short)
    one = ec.make(8, 8, 1, (1, 1), "zero")
    out["run_past_63"] = ec.header(8, 8, 1, (1, 1), one["quant"]) + bytes(bits.data).replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    # files whose marker segments and sizes are in order: only the kernels that decode the data can refuse them
    # a DC that leaves int16 in its 17th block (the 16-block neighbour, boundary_cases()' dc_near_limit, is a good file)
    out["dc_above_int16"] = _dc_file([2047] * 17)[0]
    out["dc_below_int16"] = _dc_file([-2047] * 17)[0]
    # whole bytes behind the last block's padding: one, and several 32-bit subsequences of data that belong to no block
    four = write_case(ec.make(32, 8, 1, (1, 1), "sparse", seed=33))
    out["leftover_byte"] = four[:-2] + b"\x7f" + b"\xff\xd9"
    out["leftover_many"] = four[:-2] + bytes([0x12, 0x34, 0x56, 0x78] * 8) + b"\xff\xd9"
    # one marker too many, the numbers in sequence: an empty interval in the middle, and one in front of EOI
    f = write_case(rst, restart=2)
    begin = parse(f)["scan_begin"]
    cuts = [begin - 2] + [begin + a - 1 for a in marker_offsets(f)] + [len(f) - 2]        # the SOS segment's end, every RSTn, EOI
    chunks = [f[a + 2:b] for a, b in zip(cuts, cuts[1:])]
    assert len(chunks) == 9 and all(chunks)
    for name, with_empty in (("rst_doubled", chunks[:4] + [b""] + chunks[4:]), ("rst_before_eoi", chunks + [b""])):
        out[name] = f[:begin] + b"".join((bytes([0xff, 0xd0 + (k - 1) % 8]) if k else b"") + c for k, c in enumerate(with_empty)) + b"\xff\xd9"
    assert f == f[:begin] + b"".join((bytes([0xff, 0xd0 + (k - 1) % 8]) if k else b"") + c for k, c in enumerate(chunks)) + b"\xff\xd9"
    # ... and the right number of markers with nothing between two of them: eight grey blocks, a marker behind each, the third
    # block's data gone.  Every other interval is whole, and a DC of -32768 (no differences at all) would be in range: nothing
    # but the empty interval itself is wrong with this file
    f = write_case(ec.make(64, 8, 1, (1, 1), "sparse", seed=34), restart=1)
    begin, at = parse(f)["scan_begin"], marker_offsets(f)
    out["rst_empty_interval"] = f[:begin + at[1] + 1] + f[begin + at[2] - 1:]
    want = {"cut_mid_block": ("truncated", "leftover", "code", "run"), "cut_between_blocks": ("truncated",), "rst_number_changed": ("restart",),
            "rst_removed": ("restart",), "code_in_no_table": ("code",), "run_past_63": ("run",), "dc_above_int16": ("dc",),
            "dc_below_int16": ("dc",), "leftover_byte": ("leftover",), "leftover_many": ("leftover",), "rst_doubled": ("restart",),
            "rst_before_eoi": ("restart",), "rst_empty_interval": ("truncated",)}
    assert sorted(out) == sorted(want), sorted(out)
    return {name: (data, want[name]) for name, data in out.items()}


# ---- cases aimed at where the kernels divide their work: 4-byte lanes, 256-byte chunks and 1024-byte workgroups of the
# unstuffing kernels, 256 intervals per workgroup of k_decode_intervals, 1024 elements per tile of the scans and 256 tiles per
# trip of k_scan_tiles ----
def marker_offsets(data):
    """the offset, counted from scan_begin, of the Dn byte of every RSTn marker in the entropy-coded data, in order"""
    frame = parse(data)
    out, i, end = [], frame["scan_begin"], frame["scan_end"]
    while i < end:
        if data[i] != 0xFF:
            i += 1
        elif data[i + 1] == 0:
            i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            out.append(i + 1 - frame["scan_begin"])
            i += 2
        else:
            i += 1                       # a fill byte
    return out


def place_markers(data, targets=(), fixed=None):
    """the file with FF fill bytes in front of its restart markers.  targets[m] (None, or no entry: the marker stays): as many fill
    bytes (0..255) go in front of marker m as put its Dn byte at an offset, counted from scan_begin, congruent to targets[m] modulo
    256; the markers are taken in order, because each insertion moves the later ones.  fixed = {m: n}: n fill bytes in front of
    marker m, whatever offset that gives."""
    data = bytes(data)
    begin = parse(data)["scan_begin"]
    fixed = fixed or {}
    for m in range(len(marker_offsets(data))):
        at = marker_offsets(data)[m]
        if m in fixed:
            n = fixed[m]
        elif m < len(targets) and targets[m] is not None:
            n = (targets[m] - at) % 256
        else:
            continue
        data = data[:begin + at - 1] + b"\xff" * n + data[begin + at - 1:]
    return data


EDGE_TARGETS = (0, 1, 255, 254, 4, 3)   # the Dn byte's offset modulo 256: FF | Dn across a chunk edge, the pair at a chunk's start,
#                                         at its end, one byte in front of that, and across and in front of a lane's edge


def stuffed_on_chunk_edge(data):
    """offsets from scan_begin of every stuffed FF 00 whose FF is a chunk's last byte and whose 00 the next chunk's first"""
    frame = parse(data)
    ecs = data[frame["scan_begin"]:frame["scan_end"]]
    return [i for i in range(255, len(ecs) - 1, 256) if ecs[i] == 0xFF and ecs[i + 1] == 0]


def blank_chunks(data):
    """the 256-byte chunks of the entropy-coded data that hold nothing but FF: no byte to keep and no marker"""
    frame = parse(data)
    ecs = data[frame["scan_begin"]:frame["scan_end"]]
    return [c for c in range(len(ecs) // 256) if ecs[256 * c:256 * c + 256] == b"\xff" * 256]


def _markers_on_edges_case():
    """24 MCUs of dense 4:4:4 with a restart marker behind each, the markers moved onto the unstuffing kernels' edges; the seed is
    the first that also puts a marker's FF in the last byte of a 1024-byte group and a stuffed FF | 00 across a chunk edge.
    -> (case, the file before placement, the placed file)"""
    for seed in range(1, 400):
        case = ec.make(48, 32, 3, (1, 1), "dense", seed=seed, quality=95)
        plain = write_case(case, restart=1)
        placed = place_markers(plain, [EDGE_TARGETS[m % 6] for m in range(23)])
        at = marker_offsets(placed)
        if any(a % 1024 == 0 for a in at[::6]) and stuffed_on_chunk_edge(placed):
            return case, plain, placed
    raise AssertionError("no seed puts a marker on a workgroup edge and a stuffed FF on a chunk edge")


def fibonacci_tables(counts):
    """symbol_counts' result with every table's counts replaced, in order of frequency, by consecutive Fibonacci numbers, and the
    optimal tables of that: {"dc": [(BITS, HUFFVAL)] * 2, "ac": ...}.  Such a table is almost a single chain: one code of every
    length, and with more than 15 symbols the lengths above 16 folded back."""
    def skew(n):
        out, a, b = {}, 1, 2
        for s in sorted(n, key=lambda s: (n[s], s)):
            out[s] = a
            a, b = b, a + b
        return out
    return {kind: [optimal_table(skew(n)) if n else ANNEX_K[kind][i] for i, n in enumerate(counts[kind])] for kind in ("dc", "ac")}


def _skewed_tables_case():
    """dense 4:4:4 blocks in which every second coefficient in zigzag order is zero with probability one half: runs of 0 and 1
    in front of every size, and an EOB where coefficient 63 went — an alphabet of about 20 AC symbols a table, all of which the
    file uses, coded with tables skewed so that the rare ones have codes of up to 16 bits"""
    case = ec.make(24, 40, 3, (1, 1), "dense", seed=22, quality=95)
    rng = np.random.default_rng(22)
    odd = np.array([ec.ZIGZAG[k] for k in range(1, 64, 2)])
    for a in case["coefficients"]:
        drop = rng.random(a.shape[:2] + (odd.size,)) < 0.5
        a[:, :, odd] = np.where(drop, 0, a[:, :, odd])
    tables = fibonacci_tables(symbol_counts(case["coefficients"], 24, 40, (1, 1)))
    return case, write_case(case, tables=tables)


def _dc_file(diffs):
    """a grey file of len(diffs) blocks in a row, each coding its DC difference and an EOB (written with predictor 0 for every
    block, as damaged_cases() writes run_past_63: the running sum may leave int16) -> (file, quant)"""
    bits = ec._Bits()
    block = np.zeros(64, dtype=np.int64)
    for d in diffs:
        block[0] = d
        ec._block(bits, 0, block, 0)
    short = -bits.n % 8
    bits.put((1 << short) - 1, short)
    quant = ec.quant_tables(75, 1)
    return ec.header(8 * len(diffs), 8, 1, (1, 1), quant) + bytes(bits.data).replace(b"\xff", b"\xff\x00") + b"\xff\xd9", quant


def _dc_near_limit_case():
    data, quant = _dc_file([2047] * 16)
    coefficients = np.zeros((1, 16, 64), dtype=np.int16)
    coefficients[0, :, 0] = 2047 * np.arange(1, 17)
    return {"width": 128, "height": 8, "sub": (1, 1), "quality": 75, "quant": quant, "coefficients": [coefficients]}, data


BOUNDARY = ("markers_on_edges", "fill_covers_chunks", "intervals_257_grey", "intervals_1056_420", "intervals_212_short_last", "skewed_tables",
            "dc_near_limit")
_boundary = {}


def boundary_cases():
    """{name: (case, file)} beside framing_cases(); built once a process (the arrays are shared: do not write to them)"""
    if not _boundary:
        case, plain, placed = _markers_on_edges_case()
        _boundary["markers_on_edges"] = (case, placed)
        # 600 fill bytes cover two whole chunks when they begin in a chunk's first 89 bytes: the first marker of the middle for which they do
        filled = [place_markers(plain, fixed={m: 600}) for m in range(6, 18)]
        _boundary["fill_covers_chunks"] = (case, [f for f in filled if len(blank_chunks(f)) == 2][0])
        grey = ec.make(2056, 8, 1, (1, 1), "sparse", seed=41)
        _boundary["intervals_257_grey"] = (grey, write_case(grey, restart=1))
        many = ec.make(528, 512, 3, (2, 2), "sparse", seed=42)                 # 33 x 32 MCUs
        _boundary["intervals_1056_420"] = (many, write_case(many, restart=1))
        _boundary["intervals_212_short_last"] = (many, write_case(many, restart=5))
        _boundary["skewed_tables"] = _skewed_tables_case()
        _boundary["dc_near_limit"] = _dc_near_limit_case()
        assert tuple(_boundary) == BOUNDARY
    return dict(_boundary)


# ---- one short period, repeated: a file of any size in milliseconds ----
PERIOD_SEED = 1
_period = []


def periodic_period():
    """(blocks int16[4, 64], their entropy-coded bytes before stuffing, bits): four grey blocks (a DC and one to three small ACs
    each) found by a seeded search, coded from predictor 0, such that the last block's DC is 0 (every repetition codes to the
    same bits), the bits are whole bytes (no padding), 40 to 44 a block (at 32-bit subsequences there are more subsequences than
    blocks, and blocks straddle them) and hold exactly one FF byte (the unstuffer has work in every repetition)"""
    if not _period:
        rng = np.random.default_rng(PERIOD_SEED)
        for _trial in range(100000):
            blocks = np.zeros((4, 64), dtype=np.int16)
            blocks[:3, 0] = rng.integers(-1023, 1024, size=3)
            for blk in blocks:
                for _ in range(int(rng.integers(1, 4))):
                    blk[ec.ZIGZAG[int(rng.integers(1, 12))]] = int(rng.integers(1, 32)) * (1 if rng.random() < 0.5 else -1)
            bits, pred = ec._Bits(), 0
            for blk in blocks:
                pred = ec._block(bits, 0, blk, pred)
            if bits.n % 8 == 0 and 160 <= bits.n <= 176 and bytes(bits.data).count(b"\xff") == 1:
                _period.append((blocks, bytes(bits.data), bits.n))
                break
        else:
            raise AssertionError("no period found")
    blocks, raw, n = _period[0]
    assert blocks[3, 0] == 0 and n % 8 == 0 and len(raw) * 8 == n and 40 * 4 <= n <= 44 * 4 and raw.count(b"\xff") == 1
    return blocks, raw, n


def periodic_case(bw, bh):
    """a grey file of bw x bh blocks (a multiple of four) whose scan is periodic_period() repeated, and its coefficients
    int16[bh, bw, 64]; the quantisation table is entropy_cases.quant_tables(75, 1)"""
    blocks, raw, _n = periodic_period()
    assert bw * bh % 4 == 0
    quant = ec.quant_tables(75, 1)
    data = ec.header(8 * bw, 8 * bh, 1, (1, 1), quant) + raw.replace(b"\xff", b"\xff\x00") * (bw * bh // 4) + b"\xff\xd9"
    return data, np.tile(blocks, (bw * bh // 4, 1)).reshape(bh, bw, 64)
