"""Reading a baseline JPEG file (include/jpeg2png_amd.h: "Reading a JPEG file") restated in plain Python, and a file writer for the
cases the decoder's tests share (tests/test_decode_cpu.py holds the restatement against libjpeg and the C parser against
jpeg_header(); tests/test_decode_gpu.py holds the device's decoder against the restatement).

decode(data) -> (arrays, info): per component an int16 array [blocks_h, blocks_w, 64] in natural order.  Refused files raise
Refused with .code EFORMAT or ENOTSUP and .why, a word for what was wrong.

write(...) builds on tests/entropy_cases.py — its scan order, its _block and its four kinds of content, imported and not edited —
and adds restart intervals, sampling factors beyond 2, Huffman tables other than Annex K's, fill bytes and bytes behind EOI."""
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


def write(coefficients, width, height, quant, sub=(1, 1), restart=0, tables="annex_k", fill=False, trailing=b"", dqt16=False, sof=0xC0, report=None):
    """a baseline JPEG file of the coefficients (entropy_cases' grids for sub = (sx, sy), chroma 1x1).
    restart: MCUs per restart interval (0: none).  tables: "annex_k" (slots 0 / 1 as libjpeg writes them), "swapped" (component 0 codes
    with Annex K's chroma pair from slot 2, components 1 and 2 with the luma pair from slot 3) or "own" (tables built from this
    file's own symbol counts, component 0's in slot 0, the others' in slot 1).  fill: two FF fill bytes in front of every marker
    from DQT on, the RSTn included.  trailing: bytes behind EOI.  dqt16: 16-bit DQT entries, both tables in one segment.
    report (a dict): receives 'stuffed_before_rst', how many restart markers follow a stuffed FF 00 directly."""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    grids = ec.grids(width, height, ncomp, sub)
    coefficients = [np.asarray(a).reshape(gh, gw, 64) for a, (gh, gw) in zip(coefficients, grids)]
    order = ec.scan_order(width, height, ncomp, sub)
    per_mcu = sub[0] * sub[1] + 2 if ncomp == 3 else 1
    nmcu = len(order) // per_mcu
    ri = restart or nmcu

    def code_scan():
        chunks = []
        zero = np.zeros(64, dtype=np.int64)
        for first in range(0, nmcu, ri):
            bits, pred = ec._Bits(), [0, 0, 0]
            for c, y, x in order[first * per_mcu:min(first + ri, nmcu) * per_mcu]:
                t = (0 if c == 0 else 1) if tables != "swapped" else (1 if c == 0 else 0)
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

    if tables == "own":
        counting = [_Counting(), _Counting()], [_Counting(), _Counting()]
        with _coding_with(*counting):
            code_scan()
        pairs = {"dc": [optimal_table(t.counts) if t.counts else ANNEX_K["dc"][i] for i, t in enumerate(counting[0])],
                 "ac": [optimal_table(t.counts) if t.counts else ANNEX_K["ac"][i] for i, t in enumerate(counting[1])]}
    else:
        pairs = ANNEX_K
    with _coding_with(pairs["dc"], pairs["ac"]):
        chunks = code_scan()

    slots = {"annex_k": (0, 1), "own": (0, 1), "swapped": (3, 2)}[tables]     # the slot of pair 0 (luma's, or the first own), of pair 1
    ntab = 2 if ncomp == 3 else 1
    out = b"\xff\xd8" + ec._segment(0xe0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    dqt = [bytes([(16 if dqt16 else 0) | t]) + b"".join(int(quant[t][ec.ZIGZAG[k]]).to_bytes(2 if dqt16 else 1, "big") for k in range(64)) for t in range(ntab)]
    out += _segment(0xdb, b"".join(dqt), fill) if dqt16 else b"".join(_segment(0xdb, d, fill) for d in dqt)
    body = bytes([8, height >> 8, height & 255, width >> 8, width & 255, ncomp])
    for c in range(ncomp):
        body += bytes([c + 1, (sub[0] << 4) | sub[1] if c == 0 else 0x11, 0 if c == 0 else 1])
    out += _segment(sof, body, fill)
    used = (0, 1) if ncomp == 3 else ((1,) if tables == "swapped" else (0,))
    for t in used:
        out += _segment(0xc4, bytes([slots[t]]) + bytes(pairs["dc"][t][0]) + bytes(pairs["dc"][t][1]), fill)
        out += _segment(0xc4, bytes([0x10 | slots[t]]) + bytes(pairs["ac"][t][0]) + bytes(pairs["ac"][t][1]), fill)
    if restart:
        out += _segment(0xdd, bytes([restart >> 8, restart & 255]), fill)
    body = bytes([ncomp])
    for c in range(ncomp):
        t = (0 if c == 0 else 1) if tables != "swapped" else (1 if c == 0 else 0)
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
    want = {"cut_mid_block": ("truncated", "leftover", "code", "run"), "cut_between_blocks": ("truncated",), "rst_number_changed": ("restart",),
            "rst_removed": ("restart",), "code_in_no_table": ("code",), "run_past_63": ("run",)}
    assert sorted(out) == sorted(want), sorted(out)
    return {name: (data, want[name]) for name, data in out.items()}
