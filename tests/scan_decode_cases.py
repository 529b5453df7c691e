"""Reading a progressive JPEG file (include/jpeg2png_amd.h: "Reading a progressive JPEG file") restated in plain Python on top of
tests/decode_cases.py (the baseline restatement: its Refused, its bit reader, its unstuffing), and a writer for arbitrary scan
scripts on top of tests/progressive_cases.py (scan_walk), tests/huffman_cases.py (table) and tests/entropy_cases.py (_Bits).

parse_scans(data) -> the frame of decode_cases.parse plus "progressive" and "scans": per scan its components (frame indices), ss,
se, ah, al, dc_slots, ac_slots, restart_interval, intervals, begin, end and the tables in force at its SOS ("dc", "ac": {slot:
{(length, code): symbol}}).  decode(data) -> (arrays, parsed): per component int16 [blocks_h, blocks_w, 64] in natural order.
Refused files raise decode_cases.Refused with .code and .why.

write(coefficients, width, height, quant, sub, script) -> the file of that script: a list of (components, Ss, Se, Ah, Al); a DC
scan names all components (interleaved) or one.  Every scan brings the tables made for it.  restart=, dri= and fill= give the file
restart intervals, per scan if wanted, and fill bytes in front of a scan's markers.

edge_cases() are the good files aimed at where the kernels divide their work and at what a restart interval ends;
damaged_cases() the files to refuse, each with the restatement's reason."""
import numpy as np

import decode_cases as dc
import entropy_cases as ec
import huffman_cases as hc
import progressive_cases as pc
from decode_cases import EFORMAT, ENOTSUP, Refused  # noqa: F401

SCANS_MAX, TABLES_MAX = 128, 392


def _data_end(data, pos):
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
            return end


def _frame_marker(data):
    pos = 2
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            return 0
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m in (0xD9, 0xDA):
            return 0
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m
        if pos + 2 > len(data):
            return 0
        n = int.from_bytes(data[pos:pos + 2], "big")
        if n < 2 or pos + n > len(data):
            return 0
        pos += n


def parse_scans(data):
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Refused(EFORMAT, "soi")
    if _frame_marker(data) != 0xC2:
        frame = dc.parse(data)
        comps, mcus_w, mcus_h = dc.geometry(frame)
        nmcu = mcus_w * mcus_h
        frame["progressive"] = False
        frame["scans"] = [{"components": list(range(len(comps))), "ss": 0, "se": 63, "ah": 0, "al": 0,
                           "dc_slots": [c[4] for c in frame["components"]], "ac_slots": [c[5] for c in frame["components"]],
                           "restart_interval": frame["restart_interval"], "intervals": -(-nmcu // (frame["restart_interval"] or nmcu)),
                           "begin": frame["scan_begin"], "end": frame["scan_end"], "dc": dict(frame["dc"]), "ac": dict(frame["ac"])}]
        return frame
    quant, tdc, tac, frame, ri, pos, scans, ntables = {}, {}, {}, None, 0, 2, [], 0
    last_al = {}
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise Refused(EFORMAT, "marker")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0xD9:
            if not scans:
                raise Refused(EFORMAT, "eoi")
            break
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            if scans:
                raise Refused(EFORMAT, "marker")
            continue
        if pos + 2 > len(data):
            raise Refused(EFORMAT, "segment")
        n = int.from_bytes(data[pos:pos + 2], "big")
        if n < 2 or pos + n > len(data):
            raise Refused(EFORMAT, "segment")
        body = data[pos + 2:pos + n]
        pos += n
        if m == 0xDB:
            if scans:
                raise Refused(ENOTSUP, "dqt")
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
                if ntables >= TABLES_MAX:
                    raise Refused(ENOTSUP, "tables")
                if cls == 0 and any(v > 15 for v in vals):
                    raise Refused(EFORMAT, "dht")
                (tac if cls else tdc)[slot] = dc._tables_from(bits, vals)
                ntables += 1
        elif m == 0xC2:
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
            if nc == 3 and sum(h * v for _, h, v, _ in comps) > 10:
                raise Refused(EFORMAT, "mcu")
            frame = {"width": width, "height": height, "components": comps}
        elif 0xC0 <= m <= 0xCF:
            raise Refused(EFORMAT if frame is not None else ENOTSUP, "process")
        elif m == 0xDD:
            if len(body) != 2:
                raise Refused(EFORMAT, "dri")
            ri = int.from_bytes(body, "big")
        elif m in (0xDC, 0xDE, 0xDF):
            raise Refused(ENOTSUP, "dnl" if m == 0xDC else "process")
        elif m == 0xDA:
            if frame is None or len(body) < 1 or len(body) != 4 + 2 * body[0] or body[0] == 0 or body[0] > len(frame["components"]):
                raise Refused(EFORMAT, "sos")
            if len(scans) >= SCANS_MAX:
                raise Refused(ENOTSUP, "scans")
            ns = body[0]
            ss, se, ah, al = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
            ids = [c[0] for c in frame["components"]]
            which, dslots, aslots = [], [], []
            for i in range(ns):
                if body[1 + 2 * i] not in ids:
                    raise Refused(EFORMAT, "sos")
                o = len(ids) - 1 - ids[::-1].index(body[1 + 2 * i])
                if which and o <= which[-1]:
                    raise Refused(ENOTSUP, "order")
                which.append(o)
                dslots.append(body[2 + 2 * i] >> 4)
                aslots.append(body[2 + 2 * i] & 15)
                if dslots[-1] > 3 or aslots[-1] > 3:
                    raise Refused(EFORMAT, "sos")
            if (se != 0) if ss == 0 else (ns != 1 or se < ss or se > 63):
                raise Refused(EFORMAT, "progression")
            if al > 13 or (ah != 0 and ah != al + 1):
                raise Refused(EFORMAT, "progression")
            grids, mcus_w, mcus_h = dc.geometry(frame)
            for i, o in enumerate(which):
                if ss and (o, 0) not in last_al:
                    raise Refused(EFORMAT, "progression")
                for k in range(ss, se + 1):
                    if ah != last_al.get((o, k), 0) or ((o, k) in last_al and ah == 0):
                        raise Refused(EFORMAT, "progression")
                    last_al[(o, k)] = al
                if ss == 0 and ah == 0 and dslots[i] not in tdc:
                    raise Refused(EFORMAT, "missing table")
                if ss and aslots[i] not in tac:
                    raise Refused(EFORMAT, "missing table")
            if ns == 1:
                units = grids[which[0]][0] * grids[which[0]][1]
                blocks = units
            else:
                units = mcus_w * mcus_h
                per = sum(grids[o][2] * grids[o][3] for o in which)
                if per > 10:
                    raise Refused(EFORMAT, "mcu")
                blocks = units * per
            end = _data_end(data, pos)
            nbytes, nint = end - pos, -(-units // ri) if ri else 1
            if nbytes * 8 < (-(-blocks // 32767) if ss else blocks) or nint - 1 > nbytes // 2:
                raise Refused(EFORMAT, "truncated")
            if not scans:
                for _, _, _, tq in frame["components"]:
                    if tq not in quant:
                        raise Refused(EFORMAT, "missing table")
                frame.update(restart_interval=ri, scan_begin=pos)
            scans.append({"components": which, "ss": ss, "se": se, "ah": ah, "al": al, "dc_slots": dslots, "ac_slots": aslots, "restart_interval": ri,
                          "intervals": nint, "begin": pos, "end": end, "dc": dict(tdc), "ac": dict(tac)})
            pos = end
    frame.update(quant=quant, scan_end=scans[-1]["end"], progressive=True, scans=scans, intervals=sum(s["intervals"] for s in scans))
    return frame


def _raw(rd, n):
    """n bits as an unsigned number"""
    v = 0
    for _ in range(n):
        v = (v << 1) | rd.bit()
    return v


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _scan_blocks(scan, grids, mcus_w, mcus_h):
    """per unit (MCU, or block of a one-component scan) of the scan: [(component, block row, block column or None for padding)]"""
    which = scan["components"]
    if len(which) == 1:
        gh, gw = grids[which[0]][:2]
        return [[(which[0], y, x)] for y in range(gh) for x in range(gw)]
    out = []
    for my in range(mcus_h):
        for mx in range(mcus_w):
            unit = []
            for o in which:
                gh, gw, h, v = grids[o]
                for j in range(h * v):
                    by, bx = my * v + j // h, mx * h + j % h
                    unit.append((o, by, bx) if by < gh and bx < gw else (o, None, None))
            out.append(unit)
    return out


def _refine_block(rd, table, block, ss, se, al, eobrun):
    """libjpeg's decode_mcu_AC_refine on one block (zigzag order, a list); returns the EOB run left"""
    p1, m1 = 1 << al, -(1 << al)

    def correct(k):
        if rd.bit() and (block[k] & p1) == 0:
            block[k] += p1 if block[k] >= 0 else m1

    k = ss
    if eobrun == 0:
        while k <= se:
            rs = rd.symbol(table)
            r, s = rs >> 4, rs & 15
            if s:
                if s != 1:
                    raise Refused(EFORMAT, "refine")
                s = p1 if rd.bit() else m1
            elif r != 15:
                eobrun = (1 << r) + _raw(rd, r)
                break
            found = False
            while k <= se:
                if block[k] != 0:
                    correct(k)
                else:
                    r -= 1
                    if r < 0:
                        found = True
                        break
                k += 1
            if not found:
                raise Refused(EFORMAT, "run")
            if s:
                block[k] = s
            k += 1
    if eobrun > 0:
        while k <= se:
            if block[k] != 0:
                correct(k)
            k += 1
        eobrun -= 1
    return eobrun


def decode(data):
    data = bytes(data)
    p = parse_scans(data)
    if not p["progressive"]:
        return dc.decode(data)[0], p
    grids, mcus_w, mcus_h = dc.geometry(p)
    zz = [[[[0] * 64 for _ in range(gw)] for _ in range(gh)] for gh, gw, _, _ in grids]
    for scan in p["scans"]:
        ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
        units = _scan_blocks(scan, grids, mcus_w, mcus_h)
        ri = scan["restart_interval"] or len(units)
        chunks, numbers = dc._intervals(data[scan["begin"]:scan["end"]])
        if len(chunks) != -(-len(units) // ri) or numbers != [k % 8 for k in range(len(numbers))]:
            raise Refused(EFORMAT, "restart")
        slot_of = dict(zip(scan["components"], zip(scan["dc_slots"], scan["ac_slots"])))
        for k, chunk in enumerate(chunks):
            rd, pred, eobrun = dc._Reader(chunk), {}, 0
            for unit in units[k * ri:(k + 1) * ri]:
                for c, by, bx in unit:
                    block = zz[c][by][bx] if by is not None else [0] * 64
                    if ss == 0 and ah == 0:
                        pred[c] = pred.get(c, 0) + rd.value(rd.symbol(scan["dc"][slot_of[c][0]]))
                        if not -32768 <= pred[c] << al <= 32767:
                            raise Refused(EFORMAT, "dc")
                        block[0] = pred[c] << al
                    elif ss == 0:
                        if rd.bit():
                            block[0] = _wrap16(block[0] | (1 << al))
                    elif ah == 0:
                        if eobrun > 0:
                            eobrun -= 1
                            continue
                        table, pos = scan["ac"][slot_of[c][1]], ss
                        while pos <= se:
                            rs = rd.symbol(table)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    eobrun = (1 << r) + _raw(rd, r) - 1
                                    break
                                pos += 16
                                if pos > se + 1:
                                    raise Refused(EFORMAT, "run")
                                continue
                            pos += r
                            v = rd.value(s)
                            if pos > se:
                                raise Refused(EFORMAT, "run")
                            block[pos] = _wrap16(v << al)
                            pos += 1
                    else:
                        eobrun = _refine_block(rd, scan["ac"][slot_of[c][1]], block, ss, se, al, eobrun)
            if eobrun > 0:
                raise Refused(EFORMAT, "eobrun")
            if rd.pos > rd.n or rd.n - rd.pos >= 8:
                raise Refused(EFORMAT, "leftover")
    arrays = []
    for plane in zz:
        a = np.array(plane, dtype=np.int64).astype(np.int16)
        nat = np.zeros_like(a)
        nat[:, :, ec.ZIGZAG] = a
        arrays.append(nat)
    return arrays, p


# ---- the writer ----
SPECTRAL = {1: [((0,), 0, 0, 0, 0), ((0,), 1, 1, 0, 0), ((0,), 2, 5, 0, 0), ((0,), 6, 63, 0, 0)],
            3: [((0, 1, 2), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in range(3) for a, b in ((1, 1), (2, 5), (6, 63))]}
DC_ALONE = {3: [((0,), 0, 0, 0, 1), ((1,), 0, 0, 0, 1), ((2,), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((0,), 1, 63, 0, 1), ((2,), 1, 63, 0, 0),
                ((1,), 0, 0, 1, 0), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]}
REFINE_3 = {1: [((0,), 0, 0, 0, 3), ((0,), 1, 63, 0, 3), ((0,), 0, 0, 3, 2), ((0,), 1, 63, 3, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 2, 1),
                ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)],
            3: [((0, 1, 2), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in range(3)] +
               [s for al in (2, 1, 0) for s in [((0, 1, 2), 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in range(3)]]}
STOPS_AT_1 = {1: [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 2), ((0,), 1, 63, 2, 1)],
              3: [((0, 1, 2), 0, 0, 0, 1)] + [((c,), 1, 63, 0, 2) for c in range(3)] + [((c,), 1, 63, 2, 1) for c in range(3)]}


def _scan_units(zz, width, height, sub, comps):
    """per unit of a scan (an MCU of an interleaved scan, a block of the own grid of a one-component scan): [(component, block in
    zigzag order, None for a block that pads the grid out to whole MCUs)]"""
    if len(comps) == 1:
        return [[(comps[0], block)] for row in zz[comps[0]] for block in row]
    order = ec.scan_order(width, height, len(zz), sub)
    per = sub[0] * sub[1] + 2
    return [[(c, None if y is None else zz[c][y][x]) for c, y, x in order[at:at + per]] for at in range(0, len(order), per)]


def scan_intervals(zz, width, height, sub, scan, ri=0):
    """[(operations, EOB runs as (first block of the scan, length, why), ZRLs)] per restart interval of one scan: ri of the scan's
    units each (0: one interval).  Every interval is walked on its own by the coder's restatement, so the pending EOB run is
    flushed with its waiting correction bits and the DC predictors start at 0; a padding block repeats its predecessor's DC"""
    comps, ss, se, ah, al = scan
    units = _scan_units(zz, width, height, sub, comps)
    ri = ri if 0 < ri < len(units) else len(units)
    values, last = [], [0, 0, 0]
    if ss == 0:
        for unit in units:
            row = []
            for c, block in unit:
                if block is not None:
                    last[c] = block[0]
                row.append((c, last[c] >> al))
            values.append(row)
    out = []
    for first in range(0, len(units), ri):
        ops, runs, zrls = [], [], 0
        if ss == 0:
            pc.dc_slice([v for row in values[first:first + ri] for v in row], ah, ops)
        else:
            blocks = [unit[0][1] for unit in units[first:first + ri]]
            table = ("ac", min(comps[0], 1))
            if ah:
                zrls = pc._ac_refine(blocks, table, ss, se, al, ops, runs)
            else:
                pc._ac_first(blocks, table, ss, se, al, ops, runs)
        out.append((ops, [(first + b, n, why) for b, n, why in runs], zrls))
    return out


def write(coefficients, width, height, quant, sub=(1, 1), script=None, mutate=None, restart=None, dri=None, fill=None, report=None):
    """restart = n: one DRI segment of n in front of the first SOS; dri = {scan index: n}: one in front of that scan's tables and
    SOS (0 turns restarts off from there on).  The interval counts the scan's own units (scan_intervals); behind each but the last
    the stream is padded with ones to a byte and RSTn follows, n counted modulo 8.
    fill = {scan index: {"targets": [...], "fixed": {m: n}}}: FF fill bytes in front of that scan's restart markers, as
    decode_cases.place_markers puts them: targets[m] (None, or no entry: none) is what the offset of marker m's Dn byte, counted
    from the scan's begin, is congruent to modulo 256; fixed[m] is a number of fill bytes.
    mutate(index, operations) -> operations: what damaged_cases() spoil a scan with; where a restart interval is in force the scan
    is given interval by interval, and index is (scan index, interval).
    report (a list) receives per scan {"scan", "restart_interval", "intervals": [{"runs", "zrls", "operations", "bits", "bytes"}]}:
    what scan_intervals gave (after mutate), the interval's bits before padding and its bytes after stuffing"""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    script = pc.SCANS[ncomp] if script is None else script
    zz = [np.asarray(a).reshape(gh, gw, 64)[:, :, ec.ZIGZAG].tolist() for a, (gh, gw) in zip(coefficients, ec.grids(width, height, ncomp, sub))]
    plain = ec.header(width, height, ncomp, sub, quant)
    sof, dht = plain.index(b"\xff\xc0"), plain.index(b"\xff\xc4")
    file = bytearray(plain[:sof] + b"\xff\xc2" + plain[sof + 2:dht])
    changes = dict(dri or {})
    if restart:
        changes[0] = restart
    ri = 0
    for index, scan in enumerate(script):
        if index in changes:
            ri = changes[index]
            file += ec._segment(0xdd, bytes([ri >> 8, ri & 255]))
        intervals = scan_intervals(zz, width, height, sub, scan, ri)
        if mutate is not None:
            intervals = [(mutate((index, k) if ri else index, ops), runs, zrls) for k, (ops, runs, zrls) in enumerate(intervals)]
        counts = {}
        for ops, _runs, _zrls in intervals:
            for op in ops:
                if op[0] == "s":
                    counts.setdefault(op[1], [0] * 256)[op[2]] += 1
        codes = {}
        for t, count in counts.items():
            bits, vals, _longest = hc.table(count)
            file += ec._segment(0xc4, bytes([((t[0] == "ac") << 4) | t[1]]) + bytes(bits) + bytes(vals))
            codes[t] = ec._codes(bits, vals)
        file += pc._sos(scan)
        places = (fill or {}).get(index, {})
        targets, fixed = places.get("targets", ()), places.get("fixed", {})
        data, told = bytearray(), []
        for k, (ops, runs, zrls) in enumerate(intervals):
            if k:
                m = k - 1
                if m in fixed:
                    data += b"\xff" * fixed[m]
                elif m < len(targets) and targets[m] is not None:
                    data += b"\xff" * ((targets[m] - (len(data) + 1)) % 256)
                data += bytes([0xff, 0xd0 + m % 8])
            out = ec._Bits()
            for op in ops:
                if op[0] == "s":
                    out.put(*codes[op[1]][op[2]])
                else:
                    out.put(op[1], op[2])
            nbits = out.n
            short = -out.n % 8
            out.put((1 << short) - 1, short)
            chunk = bytes(out.data).replace(b"\xff", b"\xff\x00")
            data += chunk
            told.append({"runs": runs, "zrls": zrls, "operations": ops, "bits": nbits, "bytes": len(chunk)})
        file += data
        if report is not None:
            report.append({"scan": scan, "restart_interval": ri, "intervals": told})
    return bytes(file + b"\xff\xd9")


def write_case(case, script=None, mutate=None, **kw):
    return write(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], script, mutate, **kw)


# ---- the cases ----
def pil_files():
    """{name: file}: PIL-made progressive files — grey, 4:4:4, 4:2:2, 4:2:0; five sizes; four qualities; plain and with restarts"""
    import io
    from PIL import Image
    from jpeg2png_amd import synth
    out = {}
    forms = [("plain", {}), ("rst_blocks", {"restart_marker_blocks": 3}), ("rst_rows", {"restart_marker_rows": 1})]
    for w, h in ((8, 8), (16, 8), (41, 23), (45, 38), (83, 61)):
        rgb = synth.synth_rgb(w, h, 5 * w + h).astype(np.uint8)
        for quality in (30, 75, 95, 100):
            for mode, sub in (("L", 0), ("RGB", 0), ("RGB", 1), ("RGB", 2)):
                for name, kw in forms:
                    buf = io.BytesIO()
                    Image.fromarray(rgb, "RGB").convert(mode).save(buf, "JPEG", quality=quality, progressive=True,
                                                                   **({"subsampling": sub} if mode == "RGB" else {}), **kw)
                    out[f"pil_{w}x{h}_q{quality}_{mode}{sub}_{name}"] = buf.getvalue()
    return out


def _single_coefficient_script(ncomp):
    """DC, then every AC coefficient of every component in a scan of its own"""
    return [(tuple(range(ncomp)), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(ncomp) for k in range(1, 64)]


GREY_128 = [((0,), 0, 0, 0, 1)] + [((0,), k, k, 0, 1) for k in range(1, 64)] + [((0,), 0, 0, 1, 0)] + [((0,), k, k, 1, 0) for k in range(1, 64)]


def _stopped(case, script):
    """what a script that stops above Al = 0 leaves of the case's coefficients"""
    left = {}
    for comps, ss, se, _ah, al in script:
        for c in comps:
            for k in range(ss, se + 1):
                left[(c, k)] = al
    out = []
    for c, a in enumerate(case["coefficients"]):
        a = np.asarray(a).astype(np.int64)
        zz = a.reshape(-1, 64)[:, ec.ZIGZAG]
        res = np.zeros_like(zz)
        for k in range(64):
            al = left.get((c, k))
            if al is None:
                continue
            v = zz[:, k]
            res[:, k] = (v >> al) << al if k == 0 else np.sign(v) * ((np.abs(v) >> al) << al)
        nat = np.zeros_like(res)
        nat[:, ec.ZIGZAG] = res
        out.append(nat.reshape(a.shape).astype(np.int16))
    return out


def written_cases():
    """{name: (file, the coefficients it must decode to)}: writer-made scripts"""
    grey = ec.make(41, 23, 1, (1, 1), "sparse", seed=11)
    c420 = ec.make(41, 23, 3, (2, 2), "sparse", seed=12)
    c422 = ec.make(40, 24, 3, (2, 1), "dense", seed=13)
    c444 = ec.make(24, 16, 3, (1, 1), "sparse", seed=14)
    dummy = ec.make(17, 9, 3, (2, 2), "dense", seed=15)
    tiny = ec.make(16, 8, 1, (1, 1), "dense", seed=16)
    plans = {"spectral_grey": (grey, SPECTRAL[1]), "spectral_420": (c420, SPECTRAL[3]), "dc_alone_420": (c420, DC_ALONE[3]),
             "dc_alone_17x9": (dummy, DC_ALONE[3]), "refine_3_grey": (grey, REFINE_3[1]), "refine_3_422": (c422, REFINE_3[3]),
             "refine_3_tiny": (tiny, REFINE_3[1]), "stops_at_1_grey": (grey, STOPS_AT_1[1]), "stops_at_1_444": (c444, STOPS_AT_1[3]),
             "dummy_blocks_17x9": (dummy, None), "scans_128_grey": (tiny, GREY_128)}
    return {name: (write_case(case, script), _stopped(case, script if script is not None else pc.SCANS[len(case["coefficients"])]))
            for name, (case, script) in plans.items()}


# ---- files of one scan's data taken apart: where the unstuffing kernels lay their chunks and lanes from the scan's own begin ----
def scan_chunks(data, index):
    """the entropy-coded data of scan `index`, still stuffed, cut at its RSTn markers (a file without fill bytes)"""
    s = parse_scans(data)["scans"][index]
    ecs, out, cur, i = data[s["begin"]:s["end"]], [], bytearray(), 0
    while i < len(ecs):
        if ecs[i] == 0xFF and 0xD0 <= ecs[i + 1] <= 0xD7:
            out.append(bytes(cur))
            cur = bytearray()
        else:
            cur += ecs[i:i + 2] if ecs[i] == 0xFF else ecs[i:i + 1]
        i += 2 if ecs[i] == 0xFF else 1
    return out + [bytes(cur)]


def with_chunks(data, index, chunks):
    """the file with scan `index`'s data replaced by these chunks, RSTn between them numbered in sequence"""
    s = parse_scans(data)["scans"][index]
    return data[:s["begin"]] + b"".join((bytes([0xff, 0xd0 + (k - 1) % 8]) if k else b"") + c for k, c in enumerate(chunks)) + data[s["end"]:]


def scan_marker_offsets(data, index):
    """decode_cases.marker_offsets of one scan: the offset, counted from the scan's begin, of the Dn byte of each of its RSTn"""
    s = parse_scans(data)["scans"][index]
    out, i = [], s["begin"]
    while i < s["end"]:
        if data[i] != 0xFF:
            i += 1
        elif data[i + 1] == 0:
            i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            out.append(i + 1 - s["begin"])
            i += 2
        else:
            i += 1                       # a fill byte
    return out


def scan_stuffed_on_chunk_edge(data, index):
    """decode_cases.stuffed_on_chunk_edge of one scan"""
    s = parse_scans(data)["scans"][index]
    ecs = data[s["begin"]:s["end"]]
    return [i for i in range(255, len(ecs) - 1, 256) if ecs[i] == 0xFF and ecs[i + 1] == 0]


def scan_blank_chunks(data, index):
    """decode_cases.blank_chunks of one scan"""
    s = parse_scans(data)["scans"][index]
    ecs = data[s["begin"]:s["end"]]
    return [c for c in range(len(ecs) // 256) if ecs[256 * c:256 * c + 256] == b"\xff" * 256]


# ---- good files aimed at where the kernels divide their work, and at what a restart interval ends ----
SPLIT = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 5, 1, 0), ((0,), 6, 63, 1, 0)]
FROM_13 = [((0,), 0, 0, 0, 13), ((0,), 1, 63, 0, 13)] + [s for al in range(12, -1, -1) for s in (((0,), 0, 0, al + 1, al), ((0,), 1, 63, al + 1, al))]
MOD4_RESTARTS = {1: 4, 2: 10, 3: 7}     # 18 blocks: 5 intervals (the last of 2 blocks), 2 (8), 3 (4)
DIRECTED_KINDS = "BACBAB"               # the kinds of directed_case()'s intervals of four blocks; the last has two
EDGE_SCANS = (1, 5)                     # of progressive_cases.SCANS[3]: luma's first AC scan (1..5) and its AC refinement scan (Al 2 to 1)


def directed_case():
    """grey 176x8: 22 blocks, with restart=4 five intervals of four blocks and one of two, written with SPLIT (the AC band in two,
    first at Al 1, then refined).  In the band 6..63 (zigzag positions; c: 4..7 with either sign, which is new in the first scan
    and a correction bit in the refinement scan) the four blocks of an interval of kind
      A: c at 6 | 1 at 10 | nothing | nothing: the first scan ends in an EOB run of 4, the refinement scan in one of 3
      B: c at 6 | c at 7 and 12..19 | c at 8 | nothing: the first scan ends in a run of 2, the refinement scan is ONE run of 4 that
         carries 11 waiting correction bits of three blocks
      C: as B, but the first and the last block hold c at 6 and 1 at 63: the first scan ends in a run of 1, the refinement scan
         begins with three ZRLs and the interval's rarest symbol, flushes a run of 2 with ten waiting bits and ends in no run at all
    In the band 1..5 every block holds 3 at 1 and -2 at 2, but blocks 8 and 9, the first of the middle interval: block 8 holds 1 at
    5 alone (the refinement scan codes it as run 4, size 1: no position is left behind it), block 9 holds c at 5 alone (the first
    scan codes it as run 4, size 2)"""
    case = ec.make(176, 8, 1, (1, 1), "zero")
    rng = np.random.default_rng(26)

    def c():
        return int(rng.integers(4, 8)) * (1 if rng.random() < 0.5 else -1)
    for k, kind in enumerate(DIRECTED_KINDS):
        blocks = [{6: c(), 63: 1} if kind == "C" else {6: c()}, {10: 1} if kind == "A" else {p: c() for p in (7, 12, 13, 14, 15, 16, 17, 18, 19)}, {} if kind == "A" else {8: c()},
                  {6: c(), 63: 1} if kind == "C" else {}]
        for i, values in enumerate(blocks[:22 - 4 * k]):
            b = 4 * k + i
            values.update({5: 1} if b == 8 else {5: c()} if b == 9 else {1: 3, 2: -2})
            values[0] = 2 * int(rng.integers(-100, 100)) + (b % 3 == 0)        # (its last bit: no byte of a DC refinement scan is FF)
            pc._put(case, b, values)
    return case


def _dc_scan_file(diffs, al):
    """a grey file of len(diffs) blocks in a row and one scan, DC at Al = al, that codes these differences whatever their sum is (in
    the manner of decode_cases._dc_file) -> (file, the DC values << al)"""
    def ops_of(_index, _ops):
        ops = []
        for d in diffs:
            s = abs(d).bit_length()
            ops.append(("s", ("dc", 0), s))
            pc._magnitude(ops, d, s)
        return ops
    zero = ec.make(8 * len(diffs), 8, 1, (1, 1), "zero")
    return write_case(zero, [((0,), 0, 0, 0, al)], ops_of), np.cumsum(diffs) * (1 << al)


DC_LIMIT_DIFFS = {0: [16383, 16383, 1, -16383, -16383, -16383, -16383, -3], 1: [8191, 8191, 1, -8191, -8191, -8191, -8191, -3]}


def _from_13_case():
    """grey 16x8: both signs of the int16 range with |v| >> 13 <= 3, values that appear at every Al from 13 down, and a 1 at 63"""
    case = ec.make(16, 8, 1, (1, 1), "zero")
    pc._put(case, 0, {0: 32767, 1: 32767, 2: -32767, 3: 8192, 4: -8192, 5: -8191, 9: 16384, 10: -24575, 62: 21845, 63: 1})
    pc._put(case, 1, {0: -32768, 1: -32767, 2: 32767, 63: -10923})
    for al in range(13):
        pc._put(case, 1, {20 + 2 * al: (1 << al) * (-1) ** al, 21 + 2 * al: (3 << al) - 1})
    return case


def _edges_colour_case():
    """(case, file, fills): 24 MCUs of dense 4:4:4 written with restart=1, the markers of the scans EDGE_SCANS moved onto
    decode_cases.EDGE_TARGETS counted from their own scan's begin; the seed is the first for which a stuffed FF | 00 then lies across a
    chunk edge of a scan that is not the file's first"""
    targets = [dc.EDGE_TARGETS[m % 6] for m in range(23)]
    fills = {index: {"targets": targets} for index in EDGE_SCANS}
    for seed in range(1, 400):
        case = ec.make(48, 32, 3, (1, 1), "dense", seed=seed, quality=95)
        data = write_case(case, restart=1, fill=fills)
        if any(scan_stuffed_on_chunk_edge(data, index) for index in range(1, len(pc.SCANS[3]))):
            return case, data, fills
    raise AssertionError("no seed puts a stuffed FF on a chunk edge of a later scan")


def edge_cases():
    """{name: (file, the coefficients it must decode to, or None where only the restatement says)}"""
    if "edge" in _cache:
        return _cache["edge"]
    out = {}

    def add(name, case, script, **kw):
        out[name] = (write_case(case, script, **kw), _stopped(case, script if script is not None else pc.SCANS[len(case["coefficients"])]))
    grey = ec.make(41, 23, 1, (1, 1), "sparse", seed=11)
    c420 = ec.make(41, 23, 3, (2, 2), "sparse", seed=12)
    c422 = ec.make(40, 24, 3, (2, 1), "dense", seed=13)
    c444 = ec.make(24, 16, 3, (1, 1), "sparse", seed=14)
    dummy = ec.make(17, 9, 3, (2, 2), "dense", seed=15)
    wide = ec.make(2056, 8, 1, (1, 1), "sparse", seed=41)
    add("intervals_257_grey", wide, SPECTRAL[1], restart=1)
    add("refine_257_grey", wide, REFINE_3[1], restart=1)
    for residue, restart in MOD4_RESTARTS.items():
        add(f"refine_intervals_mod4_{residue}", grey, REFINE_3[1], restart=restart)
    add("refine_3_422_rst", c422, REFINE_3[3], restart=3)
    add("dc_alone_420_rst", c420, DC_ALONE[3], restart=2)
    add("stops_at_1_444_rst", c444, STOPS_AT_1[3], restart=3)
    add("dummy_blocks_17x9_rst", dummy, None, restart=2)
    add("dri_between_grids_420", c420, None, restart=8)
    add("dri_changes", c420, None, dri={0: 2, 1: 5, 7: 0})
    add("eob_run_ends_each_interval", directed_case(), SPLIT, restart=4)
    case, data, fills = _edges_colour_case()
    out["markers_on_edges_scan_k"] = (data, _stopped(case, pc.SCANS[3]))
    # 600 fill bytes cover two whole chunks when they begin in a chunk's first 89 bytes: the first marker of the middle for which they do
    filled = [write_case(case, restart=1, fill={EDGE_SCANS[1]: {"fixed": {m: 600}}}) for m in range(4, 20)]
    filled = [f for f in filled if len(scan_blank_chunks(f, EDGE_SCANS[1])) == 2]
    if not filled:
        raise AssertionError("no marker of the refinement scan begins 600 fill bytes in a chunk's first 89 bytes")
    out["fill_covers_chunks_scan_k"] = (filled[0], _stopped(case, pc.SCANS[3]))
    add("refine_from_13", _from_13_case(), FROM_13)
    for al, diffs in DC_LIMIT_DIFFS.items():
        data, values = _dc_scan_file(diffs, al)
        want = np.zeros((1, len(diffs), 64), np.int16)
        want[0, :, 0] = values
        out[f"dc_near_limit_al{al}"] = (data, [want])
    three = ec.make(24, 8, 1, (1, 1), "zero")
    three["coefficients"][0][0, :, 0] = 30000
    add("dc_reset_by_restart", three, SPECTRAL[1], restart=1)
    _cache["edge"] = out
    return out


_cache = {}


def good_files():
    """{name: file}: every good progressive file the tests share (made once a process)"""
    if "files" not in _cache:
        out = dict(pil_files())
        out.update({f"coder_{name}": pc.encode_case(case)[0] for name, case in pc.gpu_cases().items()})
        out.update({f"written_{name}": data for name, (data, _want) in written_cases().items()})
        out.update({f"edge_{name}": data for name, (data, _want) in edge_cases().items()})
        _cache["files"] = out
    return _cache["files"]


def expected(name):
    """the restatement's decode of good_files()[name] (made once a process, never changed)"""
    key = ("want", name)
    if key not in _cache:
        arrays, _ = decode(good_files()[name])
        for a in arrays:
            a.setflags(write=False)
        _cache[key] = arrays
    return _cache[key]


def _patch_sos(data, index, ss=None, se=None, ahal=None):
    """the file with scan `index`'s Ss, Se, Ah/Al bytes replaced"""
    at = parse_scans(data)["scans"][index]["begin"]
    out = bytearray(data)
    for off, v in ((-3, ss), (-2, se), (-1, ahal)):
        if v is not None:
            out[at + off] = v
    return bytes(out)


def header_refusals():
    """{name: (file, code)}: what the marker segments alone show"""
    grey = write_case(ec.make(16, 8, 1, (1, 1), "dense", seed=16))                 # pc.SCANS[1]
    colour = write_case(ec.make(16, 16, 3, (2, 2), "sparse", seed=3))              # pc.SCANS[3]
    alone = write_case(ec.make(16, 16, 3, (2, 2), "sparse", seed=3), DC_ALONE[3])
    scans = parse_scans(grey)["scans"]
    second_sos = grey.rindex(b"\xff\xda", 0, scans[1]["begin"])
    dqt = grey.index(b"\xff\xdb")
    dqt_segment = grey[dqt:dqt + 2 + int.from_bytes(grey[dqt + 2:dqt + 4], "big")]
    dht = grey.index(b"\xff\xc4", scans[0]["end"])
    many = write_case(ec.make(8, 8, 3, (1, 1), "sparse", seed=2), _single_coefficient_script(3))
    return {
        "dc_scan_with_se": (_patch_sos(grey, 0, se=5), EFORMAT),
        "ac_se_below_ss": (_patch_sos(grey, 1, ss=5, se=1), EFORMAT),
        "se_64": (_patch_sos(grey, 2, se=64), EFORMAT),
        "al_14": (_patch_sos(grey, 0, ahal=0x0e), EFORMAT),
        "ah_is_not_al_plus_1": (_patch_sos(grey, 3, ahal=0x31), EFORMAT),
        "first_scan_with_ah": (_patch_sos(grey, 0, ahal=0x21), EFORMAT),
        "refinement_of_another_al": (_patch_sos(grey, 1, ahal=0x03), EFORMAT),
        "first_scan_twice": (_patch_sos(grey, 3, ahal=0x02), EFORMAT),
        "ac_before_dc": (_patch_sos(grey, 0, ss=1, se=1), EFORMAT),
        "ac_scan_of_three_components": (_patch_sos(colour, 0, ss=1, se=5), EFORMAT),
        "scans_129": (many, ENOTSUP),
        "dqt_behind_sos": (grey[:second_sos] + dqt_segment + grey[second_sos:], ENOTSUP),
        "multi_scan_sof0": (alone.replace(b"\xff\xc2", b"\xff\xc0", 1), ENOTSUP),
        "truncated_segment": (grey[:dht + 9], EFORMAT),
        "no_eoi": (grey[:-2], EFORMAT),
    }


def damaged_cases():
    """{name: (file, why the restatement refuses it)}: files whose marker segments are in order and whose data is not"""
    grey = ec.make(41, 23, 1, (1, 1), "sparse", seed=11)
    good = write_case(grey)
    scans = parse_scans(good)["scans"]
    out = {"scan_cut_short": (good[:scans[1]["end"] - 2] + good[scans[1]["end"]:], ("truncated", "code", "leftover", "run", "eobrun"))}
    # two blocks of zeros: every AC scan is the symbol EOB1 and one extra bit, 0 for a run of 2; set, the run is 3
    zero = {"coefficients": [np.zeros((1, 2, 64), np.int16)], "width": 16, "height": 8, "quant": grey["quant"], "sub": (1, 1)}

    def longer(index, ops):
        return [("b", 1, 1) if index == 1 and op == ("b", 0, 1) else op for op in ops]

    out["eob_run_one_too_long"] = (write_case(zero, None, longer), ("eobrun",))

    def first_symbol(want_index, change):
        def mutate(index, ops):
            ops = list(ops)
            if index == want_index:
                at = next(i for i, op in enumerate(ops) if op[0] == "s" and op[2] & 15)
                ops[at] = ("s", ops[at][1], change(ops[at][2]))
            return ops
        return mutate

    out["refinement_symbol_of_two_bits"] = (write_case(grey, None, first_symbol(3, lambda rs: (rs & 0xf0) | 2)), ("refine",))
    out["run_past_se"] = (write_case(grey, None, first_symbol(1, lambda rs: 0xf0 | (rs & 15))), ("run",))
    pil = good_files()["pil_41x23_q75_L0_rst_blocks"]
    ac = next(s for s in parse_scans(pil)["scans"] if s["ss"])
    at = pil.index(b"\xff\xd1", ac["begin"], ac["end"])
    out["restart_out_of_sequence"] = (pil[:at + 1] + b"\xd2" + pil[at + 2:], ("restart",))
    out["byte_behind_dc_refinement"] = (good[:scans[4]["end"]] + b"\x55" + good[scans[4]["end"]:], ("leftover",))
    out.update(_damaged_in_one_kernel())
    return out


def _symbol_at(ops, pick):
    """the index of the last operation that is a symbol for which pick(symbol) holds"""
    return max(i for i, op in enumerate(ops) if op[0] == "s" and pick(op[2]))


def _run_one_longer(where):
    """mutate: in the scan and interval `where`, the last EOBn symbol's extra bits count one block more (the symbol stays: the run
    is no power of two less one)"""
    def mutate(index, ops):
        ops = list(ops)
        if index == where:
            at = _symbol_at(ops, lambda rs: rs & 15 == 0 and 1 <= rs >> 4 < 15)
            _b, value, length = ops[at + 1]
            assert length == ops[at][2] >> 4 and value + 1 < 1 << length, ops[at:at + 2]
            ops[at + 1] = ("b", value + 1, length)
        return ops
    return mutate


def _symbol_swapped(where, old, new, drop_bits):
    """mutate: in the scan and interval `where` the one symbol `old` becomes `new`; drop_bits: and loses the bits behind it"""
    def mutate(index, ops):
        ops = list(ops)
        if index == where:
            at = [i for i, op in enumerate(ops) if op[0] == "s" and op[2] == old]
            assert len(at) == 1, (where, old, at)
            ops[at[0]] = ("s", ops[at[0]][1], new)
            if drop_bits:
                assert ops[at[0] + 1][0] == "b"
                del ops[at[0] + 1]
        return ops
    return mutate


# of directed_case() written with SPLIT and restart=4: the scans, and the intervals that are neither a scan's first nor its last
_DC_REFINE, _AC_REFINE_LOW, _AC_FIRST_LOW, _AC_FIRST, _AC_REFINE = 3, 4, 1, 2, 5
_KIND_A, _KIND_C, _KIND_B = 1, 2, 3


def _damaged_in_one_kernel():
    """{name: (file, (why,))}: files that both parsers accept and that have ONE fault, which one kernel alone can see (the name of
    the kernel in front): everything else in them is whole, and the faults sit in a middle interval of a scan with restarts"""
    out = {}
    # k_scans_dc: the neighbours of dc_near_limit_al0 and _al1, one step over
    for al, diffs in DC_LIMIT_DIFFS.items():
        out[f"dc_above_int16_al{al}"] = (_dc_scan_file(diffs[:2] + [2] + diffs[3:], al)[0], ("dc",))
        out[f"dc_below_int16_al{al}"] = (_dc_scan_file(diffs[:-1] + [-4], al)[0], ("dc",))
    case = directed_case()
    good = write_case(case, SPLIT, restart=4)
    # k_scans_dc_refine: 12 and 10 blocks an interval are two bytes each; the first gives its second byte to the next
    twelve = write_case(case, SPLIT, restart=12)
    a, b = scan_chunks(twelve, _DC_REFINE)
    assert len(a) == len(b) == 2 and 0xFF not in a + b
    out["dc_refine_interval_short_next_long"] = (with_chunks(twelve, _DC_REFINE, [a[:1], a[1:] + b]), ("truncated",))
    chunks = scan_chunks(good, _DC_REFINE)
    assert len(chunks) == 6
    # (the short interval alone would show only one direction of the length check: here an interval is a byte long and none is short)
    out["dc_refine_byte_behind_interval"] = (with_chunks(good, _DC_REFINE, chunks[:2] + [chunks[2] + b"\x55"] + chunks[3:]), ("leftover",))
    out["dc_refine_rst_removed"] = (with_chunks(good, _DC_REFINE, chunks[:2] + [chunks[2] + chunks[3]] + chunks[4:]), ("restart",))
    at = parse_scans(good)["scans"][_DC_REFINE]["begin"] + scan_marker_offsets(good, _DC_REFINE)[2]
    assert good[at] == 0xD2
    out["dc_refine_rst_renumbered"] = (good[:at] + b"\xd5" + good[at + 1:], ("restart",))
    # k_scans_ac_refine and scans_symbols: symbols and extra bits changed where the writer codes them
    out["eob_run_crosses_restart_refine"] = (write_case(case, SPLIT, _run_one_longer((_AC_REFINE, _KIND_B)), restart=4), ("eobrun",))
    out["eob_run_crosses_restart_first"] = (write_case(case, SPLIT, _run_one_longer((_AC_FIRST, _KIND_A)), restart=4), ("eobrun",))
    out["refine_run_past_band"] = (write_case(case, SPLIT, _symbol_swapped((_AC_REFINE_LOW, _KIND_C), 0x41, 0x51, False), restart=4), ("run",))
    out["refine_zrl_past_band"] = (write_case(case, SPLIT, _symbol_swapped((_AC_REFINE_LOW, _KIND_C), 0x41, 0xf0, True), restart=4), ("run",))
    out["first_zrl_past_band"] = (write_case(case, SPLIT, _symbol_swapped((_AC_FIRST_LOW, _KIND_C), 0x42, 0xf0, True), restart=4), ("run",))
    # k_scans_ac_refine: the bytes of interval 3, one EOB4 symbol, its two extra bits and 11 correction bits
    chunks = scan_chunks(good, _AC_REFINE)
    k = _KIND_B
    assert len(chunks) == 6 and len(chunks[k]) == 2 and 0xFF not in chunks[k]
    out["refine_byte_behind_interval"] = (with_chunks(good, _AC_REFINE, chunks[:k] + [chunks[k] + b"\x55"] + chunks[k + 1:]), ("leftover",))
    out["refine_interval_cut_short"] = (with_chunks(good, _AC_REFINE, chunks[:k] + [chunks[k][:-1]] + chunks[k + 1:]), ("truncated",))
    out["refine_rst_removed"] = (with_chunks(good, _AC_REFINE, chunks[:k] + [chunks[k] + chunks[k + 1]] + chunks[k + 2:]), ("restart",))
    out["refine_rst_doubled"] = (with_chunks(good, _AC_REFINE, chunks[:k] + [b""] + chunks[k:]), ("restart",))
    # a bit flip in a middle interval that leads to a prefix in no table, found by search against the restatement
    for k in (3, 2, 1, 4):
        begin = parse_scans(good)["scans"][_AC_REFINE]["begin"] + sum(len(c) + 2 for c in chunks[:k])
        assert good[begin:begin + len(chunks[k])] == chunks[k]
        for bit in range(8 * len(chunks[k])):
            i = begin + bit // 8
            flipped = good[:i] + bytes([good[i] ^ (0x80 >> (bit % 8))]) + good[i + 1:]
            if flipped[i] == 0xFF or good[i] == 0xFF or good[i - 1] == 0xFF:
                continue
            try:
                decode(flipped)
            except Refused as e:
                if e.why == "code":
                    out["refine_code_in_no_table"] = (flipped, ("code",))
                    return out
    raise AssertionError("no bit of a middle interval, flipped, gives a prefix in no table")
