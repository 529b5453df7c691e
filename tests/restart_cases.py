"""JPEG files with restart intervals (include/jpeg2png_amd.h: "Restart intervals") restated in plain Python on top of
tests/entropy_cases.py (header pieces, scan order, bit writer), tests/huffman_cases.py (the tables), tests/progressive_cases.py (the
scans' walks) and the interval walk of tests/scan_decode_cases.py (scan_intervals), and the cases the tests share
(tests/test_restart_cpu.py checks the restatement against libjpeg with restart_interval / restart_in_rows set,
tests/test_restart_gpu.py the device's coders against the restatement).

plan(...) is the restart plan — units, units per row, interval, intervals and whether a DRI precedes the scan — restated from the
wording alone.  encode_report(...) writes the file of one of the three coders ("baseline", "optimized", "progressive") interval by
interval: every interval is walked on its own into operations, the counts and the coded bits both read that list, and behind every
interval but a scan's last the byte is completed with 1-bits, the FFs are stuffed and FF D0+(k mod 8) follows.  The file layout is
restated here: DHT segments, then the DRI where the interval changed, then the SOS."""
import numpy as np

import entropy_cases as ec
import huffman_cases as hc
import progressive_cases as pc
import scan_decode_cases as sdc

CODERS = ("baseline", "optimized", "progressive")
RESTART_MAX = 65535


def scans_of(ncomp, coder):
    return pc.SCANS[ncomp] if coder == "progressive" else [(tuple(range(ncomp)), 0, 63, 0, 0)]


def plan(width, height, ncomp, sub, coder, n=0, r=0):
    """per scan: dict(units, units_per_row, interval, intervals, dri)"""
    grids = ec.grids(width, height, ncomp, sub if ncomp == 3 else (1, 1))
    out, last = [], 0
    for comps, _ss, _se, _ah, _al in scans_of(ncomp, coder):
        gh, gw = grids[1] if len(comps) == 3 else grids[comps[0]]       # (the chroma grid is the MCU grid)
        interval = n if n else min(r * gw, RESTART_MAX) if r else 0
        out.append({"units": gh * gw, "units_per_row": gw, "interval": interval, "intervals": -(-gh * gw // interval) if interval else 1,
                    "dri": interval != last})
        last = interval
    return out


def _baseline_interval(units):
    """the operations of one interval of the baseline scan: units as scan_decode_cases._scan_units gives them"""
    ops, pred = [], [0, 0, 0]
    for unit in units:
        for c, block in unit:
            t = min(c, 1)
            d = 0
            if block is not None:
                d, pred[c] = block[0] - pred[c], block[0]
            s = abs(d).bit_length()
            ops.append(("s", ("dc", t), s))
            pc._magnitude(ops, d, s)
            r = 0
            for k in range(1, 64):
                v = block[k] if block is not None else 0
                if v == 0:
                    r += 1
                    continue
                while r > 15:
                    ops.append(("s", ("ac", t), 0xf0))
                    r -= 16
                s = abs(v).bit_length()
                ops.append(("s", ("ac", t), (r << 4) | s))
                pc._magnitude(ops, v, s)
                r = 0
            if r > 0:
                ops.append(("s", ("ac", t), 0x00))
    return ops


def intervals_of(zz, width, height, sub, scan, interval):
    """[(operations, EOB runs, ZRLs)] per restart interval of a scan of either kind"""
    comps, ss, se, _ah, _al = scan
    if (ss, se) != (0, 63):
        return sdc.scan_intervals(zz, width, height, sub, scan, interval)
    units = sdc._scan_units(zz, width, height, sub, comps)
    step = interval if 0 < interval < len(units) else len(units)
    return [(_baseline_interval(units[at:at + step]), [], 0) for at in range(0, len(units), step)]


DEFAULT_TABLES = {("dc", t): (ec.DC_BITS[t], ec.DC_VALS, 0) for t in range(2)}
DEFAULT_TABLES.update({("ac", t): (ec.AC_BITS[t], list(ec.AC_VALS[t]), 0) for t in range(2)})


def encode_report(coefficients, width, height, quant, sub=(1, 1), coder="baseline", n=0, r=0):
    """(file, [per scan: dict(scan, plan — its entry of plan() —, counts {table: 256 counts}, tables, bits: before any padding,
    padding: the 1-bits of all intervals, stuffed: FFs that got their 00, markers, eob_runs, runs, intervals: per interval
    dict(bits, pad, data: its bytes before stuffing)])"""
    ncomp = len(coefficients)
    sub = sub if ncomp == 3 else (1, 1)
    zz = [np.asarray(a).reshape(gh, gw, 64)[:, :, ec.ZIGZAG].tolist() for a, (gh, gw) in zip(coefficients, ec.grids(width, height, ncomp, sub))]
    plain = ec.header(width, height, ncomp, sub, quant)
    sof, dht = plain.index(b"\xff\xc0"), plain.index(b"\xff\xc4")
    file = bytearray(plain[:sof] + (b"\xff\xc2" if coder == "progressive" else b"\xff\xc0") + plain[sof + 2:dht])
    report = []
    for scan, entry in zip(scans_of(ncomp, coder), plan(width, height, ncomp, sub, coder, n, r)):
        walked = intervals_of(zz, width, height, sub, scan, entry["interval"])
        assert len(walked) == entry["intervals"]
        if coder == "progressive":
            names = pc.scan_tables(ncomp, scan)
        else:
            names = [(cls, t) for t in range(2 if ncomp == 3 else 1) for cls in ("dc", "ac")]
        counts = {t: [0] * 256 for t in names}
        for ops, _runs, _zrls in walked:
            for op in ops:
                if op[0] == "s":
                    counts[op[1]][op[2]] += 1
        tables = {t: DEFAULT_TABLES[t] if coder == "baseline" else hc.table(counts[t]) for t in names}
        for t in names:
            bits, vals, _longest = tables[t]
            file += ec._segment(0xc4, bytes([((t[0] == "ac") << 4) | t[1]]) + bytes(bits) + bytes(vals))
        if entry["dri"]:
            file += ec._segment(0xdd, bytes([entry["interval"] >> 8, entry["interval"] & 255]))
        file += pc._sos(scan) if coder == "progressive" else plain[plain.index(b"\xff\xda"):]
        codes = {t: ec._codes(b, v) for t, (b, v, _) in tables.items()}
        done, runs = [], []
        for k, (ops, some, _zrls) in enumerate(walked):
            bits = ec._Bits()
            for op in ops:
                if op[0] == "s":
                    bits.put(*codes[op[1]][op[2]])
                else:
                    bits.put(op[1], op[2])
            nbits = bits.n
            pad = -nbits % 8
            bits.put((1 << pad) - 1, pad)
            data = bytes(bits.data)
            file += data.replace(b"\xff", b"\xff\x00")
            if k + 1 < len(walked):
                file += bytes([0xff, 0xd0 + (k & 7)])
            done.append({"bits": nbits, "pad": pad, "data": data})
            runs += some
        report.append({"scan": scan, "plan": entry, "counts": counts, "tables": tables, "bits": sum(i["bits"] for i in done),
                       "padding": sum(i["pad"] for i in done), "stuffed": sum(i["data"].count(b"\xff") for i in done), "markers": len(done) - 1,
                       "eob_runs": len(runs), "runs": runs, "intervals": done})
    return bytes(file + b"\xff\xd9"), report


def encode_case(case, coder, n=0, r=0):
    return encode_report(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], coder, n, r)


def parse_restarts(file):
    """per scan of a file: (the interval of the DRI segment between the previous scan's data and this SOS, or None; the interval in
    force; the n of its RSTn markers in order)"""
    out, at, interval, dri = [], 2, 0, None
    while True:
        assert file[at] == 0xff, at
        marker = file[at + 1]
        if marker == 0xd9:
            return out
        size = (file[at + 2] << 8) | file[at + 3]
        if marker == 0xdd:
            assert size == 4
            dri = interval = (file[at + 4] << 8) | file[at + 5]
        at += 2 + size
        if marker != 0xda:
            continue
        rst = []
        while True:
            at = file.index(b"\xff", at)
            if file[at + 1] == 0 or file[at + 1] == 0xff:
                at += 1 + (file[at + 1] == 0)
            elif 0xd0 <= file[at + 1] <= 0xd7:
                rst.append(file[at + 1] - 0xd0)
                at += 2
            else:
                break
        out.append((dri, interval, rst))
        dri = None


# ---- the cases ----
SHAPES = {"grey_17x9": (17, 9, 1, (1, 1)), "420_41x23": (41, 23, 3, (2, 2)), "422_40x24": (40, 24, 3, (2, 1)), "444_40x24": (40, 24, 3, (1, 1))}


def shape_settings(width, height, ncomp, sub):
    """the six settings of a shape: {name: (N, R)} — N = 1, 3, units per row of the first scan, at least the units; R = 1, 2"""
    first = plan(width, height, ncomp, sub, "baseline")[0]
    return {"n1": (1, 0), "n3": (3, 0), "nrow": (first["units_per_row"], 0), "nall": (first["units"] + 2, 0), "r1": (0, 1), "r2": (0, 2)}


def shape_cases():
    """{name: (case, coder, N, R)}: three coders x six settings x four shapes"""
    out = {}
    for k, (shape, (w, h, ncomp, sub)) in enumerate(SHAPES.items()):
        case = ec.make(w, h, ncomp, sub, "sparse", seed=300 + k)
        for setting, (n, r) in shape_settings(w, h, ncomp, sub).items():
            for coder in CODERS:
                out[f"{shape}_{coder}_{setting}"] = (case, coder, n, r)
    return out


def sweep_cases():
    """{name: (case, coder, N, R)}: every case of huffman_cases.sweep() twice — at one N (2 and 5 by turns) and at one R (1 and 2 by
    turns) — the coder by turns, another one for the R file than for the N file: 320 files"""
    out = {}
    for k, (name, case) in enumerate(hc.sweep()):
        n, r = (2, 5)[(k // 3) % 2], (1, 2)[(k // 3) % 2]
        out[f"{name}_{CODERS[k % 3]}_n{n}"] = (case, CODERS[k % 3], n, 0)
        out[f"{name}_{CODERS[(k + 1) % 3]}_r{r}"] = (case, CODERS[(k + 1) % 3], 0, r)
    return out


def _grey(width, height, blocks=None):
    """a zero grey case; blocks: {block: {zigzag position: value}}"""
    case = ec.make(width, height, 1, (1, 1), "zero")
    for b, values in (blocks or {}).items():
        pc._put(case, b, values)
    return case


def constant_dc_case():
    """4:2:0 48x32 with a DC of 1000, -900 and 800 in every block of the three components: every reset shows as a large difference"""
    case = ec.make(48, 32, 3, (2, 2), "zero")
    for a, v in zip(case["coefficients"], (1000, -900, 800)):
        a[:, :, 0] = v
    return case


def eob_crossing_case():
    """grey 128x8, sixteen blocks: block 0 holds 4 at 1 and -4 at 7 (new in scans 2 and 3), blocks 1..15 hold 2 at 2 and -3 at 9
    (nothing in the first scans: an EOB run that an interval of 5 cuts twice; in the refinement scans correction bits wait with it) and
    block 11 a 1 at 20 (the last scan's run ends there)"""
    blocks = {b: {2: 2, 9: -3} for b in range(1, 16)}
    blocks[0] = {1: 4, 7: -4}
    blocks[11] = {2: 2, 9: -3, 20: 1}
    return _grey(128, 8, blocks)


def correction_cut_case():
    """grey 320x8, forty blocks that hold 2 and -3 at every AC position (63 correction bits each in the last scan): the 937-bit rule
    cuts the run behind its fifteenth block, and an interval of 16 ends it one block later"""
    return _grey(320, 8, {b: {k: 2 if k % 2 else -3 for k in range(1, 64)} for b in range(40)})


def _search(want, coder, n, r, last=0):
    """entropy_cases._search for a file with restarts: the first seed whose 32x8 grey sparse case shows what `want` asks of its report"""
    for seed in range(1, 4000):
        case = ec.make(32, 8, 1, (1, 1), "sparse", seed=seed)
        case["coefficients"][0][0, 0, 63] = last
        if want(encode_case(case, coder, n, r)[1]):
            return case
    raise AssertionError("no seed gives the directed interval")


def has_unpadded_interval(report):
    return any(i["pad"] == 0 for r in report for i in r["intervals"][:-1])


def has_ff_by_padding(report):
    """an interval in front of a marker whose last byte is FF only through its padding: FF 00 FF Dn"""
    return any(i["pad"] > 0 and i["data"][-1] == 0xff for r in report for i in r["intervals"][:-1])


def directed_cases():
    """{name: (case, coder, N, R)}; tests/test_restart_cpu.py asserts what each is there for"""
    out = {
        "no_pad": (_search(has_unpadded_interval, "baseline", 1, 0), "baseline", 1, 0),
        "ff_by_padding": (_search(has_ff_by_padding, "baseline", 1, 0, last=255), "baseline", 1, 0),
        "wraps_d7": (ec.make(8 * 19, 8, 1, (1, 1), "sparse", seed=19), "optimized", 1, 0),
        "short_last": (ec.make(8 * 11, 16, 1, (1, 1), "sparse", seed=11), "baseline", 4, 0),
        "zero_2100": (_grey(8 * 50, 8 * 42), "baseline", 1, 0),
        "chunk_edges": (_grey(8 * 50, 8 * 42), "optimized", 1, 0),
        "constant_dc": (constant_dc_case(), "baseline", 0, 1),
        "eob_crossing": (eob_crossing_case(), "progressive", 5, 0),
        "correction_cut": (correction_cut_case(), "progressive", 16, 0),
        "prog_40x24_420_r1": (ec.make(40, 24, 3, (2, 2), "sparse", seed=4024), "progressive", 0, 1),
        "prog_40x24_420_n3": (ec.make(40, 24, 3, (2, 2), "sparse", seed=4024), "progressive", 3, 0),
    }
    for coder in CODERS:
        out[f"constant_dc_{coder}_n2"] = (constant_dc_case(), coder, 2, 0)
    return out


def large_cases():
    """the cases whose size is what they are about (seconds in plain Python; the GPU test runs them too).  libjpeg writes no image
    wider than 65500 pixels (JPEG_MAX_DIMENSION), so the 65528-pixel case is held against the restatement alone (BEYOND_LIBJPEG) and
    its neighbour of 65496 pixels, whose rows of 8187 blocks are clamped in the same way, against libjpeg too"""
    return {
        "zero_65792_n65535": (_grey(2048, 2056), "progressive", 65535, 0),
        "clamped_65528x80_r9": (_grey(65528, 80), "progressive", 0, 9),
        "clamped_65496x80_r9": (_grey(65496, 80), "progressive", 0, 9),
    }


BEYOND_LIBJPEG = ("clamped_65528x80_r9",)


PROG_40x24_R1 = ("DHT00 DHT01 DRI=3 SOS", "DHT10 DRI=5 SOS", "DHT11 DRI=3 SOS", "DHT11 SOS", "DHT10 DRI=5 SOS", "DHT10 SOS", "DRI=3 SOS", "DHT11 SOS",
                 "DHT11 SOS", "DHT10 DRI=5 SOS")


def marker_sequence(file):
    """per scan the segments between the frame header (or the previous scan's data) and the SOS, as PROG_40x24_R1 spells them"""
    out, words, at = [], [], file.index(b"\xff\xc2") if b"\xff\xc2" in file[:file.index(b"\xff\xda")] else file.index(b"\xff\xc0")
    at += 2 + ((file[at + 2] << 8) | file[at + 3])
    while file[at + 1] != 0xd9:
        marker, size = file[at + 1], (file[at + 2] << 8) | file[at + 3]
        if marker == 0xc4:
            words.append("DHT%02x" % file[at + 4])
        elif marker == 0xdd:
            words.append("DRI=%d" % ((file[at + 4] << 8) | file[at + 5]))
        at += 2 + size
        if marker != 0xda:
            continue
        out.append(" ".join(words + ["SOS"]))
        words = []
        while True:
            at = file.index(b"\xff", at)
            if file[at + 1] in (0, 0xff) or 0xd0 <= file[at + 1] <= 0xd7:
                at += 1 if file[at + 1] == 0xff else 2
            else:
                break
    return tuple(out)


def gpu_cases():
    """{name: (case, coder, N, R)}: what tests/test_restart_gpu.py sends through j2p_entropy_encode_opt"""
    out = sweep_cases()
    out.update(shape_cases())
    out.update(directed_cases())
    out.update({name: c for name, c in large_cases().items() if name != "clamped_65496x80_r9"})      # (libjpeg's stand-in for its neighbour)
    return out
