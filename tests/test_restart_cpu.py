"""Restart intervals (include/jpeg2png_amd.h: "Restart intervals"), checked without a GPU: the plain-Python restatement in
tests/restart_cases.py against libjpeg itself with restart_interval / restart_in_rows set (tests/c/write_coefficients_restart.c is
the existing helper with the coder, N and R as three more words of input), against libjpeg's reader (tests/c/read_coefficients.c,
read_component.c) and the restated decoders of tests/scan_decode_cases.py; the restart plan of jpeg2png_amd/csrc/j2p_restart.h —
through j2p_debug_restart_plan and through the stand-alone tests/c/restart_main.c, compiled plainly and once more with the address
and undefined-behaviour sanitizers — against the DRI values and RSTn counts parsed from libjpeg's files; what the directed cases
are there for, by the restatement's own report; and the refusals, which need no device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
import restart_cases as rc
import scan_decode_cases as sdc
from test_decode_cpu import libjpeg_arrays
from test_jpeg_out_cli import _helper, read_component, read_coefficients  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def write_restart(tmp_path_factory):
    """tests/c/write_coefficients_restart.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "write_coefficients_restart")


def libjpeg_file(exe, case, coder, n, r):
    k = len(case["coefficients"])
    raw = struct.pack("<9I", case["width"], case["height"], k, case["quality"], *case["sub"], rc.CODERS.index(coder), n, r)
    raw += b"".join(np.ascontiguousarray(a, dtype=np.int16).tobytes() for a in case["coefficients"])
    return subprocess.run([exe], input=raw, capture_output=True, check=True).stdout


@pytest.fixture(scope="module")
def cases():
    out = rc.sweep_cases()
    out.update(rc.shape_cases())
    out.update(rc.directed_cases())
    out.update(rc.large_cases())
    return out


@pytest.fixture(scope="module")
def reports(cases):
    """{name: (file, per-scan report)} of the restatement, computed once"""
    return {name: rc.encode_case(*c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def libjpeg_files(write_restart, cases):
    """{name: libjpeg's file}, written once; not for the case libjpeg refuses (restart_cases.BEYOND_LIBJPEG)"""
    return {name: libjpeg_file(write_restart, *c) for name, c in cases.items() if name not in rc.BEYOND_LIBJPEG}


def test_restatement_is_libjpeg_byte_for_byte(cases, reports, libjpeg_files):
    assert len(rc.sweep_cases()) == 2 * 160 and len(rc.shape_cases()) == 3 * 6 * 4 and len(rc.directed_cases()) == 14 and len(rc.large_cases()) == 3
    assert len(libjpeg_files) == len(cases) - 1 == 320 + 72 + 14 + 3 - 1
    # every case of the sweep at one N and at one R; each coder meets both, a hundred times or more
    names = {name for name, _case in hc.sweep()}
    assert len(names) == 160
    assert {k.rsplit("_", 2)[0] for k, c in rc.sweep_cases().items() if c[2]} == names == {k.rsplit("_", 2)[0] for k, c in rc.sweep_cases().items() if c[3]}
    for coder in rc.CODERS:
        mine = [c for c in rc.sweep_cases().values() if c[1] == coder]
        assert sum(1 for c in mine if c[2]) >= 53 and sum(1 for c in mine if c[3]) >= 53, coder
    for name, want in libjpeg_files.items():
        assert reports[name][0] == want, name


def test_decoders_get_the_coefficients_back(read_coefficients, read_component, cases, reports, tmp_path):  # noqa: F811
    """libjpeg's reader and the restated decoders, on every sweep, shape and directed case and on the large file libjpeg accepts"""
    names = sorted(rc.sweep_cases()) + sorted(rc.shape_cases()) + sorted(rc.directed_cases()) + ["clamped_65496x80_r9"]
    assert len(names) == 320 + 72 + 14 + 1
    for name in names:
        case, file = cases[name][0], reports[name][0]
        path = str(tmp_path / "restated.jpg")
        open(path, "wb").write(file)
        for what, got in (("libjpeg", libjpeg_arrays(read_coefficients, read_component, path, len(case["coefficients"]))), ("restated", sdc.decode(file)[0])):
            assert len(got) == len(case["coefficients"]), (name, what)
            for c, (a, b) in enumerate(zip(got, case["coefficients"])):
                assert np.array_equal(a, b), f"{name}: {what}: component {c}"


@pytest.fixture(scope="module", params=["library", "plain", "sanitized"])
def planner(request, tmp_path_factory):
    """callable: [(width, height, ncomp, sub, progressive, N, R)] -> per entry None (refused) or the plan as a list of dicts like
    restart_cases.plan's — from j2p_debug_restart_plan, or from the stand-alone tests/c/restart_main.c"""
    keys = ("units", "units_per_row", "interval", "intervals", "dri")
    if request.param == "library":
        import jpeg2png_amd as j

        def run(entries):
            out = []
            for w, h, ncomp, sub, progressive, n, r in entries:
                try:
                    out.append(j._restart_plan(w, h, ncomp, sub, progressive, restart_rows=r, restart_interval=n))
                except j.J2PError:
                    out.append(None)
            return out
        return run
    exe = str(tmp_path_factory.mktemp("restart") / "restart")
    flags = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
             if request.param == "sanitized" else ["-O2"])
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "jpeg2png_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "restart_main.c"), "-o", exe], check=True)

    def run(entries):
        text = "".join(f"{w} {h} {ncomp} {sub[0]} {sub[1]} {int(progressive)} {n} {r}\n" for w, h, ncomp, sub, progressive, n, r in entries)
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = []
        for line in p.stdout.splitlines():
            if line == "refused":
                out.append(None)
                continue
            v = [int(x) for x in line.split()]
            scans = [dict(zip(keys, v[2 + 5 * s:7 + 5 * s])) for s in range(v[0])]
            assert len(v) == 2 + 5 * v[0] and v[1] == sum(s["intervals"] - 1 for s in scans)
            out.append([dict(s, dri=bool(s["dri"])) for s in scans])
        assert len(out) == len(entries)
        return out
    return run


def test_plan_is_what_libjpeg_wrote(planner, cases, reports, libjpeg_files):
    """the C plan against the restated one for every case, and both against the DRI segments and RSTn markers of libjpeg's files"""
    names = sorted(cases)
    entries = [(c["width"], c["height"], len(c["coefficients"]), c["sub"], coder == "progressive", n, r) for c, coder, n, r in (cases[k] for k in names)]
    plans = planner(entries)
    checked = 0
    for name, entry, got in zip(names, entries, plans):
        want = rc.plan(entry[0], entry[1], entry[2], entry[3], cases[name][1], entry[5], entry[6])
        assert got == want, name
        assert [r["plan"] for r in reports[name][1]] == want, name
        if name in rc.BEYOND_LIBJPEG:
            continue
        parsed = rc.parse_restarts(libjpeg_files[name])
        assert len(parsed) == len(got), name
        for k, (scan, (dri, in_force, rst)) in enumerate(zip(got, parsed)):
            assert (dri, in_force) == (scan["interval"] if scan["dri"] else None, scan["interval"]), f"{name}: scan {k + 1}"
            assert rst == [m % 8 for m in range(scan["intervals"] - 1)], f"{name}: scan {k + 1}"
        checked += 1
    assert checked == 320 + 72 + 14 + 2


def test_plan_edges(planner):
    """the clamp at 65535, an interval of the whole scan and beyond, one unit, and the refusals"""
    got = planner([(65528, 80, 1, (1, 1), True, 0, 9), (65535, 65535, 3, (2, 2), False, 0, 65535), (8, 8, 1, (1, 1), False, 1, 0),
                   (16, 8, 1, (1, 1), False, 2, 0), (16, 8, 1, (1, 1), False, 65535, 0), (16, 16, 3, (2, 2), True, 0, 0),
                   (16, 16, 1, (1, 1), False, 65536, 0), (16, 16, 1, (1, 1), False, 0, 65536), (16, 16, 1, (1, 1), False, 1, 1),
                   (16, 16, 1, (1, 1), False, 0xffffffff, 0)])
    assert [s["interval"] for s in got[0]] == [65535] * 6 and [s["intervals"] for s in got[0]] == [2] * 6 and [s["dri"] for s in got[0]] == [True] + [False] * 5
    assert got[1] == [{"units": 4096 * 4096, "units_per_row": 4096, "interval": 65535, "intervals": 257, "dri": True}]
    assert got[2] == [{"units": 1, "units_per_row": 1, "interval": 1, "intervals": 1, "dri": True}]
    assert got[3][0]["intervals"] == 1 and got[4][0]["intervals"] == 1 and got[4][0]["dri"]
    assert len(got[5]) == 10 and all(s == dict(s, interval=0, intervals=1, dri=False) for s in got[5])
    assert got[6:] == [None] * 4


def test_prog_40x24_420_marker_sequence(cases, reports, libjpeg_files):
    file = reports["prog_40x24_420_r1"][0]
    assert rc.marker_sequence(file) == rc.PROG_40x24_R1 == rc.marker_sequence(libjpeg_files["prog_40x24_420_r1"])
    n3 = rc.marker_sequence(reports["prog_40x24_420_n3"][0])
    assert n3[0] == "DHT00 DHT01 DRI=3 SOS" and not any("DRI" in s for s in n3[1:]) and len(n3) == 10


def test_case_preconditions(cases, reports):
    """what the directed cases are there for, by the restatement alone"""
    def scans(name):
        return reports[name][1]
    assert rc.has_unpadded_interval(scans("no_pad"))
    assert rc.has_ff_by_padding(scans("ff_by_padding")) and b"\xff\x00\xff\xd0" in reports["ff_by_padding"][0]
    # at least 17 intervals: D7 is followed by D0
    w = scans("wraps_d7")[0]
    assert w["plan"]["intervals"] == 19 and b"\xff\xd7" in reports["wraps_d7"][0] and rc.parse_restarts(reports["wraps_d7"][0])[0][2][7:10] == [7, 0, 1]
    # a short last interval: 22 blocks in intervals of 4
    s = scans("short_last")[0]["plan"]
    assert s["units"] % s["interval"] == 2 and s["intervals"] == 6
    # about 2100 zero blocks, an interval each: one byte per interval, so 256 markers per 256-byte stuffing chunk, more than 1024
    # intervals (a second tile of the exclusive sum over the chunks' counts is far off, a second workgroup of the lane-per-interval
    # kernels is not), and a marker behind every byte: on every lane edge and chunk edge
    for name in ("zero_2100", "chunk_edges"):
        z = scans(name)[0]
        assert z["plan"]["intervals"] == 2100 > 1024 and all(len(i["data"]) == 1 for i in z["intervals"]), name
        ends = np.cumsum([len(i["data"]) for i in z["intervals"]])[:-1]
        assert {255, 256, 257} <= set(ends.tolist()) and {255 + 256, 256 + 256, 257 + 256} <= set(ends.tolist())
    assert all(i["pad"] > 0 for i in scans("zero_2100")[0]["intervals"])
    # the optimised tables of a zero image are two one-bit codes: 2 bits an interval
    assert all(i["bits"] == 2 for i in scans("chunk_edges")[0]["intervals"])
    # a constant large DC: every interval's first difference is the DC itself, every other difference 0
    for name in ("constant_dc", "constant_dc_baseline_n2", "constant_dc_optimized_n2", "constant_dc_progressive_n2"):
        first = scans(name)[0]
        dc0 = first["counts"][("dc", 0)]
        shift = 1 if cases[name][1] == "progressive" else 0
        assert dc0[(1000 >> shift).bit_length()] == first["plan"]["intervals"] > 1 and dc0[0] == 24 - first["plan"]["intervals"], name
    # an EOB run that interval ends cut: in the first scans (blocks 1..15 hold nothing there) and in the refinement scans, where
    # correction bits wait with it
    e = scans("eob_crossing")
    assert [s["plan"]["intervals"] for s in e] == [4] * 6
    for k in (1, 2):            # (block 0 codes its coefficient and then begins the run with its own tail)
        assert [(b, n) for b, n, _why in e[k]["runs"]] == [(0, 5), (5, 5), (10, 5), (15, 1)], k
        assert all(why == "end_of_scan" for _b, _n, why in e[k]["runs"])
    last = e[5]                 # (block 11 ends the run of block 10 and begins the next with its tail)
    assert [(b, n, why) for b, n, why in last["runs"]] == [(0, 5, "end_of_scan"), (5, 5, "end_of_scan"), (10, 1, "next_block"), (11, 4, "end_of_scan"),
                                                           (15, 1, "end_of_scan")]
    # (two correction bits a block, 2 and -3, and at least the EOBn symbol)
    assert all(i["bits"] > 2 * blocks for i, blocks in zip(last["intervals"], (5, 5, 5, 1))), "no correction bits waited with the runs"
    # the 937-bit cut inside an interval, and the interval's end next: 15 blocks of 63 bits, then one more
    c = scans("correction_cut")[5]
    assert [(b, n, why) for b, n, why in c["runs"]][:4] == [(0, 15, "limit_937"), (15, 1, "end_of_scan"), (16, 15, "limit_937"), (31, 1, "end_of_scan")]
    # 65792 zero blocks, N = 65535: runs of 32767, 32767 and 1 in the first interval, 257 in the second
    for s in scans("zero_65792_n65535")[1:4]:
        assert [(n, why) for _b, n, why in s["runs"]] == [(32767, "limit_7fff"), (32767, "limit_7fff"), (1, "end_of_scan"), (257, "end_of_scan")]
    # R = 9 on rows of 8191 (8187) blocks: 73719 (73683), clamped
    for name, per_row in (("clamped_65528x80_r9", 8191), ("clamped_65496x80_r9", 8187)):
        s = scans(name)[0]["plan"]
        assert s["units_per_row"] == per_row and 9 * per_row > 65535 == s["interval"] and s["intervals"] == 2, name


def test_refusals_need_no_device():
    """N or R above 65535, and both set: refused before the device is looked for (no coefficient is read either)"""
    import ctypes
    import jpeg2png_amd as j
    lib = j.load_library()
    case = ec.make(16, 16, 1, (1, 1), "sparse")
    for keywords, message in (({"restart_interval": 65536}, "restart_interval is above 65535"), ({"restart_rows": 65536}, "restart_in_rows is above 65535"),
                              ({"restart_interval": 70000}, "restart_interval is above 65535"),
                              ({"restart_interval": 1, "restart_rows": 1}, "both set")):
        for more in ({}, {"optimize": True}, {"progressive": True}):
            with pytest.raises(j.J2PError, match=message):
                j.entropy_encode(case["coefficients"], 16, 16, case["quant"], **keywords, **more)
    with pytest.raises(j.J2PError, match="not negative"):
        j.entropy_encode(case["coefficients"], 16, 16, case["quant"], restart_rows=-1)
    size = ctypes.c_size_t(0)
    spec, _held = j._c_jpeg(16, 16, 1, None, case["quant"], (1, 1))
    ptrs = (ctypes.c_void_p * 3)(case["coefficients"][0].ctypes.data, None, None)
    assert lib.j2p_entropy_encode_opt(0, ctypes.byref(spec), ptrs, 1, None, 0, ctypes.byref(size), None, None, None, None) == -1
    assert "options" in lib.j2p_last_error().decode()
    for options in ((2, 0, 1, 0), (0, 2, 1, 0)):
        opt = j._CJpegOptions(*options)
        assert lib.j2p_entropy_encode_opt(0, ctypes.byref(spec), ptrs, 1, None, 0, ctypes.byref(size), ctypes.byref(opt), None, None, None) == -1
    # the calls without options refuse what they refused
    assert lib.j2p_entropy_encode_ex(0, ctypes.byref(spec), ptrs, 1, None, 0, ctypes.byref(size), 2, None) == -1
    assert "unknown flag bits" in lib.j2p_last_error().decode()
