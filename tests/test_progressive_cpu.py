"""The progressive JPEG file (include/jpeg2png_amd.h: "The progressive JPEG file"), checked without a GPU: the plain-Python
restatement in tests/progressive_cases.py against libjpeg itself with jpeg_simple_progression()
(tests/c/write_coefficients_progressive.c is the optimised helper with that one call added), against libjpeg's reader
(tests/c/read_coefficients.c) and PIL, and the properties the directed cases are there for, by the restatement's own report."""
import io

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
import progressive_cases as pc
from test_entropy_cpu import libjpeg_file
from test_jpeg_out_cli import _helper, load_component, load_coefficients, read_component, read_coefficients  # noqa: F401


@pytest.fixture(scope="module")
def write_progressive(tmp_path_factory):
    """tests/c/write_coefficients_progressive.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "write_coefficients_progressive")


@pytest.fixture(scope="module")
def cases():
    out = dict(hc.sweep())
    out.update(hc.directed_cases())
    out.update(pc.new_cases())
    return out


@pytest.fixture(scope="module")
def reports(cases):
    """{name: (file, per-scan report)} of the restatement, computed once"""
    return {name: pc.encode_case(case) for name, case in cases.items()}


def ac_scans(report, refine=None):
    return [r for r in report if r["scan"][1] > 0 and (refine is None or bool(r["scan"][3]) == refine)]


def test_restatement_is_libjpeg_with_simple_progression_byte_for_byte(write_progressive, cases, reports):
    assert len([n for n in cases if n in dict(hc.sweep())]) == 160 and len(cases) >= 160 + 24 + 3 + 3 + len(pc.ROW_SIZES) + len(pc.STREAM_ENDS)
    for name, case in cases.items():
        assert reports[name][0] == libjpeg_file(write_progressive, case), name


def test_scan_counts_and_markers(cases, reports):
    for name, (file, report) in reports.items():
        n = len(cases[name]["coefficients"])
        assert len(report) == (10 if n == 3 else 6), name
        assert [r["scan"] for r in report] == pc.SCANS[n]
        assert file.count(b"\xff\xc2") >= 1 and b"\xff\xc0" not in file[:file.index(b"\xff\xda")], name
        assert file.endswith(b"\xff\xd9")


@pytest.mark.parametrize("name", ["sparse_41x23_420", "sparse_40x24_422", "sparse_41x23_440", "dense_24x40_444", "dc_swing", "sparse_368x368_420"])
def test_libjpegs_reader_gets_the_coefficients_back(read_coefficients, cases, reports, tmp_path, name):  # noqa: F811
    case = cases[name]
    path = str(tmp_path / "restated.jpg")
    open(path, "wb").write(reports[name][0])
    w, h, planes = load_coefficients(read_coefficients, path)
    assert (w, h) == (case["width"], case["height"])
    for c, (plane, (gh, gw)) in enumerate(zip(planes, ec.grids(w, h, 3, case["sub"]))):
        assert np.array_equal(plane.quant_table, case["quant"][c]), f"component {c}"
        assert np.array_equal(plane.data.reshape(gh, gw, 64), case["coefficients"][c]), f"component {c}"


@pytest.mark.parametrize("name", ["grey_17x9_dense", "correction_limit", "refine_zrl", "eobrun_limit", "cut_from_block_17", "both_limits", "row_1", "row_1025",
                                  "end_dc_refine_whole_bytes", "end_ac_first_whole_bytes"])
def test_libjpegs_reader_gets_a_grey_file_back(read_component, cases, reports, tmp_path, name):  # noqa: F811
    case = cases[name]
    path = str(tmp_path / "restated.jpg")
    open(path, "wb").write(reports[name][0])
    w, h, n, plane = load_component(read_component, path)
    gh, gw = ec.grids(w, h, 1, (1, 1))[0]
    assert (w, h, n) == (case["width"], case["height"], 1)
    assert np.array_equal(plane.data.reshape(gh, gw, 64), case["coefficients"][0])


def test_pil_opens_the_files_as_progressive(cases, reports):
    from PIL import Image
    opened = 0
    names = list(hc.directed_cases()) + list(pc.new_cases())
    for name in names:
        if "dense" in name or "last" in name or name in ("dc_swing", "run_lengths"):
            continue            # (valid files, but coefficients no decoder's range checks were written for)
        case = cases[name]
        im = Image.open(io.BytesIO(reports[name][0]))
        im.load()
        assert im.size == (case["width"], case["height"]) and im.mode == ("L" if len(case["coefficients"]) == 1 else "RGB"), name
        assert im.info.get("progressive"), name
        opened += 1
    assert opened >= 15


def corrections(case, run, al=0):
    """the correction bits of the blocks of an EOB run (first block, length, why) of a grey case in a refinement scan at Al, counted
    from the coefficients: every AC coefficient that was non-zero before the scan, where none of the blocks meets a new one"""
    first, length, _why = run
    t = np.abs(case["coefficients"][0].reshape(-1, 64)[first:first + length, 1:].astype(np.int64)) >> al
    assert not (t == 1).any()
    return int((t > 1).sum())


def cutter_preconditions(cases, reports):
    """cut_from_block_1 / _17 and both_limits, from the restatement's runs"""
    assert len(ec.scan_order(1456, 1456, 1, (1, 1))) == 33124
    for b in (1, 17):
        _file, report = reports[f"cut_from_block_{b}"]
        assert len(ac_scans(report)) == 4
        for r in ac_scans(report):
            assert r["flushes"] == {"limit_7fff": 1, "limit_937": 0, "next_block": 1, "end_of_scan": 1}, (b, r["scan"])
            assert r["runs"] == [(0, b, "next_block"), (b, 32767, "limit_7fff"), (b + 32767, 33124 - 32767 - b, "end_of_scan")], (b, r["scan"])
            cut = [run for run in r["runs"] if run[2] == "limit_7fff"]
            assert len(cut) == 1 and cut[0][0] % 4 == 1, "the run the 0x7fff rule cuts starts at a block that is not 1 (mod 4)"
    assert reports["cut_from_block_1"][1][1]["runs"][-1] == (32768, 356, "end_of_scan")
    case, (_file, report) = cases["both_limits"], reports["both_limits"]
    first_1_5, first_6_63, refine_2_1, last = ac_scans(report)
    assert last["scan"] == ((0,), 1, 63, 1, 0) and last is report[-1]
    assert last["flushes"] == {"limit_937": 1, "limit_7fff": 1, "next_block": 0, "end_of_scan": 1}
    assert [run[2] for run in last["runs"]] == ["limit_937", "limit_7fff", "end_of_scan"]
    by_937, by_7fff, behind = last["runs"]
    assert by_7fff[1] == 32767 and by_937[0] + by_937[1] == by_7fff[0] and by_7fff[0] + by_7fff[1] == behind[0]
    assert corrections(case, by_937) == 15 * 63 > pc.CORRECTION_LIMIT >= 14 * 63
    held, after = corrections(case, by_7fff), corrections(case, behind)
    assert (held, after) == (600, 400) and held <= pc.CORRECTION_LIMIT and after <= pc.CORRECTION_LIMIT < held + after
    for r in (first_1_5, first_6_63):
        assert r["flushes"] == {"limit_7fff": 1, "limit_937": 0, "next_block": 0, "end_of_scan": 1}, r["scan"]
    assert refine_2_1["flushes"] == {"limit_7fff": 0, "limit_937": 0, "next_block": 18, "end_of_scan": 1}
    assert last["bits"] == 1976 and last["bits"] % 8 == 0 and last["short"] == 0


def row_preconditions(reports):
    """the row_<n> family: what the restatement's runs show, each in at least one AC scan of one size"""
    shown = {}
    for n in pc.ROW_SIZES:
        _file, report = reports[f"row_{n}"]
        assert len(ec.scan_order(8 * n, 8, 1, (1, 1))) == n
        for r in ac_scans(report):
            runs, here = r["runs"], set()
            for k, (first, length, why) in enumerate(runs):
                here |= {f"starts at {first}"} & {"starts at 15", "starts at 16", "starts at 17"}
                if first < 16 < first + length:
                    here.add("crosses 16")
                if first + length == n and why == "end_of_scan":
                    here.add("ends at n - 1")
                if why == "limit_937" and k + 1 < len(runs) and runs[k + 1][0] % 4:
                    here.add("cut by 937, the next starts off a multiple of 4")
            if not runs:
                here.add("no run")
            if runs == [(0, n, "end_of_scan")]:
                here.add("one run")
            for what in here:
                shown.setdefault(what, []).append((n, r["scan"]))
    for what in ("starts at 15", "starts at 16", "starts at 17", "crosses 16", "ends at n - 1", "cut by 937, the next starts off a multiple of 4",
                 "no run", "one run"):
        assert shown.get(what), f"no row_<n> case shows: {what}"


def stream_end_preconditions(reports):
    """the end_<...> cases, from short and last"""
    assert set(pc.STREAM_END_NAMES) <= set(reports) and len(pc.STREAM_END_NAMES) == 9
    for name in pc.STREAM_END_NAMES:
        file, report = reports[name]
        if name == "end_whole_words":
            assert any(r["bits"] > 0 and r["bits"] % 32 == 0 and r["short"] == 0 for r in report), name
            continue
        kind = [k for k in pc.KINDS if name.startswith("end_" + k + "_")][0]
        end = name[len("end_" + kind + "_"):]
        mine = [r for r in report[:-1] if pc.scan_kind(r["scan"]) == kind]
        assert mine and end in ("whole_bytes", "ff_end"), name
        if end == "whole_bytes":
            assert any(r["short"] == 0 and r["bits"] > 0 for r in mine), name
        else:
            assert any(r["short"] > 0 and r["last"] == 0xff for r in mine), name
            assert b"\xff\x00\xff\xc4" in file, f"{name}: no scan's final byte is the 00 of its own FF, in front of the next DHT"


def test_case_preconditions(cases, reports):
    """what the directed cases are there for, by the restatement's own report"""
    cutter_preconditions(cases, reports)
    row_preconditions(reports)
    stream_end_preconditions(reports)
    # eobrun_limit: 33124 blocks, every AC scan ONE segment: a flush at the limit of 32767 and the 357 left at the end
    file, report = reports["eobrun_limit"]
    assert len(ec.scan_order(1456, 1456, 1, (1, 1))) == 182 * 182 == 33124 == 32767 + 357
    for r in ac_scans(report):
        assert r["flushes"] == {"limit_7fff": 1, "limit_937": 0, "next_block": 0, "end_of_scan": 1}, r["scan"]
        count = r["counts"][("ac", 0)]
        assert count[0xe0] == 1 and count[0x80] == 1 and sum(count) == 2, r["scan"]
    assert len(file) == 8584 and sum(r["stuffed"] for r in report) >= 1
    # correction_limit: no refinement scan meets a new coefficient; the 937-bit rule cuts, and not every 15 blocks
    _file, report = reports["correction_limit"]
    for r in ac_scans(report, refine=True):
        assert r["flushes"]["next_block"] == 0 and r["flushes"]["limit_7fff"] == 0 and r["zrls"] == 0, r["scan"]
        assert r["flushes"]["limit_937"] >= 1 and r["flushes"]["end_of_scan"] == 1, r["scan"]
    # dense: nearly every coefficient was non-zero before a refinement scan, some 60 correction bits a block: the 937-bit rule cuts
    # runs in all four of them, after 15 blocks where none of the run's blocks meets a new coefficient (15 * 63 = 945 > 937)
    _file, report = reports["dense_368x368_420"]
    blocks = 46 * 46
    assert all(r["flushes"]["limit_937"] >= 15 for r in ac_scans(report, refine=True))
    assert sum(x["stuffed"] for x in report) > 0
    # sparse 368x368: several tiles of the exclusive sums (1024 items) in every scan of component 0, runs that cross them
    _file, report = reports["sparse_368x368_420"]
    assert blocks > 2 * 1024 and all(sum(r["flushes"].values()) > 10 for r in ac_scans(report))
    # refine_zrl: a ZRL at a position that was non-zero before, no ZRL behind the last new coefficient.  Scan (2, 1): block 2's runs
    # of 21 and 22 zeros; scan (1, 0): block 0's at 39 and 60 (18 zeros since 40), block 4's three
    _file, report = reports["refine_zrl"]
    assert [r["zrls"] for r in ac_scans(report, refine=True)] == [2, 2 + 3]
    blocks = [[int(v) for v in b] for b in cases["refine_zrl"]["coefficients"][0].reshape(-1, 64)[:, ec.ZIGZAG]]
    ops, _flushes, zrls = pc.scan_operations([[blocks[:1]]], 8, 8, (1, 1), ((0,), 1, 63, 1, 0))
    at = ops.index(("s", ("ac", 0), 0xf0))
    assert zrls == 2 and ops[at + 1] == ("b", 0, 1) and ops[at + 2][0] == "s", "the ZRL is not followed by the one waiting correction bit"
    ops, _flushes, zrls = pc.scan_operations([[blocks[1:2]]], 8, 8, (1, 1), ((0,), 1, 63, 1, 0))
    assert zrls == 0 and [op for op in ops if op[0] == "s"] == [("s", ("ac", 0), 0x21), ("s", ("ac", 0), 0x00)]
    first = [r for r in report if r["scan"] == ((0,), 1, 63, 2, 1)][0]
    assert first["counts"][("ac", 0)][0x01] >= 1           # block 2: +-2 and +-3 are new in (2, 1) ...
    ops, _flushes, _zrls = pc.scan_operations([[blocks[2:3]]], 8, 8, (1, 1), ((0,), 1, 63, 1, 0))
    assert [op for op in ops if op[0] == "s"] == [("s", ("ac", 0), 0x00)] and len(ops) == 1 + 6        # ... and six corrections in (1, 0)
    # what the report's new fields say is what it counted and what the file holds
    for name, (file, report) in reports.items():
        for r in report:
            assert r["flushes"] == pc.count_by_why(r["runs"]) and r["short"] == -r["bits"] % 8, name
            assert all(a + n <= b for (a, n, _w), (b, _n, _v) in zip(r["runs"], r["runs"][1:])), name
    # dummy blocks behind odd DCs: the refinement bit of a dummy is its predecessor's
    for name in ("sparse_41x23_420", "sparse_40x24_422", "sparse_41x23_440"):
        case = cases[name]
        zz = [np.asarray(a)[:, :, ec.ZIGZAG].tolist() for a in case["coefficients"]]
        values = list(pc._dc_values(zz, case["width"], case["height"], case["sub"], 0))
        order = ec.scan_order(case["width"], case["height"], 3, case["sub"])
        assert any(y is None and v & 1 for (c, y, x), (_c, v) in zip(order, values)), name
    assert sum(1 for s in ec.scan_order(1, 1, 3, (2, 2)) if s[1] is None) == 3


def test_no_size_relation_is_claimed_but_the_headers_are_what_they_cost(cases, reports):
    """ten scan headers: a tiny image's progressive file is LARGER than its optimised one — the reason no test asserts otherwise"""
    case = cases["grey_8x8_zero"]
    assert len(reports["grey_8x8_zero"][0]) > len(hc.encode_case(case)[0])
