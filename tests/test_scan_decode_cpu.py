"""Reading a progressive JPEG file (include/jpeg2png_amd.h: "Reading a progressive JPEG file"), checked without a GPU: the
plain-Python restatement of tests/scan_decode_cases.py against libjpeg's jpeg_read_coefficients (the existing read_coefficients /
read_component helpers) on PIL-made, coder-made and writer-made files, and as the inverse of its writer; the library's C parser
(j2p_jpeg_parse_scans) against the restated one, good files and refusals; the refusals that the marker segments alone decide,
which touch no device; and the parser under sanitizers, as a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import entropy_cases as ec
import scan_decode_cases as sc
from test_decode_cpu import libjpeg_arrays
from test_jpeg_out_cli import read_component, read_coefficients  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_decoder_is_libjpeg(read_coefficients, read_component, tmp_path):  # noqa: F811
    files = sc.good_files()
    assert len(files) > 280
    for name, data in files.items():
        path = str(tmp_path / "file.jpg")
        open(path, "wb").write(data)
        got = sc.expected(name)
        want = libjpeg_arrays(read_coefficients, read_component, path, len(got))
        for c, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: component {c}"


def test_written_files_hold_their_coefficients():
    for name, (_data, want) in sc.written_cases().items():
        got = sc.expected(f"written_{name}")
        for c, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, np.asarray(b).reshape(a.shape)), f"{name}: component {c}"


def test_coder_files_hold_their_coefficients():
    import progressive_cases as pc
    for name, case in pc.gpu_cases().items():
        got = sc.expected(f"coder_{name}")
        for c, (a, b) in enumerate(zip(got, case["coefficients"])):
            assert np.array_equal(a, np.asarray(b).reshape(a.shape)), f"{name}: component {c}"


def test_a_sequential_file_is_decoded_as_before():
    import decode_cases as dc
    data = dc.write_case(ec.make(41, 23, 3, (2, 2), "sparse", seed=5), restart=2)
    got, parsed = sc.decode(data)
    want, _ = dc.decode(data)
    assert not parsed["progressive"] and len(parsed["scans"]) == 1
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def _c_parse(lib, data):
    import jpeg2png_amd as j
    raw = np.frombuffer(data, dtype=np.uint8)
    info, scans = j._CJpegInfo(), j._CJpegScans()
    return lib.j2p_jpeg_parse_scans(raw.ctypes.data, raw.size, ctypes.byref(info), ctypes.byref(scans)), info, scans


def test_c_parser_is_the_restated_parser(lib):
    import decode_cases as dc
    files = dict(sc.good_files())
    files["sequential"] = dc.write_case(ec.make(41, 23, 3, (2, 2), "sparse", seed=5), restart=2)
    for name, data in files.items():
        want = sc.parse_scans(data)
        rc, info, scans = _c_parse(lib, data)
        assert rc == 0, f"{name}: {lib.j2p_last_error().decode()}"
        grids, mcus_w, mcus_h = dc.geometry(want)
        assert (info.width, info.height, info.ncomp, info.mcus_w, info.mcus_h) == (want["width"], want["height"], len(grids), mcus_w, mcus_h), name
        assert [(k.blocks_h, k.blocks_w) for k in info.comp[:info.ncomp]] == [g[:2] for g in grids], name
        for k, comp in zip(info.comp[:info.ncomp], want["components"]):
            assert np.array_equal(np.array(k.quant, dtype=np.uint16), want["quant"][comp[3]]), name
        assert bool(scans.progressive) == want["progressive"] and scans.nscans == len(want["scans"]), name
        assert (info.scan_begin, info.scan_end, info.restart_interval) == (want["scan_begin"], want["scan_end"], want["restart_interval"]), name
        assert info.intervals == sum(s["intervals"] for s in want["scans"]), name
        for i, (q, s) in enumerate(zip(scans.scan[:scans.nscans], want["scans"])):
            got = (list(q.comp[:q.ncomp]), q.ss, q.se, q.ah, q.al, q.restart_interval, q.intervals, q.begin, q.end)
            assert got == (s["components"], s["ss"], s["se"], s["ah"], s["al"], s["restart_interval"], s["intervals"], s["begin"], s["end"]), f"{name}: scan {i}"
            if want["progressive"]:
                if s["ss"] == 0 and s["ah"] == 0:
                    assert list(q.dc_slot[:q.ncomp]) == s["dc_slots"], f"{name}: scan {i}"
                if s["ss"]:
                    assert list(q.ac_slot[:q.ncomp]) == s["ac_slots"], f"{name}: scan {i}"


def test_restated_parser_refuses_what_the_headers_show():
    for name, (data, code) in sc.header_refusals().items():
        with pytest.raises(sc.Refused) as e:
            sc.parse_scans(data)
        assert e.value.code == code, f"{name}: {e.value}"


def test_restated_decoder_refuses_damaged_data():
    for name, (data, whys) in sc.damaged_cases().items():
        sc.parse_scans(data)            # (the marker segments are in order)
        with pytest.raises(sc.Refused) as e:
            sc.decode(data)
        assert e.value.code == sc.EFORMAT and e.value.why in whys, f"{name}: {e.value}"


def test_edge_case_preconditions(lib):
    """what every edge_ file and every damaged file is named for, from the parse and the writer's reports alone"""
    import decode_cases as dc
    edge = sc.edge_cases()
    for name, (_data, want) in edge.items():
        got = sc.expected(f"edge_{name}")
        for c, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, np.asarray(b).reshape(a.shape)), f"{name}: component {c}"
    scans = {name: sc.parse_scans(data)["scans"] for name, data in sc.good_files().items()}

    def intervals(name):
        return [s["intervals"] for s in scans["edge_" + name]]
    # more first-scan intervals than a workgroup of k_scans_intervals (256) and a tile of the scan over their counts (1024) hold:
    # no other file comes near; 257 intervals of a refinement scan are 65 workgroups of four wavefronts, one live in the last
    assert intervals("intervals_257_grey") == [257] * 4 and all(s["ah"] == 0 for s in scans["edge_intervals_257_grey"])
    assert all(sum(s["intervals"] for s in ss if s["ah"] == 0) <= 150 for name, ss in scans.items() if not name.startswith("edge_"))
    assert intervals("refine_257_grey") == [257] * 8 and -(-257 // 4) == 65 and 257 % 4 == 1
    for index, s in enumerate(scans["edge_refine_257_grey"]):
        if s["ss"] == 0 and s["ah"]:        # a DC refinement interval: one bit, padded to a byte (a set bit: FF, stuffed, in front of RSTn)
            assert set(sc.scan_chunks(edge["refine_257_grey"][0], index)) == {b"\x7f", b"\xff\x00"}
    for residue, restart in sc.MOD4_RESTARTS.items():
        assert intervals(f"refine_intervals_mod4_{residue}") == [-(-18 // restart)] * 8 and -(-18 // restart) % 4 == residue and 18 % restart
    # interleaved and one-component scans cut by restarts in one file; DC refinement intervals of 12 bits (three MCUs of 4:2:2)
    for name in ("refine_3_422_rst", "stops_at_1_444_rst"):
        assert {len(s["components"]) for s in scans["edge_" + name] if s["intervals"] > 1} == {1, 3}, name
    dc_refinements = [s for s in scans["edge_refine_3_422_rst"] if s["ss"] == 0 and s["ah"]]
    assert [(len(s["components"]), s["restart_interval"], s["intervals"]) for s in dc_refinements] == [(3, 3, 3)] * 3
    assert intervals("dc_alone_420_rst") == [9, 3, 3, 3, 9, 3, 3, 9, 9] and [s["ss"] for s in scans["edge_dc_alone_420_rst"]][:3] == [0, 0, 0]
    grids, mcus_w, mcus_h = dc.geometry(sc.parse_scans(edge["dummy_blocks_17x9_rst"][0]))
    assert (mcus_h * 2, mcus_w * 2) == (2, 4) and grids[0][:2] == (2, 3) and intervals("dummy_blocks_17x9_rst")[0] == 1   # padding blocks inside the interval
    luma_ac_alone = [3 if s["components"] == [0] and s["ss"] else 1 for s in scans["edge_dri_between_grids_420"]]
    assert intervals("dummy_blocks_17x9_rst") == intervals("dri_between_grids_420") == luma_ac_alone
    assert [s["restart_interval"] for s in scans["edge_dri_changes"]] == [2] + [5] * 6 + [0] * 3
    assert all(s["ah"] for s in scans["edge_dri_changes"][7:]) and intervals("dri_changes") == [3, 4, 2, 2, 4, 4, 2, 1, 1, 1]
    scans = {name[5:]: ss for name, ss in scans.items() if name.startswith("edge_")}
    # EOB runs at the intervals' ends
    report = []
    case = sc.directed_case()
    assert sc.write_case(case, sc.SPLIT, restart=4, report=report) == edge["eob_run_ends_each_interval"][0]
    zz = case["coefficients"][0].reshape(-1, 64)[:, ec.ZIGZAG]
    for index in (2, 5):
        told = report[index]["intervals"]
        ends = [i["runs"][-1] if i["runs"] and i["runs"][-1][2] == "end_of_scan" else None for i in told]
        assert len(told) == 6 and sum(1 for r in ends if r is not None and r[1] > 1) >= 4, (index, ends)
    carried = [sum(1 for b in range(first, first + n) if (np.abs(zz[b, 6:]) >= 2).any()) for i in report[5]["intervals"] for first, n, _why in i["runs"]]
    assert max(carried) >= 3, carried           # one run's waiting correction bits come from three blocks
    # markers on the unstuffing kernels' edges, counted from the scan's own begin
    data = edge["markers_on_edges_scan_k"][0]
    for index in sc.EDGE_SCANS:
        s = scans["markers_on_edges_scan_k"][index]
        assert index > 0 and s["ss"] and bool(s["ah"]) == (index == sc.EDGE_SCANS[1])
        at = sc.scan_marker_offsets(data, index)
        assert len(at) == 23 and [a % 256 for a in at] == [dc.EDGE_TARGETS[m % 6] for m in range(23)], (index, at)
        assert any(a % 256 == 0 and a >= 256 for a in at)           # FF | Dn across a chunk edge
    assert any(scans["markers_on_edges_scan_k"][index]["begin"] % 4 for index in sc.EDGE_SCANS)         # chunks laid from an unaligned address
    assert any(sc.scan_stuffed_on_chunk_edge(data, index) for index in range(1, 10))
    data = edge["fill_covers_chunks_scan_k"][0]
    assert len(sc.scan_blank_chunks(data, sc.EDGE_SCANS[1])) == 2 and scans["fill_covers_chunks_scan_k"][sc.EDGE_SCANS[1]]["ah"]
    # the Al ladder, and the coefficients it carries
    ladder = [(s["ss"], s["ah"], s["al"]) for s in scans["refine_from_13"]]
    assert ladder == [(ss, ah, al) for _c, ss, _se, ah, al in sc.FROM_13] and len(ladder) == 28 and ladder[:2] == [(0, 0, 13), (1, 0, 13)]
    assert ladder[-2:] == [(0, 1, 0), (1, 1, 0)]
    values = np.concatenate([a.reshape(-1) for a in sc.expected("edge_refine_from_13")]).astype(np.int64)
    assert values.max() == 32767 and values.min() == -32768 and (np.abs(values.reshape(-1, 64)[:, 1:]) >> 13).max() == 3
    # the DC extremes
    for al, (top, bottom) in ((0, (32767, -32768)), (1, (32766, -32768))):
        got = sc.expected(f"edge_dc_near_limit_al{al}")[0][0, :, 0].astype(np.int64)
        assert got.max() == top and got.min() == bottom and scans[f"dc_near_limit_al{al}"][0]["al"] == al
        assert (got >> al).max() == (32767 >> al) and (got >> al).min() == -(32768 >> al)
    got = sc.expected("edge_dc_reset_by_restart")[0][0, :, 0]
    assert got.tolist() == [30000] * 3 and 3 * 30000 > 32767 and scans["dc_reset_by_restart"][0]["restart_interval"] == 1
    # the damaged files: both parsers accept them, the restatement refuses each for its one reason
    damaged = sc.damaged_cases()
    assert len(damaged) == 6 + 18
    for name, (data, whys) in damaged.items():
        sc.parse_scans(data)
        rc, _info, _scans = _c_parse(lib, data)
        assert rc == 0, f"{name}: {lib.j2p_last_error().decode()}"
        with pytest.raises(sc.Refused) as e:
            sc.decode(data)
        assert e.value.code == sc.EFORMAT and e.value.why in whys, f"{name}: {e.value}"
        assert len(whys) == 1 or name == "scan_cut_short", name


def test_header_refusals_touch_no_device(lib):
    """every new entry point refuses on the parse alone: the right code, nothing written, on a machine with or without a GPU"""
    import jpeg2png_amd as j
    for name, (data, code) in sc.header_refusals().items():
        raw = np.frombuffer(data, dtype=np.uint8)
        rc, info, scans = _c_parse(lib, data)
        assert rc == code, f"{name}: {lib.j2p_last_error().decode()}"
        assert info.width == 0 and info.ncomp == 0 and scans.nscans == 0, name
        rooms = [np.full(1 << 16, 0x5A5A, dtype=np.int16) for _ in range(3)]
        ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in rooms])
        assert lib.j2p_entropy_decode_scans(0, raw.ctypes.data, raw.size, ptrs, None, None, 0, None) == code, name
        assert all((a == 0x5A5A).all() for a in rooms), name
        h = ctypes.c_void_p()
        pw = (ctypes.c_float * 3)(0.001, 0.001, 0.001)
        assert lib.j2p_solver_create_from_jpeg_scans(ctypes.byref(h), 0, None, raw.ctypes.data, raw.size, 0.3, pw, 10, None) == code, name
        assert not h.value, name
        with pytest.raises(j.J2PError) as e:
            j.jpeg_parse(data, progressive=True)
        assert e.value.code == code and code in (j.J2P_EFORMAT, j.J2P_ENOTSUP), name


def test_the_old_entry_points_still_refuse_progressive_files(lib):
    import jpeg2png_amd as j
    data = sc.good_files()["pil_41x23_q75_RGB2_plain"]
    with pytest.raises(j.J2PError) as e:
        j.jpeg_parse(data)
    assert e.value.code == j.J2P_ENOTSUP
    assert j.jpeg_parse(data, progressive=True)["progressive"]


def test_parser_survives_prefixes_and_damage_under_sanitizers(tmp_path):
    """tests/c/jpeg_scans_main.c with the parser compiled in, -fsanitize=address,undefined: host code only, run here on the CPU"""
    gcc = shutil.which("gcc")
    assert gcc, "no gcc (the library's own build needs it)"
    exe = str(tmp_path / "jpeg_scans_main")
    csrc = os.path.join(ROOT, "jpeg2png_amd", "csrc")
    subprocess.run([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "c", "jpeg_scans_main.c"),
                    os.path.join(csrc, "j2p_jpeg_parse.c"), "-o", exe], check=True, capture_output=True)
    files = sc.good_files()
    names = []
    for name in ("pil_8x8_q75_L0_rst_blocks", "pil_16x8_q30_RGB2_plain", "written_refine_3_tiny"):
        assert len(files[name]) < 1500, (name, len(files[name]))
        names.append(str(tmp_path / f"{name}.jpg"))
        open(names[-1], "wb").write(files[name])
    r = subprocess.run([exe, *names], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accepted" in r.stdout
