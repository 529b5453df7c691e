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
