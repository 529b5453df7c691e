"""Reading a JPEG file (include/jpeg2png_amd.h: "Reading a JPEG file"), checked without a GPU: the plain-Python restatement of
tests/decode_cases.py against libjpeg's jpeg_read_coefficients (the existing read_coefficients / read_component helpers) on
writer-made and PIL-made files, and as the inverse of entropy_cases.encode; the library's C parser (j2p_jpeg_parse) against
jpeg_header(); the refusals that the marker segments alone decide, which touch no device; and the parser under sanitizers,
as a stand-alone program."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import decode_cases as dc
import entropy_cases as ec
from test_jpeg_out_cli import PREFIX, load_component, load_coefficients, read_component, read_coefficients  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_files():
    """{name: file}: PIL-made files, the whole product of sizes, qualities, samplings (and grey) and forms"""
    from PIL import Image
    from jpeg2png_amd import synth
    out = {}
    forms = [("optimize", {"optimize": True}), ("rst_blocks", {"restart_marker_blocks": 3}), ("rst_rows", {"restart_marker_rows": 1}), ("plain", {})]
    for w, h in ((1, 1), (8, 8), (17, 9), (41, 23), (64, 48)):
        rgb = synth.synth_rgb(w, h, 7 * w + h).astype(np.uint8)
        for quality in (30, 75, 95, 100):
            for mode, sub in (("RGB", 0), ("RGB", 1), ("RGB", 2), ("L", 0)):
                for name, kw in forms:
                    im = Image.fromarray(rgb, "RGB").convert(mode)
                    buf = io.BytesIO()
                    im.save(buf, "JPEG", quality=quality, **({"subsampling": sub} if mode == "RGB" else {}), **kw)
                    out[f"{w}x{h}_q{quality}_{mode}{sub}_{name}"] = buf.getvalue()
    return out


@pytest.fixture(scope="module")
def files():
    """every good file of this module: {name: file}"""
    out = {f"written_{name}": data for name, (_case, data) in dc.framing_cases().items()}
    for name, case in ec.directed_cases().items():
        if "368" not in name:
            out[f"directed_{name}"] = ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])
    out.update({f"pil_{name}": data for name, data in pil_files().items()})
    return out


def libjpeg_arrays(read3, read1, path, ncomp):
    if ncomp == 3:
        _w, _h, planes = load_coefficients(read3, path)
        return [p.data.reshape(p.h // 8, p.w // 8, 64) for p in planes]
    _w, _h, _n, p = load_component(read1, path)
    return [np.asarray(p.data).reshape(p.h // 8, p.w // 8, 64)]


def test_restated_decoder_is_libjpeg(read_coefficients, read_component, files, tmp_path):  # noqa: F811
    assert len(files) > 350
    for name, data in files.items():
        path = str(tmp_path / "file.jpg")
        open(path, "wb").write(data)
        got, frame = dc.decode(data)
        want = libjpeg_arrays(read_coefficients, read_component, path, len(frame["components"]))
        assert len(got) == len(want), name
        for c, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: component {c}"


def test_written_files_hold_their_coefficients():
    for name, (case, data) in dc.framing_cases().items():
        got, _ = dc.decode(data)
        for c, (a, b) in enumerate(zip(got, case["coefficients"])):
            assert np.array_equal(a, b), f"{name}: component {c}"


def test_written_files_are_what_their_names_say():
    cases = dc.framing_cases()
    assert any(b"\xff\x00\xff" + bytes([0xd0 + n]) in cases["stuffed_before_rst"][1] for n in range(8))
    assert cases["restart_wraps"][1].count(b"\xff\xd7") == 2 and dc.parse(cases["restart_wraps"][1])["restart_interval"] == 1
    assert b"\xff\xff\xff\xd0" in cases["fill_bytes"][1] and cases["fill_bytes"][1].endswith(b"\xff\xff\xff\xd9")
    assert not cases["trailing_bytes"][1].endswith(b"\xff\xd9")
    own, annex = dc.parse(cases["own_tables"][1]), dc.parse(cases["restart_1"][1])
    assert own["ac"][0] != annex["ac"][0] and len(cases["own_tables"][1]) < len(cases["swapped_tables"][1])
    swapped = dc.parse(cases["swapped_tables"][1])
    assert sorted(swapped["dc"]) == [2, 3] and [c[4:] for c in swapped["components"]] == [[2, 2], [3, 3], [3, 3]]
    assert swapped["ac"][2] == annex["ac"][1] and swapped["ac"][3] == annex["ac"][0]
    assert [c[1:3] for c in dc.parse(cases["sparse_41x23_411"][1])["components"]] == [[4, 1], [1, 1], [1, 1]]


def test_restated_decoder_inverts_encode():
    for name, case in ec.directed_cases().items():
        got, _ = dc.decode(ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"]))
        for c, (a, b) in enumerate(zip(got, case["coefficients"])):
            assert np.array_equal(a, b), f"{name}: component {c}"


def test_restated_decoder_refuses_the_damaged_files():
    for name, (data, whys) in dc.damaged_cases().items():
        with pytest.raises(dc.Refused) as e:
            dc.decode(data)
        assert e.value.code == dc.EFORMAT and e.value.why in whys, f"{name}: {e.value}"


def test_c_parser_agrees_with_jpeg_header(lib, files):
    import jpeg2png_amd as j
    for name, data in files.items():
        info, head, frame = j.jpeg_parse(data), j.jpeg_header(data), dc.parse(data)
        assert (info["width"], info["height"]) == (head["width"], head["height"]), name
        assert len(info["components"]) == len(head["components"]), name
        for a, b, f in zip(info["components"], head["components"], frame["components"]):
            for key in ("id", "h_samp_factor", "v_samp_factor", "w", "h", "w_samp", "h_samp"):
                assert a[key] == b[key], f"{name}: {key}"
            assert np.array_equal(a["quant_table"], b["quant_table"]), name
            assert [a["quant_slot"], a["dc_slot"], a["ac_slot"]] == f[3:], name
        assert (info["scan_begin"], info["scan_end"], info["restart_interval"]) == (frame["scan_begin"], frame["scan_end"], frame["restart_interval"]), name
        _comps, mcus_w, mcus_h = dc.geometry(frame)
        assert (info["mcus_w"], info["mcus_h"]) == (mcus_w, mcus_h), name
        ri = frame["restart_interval"] or mcus_w * mcus_h
        assert info["intervals"] == -(-mcus_w * mcus_h // ri), name


# ---- refusals the marker segments decide ----
def _replace_segment(data, marker, new_body=None, new_marker=None):
    """the file with its first segment `marker` given another body, another marker byte, or (both None) removed"""
    at = data.index(bytes([0xff, marker]))
    n = int.from_bytes(data[at + 2:at + 4], "big")
    if new_body is None and new_marker is None:
        return data[:at] + data[at + 2 + n:]
    body = data[at + 4:at + 2 + n] if new_body is None else new_body
    return data[:at] + ec._segment(marker if new_marker is None else new_marker, body) + data[at + 2 + n:]


def header_refusals():
    """{name: (file, code)}"""
    from PIL import Image
    from jpeg2png_amd import synth
    case = ec.make(16, 16, 3, (2, 2), "sparse", seed=3)
    good = dc.write_case(case)
    grey = dc.write_case(ec.make(16, 8, 1, (1, 1), "sparse", seed=4))
    sof = good[good.index(b"\xff\xc0") + 4:][:15]
    im = Image.fromarray(synth.synth_rgb(24, 16, 5).astype(np.uint8), "RGB")

    def pil(**kw):
        buf = io.BytesIO()
        (im.convert("CMYK") if kw.pop("cmyk", False) else im).save(buf, "JPEG", **kw)
        return buf.getvalue()

    out = {
        "progressive": (pil(progressive=True), dc.ENOTSUP),
        "arithmetic": (_replace_segment(good, 0xc0, new_marker=0xc9), dc.ENOTSUP),
        "lossless": (_replace_segment(good, 0xc0, new_marker=0xc3), dc.ENOTSUP),
        "hierarchical": (_replace_segment(good, 0xc0, new_marker=0xc5), dc.ENOTSUP),
        "twelve_bits": (_replace_segment(good, 0xc0, bytes([12]) + sof[1:]), dc.ENOTSUP),
        "four_components": (pil(cmyk=True), dc.ENOTSUP),
        "several_scans": (_replace_segment(grey, 0xc0, sof[:5] + bytes([3, 1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0])), dc.ENOTSUP),
        "dnl": (_replace_segment(good, 0xc0, sof[:1] + b"\0\0" + sof[3:]), dc.ENOTSUP),
        "dnl_segment": (good.replace(b"\xff\xda", ec._segment(0xdc, b"\0\x10") + b"\xff\xda", 1), dc.ENOTSUP),
        "second_scan": (good[:-2] + good[good.index(b"\xff\xda"):], dc.ENOTSUP),
        "not_a_jpeg": (b"\x89PNG\r\n\x1a\n" + good, dc.EFORMAT),
        "no_huffman_table": (_replace_segment(good, 0xc4), dc.EFORMAT),
        "no_quantisation_table": (_replace_segment(good, 0xdb), dc.EFORMAT),
        "no_frame": (_replace_segment(good, 0xc0), dc.EFORMAT),
        "truncated_header": (good[:200], dc.EFORMAT),
        # a few hundred bytes that claim 65535 x 65535 samples and a restart marker per MCU: refused, and nothing allocated
        "claims_a_huge_frame": (_replace_segment(good, 0xc0, sof[:1] + b"\xff\xff\xff\xff" + sof[5:]).replace(b"\xff\xda", ec._segment(0xdd, b"\0\1") + b"\xff\xda", 1), dc.EFORMAT),
        "truncated_scan": (good[:-2], dc.EFORMAT),
        "ends_in_ff": (good[:-1], dc.EFORMAT),
        "zero_sampling": (_replace_segment(good, 0xc0, sof[:7] + b"\x02" + sof[8:]), dc.EFORMAT),
        "eleven_blocks": (_replace_segment(good, 0xc0, sof[:7] + b"\x33" + sof[8:]), dc.EFORMAT),
        "spectral_selection": (good.replace(b"\x00\x3f\x00", b"\x01\x3f\x00", 1), dc.EFORMAT),
        "oversubscribed_table": (_replace_segment(good, 0xc4, bytes([0, 3] + [0] * 15) + bytes(3)), dc.EFORMAT),
        "dc_category_16": (_replace_segment(good, 0xc4, bytes([0, 0, 1] + [0] * 14) + bytes([16])), dc.EFORMAT),
    }
    return out


def test_restated_parser_refuses_what_the_headers_show():
    for name, (data, code) in header_refusals().items():
        with pytest.raises(dc.Refused) as e:
            dc.parse(data)
        assert e.value.code == code, f"{name}: {e.value}"


def test_header_refusals_touch_no_device(lib):
    """every entry point refuses on the parse alone: the right code, nothing written, on a machine with or without a GPU"""
    import jpeg2png_amd as j
    for name, (data, code) in header_refusals().items():
        raw = np.frombuffer(data, dtype=np.uint8)
        info = j._CJpegInfo()
        assert lib.j2p_jpeg_parse(raw.ctypes.data, raw.size, ctypes.byref(info)) == code, f"{name}: {lib.j2p_last_error().decode()}"
        assert info.width == 0 and info.ncomp == 0, name
        rooms = [np.full(1 << 16, 0x5A5A, dtype=np.int16) for _ in range(3)]
        ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in rooms])
        assert lib.j2p_entropy_decode(0, raw.ctypes.data, raw.size, ptrs, None, None) == code, name
        assert all((a == 0x5A5A).all() for a in rooms), name
        h = ctypes.c_void_p()
        pw = (ctypes.c_float * 3)(0.001, 0.001, 0.001)
        assert lib.j2p_solver_create_from_jpeg(ctypes.byref(h), 0, None, raw.ctypes.data, raw.size, 0.3, pw, 10, None) == code, name
        assert not h.value, name
        with pytest.raises(j.J2PError) as e:
            j.jpeg_parse(data)
        assert e.value.code == code and code in (j.J2P_EFORMAT, j.J2P_ENOTSUP), name


def test_subsequence_lengths_outside_the_range_are_refused(lib):
    import jpeg2png_amd as j
    data = np.frombuffer(dc.write_case(ec.make(16, 8, 1, (1, 1), "sparse", seed=4)), dtype=np.uint8)
    room = np.zeros(2 * 64, dtype=np.int16)
    ptrs = (ctypes.c_void_p * 3)(room.ctypes.data, None, None)
    for bits in (1, j.J2P_DECODE_SUBSEQUENCE_MIN - 1, j.J2P_DECODE_SUBSEQUENCE_MAX + 1):
        assert lib.j2p_entropy_decode_ex(0, data.ctypes.data, data.size, ptrs, None, None, bits, None) == -1, bits


def test_parser_survives_prefixes_and_damage_under_sanitizers(tmp_path):
    """tests/c/jpeg_parse_main.c with the parser compiled in, -fsanitize=address,undefined: host code only, run here on the CPU"""
    gcc = shutil.which("gcc")
    assert gcc, "no gcc (the library's own build needs it)"
    exe = str(tmp_path / "jpeg_parse_main")
    csrc = os.path.join(ROOT, "jpeg2png_amd", "csrc")
    subprocess.run([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "c", "jpeg_parse_main.c"),
                    os.path.join(csrc, "j2p_jpeg_parse.c"), "-o", exe], check=True, capture_output=True)
    grey = ec.make(16, 8, 1, (1, 1), "sparse", seed=4)
    small = ec.make(16, 16, 3, (2, 2), "sparse", seed=3)
    names = []
    for name, data in (("grey", dc.write_case(grey, restart=1, fill=True)), ("own", dc.write_case(small, tables="own", dqt16=True)),
                       ("swapped", dc.write_case(small, tables="swapped", trailing=b"\xff\xd9tail"))):
        assert len(data) < 1200, name
        names.append(str(tmp_path / f"{name}.jpg"))
        open(names[-1], "wb").write(data)
    r = subprocess.run([exe, *names], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accepted" in r.stdout
