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
    out = {f"written_{name}": data for name, (_case, data) in {**dc.framing_cases(), **dc.boundary_cases()}.items()}
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
    for name, (case, data) in {**dc.framing_cases(), **dc.boundary_cases()}.items():
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
    boundary_files_are_what_their_names_say()


def _scan(data):
    """(the entropy-coded data, the restated parser's frame)"""
    frame = dc.parse(data)
    return data[frame["scan_begin"]:frame["scan_end"]], frame


def boundary_files_are_what_their_names_say():
    """(the second half of test_written_files_are_what_their_names_say) every property that boundary_cases() aims at, read from
    the files' bytes: a case that stops aiming at its edge fails here.  The edges are those of k_unstuff_count / k_unstuff_copy (a lane reads 4 bytes, a wavefront 256, a workgroup 1024, counted
    from the first byte of the entropy-coded data), k_decode_intervals (256 intervals a workgroup) and the scans (1024 a tile)."""
    cases = dc.boundary_cases()
    assert tuple(cases) == dc.BOUNDARY
    # markers_on_edges: 24 MCUs, 23 markers, each Dn where its target says
    data = cases["markers_on_edges"][1]
    ecs, frame = _scan(data)
    at = dc.marker_offsets(data)
    assert frame["restart_interval"] == 1 and len(at) == 23 and len(ecs) > 4096
    assert [a % 256 for a in at] == [dc.EDGE_TARGETS[m % 6] for m in range(23)] and set(dc.EDGE_TARGETS) == {0, 1, 255, 254, 4, 3}
    assert all(ecs[a - 1] == 0xFF and ecs[a] == 0xD0 + m % 8 for m, a in enumerate(at))
    assert any(a % 1024 == 0 for a in at), "no marker's FF is the last byte of a 1024-byte group"
    edge = dc.stuffed_on_chunk_edge(data)
    assert edge and all(i % 256 == 255 and ecs[i:i + 2] == b"\xff\x00" for i in edge), "no stuffed FF | 00 across a chunk edge"
    # fill_covers_chunks: the same scan with 600 fill bytes in front of one marker of the middle: two whole chunks of nothing but FF
    data = cases["fill_covers_chunks"][1]
    ecs, frame = _scan(data)
    assert len(dc.marker_offsets(data)) == 23 and len(data) == len(dc.write_case(cases["fill_covers_chunks"][0], restart=1)) + 600
    blank = [c for c in range(len(ecs) // 256) if ecs[256 * c:256 * c + 256] == b"\xff" * 256]
    assert len(blank) == 2 and blank[1] == blank[0] + 1 and blank == dc.blank_chunks(data), f"chunks of fill bytes alone: {blank}"
    fill = ecs.index(b"\xff" * 600)                                             # 600 fill bytes, the marker's FF, its Dn
    assert fill <= 256 * blank[0] and 6 <= dc.marker_offsets(data).index(fill + 601) < 18
    # the interval counts
    for name, intervals, ri, last in (("intervals_257_grey", 257, 1, 1), ("intervals_1056_420", 1056, 1, 1), ("intervals_212_short_last", 212, 5, 1)):
        data = cases[name][1]
        ecs, frame = _scan(data)
        chunks, numbers = dc._intervals(ecs)
        _comps, mcus_w, mcus_h = dc.geometry(frame)
        assert (len(chunks), frame["restart_interval"]) == (intervals, ri) and numbers == [m % 8 for m in range(intervals - 1)], name
        assert mcus_w * mcus_h - (intervals - 1) * ri == last, name
    assert dc.geometry(dc.parse(cases["intervals_212_short_last"][1]))[1] == 33 and 33 % 5
    assert cases["intervals_1056_420"][1].count(b"\xff\xd7") == 131 and sum(a.shape[0] * a.shape[1] for a in cases["intervals_1056_420"][0]["coefficients"]) == 6336
    # skewed_tables: nearly one code a length, and the longest there is
    case, data = cases["skewed_tables"]
    frame = dc.parse(data)
    annex = dc.parse(dc.framing_cases()["restart_1"][1])
    used = dc.symbol_counts(case["coefficients"], case["width"], case["height"], case["sub"])
    for slot in (0, 1):
        lengths = {length for length, _code in frame["ac"][slot]}
        assert len(lengths) >= 12 and 16 in lengths and frame["ac"][slot] != annex["ac"][slot], sorted(lengths)
        # ... and the file uses every code of them, the 16-bit ones included
        assert sorted(frame["ac"][slot].values()) == sorted(used["ac"][slot])
    # dc_near_limit: the running DC reaches 32752 in the 16th block
    case, data = cases["dc_near_limit"]
    assert case["coefficients"][0].shape == (1, 16, 64) and int(case["coefficients"][0].max()) == 32752 == 16 * 2047
    assert np.array_equal(dc.decode(data)[0][0], case["coefficients"][0])


def test_placed_markers_keep_the_data():
    """place_markers adds fill bytes and nothing else"""
    cases = dc.boundary_cases()
    plain = dc.write_case(cases["markers_on_edges"][0], restart=1)
    for name, added in (("markers_on_edges", None), ("fill_covers_chunks", 600)):
        data = cases[name][1]
        assert dc._intervals(_scan(data)[0]) == dc._intervals(_scan(plain)[0]), name
        assert added is None or len(data) == len(plain) + added
    assert dc.place_markers(plain, []) == plain and dc.place_markers(plain, [None] * 23) == plain
    two = dc.place_markers(plain, [None, 7], fixed={0: 3})
    assert dc.marker_offsets(two)[0] == dc.marker_offsets(plain)[0] + 3 and dc.marker_offsets(two)[1] % 256 == 7
    assert dc.marker_offsets(two)[2:] == [a + len(two) - len(plain) for a in dc.marker_offsets(plain)[2:]]


def test_periodic_files(read_coefficients, read_component, tmp_path):  # noqa: F811
    """periodic_case: the 12x3 file is entropy_cases.encode's, the restatement's and libjpeg's; the 513x512 one (257 tiles of
    blocks for the scans of the device's decoder and coder, tests/test_decode_gpu.py) is the same period more often"""
    blocks, raw, nbits = dc.periodic_period()
    assert blocks.shape == (4, 64) and blocks[3, 0] == 0                        # every repetition starts from predictor 0
    assert nbits % 8 == 0 and len(raw) * 8 == nbits                             # no padding
    assert 40 <= nbits / 4 <= 44                                                # more 32-bit subsequences than blocks
    assert raw.count(b"\xff") == 1                                              # one stuffed byte a repetition
    assert all(0 < np.count_nonzero(b[1:]) <= 3 for b in blocks)
    quant = ec.quant_tables(75, 1)
    data, want = dc.periodic_case(12, 3)
    assert want.shape == (3, 12, 64) and data == ec.encode([want], 96, 24, quant)
    got, _ = dc.decode(data)
    assert np.array_equal(got[0], want)
    path = str(tmp_path / "periodic.jpg")
    open(path, "wb").write(data)
    assert np.array_equal(libjpeg_arrays(read_coefficients, read_component, path, 1)[0], want)
    big, coefficients = dc.periodic_case(513, 512)
    stuffed = raw.replace(b"\xff", b"\xff\x00")
    head = ec.header(4104, 4096, 1, (1, 1), quant)
    assert len(stuffed) == nbits // 8 + 1 and len(big) == len(head) + 65664 * len(stuffed) + 2
    assert big.startswith(head + stuffed * 12) and big.endswith(stuffed * 12 + b"\xff\xd9") and big.count(stuffed) == 65664
    assert coefficients.shape == (512, 513, 64) and coefficients.dtype == np.int16
    assert -(-513 * 512 // 1024) == 257                                         # tiles of the DC scan and of the coder's len[]
    assert np.array_equal(coefficients.reshape(-1, 4, 64)[[0, 1, 32832, 65663]], np.broadcast_to(blocks, (4, 4, 64)))
    assert np.array_equal(coefficients[:3, :12].reshape(-1, 64)[:12], want.reshape(-1, 64)[:12])


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


NEEDS_THE_KERNELS = ("dc_above_int16", "dc_below_int16", "leftover_byte", "leftover_many", "rst_doubled", "rst_before_eoi", "rst_empty_interval")


def test_some_damage_only_the_kernels_can_see(lib):
    """the C parser accepts these files: nothing in their marker segments or sizes is wrong, so it is the device's decoder that
    refuses them (tests/test_decode_gpu.py), as the restatement does only while it decodes"""
    import jpeg2png_amd as j
    damaged = dc.damaged_cases()
    for name in NEEDS_THE_KERNELS:
        data, _whys = damaged[name]
        info, frame = j.jpeg_parse(data), dc.parse(data)
        assert (info["scan_begin"], info["scan_end"]) == (frame["scan_begin"], frame["scan_end"]), name
    # the neighbours that are good files: 16 blocks of +2047 (boundary_cases) and of -2047, and the four blocks with nothing appended
    got, _ = dc.decode(dc._dc_file([-2047] * 16)[0])
    assert int(got[0].min()) == -32752
    assert damaged["dc_above_int16"][0] != dc.boundary_cases()["dc_near_limit"][1]
    ecs, _frame = _scan(damaged["leftover_many"][0])
    assert ecs.endswith(bytes([0x12, 0x34, 0x56, 0x78] * 8)) and _scan(damaged["leftover_byte"][0])[0] == ecs[:-32] + b"\x7f"
    dc.decode(damaged["leftover_byte"][0][:-3] + b"\xff\xd9")
    for name, doubled in (("rst_doubled", 4), ("rst_before_eoi", 8)):
        ecs, frame = _scan(damaged[name][0])
        chunks, numbers = dc._intervals(ecs)
        assert frame["restart_interval"] == 2 and numbers == [m % 8 for m in range(9)], name
        assert [k for k, c in enumerate(chunks) if not c] == [doubled + 1 if name == "rst_before_eoi" else doubled], name
    # the markers' count and numbers right, one interval empty, the seven others whole
    ecs, frame = _scan(damaged["rst_empty_interval"][0])
    chunks, numbers = dc._intervals(ecs)
    whole = dc._intervals(_scan(dc.write_case(ec.make(64, 8, 1, (1, 1), "sparse", seed=34), restart=1))[0])[0]
    assert frame["restart_interval"] == 1 and numbers == list(range(7)) and chunks == whole[:2] + [b""] + whole[3:] and all(whole)


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
