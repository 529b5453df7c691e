"""Sample input without a GPU: (1) the restated definition (tests/samples_cases.py) recovers every coefficient of every shared case
from its decoded 8-bit samples — the precondition of the equality tests in tests/test_samples_gpu.py: if this fails the cases are
wrong, not the kernel; (2) jpeg_header on headers assembled byte by byte, and on a file PIL wrote against libjpeg's reading of it;
(3) the refusals of j2p_solver_create_from_samples that are made before a device is looked for."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import samples_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")


# ---- 1. the restatement recovers the cases' coefficients ----

def test_there_are_seven_fixtures_and_four_synthetic_cases():
    assert len(sc.FIXTURES) == 7 and len(sc.SYNTH) == 4 and set(sc.SOLVED) <= set(sc.FIXTURES)


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_recovers_every_coefficient(oracle, name):
    c = sc.case(name)
    for i, (p, s) in enumerate(zip(c.planes, c.samples)):
        assert s.shape == (p.h, p.w) and s.dtype == np.uint8
        assert int(np.min(p.quant_table)) >= 5, f"{name}: plane {i} has a step below 5"
        assert sc.clipped(s) == 0, f"{name}: plane {i} has clipped samples"
        got = sc.expected_coefficients(s, p.w, p.h, p.quant_table)
        want = np.asarray(p.data, np.int16).reshape(p.h // 8, p.w // 8, 64)
        assert np.array_equal(got, want), f"{name}: plane {i}: {int((got != want).sum())} of {want.size} coefficients not recovered"


def test_replication_is_edge_padding():
    s = np.arange(6, dtype=np.uint8).reshape(2, 3)
    r = sc.replicate(s, 8, 8)
    assert r.shape == (8, 8) and (r[:2, :3] == s).all() and (r[:, 3:] == r[:, 2:3]).all() and (r[2:] == r[1:2]).all()
    assert (sc.replicate(s[:1, :1], 8, 16) == 0).all()


def test_range_of_the_definition(oracle):
    """all-0 and all-255 planes with steps of 1: DC -1024 and 1016, everything else 0 — the int16 range the header states"""
    ones = np.ones(64, np.uint16)
    lo = sc.expected_coefficients(np.zeros((8, 16), np.uint8), 16, 8, ones)
    hi = sc.expected_coefficients(np.full((8, 16), 255, np.uint8), 16, 8, ones)
    assert (lo[..., 0] == -1024).all() and (hi[..., 0] == 1016).all() and not lo[..., 1:].any() and not hi[..., 1:].any()


# ---- 2. jpeg_header ----

def seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def dqt_table(slot, natural, sixteen=False):
    """one table of a DQT segment's body: the steps in zigzag order"""
    import jpeg2png_amd as j
    zz = [int(natural[k]) for k in j._NATURAL_OF_ZIGZAG]
    return bytes([(16 if sixteen else 0) | slot]) + (b"".join(struct.pack(">H", v) for v in zz) if sixteen else bytes(zz))


def sof(marker, width, height, comps, precision=8):
    return seg(marker, struct.pack(">BHHB", precision, height, width, len(comps)) + b"".join(bytes([i, (h << 4) | v, t]) for i, h, v, t in comps))


SOI, SOS = b"\xff\xd8", seg(0xDA, bytes([1, 1, 0, 0, 63, 0])) + b"\x12\x34\xff\xd9"
# tables whose entries are all distinct: any slip in the zigzag order shows
Q_A = (np.arange(64) * 3 + 1).astype(np.uint16)                 # 1 .. 190
Q_B = (255 - np.arange(64) * 2).astype(np.uint16)               # 255 .. 129
Q_16 = (np.arange(64) * 997 + 300).astype(np.uint16)            # 300 .. 63111: needs 16 bits
# T.81 figure A.6, written out: the natural-order index of the k-th zigzag coefficient (its first 20 and last 4)
ZIGZAG_HEAD, ZIGZAG_TAIL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33], [47, 55, 62, 63]


def test_zigzag_table():
    import jpeg2png_amd as j
    z = j._NATURAL_OF_ZIGZAG
    assert z[:20] == ZIGZAG_HEAD and z[-4:] == ZIGZAG_TAIL and sorted(z) == list(range(64))


def check_component(c, plane, cid, hs, vs, q, w, h, ws, hsamp, sw, sh):
    assert (c["id"], c["h_samp_factor"], c["v_samp_factor"]) == (cid, hs, vs)
    assert c["quant_table"].dtype == np.uint16 and np.array_equal(c["quant_table"], q)
    assert (c["w"], c["h"], c["w_samp"], c["h_samp"], c["samples_w"], c["samples_h"]) == (w, h, ws, hsamp, sw, sh)
    assert (plane.w, plane.h, plane.w_samp, plane.h_samp) == (w, h, ws, hsamp) and plane.data is None and plane.fdata is None
    assert np.array_equal(plane.quant_table, q)


def test_header_baseline_420_two_tables_in_one_segment():
    import jpeg2png_amd as j
    data = (SOI + seg(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0") + seg(0xDB, dqt_table(0, Q_A) + dqt_table(1, Q_B)) +
            seg(0xFE, b"a comment \xff\xda inside") + sof(0xC0, 101, 67, [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]) +
            seg(0xC4, b"\x00" + bytes(16)) + seg(0xE1, b"Exif\0\0" + bytes(30)) + SOS)
    h = j.jpeg_header(data)
    assert (h["width"], h["height"], h["progressive"]) == (101, 67, False) and len(h["components"]) == 3 and len(h["planes"]) == 3
    check_component(h["components"][0], h["planes"][0], 1, 2, 2, Q_A, 104, 72, 1, 1, 101, 67)
    check_component(h["components"][1], h["planes"][1], 2, 1, 1, Q_B, 56, 40, 2, 2, 51, 34)
    check_component(h["components"][2], h["planes"][2], 3, 1, 1, Q_B, 56, 40, 2, 2, 51, 34)
    # what read_jpeg checks (jpeg.c:59-64)
    for p in h["planes"]:
        assert p.h // 8 == (67 // p.h_samp + 7) // 8 and p.w // 8 == (101 // p.w_samp + 7) // 8


def test_header_progressive_444_sixteen_bit_table():
    import jpeg2png_amd as j
    data = SOI + seg(0xDB, dqt_table(2, Q_16, sixteen=True)) + sof(0xC2, 48, 32, [(0, 1, 1, 2), (1, 1, 1, 2), (7, 1, 1, 2)]) + SOS
    h = j.jpeg_header(data)
    assert (h["width"], h["height"], h["progressive"]) == (48, 32, True)
    for c, p, cid in zip(h["components"], h["planes"], (0, 1, 7)):
        check_component(c, p, cid, 1, 1, Q_16, 48, 32, 1, 1, 48, 32)


def test_header_greyscale_extended_with_a_table_replaced():
    """SOF1, one component; slot 0 is defined twice and the later definition holds; fill bytes before a marker"""
    import jpeg2png_amd as j
    data = SOI + seg(0xDB, dqt_table(0, Q_B)) + b"\xff\xff" + seg(0xDB, dqt_table(1, Q_B) + dqt_table(0, Q_A)) + sof(0xC1, 9, 17, [(1, 1, 1, 0)]) + SOS
    h = j.jpeg_header(data)
    assert (h["width"], h["height"], h["progressive"]) == (9, 17, False) and len(h["planes"]) == 1
    check_component(h["components"][0], h["planes"][0], 1, 1, 1, Q_A, 16, 24, 1, 1, 9, 17)


def test_header_422_and_440_sampling():
    import jpeg2png_amd as j
    for comps, ws, hs, sw, sh, w, h in (([(1, 2, 1, 0), (2, 1, 1, 0), (3, 1, 1, 0)], 2, 1, 19, 21, 24, 24),
                                        ([(1, 1, 2, 0), (2, 1, 1, 0), (3, 1, 1, 0)], 1, 2, 37, 11, 40, 16)):
        got = j.jpeg_header(SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC0, 37, 21, comps) + SOS)
        check_component(got["components"][0], got["planes"][0], 1, comps[0][1], comps[0][2], Q_A, 40, 24, 1, 1, 37, 21)
        check_component(got["components"][2], got["planes"][2], 3, 1, 1, Q_A, w, h, ws, hs, sw, sh)


@pytest.mark.parametrize("what,data", [
    ("missing table", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC0, 16, 16, [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]) + SOS),
    ("four components", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC0, 16, 16, [(1, 1, 1, 0), (2, 1, 1, 0), (3, 1, 1, 0), (4, 1, 1, 0)]) + SOS),
    ("twelve bits", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC1, 16, 16, [(1, 1, 1, 0)], precision=12) + SOS),
    ("truncated DQT", SOI + seg(0xDB, dqt_table(0, Q_A))[:40]),
    ("segment longer than the file", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC0, 16, 16, [(1, 1, 1, 0)])[:-3]),
    ("table cut short inside its segment", SOI + seg(0xDB, dqt_table(0, Q_A)[:30]) + sof(0xC0, 16, 16, [(1, 1, 1, 0)]) + SOS),
    ("no SOS", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC0, 16, 16, [(1, 1, 1, 0)])),
    ("no SOF", SOI + seg(0xDB, dqt_table(0, Q_A)) + SOS),
    ("lossless", SOI + seg(0xDB, dqt_table(0, Q_A)) + sof(0xC3, 16, 16, [(1, 1, 1, 0)]) + SOS),
    ("not a JPEG", b"\x89PNG\r\n\x1a\n" + bytes(32)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_header_errors(what, data):
    import jpeg2png_amd as j
    with pytest.raises(ValueError):
        j.jpeg_header(data)


@pytest.fixture(scope="module")
def read_coefficients(tmp_path_factory):
    """tests/c/read_coefficients.c compiled against libjpeg, as tests/test_jpeg_out_cli.py does"""
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg headers not available")
    exe = str(tmp_path_factory.mktemp("rc") / "read_coefficients")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "read_coefficients.c"),
                    "-o", exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    return exe


def check_against_libjpeg(exe, path):
    """jpeg_header of a file against libjpeg's reading of it: size, planes, sampling, tables"""
    import jpeg2png_amd as j
    from test_jpeg_out_cli import load_coefficients
    w, h, planes = load_coefficients(exe, path)
    got = j.jpeg_header(open(path, "rb").read())
    assert (got["width"], got["height"]) == (w, h) and len(got["planes"]) == 3
    for c, (p, g) in enumerate(zip(planes, got["planes"])):
        assert (g.w, g.h, g.w_samp, g.h_samp) == (p.w, p.h, p.w_samp, p.h_samp), f"component {c}"
        assert np.array_equal(g.quant_table, p.quant_table), f"component {c}"
    return got


@pytest.mark.parametrize("sub,progressive", [(2, False), (1, False), (0, True)], ids=["420", "422", "444_progressive"])
def test_header_of_a_pil_file_is_what_libjpeg_reads(read_coefficients, tmp_path, sub, progressive):
    from PIL import Image
    from jpeg2png_amd import synth
    path = str(tmp_path / "a.jpg")
    Image.fromarray(synth.synth_rgb(101, 67, 4).astype(np.uint8), "RGB").save(path, "JPEG", quality=90, subsampling=sub, progressive=progressive)
    got = check_against_libjpeg(read_coefficients, path)
    assert got["progressive"] == progressive


# ---- 3. refusals before a device is looked for ----

def create(lib, planes, samples, out=True, nchannel=None):
    import jpeg2png_amd as j
    n = len(planes)
    keep = [np.ascontiguousarray(p["q"], np.uint16) for p in planes]
    cpl = (j._CPlane * n)(*[j._CPlane(p["w"], p["h"], 1, 1, p.get("data"), p.get("fdata"), q.ctypes.data) for p, q in zip(planes, keep)])
    csm = None if samples is None else (j._CSamples * n)(*[j._CSamples(*s) for s in samples])
    pw = (ctypes.c_float * n)(*[0.001] * n)
    h = ctypes.c_void_p(0xDEAD)
    rc = lib.j2p_solver_create_from_samples(ctypes.byref(h) if out else None, 0, None, n if nchannel is None else nchannel, cpl, csm, 0.3, pw, 4)
    return rc, h.value, lib.j2p_last_error().decode()


def test_create_from_samples_refuses_bad_arguments_before_touching_a_device(lib):
    """every one of these is J2P_EINVAL whether or not a GPU is there, with *out NULL"""
    host = np.full((16, 24), 100, np.uint8)
    ptr = host.ctypes.data
    plane = {"w": 24, "h": 16, "q": np.full(64, 16)}
    good = (ptr, 24, 16, 24, 1)
    other = np.zeros(16 * 24, np.int16)
    cases = [
        ("samples is NULL", [plane], None),
        ("data is NULL", [plane], [(None, 24, 16, 24, 1)]),
        ("0x16 samples", [plane], [(ptr, 0, 16, 24, 1)]),
        ("24x0 samples", [plane], [(ptr, 24, 0, 24, 1)]),
        ("25x16 samples", [plane], [(ptr, 25, 16, 24, 1)]),
        ("24x17 samples", [plane], [(ptr, 24, 17, 24, 1)]),
        ("at least 1", [plane], [(ptr, 24, 16, 0, 1)]),
        ("at least 1", [plane], [(ptr, 24, 16, 24, 0)]),
        ("at least 1", [plane], [(ptr, 24, 16, -24, 1)]),
        ("no data / fdata", [dict(plane, data=other.ctypes.data)], [good]),
        ("no data / fdata", [dict(plane, fdata=other.ctypes.data)], [good]),
        ("multiple of 8", [dict(plane, w=20)], [(ptr, 20, 16, 24, 1)]),
        ("quantization table", [dict(plane, q=np.zeros(64))], [good]),
    ]
    for msg, planes, samples in cases:
        rc, h, err = create(lib, planes, samples)
        assert rc == -1 and h is None and msg in err, (msg, rc, h, err)
    rc, h, err = create(lib, [plane] * 4, [good] * 4)
    assert rc == -1 and h is None and "nchannel" in err
    rc, _, _ = create(lib, [plane], [good], out=False)
    assert rc == -1


def test_clipped_samples_and_download_refuse_null(lib):
    n = ctypes.c_ulonglong()
    assert lib.j2p_solver_clipped_samples(None, 0, ctypes.byref(n)) == -1
    assert lib.j2p_solver_download_coefficients(None, 0, None) == -1
