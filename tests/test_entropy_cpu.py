"""The baseline JPEG file the device's entropy coder has to write (include/jpeg2png_amd.h: "The JPEG file"), checked
without a GPU: the plain-Python restatement in tests/entropy_cases.py against libjpeg itself (tests/c/write_coefficients.c
makes the calls of the command-line driver's write_jpeg() on the same arrays), against the project's existing readers and
PIL, the quality tables against PIL's, the properties the directed cases are there for, and the refusals that need no device."""
import ctypes
import io
import struct
import subprocess

import numpy as np
import pytest

import entropy_cases as ec
from test_jpeg_out_cli import _helper, load_component, load_coefficients, pil_tables, read_component, read_coefficients  # noqa: F401

SUBS = {"444": (1, 1), "420": (2, 2), "422": (2, 1), "440": (1, 2)}
SIZES = [(1, 1), (8, 8), (16, 16), (40, 24), (41, 23), (24, 40), (17, 9)]


@pytest.fixture(scope="module")
def write_coefficients(tmp_path_factory):
    """tests/c/write_coefficients.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "write_coefficients")


@pytest.fixture(scope="module")
def directed():
    return ec.directed_cases()


def libjpeg_file(exe, case):
    n = len(case["coefficients"])
    raw = struct.pack("<6I", case["width"], case["height"], n, case["quality"], *case["sub"])
    raw += b"".join(np.ascontiguousarray(a, dtype=np.int16).tobytes() for a in case["coefficients"])
    return subprocess.run([exe], input=raw, capture_output=True, check=True).stdout


def restated(case):
    return ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])


def sweep():
    """every size x component count and sampling x content, at Q 50 and 95 alternately"""
    k = 0
    for w, h in SIZES:
        for ncomp, sub in [(1, "444")] + [(3, s) for s in SUBS]:
            for kind in ("zero", "dense", "last", "sparse"):
                k += 1
                yield f"{w}x{h}_{ncomp}_{sub}_{kind}", ec.make(w, h, ncomp, SUBS[sub], kind, seed=k, quality=(50, 95)[k % 2])


def test_restatement_is_libjpeg_byte_for_byte(write_coefficients, directed):
    cases = dict(sweep())
    cases.update(directed)
    assert len(cases) > 140
    for name, case in cases.items():
        assert restated(case) == libjpeg_file(write_coefficients, case), name


@pytest.mark.parametrize("name", ["sparse_41x23_420", "sparse_40x24_422", "sparse_41x23_440", "dense_24x40_444", "dc_swing"])
def test_existing_reader_gets_the_coefficients_back(read_coefficients, directed, tmp_path, name):  # noqa: F811
    case = directed[name]
    path = str(tmp_path / "restated.jpg")
    open(path, "wb").write(restated(case))
    w, h, planes = load_coefficients(read_coefficients, path)
    assert (w, h) == (case["width"], case["height"])
    for c, (plane, (gh, gw)) in enumerate(zip(planes, ec.grids(w, h, 3, case["sub"]))):
        assert (plane.w, plane.h) == (gw * 8, gh * 8), f"component {c}"
        assert (plane.w_samp, plane.h_samp) == ((1, 1) if c == 0 else case["sub"]), f"component {c}"
        assert np.array_equal(plane.quant_table, case["quant"][c]), f"component {c}"
        assert np.array_equal(plane.data.reshape(gh, gw, 64), case["coefficients"][c]), f"component {c}"


def test_existing_reader_gets_a_grey_file_back(read_component, directed, tmp_path):  # noqa: F811
    case = directed["grey_17x9_dense"]
    path = str(tmp_path / "restated.jpg")
    open(path, "wb").write(restated(case))
    w, h, n, plane = load_component(read_component, path)
    assert (w, h, n) == (17, 9, 1) and (plane.w, plane.h, plane.w_samp, plane.h_samp) == (24, 16, 1, 1)
    assert np.array_equal(plane.quant_table, case["quant"][0])
    assert np.array_equal(plane.data.reshape(2, 3, 64), case["coefficients"][0])


def test_pil_opens_the_files(directed):
    from PIL import Image
    for name, case in directed.items():
        if "dense" in name or "last" in name or name in ("dc_swing", "run_lengths"):
            continue            # (valid files, but coefficients no decoder's range checks were written for)
        im = Image.open(io.BytesIO(restated(case)))
        im.load()
        assert im.size == (case["width"], case["height"]) and im.mode == ("L" if len(case["coefficients"]) == 1 else "RGB"), name


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quality_tables_are_pils(read_coefficients, tmp_path, quality):  # noqa: F811
    import jpeg2png_amd as j
    for ncomp in (3,):
        want = pil_tables(read_coefficients, tmp_path, quality, ncomp)
        got = j.quality_tables(quality, ncomp)
        assert len(got) == ncomp and all(t.dtype == np.uint16 and np.array_equal(t, w) for t, w in zip(got, want))
    assert np.array_equal(j.quality_tables(quality, 1)[0], j.quality_tables(quality, 3)[0])


def test_case_preconditions(directed):
    """what the directed cases are there for, by the restatement alone"""
    for name in ("dense_24x40_444", "dense_368x368_420", "grey_17x9_dense"):
        case = directed[name]
        _file, stuffed, _short = ec.encode_report(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])
        assert stuffed > 0, name
    case = directed["aligned_end"]
    assert ec.encode_report(case["coefficients"], case["width"], case["height"], case["quant"])[2] == 0
    case = directed["stuffed_end"]
    data, _stuffed, short = ec.encode_report(case["coefficients"], case["width"], case["height"], case["quant"])
    assert short > 0 and data[-4:] == b"\xff\x00\xff\xd9"
    # 368x368 4:2:0: 3174 blocks in 529 MCUs — more than one workgroup's share of the scans (1024 positions) and, dense, of
    # the stuffing pass's scan (1024 chunks of 256 bytes)
    case = directed["dense_368x368_420"]
    assert len(ec.scan_order(368, 368, 3, (2, 2))) == 3174
    assert len(restated(case)) > 1024 * 256 * 2
    # dummy blocks at the right (5 blocks across, two per MCU) and at the bottom (3 block rows, two per MCU)
    right = bottom = 0
    for w, h in ((40, 24), (41, 23)):
        for sx, sy in ((2, 2), (2, 1), (1, 2)):
            bw, bh = -(-w // 8), -(-h // 8)
            dummies = sum(1 for s in ec.scan_order(w, h, 3, (sx, sy)) if s[1] is None)
            assert dummies == -(-bw // sx) * -(-bh // sy) * sx * sy - bw * bh, (w, h, sx, sy)
            right += sx == 2 and bw % 2 == 1 and dummies > 0
            bottom += sy == 2 and bh % 2 == 1 and dummies > 0
    assert right >= 2 and bottom >= 4
    assert sum(1 for s in ec.scan_order(1, 1, 3, (2, 2)) if s[1] is None) == 3


def test_refusals_without_a_device(lib):
    import jpeg2png_amd as j
    q = j.quality_tables(75, 3)
    good = [np.zeros((1, 1, 64), dtype=np.int16)] * 3

    def rc(tables, coefficients=good, width=8, height=8, sub=(1, 1)):
        n = len(coefficients)
        held = [np.ascontiguousarray(t, dtype=np.uint16) for t in tables]
        spec = j._CJpeg(width, height, sub[0], sub[1])
        for c in range(n):
            spec.quant[c] = held[c].ctypes.data
        arrays = [np.ascontiguousarray(a, dtype=np.int16) for a in coefficients]
        ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
        size = ctypes.c_size_t(0)
        return lib.j2p_entropy_encode(0, ctypes.byref(spec), ptrs, n, None, 0, ctypes.byref(size)), lib.j2p_last_error().decode()

    big = q[0].copy()
    big[5] = 256
    assert rc([big, q[1], q[2]])[0] == -1 and "above 255" in rc([big, q[1], q[2]])[1]
    other = q[1].copy()
    other[63] += 1
    assert rc([q[0], q[1], other])[0] == -1 and "quant[2] differs" in rc([q[0], q[1], other])[1]
    zero = q[0].copy()
    zero[0] = 0
    assert rc([zero, q[1], q[2]])[0] == -1
    bad = np.zeros((1, 1, 64), dtype=np.int16)
    bad[0, 0, 7] = 1024
    code, text = rc(q, [good[0], bad, good[2]])
    assert code == -1 and "1024" in text and "component 1" in text
    bad[0, 0, 7] = -1024
    assert rc(q, [bad, good[1], good[2]])[0] == -1
    assert rc(q, good, width=0)[0] == -1 and rc(q, good, height=65536)[0] == -1
    assert rc(q, good, sub=(3, 1))[0] == -1 and rc(q, good, sub=(1, 0))[0] == -1
    assert rc(q[:2], good[:2])[0] == -1           # two components
    with pytest.raises(j.J2PError):
        j.entropy_encode(good, 8, 8, [big, q[1], q[2]])
    with pytest.raises(j.J2PError):
        j.quality_tables(75, 2)
