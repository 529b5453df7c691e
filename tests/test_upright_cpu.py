"""Upright output without a GPU: the numpy restatement of the eight maps against PIL's ImageOps.exif_transpose, the two readers
of the Orientation tag (jpeg_orientation in Python, j2p_jpeg_orientation in C) against PIL's getexif() and on damaged
structures, the C reader under sanitizers, and the ctypes mirror of j2p_job, which keeps its layout."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import upright_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_orientation(file):
    from PIL import Image
    return Image.open(io.BytesIO(file)).getexif().get(uc.TAG, 1)


def both_readers(lib, file):
    import jpeg2png_amd as j
    got = j.jpeg_orientation(file)
    assert j.jpeg_orientation_c(file) == got == uc.orientation(file)
    return got


@pytest.mark.parametrize("o", uc.ORIENTATIONS)
def test_the_restatement_is_exif_transpose(o):
    from PIL import Image, ImageOps
    rng = np.random.default_rng(o)
    for w, h, channels in ((7, 5, 3), (5, 7, 1), (1, 4, 3), (6, 1, 1)):
        pixels = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
        im = Image.fromarray(pixels if channels == 3 else pixels[:, :, 0])
        exif = Image.Exif()
        exif[uc.TAG] = o
        im.info["exif"] = exif.tobytes()
        im.getexif()[uc.TAG] = o
        want = np.asarray(ImageOps.exif_transpose(im)).reshape(uc.upright_size(o, w, h)[::-1] + (channels,))
        got = uc.upright(pixels, o)
        assert got.shape == want.shape and np.array_equal(got, want), (w, h)


def test_replication_beyond_the_upright_image():
    image = np.arange(5 * 7).reshape(5, 7)
    for o in uc.ORIENTATIONS:
        u = uc.upright(image, o)
        uh, uw = u.shape
        W, H = uc.upright_canvas(o, 7, 5)
        assert W % 16 == 0 and H % 16 == 0 and W >= uw and H >= uh
        c = uc.upright(image, o, canvas=(W, H))
        assert np.array_equal(c[:uh, :uw], u)
        assert np.array_equal(c[uh:, :uw], np.repeat(u[-1:, :], H - uh, 0)) and np.array_equal(c[:, uw:], np.repeat(c[:, uw - 1:uw], W - uw, 1))
    # a source image smaller than the array it lies in: the mirror is taken about the image, not about the array
    assert np.array_equal(uc.upright(image, 3, w=4, h=3), image[:3, :4][::-1, ::-1])


@pytest.mark.parametrize("o", uc.ORIENTATIONS)
def test_readers_against_pil_on_pil_made_files(lib, o):
    file = uc.pil_jpeg(24, 16, seed=o, orientation=o)
    assert b"MM\0*" in file[:64]
    assert both_readers(lib, file) == pil_orientation(file) == o


def test_readers_against_pil_on_hand_built_segments(lib):
    bare = uc.strip_app_segments(uc.pil_jpeg(24, 16, seed=3))
    assert both_readers(lib, bare) == pil_orientation(bare) == 1                    # no such segment
    for order in ("II", "MM"):
        for o in uc.ORIENTATIONS:
            file = uc.insert_segments(bare, uc.exif_segment(uc.orientation_tiff(order, o)))
            assert both_readers(lib, file) == pil_orientation(file) == o, (order, o)
        # IFD0 not right behind the header
        file = uc.insert_segments(bare, uc.exif_segment(uc.orientation_tiff(order, 5, ifd_offset=20, pad=b"\0" * 12)))
        assert both_readers(lib, file) == pil_orientation(file) == 5
    # APP0, COM and a second APP1 (XMP) in front of the Exif segment
    front = (uc.segment(0xe0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0") + uc.segment(0xfe, b"a comment") +
             uc.segment(0xe1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>"))
    file = uc.insert_segments(bare, front + uc.exif_segment(uc.orientation_tiff("II", 8)))
    assert both_readers(lib, file) == pil_orientation(file) == 8
    # a progressive file: nothing is decoded, so it is read like a baseline one (which the decoder refuses)
    import jpeg2png_amd as j
    progressive = uc.pil_jpeg(24, 16, seed=4, orientation=6, progressive=True)
    with pytest.raises(j.J2PError):
        j.jpeg_parse(progressive)
    assert both_readers(lib, progressive) == pil_orientation(progressive) == 6
    # the first Exif segment decides
    file = uc.insert_segments(bare, uc.exif_segment(uc.orientation_tiff("MM", 3)) + uc.exif_segment(uc.orientation_tiff("MM", 6)))
    assert both_readers(lib, file) == 3
    # a tag behind the scan's start is not looked for
    sos = bare.index(b"\xff\xda")
    assert both_readers(lib, bare[:sos] + bare[sos:] + uc.exif_segment(uc.orientation_tiff("MM", 6))) == 1


def test_readers_return_1_for_what_does_not_count(lib):
    bare = uc.strip_app_segments(uc.pil_jpeg(24, 16, seed=3))
    for order in ("II", "MM"):
        good = uc.orientation_tiff(order, 6)
        cases = {
            "absent tag": uc.tiff(order, [(0x010f, 3, 1, 7), (0x0128, 3, 1, 2)]),
            "value 0": uc.orientation_tiff(order, 0),
            "value 9": uc.orientation_tiff(order, 9),
            "LONG-typed": uc.orientation_tiff(order, 6, kind=4),
            "count 2": uc.orientation_tiff(order, 6, n=2),
            "IFD offset beyond the segment": uc.orientation_tiff(order, 6, ifd_offset=4000)[:len(good)],
            "entry count overruns the segment": uc.orientation_tiff(order, 6, count=40),
            "wrong magic": good[:2] + b"\x2b\x2b" + good[4:],
            "unknown byte order": b"XX" + good[2:],
            "truncated header": good[:7],
            "truncated entries": good[:8 + 2 + 12 + 6],
        }
        assert both_readers(lib, uc.insert_segments(bare, uc.exif_segment(good))) == 6
        for name, t in cases.items():
            assert both_readers(lib, uc.insert_segments(bare, uc.exif_segment(t))) == 1, (order, name)
    for data in (b"", b"\xff", b"\xff\xd8", b"not a jpeg at all", b"\xff\xd8\xff\xe1\x00"):
        assert both_readers(lib, data) == 1
    assert lib.j2p_jpeg_orientation(None, 0, None) == -1


def test_c_reader_survives_prefixes_and_damage_under_sanitizers(tmp_path):
    """tests/c/orientation_main.c with the reader compiled in, -fsanitize=address,undefined: host code only, run here on the CPU"""
    gcc = shutil.which("gcc")
    assert gcc, "no gcc (the library's own build needs it)"
    exe = str(tmp_path / "orientation_main")
    csrc = os.path.join(ROOT, "jpeg2png_amd", "csrc")
    subprocess.run([gcc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "c", "orientation_main.c"),
                    os.path.join(csrc, "j2p_jpeg_parse.c"), "-o", exe], check=True, capture_output=True)
    bare = uc.strip_app_segments(uc.pil_jpeg(8, 8, seed=1, grey=True, quality=20))
    front = uc.segment(0xe0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0") + uc.segment(0xe1, b"http://ns.adobe.com/xap/1.0/\0<x/>")
    names = []
    for name, data in (("ii_6", uc.insert_segments(bare, front + uc.exif_segment(uc.orientation_tiff("II", 6)))),
                       ("mm_7", uc.insert_segments(bare, uc.exif_segment(uc.orientation_tiff("MM", 7, ifd_offset=12, pad=b"\0" * 4)))),
                       ("none_1", bare)):
        assert len(data) < 1200, name
        names.append(str(tmp_path / f"{name}.jpg"))
        open(names[-1], "wb").write(data)
    r = subprocess.run([exe, *names], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "oriented" in r.stdout


def test_symbols_and_the_job_struct_that_did_not_grow(lib):
    """the orientation travels next to the job (j2p_batch_next_orientation): j2p_job and its ctypes mirror keep their layout, with
    out_tensor last"""
    import jpeg2png_amd as j
    size, off = j.job_layout()
    assert size == ctypes.sizeof(j._CJob) and off == j._CJob.out_tensor.offset and off + ctypes.sizeof(j._CTensor) == size
    for name in ("j2p_jpeg_orientation", "j2p_solver_set_orientation", "j2p_solver_orientation", "j2p_solver_upright_bytes",
                 "j2p_batch_next_orientation"):
        assert name in j.C_ABI_SYMBOLS and hasattr(lib, name)
    assert j.J2P_ORIENTATION_EXIF == 0xffffffff
    assert lib.j2p_batch_next_orientation(None, 6, 4, 4) == -1
