"""Greyscale output in the command-line driver (-g, cli/jpeg2png_gpu.c): option handling and the component-count rule on
the CPU; on the GPU the PNG of one-component and three-component JPEGs against the UNMODIFIED reference's compute(1, ...)
on component 0 (read by tests/c/read_component.c), written as png.c:37-45 writes it with Cb = Cr = 0, and the CSV log
against the reference program's `-s -c` rows of channel 0."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_grey_gpu import grey_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jpeg2png_ref")


@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    from jpeg2png_amd.buildlib import build_cli
    exe = build_cli()
    if exe is None:
        pytest.skip("libjpeg / libpng headers not available")
    return exe


@pytest.fixture(scope="module")
def read_component(tmp_path_factory):
    """tests/c/read_component.c compiled against the same libjpeg as the driver"""
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg headers not available")
    exe = str(tmp_path_factory.mktemp("rc") / "read_component")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "read_component.c"),
                    "-o", exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    return exe


def make_jpeg(path, w, h, quality, mode, seed, subsampling=2):
    from PIL import Image
    from jpeg2png_amd import synth
    rgb = synth.synth_rgb(w, h, seed).astype(np.uint8)
    im = Image.fromarray(rgb, "RGB")
    if mode == "RGB":
        im.save(path, "JPEG", quality=quality, subsampling=subsampling)
    else:
        im.convert(mode).save(path, "JPEG", quality=quality)


def run(exe, *args, env=None):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)


def load_component(exe, jpg):
    """(image w, h, number of components, Plane of component 0) as libjpeg delivers them"""
    from jpeg2png_amd.synth import Plane
    raw = subprocess.run([exe, jpg], capture_output=True, check=True).stdout
    w, h, n, cw, ch, ws, hs = struct.unpack_from("<7I", raw, 0)
    off = 28
    q = np.frombuffer(raw, np.uint16, 64, off).copy()
    off += 128
    d = np.frombuffer(raw, np.int16, cw * ch, off).copy()
    assert off + 2 * cw * ch == len(raw)
    return w, h, n, Plane(cw, ch, ws, hs, d, q)


def read_png(path):
    """(width, height, bit depth, colour type, samples) of a PNG"""
    from PIL import Image
    raw = open(path, "rb").read()
    assert raw[12:16] == b"IHDR"
    w, h, depth, ctype = struct.unpack(">IIBB", raw[16:26])
    return w, h, depth, ctype, np.asarray(Image.open(path)).astype(np.uint32)


def expected(read_component, jpg, weight, pweight, its, zoom, bits):
    import jpeg2png_amd as j
    from oracle import bindings
    w, h, n, plane = load_component(read_component, jpg)
    z = j.zoomed([plane], zoom)
    z[0].fdata = bindings.decode_plane(z[0])
    want, _, _ = bindings.ref_compute(z, weight, [pweight], its)
    return n, grey_samples(want[0], w * zoom, h * zoom, bits).astype(np.uint32)


# ---- CPU ----

def test_greyscale_in_usage(cli):
    r = run(cli)
    assert r.returncode == 1 and "-g, --greyscale" in r.stdout and "joint" in r.stdout


@pytest.mark.parametrize("args,msg", [
    (["-z", "0"], "invalid zoom factor"),
    (["-z", "5"], "invalid zoom factor"),
    (["-w", "1,2,3"], "different weights are only possible when using separated components"),
    (["-i", "1,2,3"], "different iteration counts are only possible when using separated components"),
])
def test_option_errors_are_unchanged_with_g(cli, args, msg):
    r = run(cli, "x.jpg", "-g", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg


def test_four_component_jpeg_is_refused_with_g_before_gpu_work(cli, tmp_path):
    jpg = str(tmp_path / "cmyk.jpg")
    make_jpeg(jpg, 40, 24, 50, "CMYK", seed=1)
    png = str(tmp_path / "cmyk.png")
    r = run(cli, jpg, "-g", "-o", png, "-q")
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: only 1 and 3 component jpegs are supported with -g"
    assert not os.path.exists(png)


# ---- GPU ----

GREY_CASES = [  # (name, w, h, quality, iterations, flags, zoom, bits)
    ("q10_i5", 37, 29, 10, 5, [], 1, 8),
    ("q40_i12_16bit", 101, 67, 40, 12, ["-1"], 1, 16),
    ("q75_i20_z2", 45, 38, 75, 20, ["-z", "2"], 2, 8),
    ("q25_i8_16bit_z2", 58, 21, 25, 8, ["-1", "-z", "2"], 2, 16),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GREY_CASES, ids=[c[0] for c in GREY_CASES])
def test_one_component_png_is_the_reference_luma(cli, read_component, oracle, tmp_path, case):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    name, w, h, q, its, flags, zoom, bits = case
    jpg, png = str(tmp_path / "g.jpg"), str(tmp_path / "g.png")
    make_jpeg(jpg, w, h, q, "L", seed=len(name))
    r = run(cli, jpg, "-g", "-i", str(its), "-o", png, "-q", *flags)
    assert r.returncode == 0, r.stderr
    n, want = expected(read_component, jpg, 0.3, 0.001, its, zoom, bits)
    assert n == 1
    pw, ph, depth, ctype, got = read_png(png)
    assert (pw, ph, depth, ctype) == (w * zoom, h * zoom, bits, 0)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_one_component_jpeg_without_g_is_still_refused(cli, tmp_path):
    jpg = str(tmp_path / "g.jpg")
    make_jpeg(jpg, 32, 16, 50, "L", seed=2)
    r = run(cli, jpg, "-o", str(tmp_path / "g.png"), "-q")
    assert r.returncode == 1 and r.stderr.strip() == "jpeg2png: only 3 component jpegs are supported"


@pytest.mark.gpu
@pytest.mark.parametrize("sub,flags,weight,pweight,its", [
    (2, ["-i", "9"], 0.3, 0.001, 9),
    (0, ["-s", "-w", "0.5,0.1,0", "-p", "0.002,0.001,0.001", "-i", "7,3,2", "-1"], 0.5, 0.002, 7),
], ids=["420", "444_s_lists_16bit"])
def test_colour_png_is_the_reference_y_and_csv_is_channel_0_of_s(cli, read_component, oracle, tmp_path, sub, flags, weight,
                                                                 pweight, its):
    if not (oracle.have_ref() and os.path.exists(REF_CLI)):
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    w, h = 83, 61
    jpg, png, csv = str(tmp_path / "c.jpg"), str(tmp_path / "c.png"), str(tmp_path / "c.csv")
    make_jpeg(jpg, w, h, 20, "RGB", seed=7, subsampling=sub)
    r = run(cli, jpg, "-g", "-o", png, "-q", "-c", csv, *flags)
    assert r.returncode == 0, r.stderr
    bits = 16 if "-1" in flags else 8
    n, want = expected(read_component, jpg, weight, pweight, its, 1, bits)
    assert n == 3
    pw, ph, depth, ctype, got = read_png(png)
    assert (pw, ph, depth, ctype) == (w, h, bits, 0)
    assert np.array_equal(got, want)

    ref_csv = str(tmp_path / "ref.csv")
    ref_flags = [f for f in flags if f != "-s"]
    if "-s" not in flags:
        ref_flags = ["-i", str(its)]
    rr = run(REF_CLI, jpg, "-o", str(tmp_path / "ref.png"), "-q", "-t", "1", "-s", "-c", ref_csv, *ref_flags)
    assert rr.returncode == 0, rr.stderr
    cols = (1, 2, 3, 4, 5, 6)
    ref_rows = np.loadtxt(ref_csv, delimiter=",", skiprows=1, usecols=cols, ndmin=2)
    ref_rows = ref_rows[ref_rows[:, 0] == 0]
    gpu_rows = np.loadtxt(csv, delimiter=",", skiprows=1, usecols=cols, ndmin=2)
    assert gpu_rows.shape == ref_rows.shape == (its, 6)
    gpu_rows = gpu_rows[np.argsort(gpu_rows[:, 1])]
    ref_rows = ref_rows[np.argsort(ref_rows[:, 1])]
    np.testing.assert_allclose(gpu_rows, ref_rows, rtol=0, atol=2e-6 * max(1.0, np.abs(ref_rows).max()))


@pytest.mark.gpu
def test_mixed_files_threads_and_row_tiling_give_the_single_file_bytes(cli, tmp_path):
    """colour and grey JPEGs in one -g call with -t 2, and one file row-tiled over J2P_DEVICES (the GPU twice where
    there is one; the band gate lowered): every PNG equals that file's PNG from a run of its own"""
    names = []
    for i, mode in enumerate(["L", "RGB", "L"]):
        p = str(tmp_path / f"m{i}.jpg")
        make_jpeg(p, 48 + 16 * i, 40, 30, mode, seed=20 + i)
        names.append(p)
    alone = []
    for i, p in enumerate(names):
        out = str(tmp_path / f"alone{i}.png")
        r = run(cli, p, "-g", "-i", "6", "-o", out, "-q")
        assert r.returncode == 0, r.stderr
        alone.append(open(out, "rb").read())
    r = run(cli, *names, "-g", "-i", "6", "-t", "2", "-q")
    assert r.returncode == 0, r.stderr
    for i in range(3):
        assert open(str(tmp_path / f"m{i}.png"), "rb").read() == alone[i], i

    big = str(tmp_path / "big.jpg")
    make_jpeg(big, 64, 200, 30, "L", seed=4)
    one, two = str(tmp_path / "one.png"), str(tmp_path / "two.png")
    r = run(cli, big, "-g", "-i", "6", "-o", one, "-q")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, J2P_DEVICES="0,0", J2P_TILE_MIN_BAND_PIXELS="1")
    r = run(cli, big, "-g", "-i", "6", "-o", two, "-q", env=env)
    assert r.returncode == 0 and "not row-tiling" not in r.stderr, r.stderr
    assert open(one, "rb").read() == open(two, "rb").read()
