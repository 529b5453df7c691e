"""Zooming in the command-line driver (-z N, cli/jpeg2png_gpu.c): option errors and the canvas limit on the CPU; on the
GPU the zoomed PNG against the library's batch engine on the same coefficients (read by tests/c/read_coefficients.c)
and those planes against the UNMODIFIED reference's compute() on the zoomed sampling factors."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")


@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    from jpeg2png_amd.buildlib import build_cli
    exe = build_cli()
    if exe is None:
        pytest.skip("libjpeg / libpng headers not available")
    return exe


@pytest.fixture(scope="module")
def read_coefficients(tmp_path_factory):
    """tests/c/read_coefficients.c compiled against the same libjpeg as the driver"""
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg headers not available")
    exe = str(tmp_path_factory.mktemp("rc") / "read_coefficients")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "read_coefficients.c"),
                    "-o", exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    return exe


def make_jpeg(path, w, h, quality, subsampling, seed):
    from PIL import Image
    from jpeg2png_amd import synth
    rgb = synth.synth_rgb(w, h, seed).astype(np.uint8)
    Image.fromarray(rgb, "RGB").save(path, "JPEG", quality=quality, subsampling=subsampling)


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def load_coefficients(exe, jpg):
    """(image w, h, [Plane] of the three components) as libjpeg delivers them"""
    from jpeg2png_amd.synth import Plane
    raw = subprocess.run([exe, jpg], capture_output=True, check=True).stdout
    w, h = struct.unpack_from("<2I", raw, 0)
    off, planes = 8, []
    for _ in range(3):
        cw, ch, ws, hs = struct.unpack_from("<4I", raw, off)
        off += 16
        q = np.frombuffer(raw, np.uint16, 64, off).copy()
        off += 128
        n = cw * ch
        d = np.frombuffer(raw, np.int16, n, off).copy()
        off += 2 * n
        planes.append(Plane(cw, ch, ws, hs, d, q))
    assert off == len(raw)
    return w, h, planes


@pytest.mark.parametrize("value", ["0", "5", "x", "2x", "-1", ""])
def test_invalid_zoom_factor(cli, value):
    r = run(cli, "x.jpg", "-z", value)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: invalid zoom factor"


def test_zoom_in_usage(cli):
    r = run(cli)
    assert r.returncode == 1 and "-z, --zoom N" in r.stdout


def test_zoomed_canvas_above_the_height_limit_is_refused_before_any_gpu_work(cli, tmp_path):
    """16392 columns of 4:2:0 zoomed 4 times: a 65600-pixel-wide canvas (the chroma planes pad to 8200 columns), refused
    with a message before any GPU work"""
    jpg = str(tmp_path / "wide.jpg")
    make_jpeg(jpg, 16392, 16, 50, 2, seed=3)
    r = run(cli, jpg, "-z", "4", "-o", str(tmp_path / "wide.png"), "-q")
    assert r.returncode == 1
    assert "zoomed canvas" in r.stderr and "65600x64" in r.stderr and "at most 65536 per side" in r.stderr
    assert not os.path.exists(tmp_path / "wide.png")


@pytest.mark.gpu
def test_zoom_2_png_equals_batch_rgb_and_reference_planes(cli, read_coefficients, tmp_path, lib, oracle):
    from PIL import Image
    import jpeg2png_amd as j
    w, h, its = 150, 100, 6
    jpg = str(tmp_path / "a.jpg")
    make_jpeg(jpg, w, h, 30, 2, seed=11)                              # 4:2:0
    png = str(tmp_path / "a.png")
    r = run(cli, jpg, "-z", "2", "-i", str(its), "-o", png, "-q")
    assert r.returncode == 0, r.stderr
    img = np.asarray(Image.open(png).convert("RGB"))
    assert img.shape == (2 * h, 2 * w, 3)

    iw, ih, planes = load_coefficients(read_coefficients, jpg)
    assert (iw, ih) == (w, h) and [(p.w_samp, p.h_samp) for p in planes] == [(1, 1), (2, 2), (2, 2)]
    z = j.zoomed(planes, 2)
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        rgb = b.wait(b.submit(z, 0.3, [0.001] * 3, its, width=2 * w, height=2 * h, bits=8))
        got = b.wait(b.submit(z, 0.3, [0.001] * 3, its))
    assert np.array_equal(img, rgb)

    for p in z:
        p.fdata = oracle.decode_plane(p)
    want, _, _ = oracle.ref_compute(z, 0.3, [0.001] * 3, its)
    for c in range(3):
        assert got[c].shape == want[c].shape == (max(p.h * p.h_samp for p in z), max(p.w * p.w_samp for p in z))
        assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), f"channel {c}"


@pytest.mark.gpu
def test_zoom_1_is_byte_identical_to_no_flag_and_zoom_runs_separate_and_16_bit(cli, tmp_path):
    from PIL import Image
    jpg = str(tmp_path / "b.jpg")
    make_jpeg(jpg, 120, 72, 40, 2, seed=5)
    outs = {}
    for name, extra in [("plain", []), ("z1", ["-z", "1"]), ("z2s", ["-z", "2", "-s"]), ("z2_16", ["--zoom", "2", "-1"]),
                        ("z3", ["-z", "3"])]:
        out = str(tmp_path / f"{name}.png")
        r = run(cli, jpg, "-i", "4", "-o", out, "-q", *extra)
        assert r.returncode == 0, (name, r.stderr)
        outs[name] = out
    assert open(outs["plain"], "rb").read() == open(outs["z1"], "rb").read()
    for name, scale, mode in [("z2s", 2, "RGB"), ("z2_16", 2, None), ("z3", 3, "RGB")]:
        im = Image.open(outs[name])
        assert im.size == (120 * scale, 72 * scale), name
        if mode:
            assert im.mode == mode
