"""-a / --auto-orient of the command-line driver (cli/jpeg2png_gpu.c): on PIL-made files with Orientation tags the PNG's pixels —
through libpng and through -P — are the restatement's permutation (tests/upright_cases.py) of the run without -a, the
coefficients of the file -j 90 -e writes are those of the library path (Solver.from_jpeg(upright=True).to_jpeg), a file without
the tag gives the same bytes with and without -a, and a row-tiled run refuses -a with one line."""
import os

import numpy as np
import pytest

import upright_cases as uc
from test_jpeg_out_cli import cli, load_coefficients, read_coefficients, run  # noqa: F401

ITS = 4
W, H = 45, 38


def tagged_file(tmp_path, o):
    path = str(tmp_path / f"tag{o}.jpg")
    data = uc.pil_jpeg(W, H, seed=21, orientation=o)
    open(path, "wb").write(data)
    return path, data


def pixels(path):
    from PIL import Image
    im = Image.open(path)
    assert "exif" not in im.info
    return np.asarray(im)


def convert(cli, jpg, out, *flags):  # noqa: F811
    r = run(cli, jpg, "-o", out, "-q", "-i", str(ITS), *flags)
    assert r.returncode == 0, r.stderr
    return out


# ---- CPU ----

def test_usage_names_the_option(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-a, --auto-orient" in r.stdout


def test_row_tiled_run_refuses_auto_orient_with_one_line(cli, tmp_path):  # noqa: F811
    """two GPUs named for one file: the image would be row-tiled over them.  Refused before anything is opened."""
    import subprocess
    out = str(tmp_path / "o.png")
    r = subprocess.run([cli, "x.jpg", "-a", "-o", out, "-q"], capture_output=True, text=True, timeout=60, env={**os.environ, "J2P_DEVICES": "0,0"})
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: -a is not supported for row-tiled images (fewer files than GPUs)"
    assert len(r.stderr.strip().splitlines()) == 1 and not os.path.exists(out)


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("o", [1, 6, 7])
def test_png_pixels_are_the_permuted_pixels_of_the_run_without(cli, tmp_path, o):  # noqa: F811
    jpg, _ = tagged_file(tmp_path, o)
    for name, flags in (("libpng", []), ("gpu", ["-P"]), ("libpng16", ["-1"]), ("decoded_on_gpu", ["-d", "-P"])):
        plain = pixels(convert(cli, jpg, str(tmp_path / f"plain_{name}.png"), *flags))
        assert plain.shape == (H, W, 3)
        turned = pixels(convert(cli, jpg, str(tmp_path / f"turned_{name}.png"), "-a", *flags))
        assert np.array_equal(turned, uc.upright(plain, o)), (o, name)
    # -s: three solvers of one channel each
    plain = pixels(convert(cli, jpg, str(tmp_path / "plain_s.png"), "-s"))
    turned = pixels(convert(cli, jpg, str(tmp_path / "turned_s.png"), "-s", "-a"))
    assert np.array_equal(turned, uc.upright(plain, o))
    # -g and -z: greyscale, zoomed 2x
    plain = pixels(convert(cli, jpg, str(tmp_path / "plain_gz.png"), "-g", "-z", "2"))
    turned = pixels(convert(cli, jpg, str(tmp_path / "turned_gz.png"), "-g", "-z", "2", "--auto-orient"))
    assert plain.shape == (2 * H, 2 * W) and np.array_equal(turned, uc.upright(plain, o))


@pytest.mark.gpu
@pytest.mark.parametrize("o", [1, 6, 7])
def test_jpeg_coefficients_are_the_library_paths(lib, cli, read_coefficients, tmp_path, o):  # noqa: F811
    import jpeg2png_amd as j
    jpg, data = tagged_file(tmp_path, o)
    uw, uh = uc.upright_size(o, W, H)
    with j.Solver.from_jpeg(data, 0.3, [0.001] * 3, ITS, upright=True) as s:
        assert s.orientation == o
        s.run(ITS)
        want = {"444": s.to_jpeg(uw, uh, quality=90), "420": s.to_jpeg(uw, uh, quality=90, subsampling=(2, 2))}
    for sub, flags in (("444", ["-e"]), ("420", ["-e", "-S", "420"]), ("444", [])):
        out = convert(cli, jpg, str(tmp_path / f"out_{sub}_{len(flags)}.jpg"), "-a", "-j", "90", *flags)
        assert uc.orientation(open(out, "rb").read()) == 1
        path = str(tmp_path / f"want_{sub}.jpg")
        open(path, "wb").write(want[sub])
        gw, gh, got = load_coefficients(read_coefficients, out)
        ww, wh, exp = load_coefficients(read_coefficients, path)
        assert (gw, gh) == (ww, wh) == (uw, uh)
        for c in range(3):
            assert (got[c].w, got[c].h, got[c].w_samp, got[c].h_samp) == (exp[c].w, exp[c].h, exp[c].w_samp, exp[c].h_samp)
            assert np.array_equal(got[c].quant_table, exp[c].quant_table) and np.array_equal(got[c].data, exp[c].data), (o, sub, flags, c)


@pytest.mark.gpu
def test_a_file_without_the_tag_gives_the_same_bytes(cli, tmp_path):  # noqa: F811
    jpg = str(tmp_path / "bare.jpg")
    open(jpg, "wb").write(uc.strip_app_segments(uc.pil_jpeg(W, H, seed=22, orientation=6)))
    for name, flags in (("a.png", []), ("b.png", ["-P"]), ("c.jpg", ["-j", "90", "-e"]), ("d.jpg", ["-j", "90", "-S", "420"])):
        without = open(convert(cli, jpg, str(tmp_path / ("without_" + name)), *flags), "rb").read()
        with_a = open(convert(cli, jpg, str(tmp_path / ("with_" + name)), "-a", *flags), "rb").read()
        assert without == with_a, name


@pytest.mark.gpu
@pytest.mark.parametrize("o", [3, 6, 7])
def test_separate_components_of_an_image_whose_canvases_differ(cli, tmp_path, o):  # noqa: F811
    """-s -a at 23x9 4:2:0: the luma's canvas is 24 columns wide, the chroma's 32, so the three solvers' planes are permuted with
    different source strides — through the libpng path, -P and -j -e.  (23, not 17: the driver, as the reference program, refuses
    files whose chroma width in blocks is not that of floor(width / 2).)"""
    jpg = str(tmp_path / f"small{o}.jpg")
    open(jpg, "wb").write(uc.pil_jpeg(23, 9, seed=23, orientation=o))
    for name, flags in (("libpng", []), ("gpu", ["-P"])):
        plain = pixels(convert(cli, jpg, str(tmp_path / f"plain_{name}.png"), "-s", *flags))
        assert plain.shape == (9, 23, 3)
        turned = pixels(convert(cli, jpg, str(tmp_path / f"turned_{name}.png"), "-s", "-a", *flags))
        assert np.array_equal(turned, uc.upright(plain, o)), (o, name)
    # the file the GPU codes is the file libjpeg codes from the coefficients that came down
    on_gpu = open(convert(cli, jpg, str(tmp_path / "e.jpg"), "-s", "-a", "-j", "90", "-e"), "rb").read()
    on_host = open(convert(cli, jpg, str(tmp_path / "h.jpg"), "-s", "-a", "-j", "90"), "rb").read()
    assert on_gpu == on_host
