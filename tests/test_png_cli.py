"""PNG coded on the GPU by the command-line driver (-P, cli/jpeg2png_gpu.c): option handling on the CPU; on the GPU the pixels of the
file written — with and without -1, -g, -z 2, -s and -d, on 45x38 inputs — against the same run without -P, whose files the existing
command-line tests hold byte-identical to the reference program's; and the file itself against the restatement of those pixels."""
import numpy as np
import pytest

import png_cases as pc
from test_jpeg_out_cli import cli, make_jpeg, run  # noqa: F401  (cli: the fixture)


def test_refused_combinations_die_with_their_message(cli, tmp_path):      # noqa: F811
    jpg, out = str(tmp_path / "a.jpg"), str(tmp_path / "a.out")
    make_jpeg(jpg, 45, 38, 60, 2, seed=1)
    r = run(cli, jpg, "-o", out, "-P", "-j", "80")
    assert r.returncode != 0 and "jpeg2png: -P writes a PNG: not with JPEG output (-j)" in r.stderr
    r = run(cli, jpg, "-o", out, "-P", "-j", "80", "-e")
    assert r.returncode != 0 and "-P writes a PNG" in r.stderr
    r = run(cli, jpg, "-o", out, "-P", "-e")
    assert r.returncode != 0 and "-e needs JPEG output (-j)" in r.stderr
    r = run(cli, jpg, "-o", out, "--png-on-gpu", "-O")
    assert r.returncode != 0 and "-O needs JPEG output (-j)" in r.stderr
    r = run(cli, "-h")
    assert "-P, --png-on-gpu" in r.stdout


def pixels(path):
    """(mode, the samples as bytes a row: 16-bit ones high byte first) of a PNG file; 16-bit colour through the restatement's own
    reading of the file, since PIL keeps 8 bits of it"""
    import zlib
    from test_png_cpu import unfiltered
    data = open(path, "rb").read()
    idat, kinds = pc.idat_data(data)
    w, h, bits, colour = int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big"), data[24], data[25]
    bpp = (3 if colour == 2 else 1) * bits // 8
    assert data[26:29] == b"\0\0\0" and colour in (0, 2)
    return (w, h, bits, colour), unfiltered(zlib.decompress(idat), h, w * bpp, bpp), kinds


FLAGS = [(), ("-1",), ("-g",), ("-z", "2"), ("-s",), ("-d",), ("-1", "-g", "-z", "2"), ("-s", "-d", "-1")]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=["".join(f) or "plain" for f in FLAGS])
def test_png_on_gpu_holds_the_pixels_of_the_run_without_it(cli, tmp_path, flags):        # noqa: F811
    from PIL import Image
    jpg, a, b = str(tmp_path / "in.jpg"), str(tmp_path / "libpng.png"), str(tmp_path / "gpu.png")
    make_jpeg(jpg, 45, 38, 60, 2, seed=9)
    common = ["-q", "-i", "8", *flags]
    r = run(cli, jpg, "-o", a, *common)
    assert r.returncode == 0, r.stderr
    r = run(cli, jpg, "-o", b, "-P", *common)
    assert r.returncode == 0, r.stderr
    head_a, want, _ = pixels(a)
    head_b, got, kinds = pixels(b)
    zoom = 2 if "-z" in flags else 1
    assert head_a == head_b == (45 * zoom, 38 * zoom, 16 if "-1" in flags else 8, 0 if "-g" in flags else 2)
    assert np.array_equal(got, want)
    assert kinds == [b"IHDR"] + [b"IDAT"] * (len(kinds) - 2) + [b"IEND"]
    # the file is the restatement's of those pixels, and PIL reads it
    w, h, bits, colour = head_b
    assert open(b, "rb").read() == pc.encode(got, w, h, bits=bits, channels=3 if colour == 2 else 1)[0]
    im = Image.open(b)
    im.load()
    assert im.size == (w, h)
