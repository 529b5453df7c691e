"""-O / --optimize of the command-line driver (cli/jpeg2png_gpu.c): with -j Q the file gets Huffman tables made for the image —
by libjpeg's optimize_coding in a run without -e, from symbol counts taken on the GPU (J2P_JPEG_OPTIMIZE) in a run with it — and
both runs write the same bytes, fewer than without -O; option handling on the CPU."""
import os

import pytest

from test_jpeg_out_cli import cli, make_jpeg, run  # noqa: F401


@pytest.mark.parametrize("args,msg", [
    (["-O", "-o", "y.png"], "-O needs JPEG output (-j)"),
    (["--optimize", "-o", "y.png"], "-O needs JPEG output (-j)"),
    (["-O", "-e", "-o", "y.png"], "-e needs JPEG output (-j)"),
    (["-O", "-j", "90"], "-j needs an output file name (-o) for every input"),
])
def test_option_errors(cli, args, msg):  # noqa: F811
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg") and not os.path.exists("y.png")


def test_optimize_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-O, --optimize" in r.stdout


CASES = [  # (name, w, h, input quality, input subsampling (PIL), mode, flags)
    ("colour_420", 83, 61, 40, 2, "RGB", ["-i", "5", "-j", "90", "-S", "420"]),
    ("grey", 61, 35, 30, 2, "L", ["-g", "-i", "5", "-j", "90"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_O_and_O_e_write_the_same_smaller_file(cli, tmp_path, case):  # noqa: F811
    name, w, h, q, sub, mode, flags = case
    jpg, plain, host, device = (str(tmp_path / n) for n in ("in.jpg", "plain.jpg", "host.jpg", "device.jpg"))
    make_jpeg(jpg, w, h, q, sub, seed=len(name), mode=mode)
    for out, extra in ((plain, []), (host, ["-O"]), (device, ["--optimize" if len(name) % 2 else "-O", "-e"])):
        r = run(cli, jpg, "-o", out, "-q", *flags, *extra)
        assert r.returncode == 0, r.stderr
    plain, host, device = (open(p, "rb").read() for p in (plain, host, device))
    assert device == host, f"{name}: -O -e writes {len(device)} bytes, -O {len(host)}"
    assert 300 < len(host) < len(plain)
    # the same image: only the DHT segments and the scan's bits differ
    from PIL import Image
    import io
    import numpy as np
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(host))), np.asarray(Image.open(io.BytesIO(plain))))
