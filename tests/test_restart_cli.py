"""-R / --restart of the command-line driver (cli/jpeg2png_gpu.c): with -j Q the file gets restart markers every N MCU rows (-R N) or
every N MCUs (-R NB), as cjpeg -restart spells them — written by libjpeg (restart_in_rows / restart_interval) in a run without -e, on
the GPU (j2p_batch_submit_jpeg_opt, j2p_batch_submit_file_jpeg_opt) in a run with it — and both runs write the same bytes, with and
without -O and -r; option handling on the CPU."""
import io
import os

import numpy as np
import pytest

import restart_cases as rc
from test_jpeg_out_cli import cli, make_jpeg, run  # noqa: F401


@pytest.mark.parametrize("args,msg", [
    (["-R", "1", "-o", "y.png"], "-R needs JPEG output (-j)"),
    (["--restart", "3B", "-o", "y.png"], "-R needs JPEG output (-j)"),
    (["-R", "1", "-e", "-o", "y.png"], "-e needs JPEG output (-j)"),
    (["-R", "0", "-j", "90", "-o", "y.jpg"], "invalid restart interval"),
    (["-R", "65536", "-j", "90", "-o", "y.jpg"], "invalid restart interval"),
    (["-R", "3X", "-j", "90", "-o", "y.jpg"], "invalid restart interval"),
    (["-R", "-1", "-j", "90", "-o", "y.jpg"], "invalid restart interval"),
    (["-R", "B", "-j", "90", "-o", "y.jpg"], "invalid restart interval"),
])
def test_option_errors(cli, args, msg):  # noqa: F811
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg") and not os.path.exists("y.png")


def test_restart_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-R, --restart N | NB" in r.stdout


CASES = [  # (name, w, h, input quality, input subsampling (PIL), mode, flags, MCUs per row of the output, MCU rows)
    ("colour_420", 83, 61, 40, 2, "RGB", ["-i", "5", "-j", "90", "-S", "420"], 6, 4),
    ("grey", 61, 35, 30, 2, "L", ["-g", "-i", "5", "-j", "90"], 8, 5),
]
CODERS = [("baseline", []), ("optimized", ["-O"]), ("progressive", ["-r"])]


@pytest.mark.gpu
@pytest.mark.parametrize("coder", CODERS, ids=[c[0] for c in CODERS])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_R_and_R_e_write_the_same_file(cli, tmp_path, case, coder):  # noqa: F811
    from PIL import Image
    name, w, h, q, sub, mode, flags, per_row, rows = case
    jpg, plain = str(tmp_path / "in.jpg"), str(tmp_path / "plain.jpg")
    make_jpeg(jpg, w, h, q, sub, seed=len(name), mode=mode)
    r = run(cli, jpg, "-o", plain, "-q", *flags, *coder[1])
    assert r.returncode == 0, r.stderr
    plain = open(plain, "rb").read()
    for restart, interval in (("1", per_row), ("3B", 3)):
        host, device = str(tmp_path / f"host_{restart}.jpg"), str(tmp_path / f"device_{restart}.jpg")
        for out, extra in ((host, ["-R", restart]), (device, ["--restart", restart, "-e"])):
            r = run(cli, jpg, "-o", out, "-q", *flags, *coder[1], *extra)
            assert r.returncode == 0, r.stderr
        host, device = open(host, "rb").read(), open(device, "rb").read()
        assert device == host, f"{name}, {coder[0]}, -R {restart}: -e writes {len(device)} bytes, libjpeg {len(host)}"
        # the first scan counts MCUs: its interval and its markers are the option's
        dri, in_force, rst = rc.parse_restarts(host)[0]
        markers = -(-per_row * rows // interval) - 1
        assert (dri, in_force, rst) == (interval, interval, [k % 8 for k in range(markers)])
        assert len(host) > len(plain)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(host))), np.asarray(Image.open(io.BytesIO(plain))))
