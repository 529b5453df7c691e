"""`-r` / `--progressive` of the command-line driver: with -j the progressive file of libjpeg's jpeg_simple_progression(); with -e the
GPU codes every scan (j2p_batch_submit_jpeg_progressive, j2p_batch_submit_file_jpeg_progressive), without it libjpeg does — the same
bytes either way."""
import io
import os

import numpy as np
import pytest

from test_jpeg_out_cli import cli, make_jpeg, run  # noqa: F401


@pytest.mark.parametrize("args,msg", [
    (["-r", "-o", "y.png"], "-r needs JPEG output (-j)"),
    (["--progressive", "-o", "y.png"], "-r needs JPEG output (-j)"),
    (["-r", "-e", "-o", "y.png"], "-e needs JPEG output (-j)"),
    (["-r", "-j", "90"], "-j needs an output file name (-o) for every input"),
    (["-r", "-P", "-j", "90", "-o", "y.jpg"], "-P writes a PNG: not with JPEG output (-j)"),
])
def test_option_errors(cli, args, msg):  # noqa: F811
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg") and not os.path.exists("y.png")


def test_progressive_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-r, --progressive" in r.stdout


CASES = [  # (name, w, h, input quality, input subsampling (PIL), mode, flags)
    ("colour_420", 83, 61, 40, 2, "RGB", ["-i", "5", "-j", "90", "-S", "420"]),
    ("grey", 61, 35, 30, 2, "L", ["-g", "-i", "5", "-j", "90"]),
    ("colour_420_d_a_z", 45, 38, 50, 2, "RGB", ["-i", "3", "-j", "85", "-S", "420", "-d", "-a", "-z", "2"]),
    ("separate_444", 40, 24, 60, 0, "RGB", ["-i", "3", "-j", "75", "-s"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_r_and_r_e_write_the_same_progressive_file(cli, tmp_path, case):  # noqa: F811
    from PIL import Image
    name, w, h, q, sub, mode, flags = case
    jpg, plain, host, device, both = (str(tmp_path / n) for n in ("in.jpg", "plain.jpg", "host.jpg", "device.jpg", "both.jpg"))
    make_jpeg(jpg, w, h, q, sub, seed=len(name), mode=mode)
    for out, extra in ((plain, []), (host, ["-r"]), (device, ["--progressive" if len(name) % 2 else "-r", "-e"]), (both, ["-r", "-O", "-e"])):
        r = run(cli, jpg, "-o", out, "-q", *flags, *extra)
        assert r.returncode == 0, r.stderr
    plain, host, device, both = (open(p, "rb").read() for p in (plain, host, device, both))
    assert device == host, f"{name}: -r -e writes {len(device)} bytes, -r {len(host)}"
    assert both == host, "-O changed the progressive file"
    scans = 6 if mode == "L" or "-g" in flags else 10
    assert host.count(b"\xff\xda") >= scans and b"\xff\xc2" in host[:700]
    im, base = Image.open(io.BytesIO(host)), Image.open(io.BytesIO(plain))
    assert im.info.get("progressive") and not base.info.get("progressive")
    # the same coefficients: the same decoded image
    assert np.array_equal(np.asarray(im), np.asarray(base))
