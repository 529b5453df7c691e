"""-e / --encode-on-gpu of the command-line driver (cli/jpeg2png_gpu.c): with -j Q the file is entropy-coded on the GPU
(j2p_batch_submit_jpeg) and written as it comes down — the very bytes libjpeg writes in a run without -e; option handling on
the CPU."""
import os

import pytest

from test_jpeg_out_cli import cli, make_jpeg, run  # noqa: F401


@pytest.mark.parametrize("args,msg", [
    (["-e", "-o", "y.png"], "-e needs JPEG output (-j)"),
    (["--encode-on-gpu", "-o", "y.png"], "-e needs JPEG output (-j)"),
    (["-e", "-S", "420", "-o", "y.jpg"], "-S needs JPEG output (-j)"),
    (["-e", "-j", "101", "-o", "y.jpg"], "invalid jpeg quality"),
    (["-e", "-j", "90"], "-j needs an output file name (-o) for every input"),
])
def test_option_errors(cli, args, msg):  # noqa: F811
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg") and not os.path.exists("y.png")


def test_encode_on_gpu_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-e, --encode-on-gpu" in r.stdout


CASES = [  # (name, w, h, input quality, input subsampling (PIL), mode, flags)
    ("joint_444", 45, 38, 40, 0, "RGB", ["-i", "6", "-j", "90"]),
    ("separate", 83, 61, 20, 2, "RGB", ["-s", "-i", "5,3,2", "-j", "75"]),
    ("grey", 61, 35, 30, 2, "RGB", ["-g", "-i", "5", "-j", "95"]),
    ("grey_file", 40, 24, 30, 2, "L", ["-g", "-i", "4", "-j", "50"]),
    ("zoom_2", 37, 29, 40, 2, "RGB", ["-z", "2", "-i", "4", "-j", "90"]),
    ("S420", 101, 67, 30, 2, "RGB", ["-i", "6", "-j", "90", "-S", "420"]),
    ("S422", 45, 38, 40, 1, "RGB", ["-i", "5", "-j", "100", "-S", "422"]),
    ("S440_replicated", 40, 24, 20, 0, "RGB", ["-i", "5", "-j", "85", "--chroma-subsampling", "440"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_e_writes_the_bytes_libjpeg_writes(cli, tmp_path, case):  # noqa: F811
    name, w, h, q, sub, mode, flags = case
    jpg, plain, coded = (str(tmp_path / n) for n in ("in.jpg", "plain.jpg", "coded.jpg"))
    make_jpeg(jpg, w, h, q, sub, seed=len(name), mode=mode)
    r = run(cli, jpg, "-o", plain, "-q", *flags)
    assert r.returncode == 0, r.stderr
    r = run(cli, jpg, "-o", coded, "-q", *flags, "--encode-on-gpu" if len(name) % 2 else "-e")
    assert r.returncode == 0, r.stderr
    want, got = open(plain, "rb").read(), open(coded, "rb").read()
    assert len(want) > 300 and got == want
