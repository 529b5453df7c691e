"""-D / --decode-any-on-gpu of the command-line driver (cli/jpeg2png_gpu.c): -d, and a progressive input's scans are all decoded
on the GPU (j2p_batch_next_file_scans) in place of libjpeg's jpeg_read_coefficients; every output is, byte for byte, the one of a
run without it, and nothing is printed."""
import pytest

from test_decode_cli import pil_jpeg
from test_jpeg_out_cli import cli, run  # noqa: F401


def test_decode_any_on_gpu_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-D, --decode-any-on-gpu" in r.stdout and "-d, --decode-on-gpu" in r.stdout


CASES = [  # (name, w, h, quality, PIL keywords, flags)
    ("progressive_420_odd", 83, 61, 75, {"subsampling": 2, "progressive": True}, ["-i", "5"]),
    ("progressive_grey", 40, 24, 30, {"mode": "L", "progressive": True}, ["-g", "-i", "4"]),
    ("progressive_restarts_422", 45, 38, 95, {"subsampling": 1, "progressive": True, "restart_marker_blocks": 3}, ["-s", "-i", "4,3,2"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_D_changes_no_byte_of_the_png_or_the_jpeg(cli, tmp_path, case):  # noqa: F811
    name, w, h, q, kw, flags = case
    jpg = str(tmp_path / "in.jpg")
    pil_jpeg(jpg, w, h, q, seed=len(name), **kw)
    for out, extra in (("png", []), ("jpg", ["-j", "90", "-e"])):
        plain, decoded = str(tmp_path / f"plain.{out}"), str(tmp_path / f"decoded.{out}")
        r = run(cli, jpg, "-o", plain, "-q", *flags, *extra)
        assert r.returncode == 0, r.stderr
        r = run(cli, jpg, "-o", decoded, "-q", *flags, *extra, "--decode-any-on-gpu" if len(name) % 2 else "-D")
        assert r.returncode == 0 and r.stderr == "", r.stderr
        want, got = open(plain, "rb").read(), open(decoded, "rb").read()
        assert len(want) > 300 and got == want, f"{name}: {out}"


@pytest.mark.gpu
def test_D_on_a_baseline_file_is_d(cli, tmp_path):  # noqa: F811
    jpg = str(tmp_path / "in.jpg")
    pil_jpeg(jpg, 64, 48, 75, 9, subsampling=2, restart_marker_blocks=3)
    outs = []
    for flag in ("-d", "-D"):
        out = str(tmp_path / f"out{flag}.png")
        r = run(cli, jpg, "-o", out, "-q", "-i", "5", flag)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        outs.append(open(out, "rb").read())
    assert len(outs[0]) > 300 and outs[0] == outs[1]
