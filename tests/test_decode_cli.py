"""-d / --decode-on-gpu of the command-line driver (cli/jpeg2png_gpu.c): the input's scan is Huffman-decoded on the GPU
(j2p_entropy_decode) in place of libjpeg's jpeg_read_coefficients, and every output is, byte for byte, the one of a run without
-d; files the decoder does not read fall back to libjpeg after one line on stderr; damaged ones fail."""
import io

import numpy as np
import pytest

from test_jpeg_out_cli import cli, run  # noqa: F401


def pil_jpeg(path, w, h, quality, seed, mode="RGB", **kw):
    from PIL import Image
    from jpeg2png_amd import synth
    im = Image.fromarray(synth.synth_rgb(w, h, seed).astype(np.uint8), "RGB").convert(mode)
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    open(path, "wb").write(buf.getvalue())
    return buf.getvalue()


def test_decode_on_gpu_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-d, --decode-on-gpu" in r.stdout


CASES = [  # (name, w, h, quality, PIL keywords, flags)
    ("baseline_420", 64, 48, 75, {"subsampling": 2}, ["-i", "6"]),
    ("optimised_444", 45, 38, 95, {"subsampling": 0, "optimize": True}, ["-i", "5"]),
    ("restarts_420_odd", 83, 61, 30, {"subsampling": 2, "restart_marker_blocks": 3}, ["-s", "-i", "5,3,2"]),
    ("restart_rows_422", 41, 23, 100, {"subsampling": 1, "restart_marker_rows": 1}, ["-i", "4", "-z", "2"]),
    ("grey_of_colour", 61, 35, 50, {"subsampling": 2, "optimize": True}, ["-g", "-i", "5"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_d_changes_no_byte_of_the_png_or_the_jpeg(cli, tmp_path, case):  # noqa: F811
    name, w, h, q, kw, flags = case
    jpg = str(tmp_path / "in.jpg")
    pil_jpeg(jpg, w, h, q, seed=len(name), **kw)
    for out, extra in (("png", []), ("jpg", ["-j", "90", "-e"])):
        plain, decoded = str(tmp_path / f"plain.{out}"), str(tmp_path / f"decoded.{out}")
        r = run(cli, jpg, "-o", plain, "-q", *flags, *extra)
        assert r.returncode == 0, r.stderr
        r = run(cli, jpg, "-o", decoded, "-q", *flags, *extra, "--decode-on-gpu" if len(name) % 2 else "-d")
        assert r.returncode == 0 and r.stderr == "", r.stderr
        want, got = open(plain, "rb").read(), open(decoded, "rb").read()
        assert len(want) > 300 and got == want, f"{name}: {out}"


@pytest.mark.gpu
def test_a_grey_file_and_a_csv_log(cli, tmp_path):  # noqa: F811
    jpg = str(tmp_path / "in.jpg")
    pil_jpeg(jpg, 40, 24, 30, 3, mode="L")
    logs = []
    for name, extra in (("plain", []), ("decoded", ["-d"])):
        out, csv = str(tmp_path / f"{name}.png"), str(tmp_path / f"{name}.csv")
        r = run(cli, jpg, "-o", out, "-q", "-g", "-i", "4", "-t", "1", "-c", csv, *extra)
        assert r.returncode == 0, r.stderr
        logs.append((open(out, "rb").read(), open(csv).read()))
    assert logs[0] == logs[1] and len(logs[0][1].splitlines()) >= 4


@pytest.mark.gpu
def test_a_progressive_file_falls_back_to_libjpeg(cli, tmp_path):  # noqa: F811
    jpg, plain, decoded = (str(tmp_path / n) for n in ("in.jpg", "plain.png", "decoded.png"))
    pil_jpeg(jpg, 45, 38, 60, 7, subsampling=2, progressive=True)
    assert run(cli, jpg, "-o", plain, "-q", "-i", "4").returncode == 0
    r = run(cli, jpg, "-o", decoded, "-q", "-i", "4", "-d")
    assert r.returncode == 0, r.stderr
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("jpeg2png: ") and "progressive" in lines[0] and lines[0].endswith("decoding with libjpeg")
    assert open(plain, "rb").read() == open(decoded, "rb").read()


@pytest.mark.gpu
def test_a_truncated_file_fails(cli, tmp_path):  # noqa: F811
    jpg, out = str(tmp_path / "in.jpg"), str(tmp_path / "out.png")
    data = pil_jpeg(jpg, 64, 48, 75, 5, subsampling=2)
    cut = data[:len(data) * 2 // 3]
    open(jpg, "wb").write(cut)
    r = run(cli, jpg, "-o", out, "-q", "-i", "3", "-d")
    assert r.returncode != 0 and r.stderr.startswith("jpeg2png: ") and "jpeg:" in r.stderr
    # ... and so does a scan that ends early in front of an intact EOI
    open(jpg, "wb").write(cut + b"\xff\xd9")
    r = run(cli, jpg, "-o", out, "-q", "-i", "3", "-d")
    assert r.returncode != 0 and "jpeg:" in r.stderr
