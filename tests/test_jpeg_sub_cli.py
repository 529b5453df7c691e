"""Subsampled JPEG output of the command-line driver (-j Q -S 422|420|440, cli/jpeg2png_gpu.c): option handling on the
CPU; on the GPU the file written — size, per-component sampling and plane sizes as libjpeg reads them back, libjpeg's
tables for Q, and every quantised coefficient — against the definition (test_jpeg_sub_gpu.sub_means, then
expected_coefficients) applied to the UNMODIFIED reference's solve of the same input, for joint, zoomed and separate
runs and for a grid that overhangs the canvas; and the decoded file against the detour it replaces (the run's 8-bit PNG
encoded by PIL at the same quality and subsampling), for subsampled sources."""
import io
import os
import subprocess

import numpy as np
import pytest

from test_jpeg_out_cli import (cli, float_rgb, load_coefficients, make_jpeg, pil_tables, psnr_to, read_coefficients,  # noqa: F401
                               reference_planes, run)
from test_jpeg_out_gpu import expected_coefficients
from test_jpeg_sub_gpu import ceil_div, expected_sub

FACTORS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}


# ---- CPU ----

@pytest.mark.parametrize("args,msg", [
    (["-j", "90", "-S", "411", "-o", "y.jpg"], "invalid chroma subsampling"),
    (["-j", "90", "-S", "", "-o", "y.jpg"], "invalid chroma subsampling"),
    (["-j", "90", "--chroma-subsampling", "4:2:0", "-o", "y.jpg"], "invalid chroma subsampling"),
    (["-S", "421", "-o", "y.jpg"], "invalid chroma subsampling"),
    (["-S", "420", "-o", "y.png"], "-S needs JPEG output (-j)"),
    (["-S", "444", "-o", "y.png"], "-S needs JPEG output (-j)"),
    (["-j", "90", "-g", "-S", "420", "-o", "y.jpg"], "chroma subsampling needs a colour output"),
    (["-j", "90", "-g", "--chroma-subsampling", "440", "-o", "y.jpg"], "chroma subsampling needs a colour output"),
])
def test_new_option_errors(cli, args, msg):  # noqa: F811
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg") and not os.path.exists("y.png")


def test_chroma_subsampling_in_usage(cli):  # noqa: F811
    r = run(cli)
    assert r.returncode == 1 and "-S, --chroma-subsampling 444|422|420|440" in r.stdout


# ---- GPU ----

CASES = [  # (name, w, h, input quality, input subsampling (PIL), flags, zoom, separate, iterations, -S, Q)
    ("420_q30_i20_S420", 101, 67, 30, 2, ["-i", "20"], 1, False, [20] * 3, "420", 90),
    ("444_q20_i5_S420_replicated", 40, 24, 20, 0, ["-i", "5"], 1, False, [5] * 3, "420", 95),
    ("420_z2_i8_S422", 45, 38, 40, 2, ["-z", "2", "-i", "8"], 2, False, [8] * 3, "422", 75),
    ("420_s_i10_6_4_S420", 83, 61, 20, 2, ["-s", "-i", "10,6,4"], 1, True, [10, 6, 4], "420", 90),
    ("422_q60_i6_S440", 37, 29, 60, 1, ["-i", "6"], 1, False, [6] * 3, "440", 100),
]


def run_case(cli, tmp_path, case, seed, quality=None, sampling=None, png=False):  # noqa: F811
    name, w, h, q, sub, flags, zoom, separate, its, S, Q = case
    jpg = str(tmp_path / "in.jpg")
    make_jpeg(jpg, w, h, q, sub, seed=seed)
    sampling = sampling or S
    out = str(tmp_path / ("out.png" if png else f"out_{sampling}.jpg"))
    r = run(cli, jpg, "-o", out, "-q", *flags, *([] if png else ["-j", str(quality or Q), "-S", sampling]))
    assert r.returncode == 0, r.stderr
    return jpg, out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_file_holds_the_expected_coefficients(cli, read_coefficients, oracle, tmp_path, case):  # noqa: F811
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    name, w, h, q, sub, flags, zoom, separate, its, S, Q = case
    jpg, out = run_case(cli, tmp_path, case, seed=len(name))
    iw, ih, planes = load_coefficients(read_coefficients, jpg)
    assert (iw, ih) == (w, h)
    ow, oh, got = load_coefficients(read_coefficients, out)
    assert (ow, oh) == (w * zoom, h * zoom)
    bw, bh = (ow + 7) // 8, (oh + 7) // 8
    tables = pil_tables(read_coefficients, tmp_path, Q, 3)
    weights = [0.3, 0.0, 0.0] if separate else [0.3] * 3          # the defaults of -w with and without -s
    want = reference_planes(oracle, planes, zoom, separate, weights, [0.001] * 3, its)
    for c in range(3):
        sx, sy = (1, 1) if c == 0 else FACTORS[S]
        cbw, cbh = ceil_div(bw, sx), ceil_div(bh, sy)
        assert (got[c].w_samp, got[c].h_samp) == (sx, sy) and (got[c].w, got[c].h) == (cbw * 8, cbh * 8), f"component {c}"
        assert np.array_equal(got[c].quant_table, tables[c]), f"component {c}: not PIL's table for quality {Q}"
        if c == 0:
            exp = expected_coefficients(oracle, want[c], tables[c], cbw, cbh)
        else:
            exp = expected_sub(oracle, want[c], tables[c], (sx, sy), cbw, cbh)
        assert np.array_equal(got[c].data.reshape(cbh, cbw, 64), exp), f"component {c}"


@pytest.mark.gpu
def test_S_444_writes_the_bytes_of_a_run_without_S(cli, tmp_path):  # noqa: F811
    jpg = str(tmp_path / "in.jpg")
    make_jpeg(jpg, 45, 38, 40, 2, seed=7)
    outs = [str(tmp_path / n) for n in ("plain.jpg", "s444.jpg", "s420.jpg")]
    for out, extra in zip(outs, ([], ["-S", "444"], ["--chroma-subsampling", "420"])):
        r = run(cli, jpg, "-o", out, "-q", "-i", "6", "-j", "90", *extra)
        assert r.returncode == 0, r.stderr
    plain, s444, s420 = (open(o, "rb").read() for o in outs)
    assert plain == s444
    assert s420 != plain


@pytest.mark.gpu
def test_row_tiled_run_writes_the_bytes_of_the_untiled_one(cli, tmp_path):  # noqa: F811
    """one file over two GPUs (the GPU twice where there is one): 64x104 4:4:4, whose chroma grid's last block row is
    replicated by the last band"""
    jpg, one, two = (str(tmp_path / n) for n in ("in.jpg", "one.jpg", "two.jpg"))
    make_jpeg(jpg, 64, 104, 30, 0, seed=11)
    r = run(cli, jpg, "-i", "6", "-j", "90", "-S", "420", "-o", one, "-q")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, J2P_DEVICES="0,0", J2P_TILE_MIN_BAND_PIXELS="1")
    r = subprocess.run([cli, jpg, "-i", "6", "-j", "90", "-S", "420", "-o", two, "-q"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "not row-tiling" not in r.stderr, r.stderr
    assert open(one, "rb").read() == open(two, "rb").read()


QUALITY_CASES = [  # subsampled sources only: the inputs of the CPU simulation in DESIGN.md (synth_rgb(w, h, seed=w))
    ("420_q30_i20_S420", 101, 67, 30, 2, ["-i", "20"], 1, False, [20] * 3, "420", None),
    ("422_q60_i10_S422", 37, 29, 60, 1, ["-i", "10"], 1, False, [10] * 3, "422", None),
]
PIL_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [90, 100])
@pytest.mark.parametrize("case", QUALITY_CASES, ids=[c[0] for c in QUALITY_CASES])
def test_file_decodes_and_is_no_worse_than_encoding_the_png(cli, read_coefficients, oracle, tmp_path, case, Q):  # noqa: F811
    """PSNR against the float RGB the reference's planes define: the direct file against PIL's encoding (same quality,
    same subsampling) of the same run's 8-bit PNG; and the file against the same run's 4:4:4 file.  All figures are
    deterministic; no margin."""
    from PIL import Image
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    name, w, h, q, sub, flags, zoom, separate, its, S, _ = case
    jpg, out = run_case(cli, tmp_path, case, seed=w, quality=Q)
    _, out444 = run_case(cli, tmp_path, case, seed=w, quality=Q, sampling="444")
    _, png = run_case(cli, tmp_path, case, seed=w, png=True)
    direct = Image.open(out)
    assert direct.mode == "RGB" and direct.size == (w, h)
    direct = np.asarray(direct)
    buf = io.BytesIO()
    Image.open(png).convert("RGB").save(buf, "JPEG", quality=Q, subsampling=PIL_SUBSAMPLING[S])
    detour_bytes = buf.tell()
    buf.seek(0)
    detour = np.asarray(Image.open(buf).convert("RGB"))
    _, _, planes = load_coefficients(read_coefficients, jpg)
    truth = float_rgb(reference_planes(oracle, planes, 1, False, [0.3] * 3, [0.001] * 3, its), w, h)
    p_direct, p_detour = psnr_to(truth, direct), psnr_to(truth, detour)
    size, size444 = os.path.getsize(out), os.path.getsize(out444)
    print(f"{name} Q{Q}: direct {p_direct:.3f} dB, {size} bytes (4:4:4: {size444} bytes); PNG -> PIL {p_detour:.3f} dB, {detour_bytes} bytes")
    assert p_direct >= p_detour
    assert size < size444
