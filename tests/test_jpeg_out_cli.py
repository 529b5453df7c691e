"""JPEG output of the command-line driver (-j Q, cli/jpeg2png_gpu.c): option handling on the CPU; on the GPU the file
written — size, sampling, libjpeg's tables for Q, and every quantised coefficient — against the definition applied to
the UNMODIFIED reference's solve of the same input (dct8x8s of its planes, float32 division, round to nearest even,
clamp), for joint, zoomed, separate and greyscale runs; and the decoded file against the detour it replaces (the run's
8-bit PNG encoded by PIL at the same quality)."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_jpeg_out_gpu import expected_coefficients

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


def _helper(tmp_path_factory, name):
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg headers not available")
    exe = str(tmp_path_factory.mktemp("rc") / name)
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", name + ".c"),
                    "-o", exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    return exe


@pytest.fixture(scope="module")
def read_coefficients(tmp_path_factory):
    """tests/c/read_coefficients.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "read_coefficients")


@pytest.fixture(scope="module")
def read_component(tmp_path_factory):
    """tests/c/read_component.c compiled against the same libjpeg as the driver"""
    return _helper(tmp_path_factory, "read_component")


def make_jpeg(path, w, h, quality, subsampling, seed, mode="RGB"):
    from PIL import Image
    from jpeg2png_amd import synth
    im = Image.fromarray(synth.synth_rgb(w, h, seed).astype(np.uint8), "RGB")
    if mode == "RGB":
        im.save(path, "JPEG", quality=quality, subsampling=subsampling)
    else:
        im.convert(mode).save(path, "JPEG", quality=quality)


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
        d = np.frombuffer(raw, np.int16, cw * ch, off).copy()
        off += 2 * cw * ch
        planes.append(Plane(cw, ch, ws, hs, d, q))
    assert off == len(raw)
    return w, h, planes


def load_component(exe, jpg):
    """(image w, h, number of components, Plane of component 0) as libjpeg delivers them"""
    from jpeg2png_amd.synth import Plane
    raw = subprocess.run([exe, jpg], capture_output=True, check=True).stdout
    w, h, n, cw, ch, ws, hs = struct.unpack_from("<7I", raw, 0)
    q = np.frombuffer(raw, np.uint16, 64, 28).copy()
    d = np.frombuffer(raw, np.int16, cw * ch, 156).copy()
    assert 156 + 2 * cw * ch == len(raw)
    return w, h, n, Plane(cw, ch, ws, hs, d, q)


def pil_tables(exe, tmp_path, quality, ncomp):
    """the quantisation tables (natural order, one per component) of a file PIL saved at `quality`"""
    from PIL import Image
    path = str(tmp_path / f"tables_q{quality}_{ncomp}.jpg")
    rgb = np.arange(16 * 16 * 3, dtype=np.uint8).reshape(16, 16, 3)
    if ncomp == 3:
        Image.fromarray(rgb, "RGB").save(path, "JPEG", quality=quality, subsampling=0)
        return [p.quant_table for p in load_coefficients(exe, path)[2]]
    Image.fromarray(rgb[:, :, 0], "L").save(path, "JPEG", quality=quality)
    return [load_component(exe, path)[3].quant_table]


def reference_planes(oracle, planes, zoom, separate, weights, pweights, its):
    """the reference's own solve of the input's planes: one compute(3, ...) or — separate — three compute(1, ...)"""
    import jpeg2png_amd as j
    z = j.zoomed(planes, zoom)
    for p in z:
        p.fdata = oracle.decode_plane(p)
    if not separate:
        return oracle.ref_compute(z, weights[0], pweights, its[0])[0]
    return [oracle.ref_compute([z[c]], weights[c], [pweights[c]], its[c])[0][0] for c in range(len(z))]


# ---- CPU ----

@pytest.mark.parametrize("args,msg", [
    (["-j", "0", "-o", "y.jpg"], "invalid jpeg quality"),
    (["-j", "101", "-o", "y.jpg"], "invalid jpeg quality"),
    (["-j", "9x", "-o", "y.jpg"], "invalid jpeg quality"),
    (["-j", "-5", "-o", "y.jpg"], "invalid jpeg quality"),
    (["--jpeg", "", "-o", "y.jpg"], "invalid jpeg quality"),
    (["-j", "90", "-1", "-o", "y.jpg"], "16-bit output is only possible for PNG"),
    (["-j", "90"], "-j needs an output file name (-o) for every input"),
])
def test_new_option_errors(cli, args, msg):
    r = run(cli, "x.jpg", *args)
    assert r.returncode == 1
    assert r.stderr.strip() == "jpeg2png: " + msg
    assert not os.path.exists("y.jpg")


def test_jpeg_in_usage(cli):
    r = run(cli)
    assert r.returncode == 1 and "-j, --jpeg Q" in r.stdout


def test_missing_input_is_reported_as_before(cli, tmp_path):
    out = str(tmp_path / "o.jpg")
    r = run(cli, "/nonexistent/x.jpg", "-j", "90", "-o", out, "-q")
    assert r.returncode == 1
    assert r.stderr.strip().startswith("jpeg2png: could not open input file `/nonexistent/x.jpg`")
    assert not os.path.exists(out)


# ---- GPU ----

COLOUR_CASES = [  # (name, w, h, input quality, subsampling, flags, zoom, separate, iterations, Q)
    ("420_q30_i20_Q90", 101, 67, 30, 2, ["-i", "20"], 1, False, [20] * 3, 90),
    ("444_q10_i30_Q100", 64, 48, 10, 0, ["-i", "30"], 1, False, [30] * 3, 100),
    ("420_z2_Q75", 45, 38, 40, 2, ["-z", "2", "-i", "8"], 2, False, [8] * 3, 75),
    ("420_s_i10_6_4_Q90", 83, 61, 20, 2, ["-s", "-i", "10,6,4"], 1, True, [10, 6, 4], 90),
]


def run_case(cli, tmp_path, case, quality=None, png=False):
    name, w, h, q, sub, flags, zoom, separate, its, Q = case
    jpg = str(tmp_path / "in.jpg")
    make_jpeg(jpg, w, h, q, sub, seed=len(name))
    out = str(tmp_path / ("out.png" if png else "out.jpg"))
    r = run(cli, jpg, "-o", out, "-q", *flags, *([] if png else ["-j", str(quality or Q)]))
    assert r.returncode == 0, r.stderr
    return jpg, out


@pytest.mark.gpu
@pytest.mark.parametrize("case", COLOUR_CASES, ids=[c[0] for c in COLOUR_CASES])
def test_file_holds_the_expected_coefficients(cli, read_coefficients, oracle, tmp_path, case):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    name, w, h, q, sub, flags, zoom, separate, its, Q = case
    jpg, out = run_case(cli, tmp_path, case)
    iw, ih, planes = load_coefficients(read_coefficients, jpg)
    assert (iw, ih) == (w, h)
    ow, oh, got = load_coefficients(read_coefficients, out)
    assert (ow, oh) == (w * zoom, h * zoom)
    bw, bh = (ow + 7) // 8, (oh + 7) // 8
    tables = pil_tables(read_coefficients, tmp_path, Q, 3)
    weights = [0.3, 0.0, 0.0] if separate else [0.3] * 3          # the defaults of -w with and without -s
    want = reference_planes(oracle, planes, zoom, separate, weights, [0.001] * 3, its)
    for c in range(3):
        assert (got[c].w_samp, got[c].h_samp) == (1, 1) and (got[c].w, got[c].h) == (bw * 8, bh * 8), f"component {c}"
        assert np.array_equal(got[c].quant_table, tables[c]), f"component {c}: not PIL's table for quality {Q}"
        exp = expected_coefficients(oracle, want[c], tables[c], bw, bh)
        assert np.array_equal(got[c].data.reshape(bh, bw, 64), exp), f"component {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode,sub", [("L", 0), ("RGB", 2)], ids=["one_component", "three_components"])
def test_greyscale_file_is_the_reference_compute_1_of_component_0(cli, read_component, oracle, tmp_path, mode, sub):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    w, h, its, Q = 83, 61, 9, 90
    jpg, out = str(tmp_path / "g.jpg"), str(tmp_path / "g_out.jpg")
    make_jpeg(jpg, w, h, 25, sub, seed=12, mode=mode)
    r = run(cli, jpg, "-g", "-j", str(Q), "-i", str(its), "-o", out, "-q")
    assert r.returncode == 0, r.stderr
    iw, ih, n, plane = load_component(read_component, jpg)
    assert (iw, ih, n) == (w, h, 1 if mode == "L" else 3)
    ow, oh, on, got = load_component(read_component, out)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    assert (ow, oh, on) == (w, h, 1) and (got.w, got.h, got.w_samp, got.h_samp) == (bw * 8, bh * 8, 1, 1)
    table = pil_tables(read_component, tmp_path, Q, 1)[0]
    assert np.array_equal(got.quant_table, table)
    want = reference_planes(oracle, [plane], 1, True, [0.3], [0.001], [its])[0]
    assert np.array_equal(got.data.reshape(bh, bw, 64), expected_coefficients(oracle, want, table, bw, bh))


def float_rgb(planes, w, h):
    """png.c:37-62 without the truncation to samples: the colour matrix in double, narrowed to float, clamped to
    [0, 255], after the luma +128 of jpeg2png.c:156-159; cropped to w x h"""
    y = (planes[0][:h, :w].astype(np.float64) + 128.0).astype(np.float32).astype(np.float64)
    cb, cr = planes[1][:h, :w].astype(np.float64), planes[2][:h, :w].astype(np.float64)
    rgb = np.stack([y + 1.402 * cr, y - 0.34414 * cb - 0.71414 * cr, y + 1.772 * cb], axis=2).astype(np.float32)
    return np.clip(rgb.astype(np.float64), 0.0, 255.0)


def psnr_to(truth, rgb8):
    mse = float(np.mean((truth - rgb8.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [90, 100])
@pytest.mark.parametrize("case", COLOUR_CASES[:2], ids=[c[0].rsplit("_", 1)[0] for c in COLOUR_CASES[:2]])
def test_file_decodes_and_is_no_worse_than_encoding_the_png(cli, read_coefficients, oracle, tmp_path, case, Q):
    """PSNR against the float RGB the reference's planes define: the direct file against PIL's encoding (same quality,
    4:4:4) of the same run's 8-bit PNG.  Both figures are deterministic; no margin."""
    from PIL import Image
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    name, w, h, q, sub, flags, zoom, separate, its, _ = case
    jpg, out = run_case(cli, tmp_path, case, quality=Q)
    _, png = run_case(cli, tmp_path, case, png=True)
    direct = Image.open(out)
    assert direct.mode == "RGB" and direct.size == (w, h)
    direct = np.asarray(direct)
    buf = io.BytesIO()
    Image.open(png).convert("RGB").save(buf, "JPEG", quality=Q, subsampling=0)
    detour_bytes = buf.tell()
    buf.seek(0)
    detour = np.asarray(Image.open(buf).convert("RGB"))
    _, _, planes = load_coefficients(read_coefficients, jpg)
    truth = float_rgb(reference_planes(oracle, planes, 1, False, [0.3] * 3, [0.001] * 3, its), w, h)
    p_direct, p_detour = psnr_to(truth, direct), psnr_to(truth, detour)
    print(f"{name} Q{Q}: direct {p_direct:.3f} dB, {os.path.getsize(out)} bytes; PNG -> PIL {p_detour:.3f} dB, {detour_bytes} bytes")
    assert p_direct >= p_detour
