"""JPEG output from the solved planes (k_quantise_blocks<1, 1>, j2p_planes_to_coefficients / j2p_planes_rows_to_coefficients,
Solver.coefficients, Batch.submit(quant_tables=...)): the int16 coefficients are, array for array, the compiled
reference's dct8x8s (ooura/dct.c:98-130) of every 8x8 block of the downloaded plane, divided by the output table in
float32, rounded to nearest even and clamped to +-1023 — for one block, for more blocks per row than a wavefront owns,
for a cropped rectangle, for every channel of a joint 4:2:0 solve, through the batch engine (joint, separate, row-tiled).
Without the reference: a requantisation with the input's own table returns the input coefficients exactly, and
saturation is exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import band_devices, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = os.environ.get("J2P_IMG_PREFIX", "/opt/conda")


def _need_ref(oracle):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")


def expected_coefficients(oracle, canvas, table, bw, bh):
    """the definition, on the CPU: blocks of the float plane -> the reference's dct8x8s -> float32 `/` -> rint -> clip"""
    blocks = np.ascontiguousarray(canvas[:bh * 8, :bw * 8], np.float32).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    d = oracle.dct_blocks(blocks, which="ref")
    assert d.dtype == np.float32
    v = d / np.asarray(table, np.uint16).astype(np.float32)[None, :]
    assert v.dtype == np.float32
    return np.clip(np.rint(v), -1023, 1023).astype(np.int16).reshape(bh, bw, 64)


def tables():
    rng = np.random.default_rng(64)
    big = rng.integers(1, 65536, 64)
    big[:8] = [65535, 256, 257, 1000, 4096, 300, 32768, 511]
    return {"ones": np.ones(64, np.uint16), "random": rng.integers(1, 256, 64).astype(np.uint16),
            "all255": np.full(64, 255, np.uint16), "above255": big.astype(np.uint16)}


CASES = [  # (name, W, H, subsampling, iterations, blocks_w, blocks_h)
    ("one_block", 8, 8, None, 3, None, None),
    ("nine_blocks_per_row", 72, 40, None, 5, None, None),
    ("cropped_13x2_of_17x3", 136, 24, None, 4, 13, 2),
    ("joint_420", 48, 32, "420", 4, None, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_coefficients_equal_the_reference_transform_of_the_plane(lib, oracle, case):
    import jpeg2png_amd as j
    _need_ref(oracle)
    name, W, H, sub, its, bw, bh = case
    planes = make_case(W, H, sub or "444", 25, seed=len(name), y_only=sub is None)
    pw = [0.001] * len(planes)
    with j.Solver(planes, 0.3, pw, its) as s:
        assert (s.W, s.H) == (W, H)
        s.run(its)
        for c in range(len(planes)):
            canvas = s.download(c)
            for tname, table in tables().items():
                got = s.coefficients(c, table, blocks_w=bw, blocks_h=bh)
                ebw, ebh = bw or W // 8, bh or H // 8
                assert got.shape == (ebh, ebw, 64) and got.dtype == np.int16
                want = expected_coefficients(oracle, canvas, table, ebw, ebh)
                assert np.array_equal(got, want), f"channel {c}, table {tname}: {int((got != want).sum())} coefficients differ"
            # the plane itself is untouched
            assert np.array_equal(s.download(c).view(np.uint32), canvas.view(np.uint32))


@pytest.mark.gpu
def test_requantising_with_the_input_table_returns_the_input_coefficients(lib):
    """0 iterations: the plane is the decoded input, so coefficients(own table) is the input, exactly (51 200 coefficients;
    |d| <= 32 and steps <= 32 keep the transforms' rounding error far below half a step)"""
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    rng = np.random.default_rng(2)
    w, h = 320, 160
    data = rng.integers(-32, 33, size=w * h).astype(np.int16)
    q = rng.integers(1, 33, 64).astype(np.uint16)
    with j.Solver([Plane(w, h, 1, 1, data, q)], 0.3, [0.001], 0) as s:
        got = s.coefficients(0, q)
    assert got.shape == (h // 8, w // 8, 64)
    assert np.array_equal(got.reshape(-1), data)


@pytest.mark.gpu
def test_saturation_is_exactly_1023_with_the_sign_of_the_value(lib):
    """coefficients +-1023 with steps of 255, requantised with steps of 1: every unclamped value is far beyond 1023 and has
    the sign of the input coefficient"""
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    rng = np.random.default_rng(3)
    w, h = 72, 40
    data = (rng.integers(0, 2, size=w * h) * 2 - 1).astype(np.int16) * 1023
    with j.Solver([Plane(w, h, 1, 1, data, np.full(64, 255, np.uint16))], 0.3, [0.001], 0) as s:
        got = s.coefficients(0, np.ones(64, np.uint16))
    assert np.array_equal(got.reshape(-1), data)
    assert (got == 1023).any() and (got == -1023).any()


# ---- batch engine ----

@pytest.fixture(scope="module")
def read_coefficients(tmp_path_factory):
    """tests/c/read_coefficients.c compiled against the same libjpeg as the driver"""
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg headers not available")
    exe = str(tmp_path_factory.mktemp("rc") / "read_coefficients")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "read_coefficients.c"),
                    "-o", exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    return exe


def jpeg_planes(exe, path, w, h, quality, subsampling, seed):
    """the three components of a PIL-made JPEG of the synthetic image, as libjpeg delivers them"""
    from PIL import Image
    from jpeg2png_amd import synth
    from jpeg2png_amd.synth import Plane
    Image.fromarray(synth.synth_rgb(w, h, seed).astype(np.uint8), "RGB").save(path, "JPEG", quality=quality, subsampling=subsampling)
    raw = subprocess.run([exe, path], capture_output=True, check=True).stdout
    iw, ih = struct.unpack_from("<2I", raw, 0)
    assert (iw, ih) == (w, h)
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
    return planes


@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_batch_job_equals_the_solver_recipe(lib, oracle, read_coefficients, tmp_path, separate):
    import jpeg2png_amd as j
    _need_ref(oracle)
    w, h, its = 101, 67, 20
    planes = jpeg_planes(read_coefficients, str(tmp_path / "a.jpg"), w, h, 30, 2, seed=4)      # 4:2:0, q30
    assert [(p.w_samp, p.h_samp) for p in planes] == [(1, 1), (2, 2), (2, 2)]
    t = tables()
    qt = [t["random"], t["all255"], t["ones"]]
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        got = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt))
    bw, bh = (w + 7) // 8, (h + 7) // 8
    assert len(got) == 3 and all(g.shape == (bh, bw, 64) and g.dtype == np.int16 for g in got)
    if separate:
        canvases = []
        for c in range(3):
            with j.Solver([planes[c]], 0.3, [0.001], its) as s:
                s.run(its)
                canvases.append(s.download(0))
    else:
        with j.Solver(planes, 0.3, [0.001] * 3, its) as s:
            s.run(its)
            canvases = [s.download(c) for c in range(3)]
    for c in range(3):
        want = expected_coefficients(oracle, canvases[c], qt[c], bw, bh)
        assert np.array_equal(got[c], want), f"channel {c}: {int((got[c] != want).sum())} coefficients differ"


@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_row_tiled_job_equals_the_untiled_one(lib, read_coefficients, tmp_path, capfd, separate):
    """64x112 4:2:0: two bands of at least 48 rows, each quantising its own block rows on its own GPU (the GPU twice where
    there is one) through j2p_planes_rows_to_coefficients"""
    import jpeg2png_amd as j
    w, h, its = 64, 112, 20
    planes = jpeg_planes(read_coefficients, str(tmp_path / "t.jpg"), w, h, 30, 2, seed=5)
    t = tables()
    qt = [t["random"], t["ones"], t["above255"]]
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        one = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt))
        capfd.readouterr()
        two = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt, tile=True,
                              tile_min_band_pixels=0))
    assert "not row-tiling" not in capfd.readouterr().err          # (the single-solver fallback says so)
    for c in range(3):
        assert one[c].shape == (14, 8, 64) and one[c].any()
        assert np.array_equal(one[c], two[c]), f"channel {c}"


# ---- errors ----

@pytest.mark.gpu
def test_errors(lib):
    import jpeg2png_amd as j
    planes = make_case(72, 40, "444", 30, seed=1, y_only=True)
    ones = np.ones(64, np.uint16)
    zero = ones.copy()
    zero[37] = 0
    with j.Solver(planes, 0.3, [0.001], 1) as s:
        with pytest.raises(j.J2PError, match="zero"):
            s.coefficients(0, zero)
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, ones, blocks_w=10)
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, ones, blocks_h=6)
        with pytest.raises(j.J2PError):
            s.coefficients(1, ones)
        assert s.coefficients(0, ones).shape == (5, 9, 64)
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        with pytest.raises(j.J2PError, match="bits"):
            b.submit(planes, 0.3, [0.001], 1, width=72, height=40, bits=8, quant_tables=[ones])
        with pytest.raises(j.J2PError, match="zero"):
            b.wait(b.submit(planes, 0.3, [0.001], 1, width=72, height=40, quant_tables=[zero]))
        with pytest.raises(j.J2PError, match="not inside"):
            b.wait(b.submit(planes, 0.3, [0.001], 1, width=81, height=40, quant_tables=[ones]))
        assert b.wait(b.submit(planes, 0.3, [0.001], 1, width=65, height=33, quant_tables=[ones]))[0].shape == (5, 9, 64)
