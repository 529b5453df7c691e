"""Subsampled JPEG output from the solved planes (k_quantise_blocks<SX, SY>, j2p_planes_to_coefficients_sub /
j2p_planes_rows_to_coefficients_sub, Solver.coefficients(subsampling=), Batch.submit(subsampling=)): the int16
coefficients are, array for array, the definition computed here in numpy — every output sample the float32 mean of its
sy x sx canvas values (accumulator from 0, raster order, one addition each, divided by float32(sx * sy); indices beyond
the canvas's last row / column read the last row / column), then the compiled reference's dct8x8s of every 8x8 block of
those means, the float32 quotient by the table, round to nearest even, clamp to +-1023 (expected_coefficients)."""
import ctypes

import numpy as np
import pytest

from conftest import band_devices, make_case
from test_jpeg_out_gpu import _need_ref, expected_coefficients, jpeg_planes, read_coefficients, tables  # noqa: F401


def sub_means(canvas, sx, sy, bw, bh):
    """the plane an output component of sampling (sx, sy) is the transform of: 8 * bh x 8 * bw float32 means"""
    canvas = np.ascontiguousarray(canvas, np.float32)
    H, W = canvas.shape
    assert 8 * sx * (bw - 1) < W and 8 * sy * (bh - 1) < H          # every block starts inside the canvas
    acc = np.zeros((8 * bh, 8 * bw), np.float32)
    for jj in range(sy):
        ys = np.minimum(np.arange(8 * bh) * sy + jj, H - 1)
        for ii in range(sx):
            xs = np.minimum(np.arange(8 * bw) * sx + ii, W - 1)
            acc = acc + canvas[np.ix_(ys, xs)]
            assert acc.dtype == np.float32
    return acc / np.float32(sx * sy)


def expected_sub(oracle, canvas, table, sub, bw, bh):
    return expected_coefficients(oracle, sub_means(canvas, sub[0], sub[1], bw, bh), table, bw, bh)


def ceil_div(a, b):
    return -(-a // b)


Y_CASES = [  # (name, W, H, iterations, (sx, sy), blocks_w, blocks_h; None = the default grid)
    ("one_block_2x2", 16, 16, 3, (2, 2), None, None),
    ("1x2_blocks_2x1", 16, 16, 3, (2, 1), None, None),
    ("2x1_blocks_1x2", 16, 16, 3, (1, 2), None, None),
    ("nine_blocks_per_row_2x2", 144, 32, 4, (2, 2), None, None),
    ("replicated_columns_and_rows_2x2", 40, 24, 4, (2, 2), 3, 2),
    ("replicated_columns_2x1", 40, 24, 4, (2, 1), 3, 3),
    ("cropped_13x2_of_17x3_2x2", 272, 48, 3, (2, 2), 13, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", Y_CASES, ids=[c[0] for c in Y_CASES])
def test_coefficients_equal_the_definition(lib, oracle, case):
    import jpeg2png_amd as j
    _need_ref(oracle)
    name, W, H, its, sub, bw, bh = case
    planes = make_case(W, H, "444", 25, seed=len(name), y_only=True)
    with j.Solver(planes, 0.3, [0.001], its) as s:
        assert (s.W, s.H) == (W, H)
        s.run(its)
        canvas = s.download(0)
        ebw, ebh = bw or ceil_div(W // 8, sub[0]), bh or ceil_div(H // 8, sub[1])
        for tname, table in tables().items():
            got = s.coefficients(0, table, blocks_w=bw, blocks_h=bh, subsampling=sub)
            assert got.shape == (ebh, ebw, 64) and got.dtype == np.int16
            want = expected_sub(oracle, canvas, table, sub, ebw, ebh)
            assert np.array_equal(got, want), f"table {tname}: {int((got != want).sum())} coefficients differ"
        assert np.array_equal(s.download(0).view(np.uint32), canvas.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("zoom", [1, 2], ids=["joint_420", "joint_420_zoomed_2x"])
def test_joint_solve_every_channel(lib, oracle, zoom):
    """48x32 4:2:0: every channel at all four samplings; zoomed 2x (wide-footprint projection path) at (2, 2)"""
    import jpeg2png_amd as j
    _need_ref(oracle)
    planes = j.zoomed(make_case(48, 32, "420", 25, seed=9), zoom)
    its = 4
    table = tables()["random"]
    with j.Solver(planes, 0.3, [0.001] * 3, its) as s:
        assert (s.W, s.H) == (48 * zoom, 32 * zoom)
        s.run(its)
        for c in range(3):
            canvas = s.download(c)
            for sub in ([(1, 1), (2, 1), (1, 2), (2, 2)] if zoom == 1 else [(2, 2)]):
                got = s.coefficients(c, table, subsampling=sub)
                bw, bh = ceil_div(s.W // 8, sub[0]), ceil_div(s.H // 8, sub[1])
                assert got.shape == (bh, bw, 64)
                want = expected_sub(oracle, canvas, table, sub, bw, bh)
                assert np.array_equal(got, want), f"channel {c}, sampling {sub}: {int((got != want).sum())} coefficients differ"
            assert np.array_equal(s.download(c).view(np.uint32), canvas.view(np.uint32)), "the plane changed"


@pytest.mark.gpu
def test_sampling_1x1_is_the_function_without_the_argument(lib):
    import jpeg2png_amd as j
    planes = make_case(72, 40, "444", 25, seed=3, y_only=True)
    with j.Solver(planes, 0.3, [0.001], 3) as s:
        s.run(3)
        for table in tables().values():
            assert np.array_equal(s.coefficients(0, table, subsampling=(1, 1)), s.coefficients(0, table))
            assert np.array_equal(s.coefficients(0, table, 5, 2, subsampling=(1, 1)), s.coefficients(0, table, 5, 2))
        # (1, 1) keeps the stricter check: the whole grid inside the canvas
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, np.ones(64, np.uint16), blocks_w=10, subsampling=(1, 1))


# ---- batch engine ----

SUBS = [(1, 1), (2, 2), (2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_batch_job_equals_the_solver_recipe(lib, oracle, read_coefficients, tmp_path, separate):  # noqa: F811
    import jpeg2png_amd as j
    _need_ref(oracle)
    w, h, its = 101, 67, 20
    planes = jpeg_planes(read_coefficients, str(tmp_path / "a.jpg"), w, h, 30, 2, seed=4)      # 4:2:0, q30
    t = tables()
    qt = [t["random"], t["all255"], t["ones"]]
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        got = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt, subsampling=SUBS))
    bw, bh = (w + 7) // 8, (h + 7) // 8
    grids = [(ceil_div(bh, sy), ceil_div(bw, sx), 64) for sx, sy in SUBS]
    assert grids == [(9, 13, 64), (5, 7, 64), (5, 7, 64)]
    assert len(got) == 3 and all(g.shape == grids[c] and g.dtype == np.int16 for c, g in enumerate(got))
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
        want = expected_sub(oracle, canvases[c], qt[c], SUBS[c], grids[c][1], grids[c][0])
        assert np.array_equal(got[c], want), f"channel {c}: {int((got[c] != want).sum())} coefficients differ"


@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_row_tiled_job_equals_the_untiled_one(lib, read_coefficients, tmp_path, capfd, separate):  # noqa: F811
    """64x112 4:2:0: two bands (rows 0..47 and 48..111); the chroma grid's 7 block rows of 16 canvas rows are 3 of the
    first band and 4 of the last"""
    import jpeg2png_amd as j
    w, h, its = 64, 112, 20
    planes = jpeg_planes(read_coefficients, str(tmp_path / "t.jpg"), w, h, 30, 2, seed=5)
    t = tables()
    qt = [t["random"], t["ones"], t["ones"]]                  # (steps of 1 for chroma: no plane quantises to all zeros)
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        one = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt, subsampling=SUBS))
        capfd.readouterr()
        two = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, width=w, height=h, quant_tables=qt, subsampling=SUBS,
                              tile=True, tile_min_band_pixels=0))
    assert "not row-tiling" not in capfd.readouterr().err          # (the single-solver fallback says so)
    for c in range(3):
        assert one[c].shape == ((14, 8, 64) if c == 0 else (7, 4, 64)) and one[c].any()
        assert np.array_equal(one[c], two[c]), f"channel {c}"


@pytest.mark.gpu
def test_row_tiled_job_with_a_replicated_last_block_row(lib, read_coefficients, tmp_path, capfd):  # noqa: F811
    """64x104: the canvas's 104 rows end in the middle of the chroma grid's 7th block row, which the last band replicates"""
    import jpeg2png_amd as j
    w, h, its = 64, 104, 6
    planes = jpeg_planes(read_coefficients, str(tmp_path / "r.jpg"), w, h, 30, 0, seed=6)      # 4:4:4: a 64x104 canvas
    qt = [tables()["random"]] * 3
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        one = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, width=w, height=h, quant_tables=qt, subsampling=SUBS))
        capfd.readouterr()
        two = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, width=w, height=h, quant_tables=qt, subsampling=SUBS, tile=True,
                              tile_min_band_pixels=0))
    assert "not row-tiling" not in capfd.readouterr().err
    for c in range(3):
        assert one[c].shape == ((13, 8, 64) if c == 0 else (7, 4, 64))
        assert np.array_equal(one[c], two[c]), f"channel {c}"


# ---- bands and errors ----

def _rows_sub(s, sub, bw, r0, r1, table):
    import jpeg2png_amd as j
    out = np.zeros((r1 - r0, bw, 64), np.int16)
    q = np.ascontiguousarray(table, np.uint16)
    ref = j._CPlaneRef(s._h, 0)
    j._check(s._lib.j2p_planes_rows_to_coefficients_sub(ctypes.byref(ref), sub[0], sub[1], bw, r0, r1, q.ctypes.data, out.ctypes.data))
    return out


@pytest.mark.gpu
def test_band_solvers_give_their_own_block_rows_and_refuse_the_others(lib):
    """0 iterations: a band's plane is the decoded input, as the whole canvas's.  Band [0, 48) of 112 rows owns the (2, 2)
    block rows 0..2, band [48, 112) rows 3..6; a block row that starts outside the band is refused, as is one that would
    need rows beyond a band that is not the canvas's last"""
    import jpeg2png_amd as j
    planes = make_case(64, 112, "444", 30, seed=8, y_only=True)
    table = tables()["random"]
    with j.Solver(planes, 0.3, [0.001], 0) as s:
        whole = s.coefficients(0, table, subsampling=(2, 2))
        assert whole.shape == (7, 4, 64)
    with j.Solver(planes, 0.3, [0.001], 0, band=(0, 48)) as s:
        assert np.array_equal(s.coefficients(0, table, subsampling=(2, 2)), whole[:3])
        with pytest.raises(j.J2PError, match="not inside"):
            _rows_sub(s, (2, 2), 4, 2, 4, table)                     # block row 3 starts at row 48
    with j.Solver(planes, 0.3, [0.001], 0, band=(48, 112)) as s:
        assert np.array_equal(s.coefficients(0, table, subsampling=(2, 2)), whole[3:])
        assert np.array_equal(_rows_sub(s, (2, 2), 4, 3, 7, table), whole[3:])
        with pytest.raises(j.J2PError, match="not inside"):
            _rows_sub(s, (2, 2), 4, 2, 4, table)                     # block row 2 starts at row 32
        with pytest.raises(j.J2PError, match="not inside"):
            _rows_sub(s, (2, 2), 4, 6, 8, table)                     # block row 7 starts at row 112


@pytest.mark.gpu
def test_errors(lib):
    import jpeg2png_amd as j
    planes = make_case(40, 24, "444", 30, seed=1, y_only=True)
    ones = np.ones(64, np.uint16)
    zero = ones.copy()
    zero[37] = 0
    with j.Solver(planes, 0.3, [0.001], 1) as s:
        for bad in [(0, 1), (1, 0), (3, 1), (2, 3), (4, 4), (2, 4)]:
            with pytest.raises(j.J2PError, match="sampling factors"):
                s.coefficients(0, ones, subsampling=bad)
            with pytest.raises(j.J2PError, match="sampling factors"):
                _rows_sub(s, bad, 1, 0, 1, ones)
        with pytest.raises(j.J2PError, match="zero"):
            s.coefficients(0, zero, subsampling=(2, 2))
        # 40 columns: the fourth (2, x) block would start at column 48; 24 rows: the third (x, 2) block row at row 32
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, ones, blocks_w=4, subsampling=(2, 2))
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, ones, blocks_h=3, subsampling=(2, 2))
        with pytest.raises(j.J2PError, match="not inside"):
            s.coefficients(0, ones, blocks_h=4, subsampling=(2, 1))
        with pytest.raises(j.J2PError):
            s.coefficients(1, ones, subsampling=(2, 2))
        assert s.coefficients(0, ones, subsampling=(2, 2)).shape == (2, 3, 64)
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        with pytest.raises(j.J2PError, match="bits"):
            b.submit(planes, 0.3, [0.001], 1, width=40, height=24, bits=8, quant_tables=[ones], subsampling=[(2, 2)])
        with pytest.raises(j.J2PError, match="quant_tables"):
            b.submit(planes, 0.3, [0.001], 1, width=40, height=24, subsampling=[(2, 2)])
        with pytest.raises(j.J2PError, match="sampling factors"):
            b.submit(planes, 0.3, [0.001], 1, width=40, height=24, quant_tables=[ones], subsampling=[(3, 1)])
        with pytest.raises(j.J2PError, match="one \\(sx, sy\\) pair per plane"):
            b.submit(planes, 0.3, [0.001], 1, width=40, height=24, quant_tables=[ones], subsampling=[(2, 2), (2, 2)])
        with pytest.raises(j.J2PError, match="zero"):
            b.wait(b.submit(planes, 0.3, [0.001], 1, width=40, height=24, quant_tables=[zero], subsampling=[(2, 2)]))
        with pytest.raises(j.J2PError, match="not inside"):
            b.wait(b.submit(planes, 0.3, [0.001], 1, width=49, height=24, quant_tables=[ones], subsampling=[(2, 2)]))
        assert b.wait(b.submit(planes, 0.3, [0.001], 1, width=40, height=24, quant_tables=[ones], subsampling=[(2, 2)]))[0].shape == (2, 3, 64)
