"""The output stage behind its twelve C entry points (j2p_planes[_rows]_to_{rgb,grey,coefficients,coefficients_sub}) and
behind the batch engine's one job path.  Every family has one worker: the whole-canvas form is the rows form over all
rows plus the refusal of band solvers, so whole form, rows form and the rows form called band by band return the same
bytes; `_sub` with (1, 1) is the plain form.  A row-tiled job and an untiled one go through the same loop and the same
output stage (an engine that is one j2p_solver or one j2p_tiled) and return the same arrays, joint and separate."""
import ctypes

import numpy as np
import pytest

from conftest import band_devices, bit_equal, make_case

J2P_ESTATE = -4
SUBS = [(1, 1), (2, 1), (1, 2), (2, 2)]


def ceil_div(a, b):
    return -(-a // b)


def table():
    """small steps: no plane of the small test images quantises to all zeros"""
    return np.random.default_rng(64).integers(1, 4, 64).astype(np.uint16)


class Forms:
    """the twelve entry points on one solver, straight through ctypes; every call returns (rc, bytes written into)"""

    def __init__(self, j, solver):
        u, p = ctypes.c_uint, ctypes.c_void_p
        ref = ctypes.POINTER(j._CPlaneRef)
        lib = self.lib = solver._lib
        lib.j2p_planes_to_rgb.argtypes = lib.j2p_planes_to_grey.argtypes = [ref, u, u, u, p]
        lib.j2p_planes_rows_to_rgb.argtypes = lib.j2p_planes_rows_to_grey.argtypes = [ref, u, u, u, u, p]
        lib.j2p_planes_to_coefficients.argtypes = [ref, u, u, p, p]
        lib.j2p_planes_rows_to_coefficients.argtypes = [ref, u, u, u, p, p]
        lib.j2p_planes_to_coefficients_sub.argtypes = [ref, u, u, u, u, p, p]
        lib.j2p_planes_rows_to_coefficients_sub.argtypes = [ref, u, u, u, u, u, p, p]
        self.s = solver
        self.refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(solver._h, c) for c in range(3)])
        self.q = table()

    def samples(self, kind, bits, w, rows=None, whole_h=None):
        """kind "rgb" / "grey"; rows=(y0, y1): the rows form, whole_h: the whole-canvas form"""
        n = 3 if kind == "rgb" else 1
        h = whole_h if rows is None else rows[1] - rows[0]
        out = np.zeros(h * w * n * (bits // 8), np.uint8)
        if rows is None:
            rc = getattr(self.lib, f"j2p_planes_to_{kind}")(self.refs, w, h, bits, out.ctypes.data)
        else:
            rc = getattr(self.lib, f"j2p_planes_rows_to_{kind}")(self.refs, w, rows[0], rows[1], bits, out.ctypes.data)
        return rc, out

    def coefficients(self, c, sub, bw, rows=None, whole_h=None):
        """sub None: the plain family, (sx, sy): the _sub family; rows=(r0, r1) block rows or whole_h block rows"""
        bh = whole_h if rows is None else rows[1] - rows[0]
        out = np.zeros(bh * bw * 64, np.int16)
        ref = ctypes.pointer(self.refs[c])
        q, o = self.q.ctypes.data, out.ctypes.data
        if sub is None:
            rc = (self.lib.j2p_planes_to_coefficients(ref, bw, bh, q, o) if rows is None else
                  self.lib.j2p_planes_rows_to_coefficients(ref, bw, rows[0], rows[1], q, o))
        else:
            rc = (self.lib.j2p_planes_to_coefficients_sub(ref, sub[0], sub[1], bw, bh, q, o) if rows is None else
                  self.lib.j2p_planes_rows_to_coefficients_sub(ref, sub[0], sub[1], bw, rows[0], rows[1], q, o))
        return rc, out


def ok(result):
    rc, out = result
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def joint_420(lib):
    """one joint 4:2:0 solve of a 48x32 image, 2 iterations, shared and left unchanged by the tests below"""
    import jpeg2png_amd as j
    planes = make_case(48, 32, "420", 25, seed=11)
    with j.Solver(planes, 0.3, [0.001] * 3, 2) as s:
        assert (s.W, s.H) == (48, 32)
        s.run(2)
        yield Forms(j, s)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("kind", ["rgb", "grey"])
def test_samples_whole_rows_and_halves_are_the_same_bytes(joint_420, kind, bits):
    f = joint_420
    whole = ok(f.samples(kind, bits, 48, whole_h=32))
    assert whole.any()
    assert np.array_equal(ok(f.samples(kind, bits, 48, rows=(0, 32))), whole)
    halves = np.concatenate([ok(f.samples(kind, bits, 48, rows=(0, 16))), ok(f.samples(kind, bits, 48, rows=(16, 32)))])
    assert np.array_equal(halves, whole)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [None] + SUBS, ids=["plain", "1x1", "2x1", "1x2", "2x2"])
def test_coefficients_whole_rows_and_halves_are_the_same_bytes(joint_420, sub):
    f = joint_420
    sx, sy = sub or (1, 1)
    bw, bh = ceil_div(6, sx), ceil_div(4, sy)
    split = 16 // (8 * sy)                                   # the block row that starts at canvas row 16
    for c in range(3):
        whole = ok(f.coefficients(c, sub, bw, whole_h=bh))
        assert whole.any()
        assert np.array_equal(ok(f.coefficients(c, sub, bw, rows=(0, bh))), whole)
        halves = np.concatenate([ok(f.coefficients(c, sub, bw, rows=(0, split))), ok(f.coefficients(c, sub, bw, rows=(split, bh)))])
        assert np.array_equal(halves, whole)
        if sub == (1, 1):
            assert np.array_equal(ok(f.coefficients(c, None, bw, whole_h=bh)), whole), "_sub with (1, 1) is the plain form"
            assert np.array_equal(ok(f.coefficients(c, None, bw, rows=(0, bh))), whole)


@pytest.mark.gpu
def test_replicated_last_column_and_row(lib):
    """40x24 at (2, 2) with a 3x2 block grid: the third block column and the second block row overhang the canvas"""
    import jpeg2png_amd as j
    planes = make_case(40, 24, "444", 25, seed=12, y_only=True)
    with j.Solver(planes, 0.3, [0.001], 2) as s:
        s.run(2)
        f = Forms(j, s)
        whole = ok(f.coefficients(0, (2, 2), 3, whole_h=2))
        assert whole.reshape(2, 3, 64)[1, 2].any()
        assert np.array_equal(ok(f.coefficients(0, (2, 2), 3, rows=(0, 2))), whole)


@pytest.mark.gpu
def test_one_block_y_only(lib):
    import jpeg2png_amd as j
    planes = make_case(8, 8, "444", 25, seed=13, y_only=True)
    with j.Solver(planes, 0.3, [0.001], 2) as s:
        s.run(2)
        f = Forms(j, s)
        for bits in (8, 16):
            whole = ok(f.samples("grey", bits, 8, whole_h=8))
            assert whole.any() and np.array_equal(ok(f.samples("grey", bits, 8, rows=(0, 8))), whole)
        plain = ok(f.coefficients(0, None, 1, whole_h=1))
        assert plain.any() and np.array_equal(ok(f.coefficients(0, None, 1, rows=(0, 1))), plain)
        for sub in SUBS:
            whole = ok(f.coefficients(0, sub, 1, whole_h=1))
            assert np.array_equal(ok(f.coefficients(0, sub, 1, rows=(0, 1))), whole)
        assert np.array_equal(ok(f.coefficients(0, (1, 1), 1, whole_h=1)), plain)


@pytest.mark.gpu
def test_band_solver_refuses_the_whole_forms_and_serves_the_rows_forms(lib):
    """band [0, 16) of a 48-row canvas, 0 iterations (the band's plane is the decoded input, as the whole canvas's): the whole
    forms of all four families are state errors, the rows forms give what the whole-canvas solver gives for those rows"""
    import jpeg2png_amd as j
    planes = make_case(32, 48, "420", 25, seed=14)
    with j.Solver(planes, 0.3, [0.001] * 3, 0) as s:
        assert (s.W, s.H) == (32, 48)
        f = Forms(j, s)
        want = {"rgb": ok(f.samples("rgb", 8, 32, rows=(0, 16))), "grey": ok(f.samples("grey", 16, 32, rows=(0, 16))),
                "plain": ok(f.coefficients(1, None, 4, rows=(0, 2))), "sub": ok(f.coefficients(2, (2, 2), 2, rows=(0, 1)))}
    with j.Solver(planes, 0.3, [0.001] * 3, 0, band=(0, 16)) as s:
        f = Forms(j, s)
        assert f.samples("rgb", 8, 32, whole_h=16)[0] == J2P_ESTATE
        assert f.samples("grey", 16, 32, whole_h=16)[0] == J2P_ESTATE
        assert f.coefficients(1, None, 4, whole_h=2)[0] == J2P_ESTATE
        assert f.coefficients(2, (2, 2), 2, whole_h=1)[0] == J2P_ESTATE
        assert np.array_equal(ok(f.samples("rgb", 8, 32, rows=(0, 16))), want["rgb"])
        assert np.array_equal(ok(f.samples("grey", 16, 32, rows=(0, 16))), want["grey"])
        assert np.array_equal(ok(f.coefficients(1, None, 4, rows=(0, 2))), want["plain"])
        assert np.array_equal(ok(f.coefficients(2, (2, 2), 2, rows=(0, 1))), want["sub"])
    assert all(w.any() for w in want.values())


# ---- the batch engine: one job path over either engine ----

@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_row_tiled_job_equals_the_untiled_one_for_every_output(lib, capfd, separate):
    """64x112 4:2:0, two bands: float planes, 8-bit RGB (with a progress callback: the chunked loop) and coefficients at
    [(1, 1), (2, 2), (2, 2)], each from the untiled and from the row-tiled job"""
    import jpeg2png_amd as j
    w, h, its = 64, 112, 6
    planes = make_case(w, h, "420", 25, seed=15)
    qt = [table(), np.ones(64, np.uint16), np.ones(64, np.uint16)]
    outputs = {"planes": {}, "rgb8": {"width": w, "height": h, "bits": 8},
               "coefficients": {"width": w, "height": h, "quant_tables": qt, "subsampling": [(1, 1), (2, 2), (2, 2)]}}
    got = {}
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        for tile in (False, True):
            capfd.readouterr()
            for name, kw in outputs.items():
                ticks = []
                extra = {"tile": True, "tile_min_band_pixels": 0} if tile else {}
                if name == "rgb8":
                    extra["on_progress"] = ticks.append
                got[name, tile] = b.wait(b.submit(planes, 0.3, [0.001] * 3, its, separate=separate, **kw, **extra))
                if name == "rgb8":
                    assert sum(ticks) == (3 * its if separate else its)
            if tile:
                assert "not row-tiling" not in capfd.readouterr().err          # (the single-solver fallback says so)
    for c in range(3):
        assert got["planes", False][c].shape == (h, w) and got["planes", False][c].any()
        assert bit_equal(got["planes", False][c], got["planes", True][c]), f"plane {c}"
        assert got["coefficients", False][c].shape == ((14, 8, 64) if c == 0 else (7, 4, 64)) and got["coefficients", False][c].any()
        assert np.array_equal(got["coefficients", False][c], got["coefficients", True][c]), f"coefficients of channel {c}"
    assert got["rgb8", False].shape == (h, w, 3) and got["rgb8", False].any()
    assert np.array_equal(got["rgb8", False], got["rgb8", True])
