"""Flat and uniformly coloured planes on every solver path (cases and preconditions: tests/degenerate_cases.py,
tests/test_degenerate_cpu.py).  Two regimes the texture of the parity suite never reaches: ||g|| == 0 for a whole channel
(the `norm != 0` test of compute.c:212 on every projection path, norm reductions that must deliver an exact 0.0, CSV sums
that must be exact zeros) and 0 < ||g|| < 2^-20 (den_ok() switches phase B's short division off).  Expected planes are the
oracle's — and the compiled reference's where it is built — compared bit for bit; log rows with the suite's tolerances
(rtol 1e-9 / atol 1e-9 against the oracle, atol 2e-6 against the reference's CSV), exactly 0.0 for K0 / K1."""
import numpy as np
import pytest

import degenerate_cases as dc
from conftest import band_devices, bit_equal, parity_note
from test_parity_gpu import SCHEDULE_SETTINGS
from test_tensor_gpu import expected_sample_bytes

pytestmark = pytest.mark.gpu

WIDE = (3, 4, 6, 8)                     # the sampling factors of the wide-footprint projection path
ITS = dc.ITERATIONS
one_value, clean = dc.one_value, dc.clean


def run_1_then_5(s, log):
    """the zero-norm iteration and the tiny-norm iterations in different calls"""
    first, rest = s.run(1, log=log), s.run(ITS - 1, log=log)
    return np.concatenate([first, rest]) if log else None


def check_planes(got, planes, e, kind, what):
    for c in range(len(planes)):
        assert bit_equal(got[c], e["want"][c]), f"{what}: channel {c} against the oracle"
        if e["ref"] is not None:
            assert bit_equal(got[c], e["ref"][c]), f"{what}: channel {c} against the reference"
    if kind in ("K0", "K1"):
        for c in range(len(planes)):
            assert bit_equal(got[c], e["input"][c]), f"{what}: channel {c} is not the up-sampled input"
            assert clean(got[c]), f"{what}: channel {c}"
    for c in dc.uniform_channels(planes, kind):
        assert one_value(got[c]), f"{what}: channel {c} is not uniform"


def check_rows(rows, e, kind, what):
    assert rows.shape == (ITS, 4), what
    if kind in ("K0", "K1"):
        assert (rows == 0.0).all() and clean(rows), f"{what}: {rows}"
    np.testing.assert_allclose(rows, e["rows"], rtol=1e-9, atol=1e-9, err_msg=what)
    if e["ref_rows"] is not None:
        np.testing.assert_allclose(rows[:, 1:], e["ref_rows"][:, 1:], rtol=1e-9, atol=2e-6, err_msg=what)


@pytest.mark.parametrize("shape,kind", dc.CASES, ids=lambda v: v)
def test_every_schedule_on_flat_and_uniform_planes(exp_lib, oracle, shape, kind):
    """every case through the schedule settings of test_every_schedule_switch_leaves_the_bits_alone, one solver per
    setting, logged and not, 1 + 5 iterations.  The zoomed shape runs with J2P_OPT_MIXED_PROJECT 0 and the wide-footprint
    path on and off; the 4128-row canvas has more tile rows than one tree takes (tickets, then k_norm_finish)"""
    import jpeg2png_amd as j
    planes, e = dc.case(shape, kind)
    n = len(planes)
    pw = [dc.PWEIGHT] * n
    zoomed = dc.SHAPES[shape].get("zoom", 1) > 1
    for wide in ((1, 0) if zoomed else (None,)):
        for opts in SCHEDULE_SETTINGS:
            for log in (False, True):
                what = f"{shape} {kind} options {opts} wide {wide} log {log}"
                with j.Solver(planes, dc.WEIGHT, pw, ITS) as s:
                    if shape == "y_64x4128" and not opts:
                        assert s.launches_per_iteration() == 3
                    for k, v in opts.items():
                        s.debug_option(k, v)
                    if zoomed:
                        s.debug_option(j.J2P_OPT_MIXED_PROJECT, 0)
                        s.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, wide)
                        assert [s.wide_footprint(c) for c in range(n)] == [bool(wide) and p.w_samp in WIDE for p in planes], what
                    rows = run_1_then_5(s, log)
                    got = [s.download(c) for c in range(n)]
                check_planes(got, planes, e, kind, what)
                if log:
                    check_rows(rows, e, kind, what)
    parity_note(f"degenerate {shape} {kind}: {len(SCHEDULE_SETTINGS)} schedule settings x log on / off"
                + (" x wide footprint on / off" if zoomed else "") + ": "
                + ("bit-identical to the reference and the oracle" if e["ref"] is not None else
                   "bit-identical to the oracle (the reference is not built)"))


TALL = ["y_200x136", "420_157x101_x3", "y_64x4128"]          # the canvases of at least 128 rows (136, 336 and 4128)
BAND_CASES = [(s, k) for s in TALL for k in ("K0", "K2", "K3b", "K4") if k in dc.SHAPE_KINDS[s]]


@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("shape,kind", BAND_CASES, ids=lambda v: v)
def test_row_bands_on_flat_and_uniform_planes(lib, oracle, shape, kind, nband, monkeypatch):
    """the same expected bits from 2 and 3 row bands with the direct and the copy exchange; K4 is cut so that the first
    band holds nothing but zeros (every row sum it contributes is exactly 0).  The 4128-row canvas has more tile rows than
    the tree k_project runs for linked bands can hold: asked for `direct`, the engine demotes it to `copy`"""
    import jpeg2png_amd as j
    planes, e = dc.case(shape, kind)
    n = len(planes)
    assert e["input"][0].shape[0] >= 128
    pw = [dc.PWEIGHT] * n
    cuts = dc.k4_cuts(planes, nband) if kind == "K4" else None
    for exchange in ("direct", "copy"):
        monkeypatch.setenv("J2P_TILED_EXCHANGE", exchange)
        what = f"{shape} {kind} {nband} bands, exchange {exchange}"
        with j.TiledSolver(planes, dc.WEIGHT, pw, ITS, devices=band_devices(nband), cuts=cuts) as t:
            assert t.exchange() == ("copy" if shape == "y_64x4128" else exchange), what
            if cuts:
                assert [(r0, r1) for _, r0, r1 in t.bands()] == list(zip(cuts, cuts[1:]))
            rows = run_1_then_5(t, True)
            check_planes([t.download(c) for c in range(n)], planes, e, kind, what + ", logged")
            check_rows(rows, e, kind, what)
            t.reset()
            run_1_then_5(t, False)
            check_planes([t.download(c) for c in range(n)], planes, e, kind, what)


@pytest.mark.parametrize("shape", [s for s in dc.SHAPES if "K2" in dc.SHAPE_KINDS[s]])
def test_gradient_norm_is_zero_and_then_below_the_division_screen(lib, shape, capsys):
    """not resting on the oracle: the gradient the solver itself wrote for a uniform channel has norm 0 before the first
    iteration and a norm in (0, 2^-20) — below den_ok()'s bound, j2p_kernels.hip.h — after it; in K3b beside a luma norm
    of ordinary size"""
    import jpeg2png_amd as j
    for kind in ("K2", "K3b"):
        if kind not in dc.SHAPE_KINDS[shape]:
            continue
        planes, _ = dc.case(shape, kind)
        n = len(planes)
        pw = [dc.PWEIGHT] * n
        channels = range(n) if kind == "K2" else (1, 2)

        def norms(s):
            return [float(np.sqrt((s.download_gradient(c).astype(np.float64) ** 2).sum())) for c in range(n)]
        with j.Solver(planes, dc.WEIGHT, pw, ITS) as s:
            s.phase_gradient()
            before = norms(s)
        with j.Solver(planes, dc.WEIGHT, pw, ITS) as s:
            s.run(1)
            s.phase_gradient()
            after = norms(s)
        restated = [dc.restated_norm(p, dc.PWEIGHT) for p in planes]
        with capsys.disabled():
            print(f"\n{shape} {kind}: ||g|| before iteration 0 {before}, after 1 iteration {after}, restated {restated}")
        for c in channels:
            assert before[c] == 0.0, f"{kind} channel {c}"
            assert 0 < after[c] < dc.DEN_OK_MIN, f"{kind} channel {c}: {after[c]!r}"
        if kind == "K3b":
            assert before[0] > 1.0 and after[0] > 1.0


@pytest.mark.parametrize("kind", ["K3a", "K3b"])
@pytest.mark.parametrize("shape", [("420", 154, 101), ("440", 152, 101)], ids=lambda v: f"{v[0]}_{v[1]}x{v[2]}")
def test_separate_solves_of_grey_and_tinted_images(lib, oracle, capfd, shape, kind):
    """what `-s` does: every channel a solve of its own — the zero chroma planes of a grey photograph with ||g|| = 0
    throughout, the tinted ones with the tiny norm — against the oracle (and the reference) channel by channel; then as
    separate batch jobs: float planes, 8- and 16-bit samples against the numpy restatement of the sample forms, and the
    row-tiled job equal to the untiled one.  101 image rows: the batch engine tiles a job only when the shortest of its
    solves has two bands of three 16-row segments (run_job_tiled, j2p_batch.hip) — here the luma solve has 104 rows and
    the chroma solves 112, so every solve of the tiled job runs as two bands; a shorter image would quietly be solved
    whole and the comparison with the untiled job would say nothing"""
    import jpeg2png_amd as j
    sub, w, h = shape
    planes = dc.make(kind, w, h, sub, seed=7)
    assert [p.h * p.h_samp for p in planes] == [104, 112, 112] and all(p.h_samp in (1, 2) for p in planes)
    assert min(p.h * p.h_samp for p in planes) // (3 * j.J2P_TILE_ROWS) >= 2
    shape = f"{sub}_{w}x{h}"
    alone = []
    for c, p in enumerate(planes):
        want, _ = oracle.oracle_compute([p], dc.WEIGHT, [dc.PWEIGHT], ITS)
        with j.Solver([p], dc.WEIGHT, [dc.PWEIGHT], ITS) as s:
            run_1_then_5(s, False)
            got = s.download(0)
        assert bit_equal(got, want[0]), f"channel {c} alone against the oracle"
        if oracle.have_ref():
            ref, _, _ = oracle.ref_compute([p], dc.WEIGHT, [dc.PWEIGHT], ITS)
            assert bit_equal(got, ref[0]), f"channel {c} alone against the reference"
        if c > 0:
            assert one_value(got), f"channel {c}"
            if kind == "K3a":
                assert not got.any() and clean(got), f"channel {c}"
        alone.append(got)
    got = {}
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        for tile in (False, True):
            capfd.readouterr()
            extra = {"tile": True, "tile_min_band_pixels": 0} if tile else {}
            got["planes", tile] = b.wait(b.submit(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, ITS, separate=True, **extra))
            for bits in (8, 16):
                got[bits, tile] = b.wait(b.submit(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, ITS, separate=True, width=w, height=h,
                                                  bits=bits, **extra))
            if tile:
                assert "not row-tiling" not in capfd.readouterr().err
    for c in range(3):
        assert bit_equal(got["planes", False][c], alone[c]), f"separate job, channel {c}"
        assert bit_equal(got["planes", True][c], alone[c]), f"row-tiled separate job, channel {c}"
    for bits in (8, 16):
        assert got[bits, False].tobytes() == expected_sample_bytes(alone, w, h, bits), f"{bits}-bit samples"
        assert np.array_equal(got[bits, True], got[bits, False]), f"{bits}-bit samples of the row-tiled job"
    if oracle.have_ref():
        parity_note(f"degenerate {shape} {kind}: each channel solved alone bit-identical to the reference")


def test_flat_planes_in_a_recycled_arena(lib, oracle):
    """a live 256x192 solve leaves its partials, tickets, CSV sums and gradient behind in the arena; the all-zero and then
    the tinted 240x176 image that get that arena next must not see any of it (test_pool_recycles_arenas reuses the same job,
    so the stale contents it reads back are the right answer)"""
    import jpeg2png_amd as j
    from conftest import make_case

    def arena(s):
        # the two canvases differ in width, so plane_ptr itself cannot be compared as test_pool_recycles_arenas does.  This
        # leans on the solver's layout: the first thing carved from an arena is channel 0's first plane buffer (the current
        # one right after creation), whose image rows start behind its halo rows.  Should that order change, this fails —
        # loudly, not vacuously — for a reason that has nothing to do with recycling: adjust it here
        return s.plane_ptr(0) - 4 * j.J2P_HALO_ROWS * s.W
    lib.j2p_pool_trim()
    try:
        live = make_case(256, 192, "420", 10, seed=8)
        with j.Solver(live, dc.WEIGHT, [dc.PWEIGHT] * 3, 4) as s:
            first = arena(s)
            rows = s.run(4, log=True)
            assert np.isfinite(rows).all() and rows[:, 2].min() > 0
        for kind in ("K0", "K3b"):
            planes = dc.make(kind, 240, 176, "420", seed=7)
            want, want_rows = oracle.oracle_compute(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, ITS, log=True)
            e = {"want": want, "rows": want_rows, "input": dc.upsampled(planes), "ref": None, "ref_rows": None}
            if oracle.have_ref():
                e["ref"], e["ref_rows"], _ = oracle.ref_compute(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, ITS, log=True)
            for log in (True, False):
                with j.Solver(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, ITS) as s:
                    assert arena(s) == first, f"{kind}: the arena was not reused"
                    rows = run_1_then_5(s, log)
                    got = [s.download(c) for c in range(3)]
                check_planes(got, planes, e, kind, f"recycled arena, {kind}, log {log}")
                if log:
                    check_rows(rows, e, kind, f"recycled arena, {kind}")
    finally:
        lib.j2p_pool_trim()
