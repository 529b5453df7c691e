"""One buffer for the gradient and the prob state of a channel (j2p_geometry.h: j2p_shares_state).
k_gradient writes g over the prob state it has just read, k_project the next prob state over the g of its own blocks: the
bits must be those of two buffers.  Every comparison here is bitwise — against the CPU oracle's per-iteration trace
(tests/oracle_trace.py), and between the shared form (the release library), the form with two buffers (the experiments
library with J2P_SHARE_STATE=0) and the checked build.  The references are computed once per module."""
import copy

import numpy as np
import pytest

import norm_cases as nc
from conftest import band_devices, bit_equal, make_case
from oracle_trace import first_difference, oracle_trace

pytestmark = pytest.mark.gpu

WEIGHT, PW = 0.3, 0.001
SMALL = (264, 40, 6)            # three strips: left edge, free, right edge; 40 rows: the last 16-row tile row is short
HOT = (2048, 2048, 3)           # the smallest square canvas with 16-row strips: the instantiation of the headline


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Case:
    def __init__(self, W, H, its, sub="444", y_only=True, pweights=None, seed=71):
        self.planes = make_case(W, H, sub, 10, seed=seed, y_only=y_only)
        self.pweights = pweights or [PW] * len(self.planes)
        self.its = its
        self.trace, self.want = oracle_trace(self.planes, WEIGHT, self.pweights, its)
        self.trace.setflags(write=False)

    def solver(self, **kw):
        import jpeg2png_amd as j
        return j.Solver(self.planes, WEIGHT, self.pweights, self.its, **kw)


@pytest.fixture(scope="module")
def small(oracle):
    return Case(*SMALL)


@pytest.fixture(scope="module")
def hot(oracle):
    return Case(*HOT)


@pytest.fixture(scope="module")
def small_rows(small, oracle):
    return oracle.oracle_compute(small.planes, WEIGHT, small.pweights, small.its, log=True)[1]


@pytest.fixture
def two_buffers(exp_lib, monkeypatch):
    """the experiments library with J2P_SHARE_STATE=0 for the solvers created in the test"""
    monkeypatch.setenv("J2P_SHARE_STATE", "0")
    return exp_lib


def traced(case):
    """a whole-canvas solver of the current library, phase by phase: the gradient after every phase_gradient and the iterate
    after every phase_project against the trace"""
    d = first_difference(case.planes, WEIGHT, case.pweights, case.its, case.trace)
    assert d is None, str(d)


def partials_and_plane(case):
    """(|strip partials| of the LAST iteration's gradient phase [channel, tile row, strip], rows per tile row, final planes,
    which channels share)"""
    import torch
    from jpeg2png_amd.tiled import alias_tensor
    with case.solver() as s:
        s.run(case.its - 1)
        s.phase_gradient()
        ptr, ntx, ntr, rpw = s.debug_partials()
        s.sync()
        part = alias_tensor(ptr, s.nch * ntr * ntx, torch.float64, torch.device("cuda", 0)).cpu().numpy().copy().reshape(s.nch, ntr, ntx)
        s.phase_project()
        return np.abs(part), rpw, [s.download(c) for c in range(s.nch)], [s.shares_state(c) for c in range(s.nch)]


def check_norm_and_plane(case, shared):
    part, rpw, planes, flags = partials_and_plane(case)
    assert flags == shared
    for c in range(len(case.planes)):
        assert bit_equal(planes[c], case.want[c]), f"channel {c}: final plane"
        # ||g||: the kernel's own sums of g^2 are those of the oracle's gradient, added in march_rows' order
        assert np.array_equal(bits64(part[c]), bits64(nc.strip_partials(case.trace[-1, c, 0], rpw))), f"channel {c}: partials of g^2"
    return part, planes


# ---- the kernel forms, both build forms, against the trace ----
@pytest.mark.parametrize("which", ["small", "hot"])
def test_shared_buffer_reproduces_the_oracles_trace(lib, which, request):
    case = request.getfixturevalue(which)
    with case.solver() as s:
        assert s.shares_state(0) is True
        if which == "hot":
            assert s.debug_partials()[3] == 16
    traced(case)
    check_norm_and_plane(case, [True])


@pytest.mark.parametrize("which", ["small", "hot"])
def test_two_buffers_reproduce_it_too_and_the_getter_tells_them_apart(two_buffers, which, request):
    case = request.getfixturevalue(which)
    traced(case)
    check_norm_and_plane(case, [False])


def test_release_library_ignores_the_knob(lib, small, monkeypatch):
    monkeypatch.setenv("J2P_SHARE_STATE", "0")
    with small.solver() as s:
        assert s.shares_state(0) is True


def test_arena_shrinks_by_one_plane_per_shared_channel(exp_lib, monkeypatch):
    """what a shared channel no longer has is its prob-state buffer: rows x W floats where the channel covers the canvas —
    the luma of 128 x 40 4:2:0 (canvas 128 x 48) had 40 rows of it"""
    import jpeg2png_amd as j
    for W, H, sub, y_only, nshared, floats in ((264, 40, "444", True, 1, 40 * 264), (136, 40, "444", False, 3, 40 * 136),
                                               (128, 40, "420", False, 1, 40 * 128), (136, 40, "420", False, 0, 0)):
        planes = make_case(W, H, sub, 10, seed=5, y_only=y_only)
        monkeypatch.delenv("J2P_SHARE_STATE", raising=False)
        with j.Solver(planes, WEIGHT, [PW] * len(planes), 2) as s:
            shared_bytes = s.arena_bytes()
            assert sum(s.shares_state(c) for c in range(s.nch)) == nshared
            if sub == "444":
                assert floats == (s.row_end - s.row_begin) * s.W
        monkeypatch.setenv("J2P_SHARE_STATE", "0")
        with j.Solver(planes, WEIGHT, [PW] * len(planes), 2) as s:
            assert not any(s.shares_state(c) for c in range(s.nch))
            # (every carved block starts at a multiple of 256 bytes: a block of N bytes less is N, rounded up, less)
            saved = s.arena_bytes() - shared_bytes
            assert nshared * floats * 4 <= saved < nshared * (floats * 4 + 256) + 1, (W, H, sub)


# ---- variants of 264 x 40 ----
def test_logging_gives_the_same_sums(lib, small, small_rows):
    with small.solver() as s:
        rows = s.run(small.its, log=True)
        assert bit_equal(s.download(0), small.want[0])
    assert np.allclose(rows, small_rows, rtol=1e-9, atol=1e-9)


def test_logging_with_two_buffers_gives_the_same_bits(two_buffers, small, small_rows):
    with small.solver() as s:
        assert s.shares_state(0) is False
        rows = s.run(small.its, log=True)
        assert bit_equal(s.download(0), small.want[0])
    assert np.allclose(rows, small_rows, rtol=1e-9, atol=1e-9)
    import jpeg2png_amd as j
    with j.library(j.LIB_PATH):
        with small.solver() as s:
            assert s.shares_state(0) is True
            assert np.array_equal(bits64(s.run(small.its, log=True)), bits64(rows)), "CSV sums: one buffer against two"


def test_tv_only(lib, oracle):
    import jpeg2png_amd as j
    planes = make_case(*SMALL[:2], "444", 10, seed=71, y_only=True)
    want, _ = oracle.oracle_compute(planes, 0.0, [PW], SMALL[2])
    with j.Solver(planes, 0.0, [PW], SMALL[2]) as s:
        assert s.shares_state(0) is True
        s.run(SMALL[2])
        assert bit_equal(s.download(0), want[0])


def test_two_bands_cut_at_row_16_against_the_whole_canvas(lib, small):
    import jpeg2png_amd as j
    with j.TiledSolver(small.planes, WEIGHT, small.pweights, small.its, devices=band_devices(2), cuts=[0, 16, SMALL[1]]) as t:
        assert [t.band_solver(b).shares_state(0) for b in range(2)] == [True, True]      # crow0 == row0 in both
        t.run(small.its)
        assert bit_equal(t.download(0), small.want[0])


@pytest.mark.parametrize("zones", [(0, 256, 0, 0), (0, 0, 256, 1), (256, 0, 0, 0), (128, 64, 32, 1), (0, 26, 10, 0)])
def test_half_quarter_and_double_items(exp_lib, small, zones, monkeypatch):
    """who marches a row — and in which order the rows of a strip meet the buffer — must not change a bit"""
    import jpeg2png_amd as j
    zd, zb, zc, rev = zones
    monkeypatch.setenv("J2P_RPW", "16")
    monkeypatch.setenv("J2P_ZONE_D", str(zd))
    monkeypatch.setenv("J2P_ZONE_B", str(zb))
    monkeypatch.setenv("J2P_ZONE_C", str(zc))
    monkeypatch.setenv("J2P_GRAD_REVERSE", str(rev))
    with small.solver() as s:
        assert s.shares_state(0) is True and s.debug_partials()[3] == 16
    traced(small)
    got = copy.deepcopy(small.planes)
    j.compute(got, WEIGHT, small.pweights, small.its)
    assert bit_equal(got[0].fdata, small.want[0])


def test_reset_and_a_second_solve_give_the_first_solves_bits(lib, small):
    with small.solver() as s:
        s.run(small.its)
        first = s.download(0)
        s.reset()
        s.run(small.its)
        assert bit_equal(s.download(0), first) and bit_equal(first, small.want[0])
        # ... also when the reset comes between the phases, with a gradient in the buffer
        s.reset()
        s.phase_gradient()
        s.reset()
        s.run(small.its)
        assert bit_equal(s.download(0), first)


# ---- joint images ----
@pytest.fixture(scope="module")
def joint444(oracle):
    return Case(136, 40, 6, y_only=False)


def test_444_joint_shares_all_three(lib, joint444):
    traced(joint444)
    check_norm_and_plane(joint444, [True, True, True])


def test_444_joint_two_buffers(two_buffers, joint444):
    traced(joint444)
    check_norm_and_plane(joint444, [False, False, False])


@pytest.mark.parametrize("shape,shared", [((136, 40), [False, False, False]), ((128, 40), [True, False, False])])
def test_420_joint(lib, oracle, shape, shared):
    """136 x 40: the chroma planes pad the canvas to 144 x 48 — the luma raster is narrower than the canvas and keeps two
    buffers.  128 x 40: the canvas is 128 x 48 — the luma has the canvas's pitch but eight rows fewer, and shares: nobody
    writes or uses a prob state beyond its coverage (the decision of DESIGN.md section 3).  Chroma never shares."""
    case = Case(*shape, 6, sub="420", y_only=False)
    with case.solver() as s:
        assert (s.W, s.H) == ((144, 48) if shape[0] == 136 else (128, 48))
    traced(case)
    check_norm_and_plane(case, shared)


def test_a_channel_without_the_prob_term_keeps_two_buffers(lib, oracle):
    case = Case(136, 40, 6, y_only=False, pweights=[PW, 0.0, PW])
    traced(case)
    check_norm_and_plane(case, [True, False, True])


# ---- the checked build ----
def test_checked_build_no_violations_same_bits(lib, small, small_rows):
    import jpeg2png_amd as j
    from jpeg2png_amd.buildlib import build_debug
    with j.library(build_debug()):
        assert j.debug_build() is True
        with small.solver() as s:
            assert s.shares_state(0) is True
            for _ in range(small.its):
                s.phase_gradient()
                s.phase_project()
            assert bit_equal(s.download(0), small.want[0])
            assert s.debug_violations()[0] == 0, s.debug_violations()
            s.reset()
            rows = s.run(small.its, log=True)
            assert bit_equal(s.download(0), small.want[0]) and np.allclose(rows, small_rows, rtol=1e-9, atol=1e-9)
            assert s.debug_violations()[0] == 0, s.debug_violations()
        with j.TiledSolver(small.planes, WEIGHT, small.pweights, small.its, devices=band_devices(2), cuts=[0, 16, SMALL[1]]) as t:
            t.run(small.its)
            assert bit_equal(t.download(0), small.want[0])
            assert [t.band_solver(b).debug_violations()[0] for b in range(2)] == [0, 0]
        case = Case(128, 40, 4, sub="420", y_only=False)          # a shared luma with rows beyond its coverage
        with case.solver() as s:
            assert s.shares_state(0) is True
            s.run(case.its)
            assert all(bit_equal(s.download(c), case.want[c]) for c in range(3))
            assert s.debug_violations()[0] == 0, s.debug_violations()
