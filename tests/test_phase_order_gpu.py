"""The order in which the XCDs walk their runs of the two phase launches (J2P_OPT_PHASE_ORDER, the environment's
J2P_PHASE_ORDER) is schedule only: for every combination of forward and reversed gradient and projection phases the solved
planes are the reference's bit for bit (oracle/_ref where it is built, else the restated oracle), and the strips' partial
sums of g^2 are the same bits whatever the order.  The shapes are the smallest that reach each launch form: one workgroup,
a few, uneven runs with a partly active last workgroup, the one-launch projection of small joint canvases, one launch per
sampling class (grid.z == 2), the logging kernels, linked bands with their halo pushes, every kind of gradient item, and the
wide-footprint projection path."""
import copy

import numpy as np
import pytest

from conftest import band_devices, bit_equal, make_case

pytestmark = pytest.mark.gpu

WEIGHT, PW = 0.3, 0.001
F, R = 0, 1                         # J2P_ORDER_FORWARD, J2P_ORDER_REVERSE
ORDERS = [(F, F), (R, F), (F, R), (R, R)]          # (gradient, projection)


def reference(oracle, planes, weight, pw, its, log=False):
    """(planes, log rows) of the compiled reference where it is built, else of the restated oracle"""
    if oracle.have_ref():
        want, rows, _ = oracle.ref_compute(planes, weight, pw, its, log=log)
        return want, rows
    return oracle.oracle_compute(planes, weight, pw, its, log=log)


def solve(planes, its, order, weight=WEIGHT, options=()):
    """(planes, raw bits of the strip partials of the last gradient phase) of a whole-canvas solve in `order`"""
    import torch
    import jpeg2png_amd as j
    from jpeg2png_amd.tiled import alias_tensor
    with j.Solver(planes, weight, [PW] * len(planes), its) as s:
        for k, v in options:
            s.debug_option(k, v)
        s.debug_option(j.J2P_OPT_PHASE_ORDER, j.phase_order(*order))
        assert s.phase_order() == order
        s.run(its - 1)
        s.phase_gradient()
        ptr, ntx, ntr, _ = s.debug_partials()
        s.sync()
        part = alias_tensor(ptr, s.nch * ntr * ntx, torch.float64, torch.device("cuda", 0)).cpu().numpy().view(np.uint64).copy()
        s.phase_project()
        return [s.download(c) for c in range(s.nch)], part


def check_every_order(planes, its, want, weight=WEIGHT, options=()):
    first = None
    for order in ORDERS:
        got, part = solve(planes, its, order, weight, options)
        for c in range(len(planes)):
            if want is not None:
                assert bit_equal(got[c], want[c]), f"order {order}, channel {c}: not the reference's plane"
            if first is not None:
                assert bit_equal(got[c], first[0][c]), f"order {order}, channel {c}: differs from the forward order"
        if first is None:
            first = (got, part)
        assert np.array_equal(part, first[1]), f"order {order}: the strips' partial sums of g^2 differ from the forward order's"


# W, H, subsampling, Y only, iterations
SHAPES = [
    pytest.param(64, 8, "444", True, 3, id="64x8 Y: one workgroup"),
    pytest.param(200, 24, "444", True, 20, id="200x24 Y: three workgroups"),
    pytest.param(520, 72, "444", True, 20, id="520x72 Y: uneven runs, partly active last workgroup"),
    pytest.param(264, 136, "420", False, 20, id="264x136 4:2:0 joint: padding, k_project_mixed"),
    pytest.param(1040, 1032, "420", False, 3, id="1040x1032 4:2:0 joint: one launch per sampling class, grid.z == 2"),
]


@pytest.mark.parametrize("W,H,sub,y_only,its", SHAPES)
def test_every_order_gives_the_references_bits(lib, oracle, W, H, sub, y_only, its):
    import jpeg2png_amd as j
    planes = make_case(W, H, sub, 10, seed=311, y_only=y_only)
    want, _ = reference(oracle, planes, WEIGHT, [PW] * len(planes), its)
    check_every_order(planes, its, want)
    with j.Solver(planes, WEIGHT, [PW] * len(planes), its) as s:
        assert s.phase_order() == (R, F), "a whole canvas: the gradient phase bottom-up, the projection top-down"
        with pytest.raises(j.J2PError):
            s.debug_option(j.J2P_OPT_PHASE_ORDER, 4)
        s.debug_option(j.J2P_OPT_PHASE_ORDER, j.phase_order(F, R))
        s.debug_option(j.J2P_OPT_PHASE_ORDER, -1)
        assert s.phase_order() == (R, F)


def test_logged_runs(lib, oracle):
    """200x24 with the CSV sums: the LOG instantiations of both kernels"""
    import jpeg2png_amd as j
    planes = make_case(200, 24, "444", 10, seed=312, y_only=True)
    its = 6
    want, want_rows = reference(oracle, planes, WEIGHT, [PW], its, log=True)
    first = None
    for order in ORDERS:
        with j.Solver(planes, WEIGHT, [PW], its) as s:
            s.debug_option(j.J2P_OPT_PHASE_ORDER, j.phase_order(*order))
            rows = s.run(its, log=True)
            assert bit_equal(s.download(0), want[0]), f"order {order}"
        # (the reference's CSV holds 6 decimals; the restated oracle returns the doubles)
        np.testing.assert_allclose(rows[:, 1:], np.asarray(want_rows)[:, 1:], rtol=1e-9, atol=2e-6 if oracle.have_ref() else 1e-9)
        if first is None:
            first = rows
        assert np.array_equal(rows.view(np.uint64), first.view(np.uint64)), f"order {order}: CSV sums differ from the forward order's"


def test_two_linked_bands_on_one_gpu(lib, oracle, monkeypatch):
    """136x64 as two bands that write each other's halo rows from k_project (the NIP 2 forms); the order comes from the
    environment, as every band solver reads it at create"""
    import jpeg2png_amd as j
    planes = make_case(136, 64, "444", 10, seed=313, y_only=True)
    its = 9
    want, _ = reference(oracle, planes, WEIGHT, [PW], its)
    for order in ORDERS:
        monkeypatch.setenv("J2P_PHASE_ORDER", str(j.phase_order(*order)))
        with j.TiledSolver(planes, WEIGHT, [PW], its, devices=band_devices(2), cuts=[0, 32, 64]) as t:
            assert t.nband == 2
            assert [t.band_solver(b).phase_order() for b in range(2)] == [order, order]
            t.run(its)
            assert bit_equal(t.download(0), want[0]), f"order {order}, exchange {t.exchange()}"
    monkeypatch.delenv("J2P_PHASE_ORDER")
    with j.TiledSolver(planes, WEIGHT, [PW], its, devices=band_devices(2), cuts=[0, 32, 64]) as t:
        assert [t.band_solver(b).phase_order() for b in range(2)] == [(F, F)] * 2, "bands within the cache keep the forward order"


@pytest.mark.parametrize("W,H,zones", [(520, 72, (256, 0, 0)), (520, 72, (0, 256, 0)), (520, 72, (0, 0, 256)), (2000, 488, (64, 64, 64))],
                         ids=["520x72 doubles", "520x72 halves", "520x72 quarters", "2000x488 every kind in one launch"])
def test_zone_shares_forced(exp_lib, oracle, monkeypatch, W, H, zones):
    """doubles, halves and quarters, forced as tests/test_parity_gpu.py's half-and-quarter test forces them.  An XCD's run
    of 520x72 is one unit or none, so a launch there holds one kind at a time; 2000x488 (runs of 8 and 9 units, short last
    tile row) holds all of them at once"""
    import jpeg2png_amd as j
    planes = make_case(W, H, "444", 10, seed=314, y_only=True)
    its = 20 if W == 520 else 3
    want, _ = reference(oracle, planes, WEIGHT, [PW], its)
    monkeypatch.setenv("J2P_RPW", "16")
    for name, share in zip(("J2P_ZONE_D", "J2P_ZONE_B", "J2P_ZONE_C"), zones):
        monkeypatch.setenv(name, str(share))
    check_every_order(planes, its, want)
    # ... and through the drop-in entry point with the order taken from the environment
    for order in ORDERS:
        monkeypatch.setenv("J2P_PHASE_ORDER", str(j.phase_order(*order)))
        got = copy.deepcopy(planes)
        j.compute(got, WEIGHT, [PW], its)
        assert bit_equal(got[0].fdata, want[0]), f"zones {zones}, order {order}"


def test_wide_footprint_path(lib, oracle):
    """4:2:0 zoomed twice: the 4x4 chroma channels take the wide-footprint projection path (one launch per sampling class)"""
    import jpeg2png_amd as j
    z = j.zoomed(make_case(157, 101, "420", 30, seed=315), 2)
    its = 5
    want = oracle.ref_compute(z, WEIGHT, [PW] * 3, its)[0] if oracle.have_ref() else None
    options = ((j.J2P_OPT_MIXED_PROJECT, 0), (j.J2P_OPT_WIDE_FOOTPRINT, 1))
    with j.Solver(z, WEIGHT, [PW] * 3, its) as s:
        for k, v in options:
            s.debug_option(k, v)
        assert [s.wide_footprint(c) for c in range(3)] == [False, True, True]
    check_every_order(z, its, want, options=options)
