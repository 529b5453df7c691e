"""The order in which every XCD walks its run of the two phase launches (j2p_kernels.hip.h: project_item, grad_item; the policy
j2p_geometry.h: j2p_phase_order_of), evaluated on the host through the debug exports — no GPU needed.  Workgroup b runs on
XCD b % 8; whatever the order, a launch's workgroups must cover its work exactly once, every XCD's share must be one
contiguous run of the launch, and the per-run reversal must visit, XCD by XCD, exactly the forward order's work backwards."""
import ctypes

import numpy as np
import pytest

import jpeg2png_amd as j

FORWARD, REVERSE = j.J2P_ORDER_FORWARD, j.J2P_ORDER_REVERSE
MIB = 1 << 20


@pytest.fixture(scope="module")
def hooks(lib):
    """the library with the debug exports' argument types set"""
    u, pu = ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)
    lib.j2p_debug_project_items.argtypes = [u, u, u, u, ctypes.c_int, ctypes.c_void_p, u, pu, pu]
    lib.j2p_debug_grad_items_workgroups.argtypes = [u] * 7 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, u, pu, pu]
    lib.j2p_debug_phase_order.argtypes = [ctypes.c_size_t, ctypes.c_size_t, u, u, ctypes.c_int, pu, pu]
    return lib


def project_items(lib, strips_x, nby, by_offset, by_mul, order):
    buf = np.zeros((strips_x * nby + 8, 4), np.uint32)
    n, wgs = ctypes.c_uint(), ctypes.c_uint()
    assert lib.j2p_debug_project_items(strips_x, nby, by_offset, by_mul, order, buf.ctypes.data, buf.shape[0], ctypes.byref(n), ctypes.byref(wgs)) == 0
    assert n.value <= buf.shape[0]
    return buf[:n.value].astype(np.int64), wgs.value


def grad_items(lib, W, rows, rpw, waves, zones, order):
    buf = np.zeros((1 << 18, 5), np.uint32)
    wg = np.zeros(1 << 18, np.uint32)
    n, wgs = ctypes.c_uint(), ctypes.c_uint()
    rc = lib.j2p_debug_grad_items_workgroups(W, rows, rpw, waves, *zones, order, buf.ctypes.data, wg.ctypes.data, buf.shape[0], ctypes.byref(n), ctypes.byref(wgs))
    assert rc == 0 and n.value <= buf.shape[0]
    return buf[:n.value].astype(np.int64), wg[:n.value].astype(np.int64), wgs.value


def runs_in_dispatch_order(xcd, key):
    """per XCD the keys its workgroups take, in dispatch order, consecutive repeats dropped"""
    out = {}
    for q, k in zip(xcd, key):
        seq = out.setdefault(int(q), [])
        if not seq or seq[-1] != k:
            seq.append(int(k))
    return out


def check_contiguous_tiling(runs, total):
    """every XCD's keys are one contiguous range; the ranges tile [0, total) in the order of the XCDs"""
    spans = sorted((q, min(seq), max(seq), len(set(seq))) for q, seq in runs.items())
    at = 0
    for _, lo, hi, count in spans:
        assert lo == at and count == hi - lo + 1, f"runs {spans} do not tile 0..{total}"
        at = hi + 1
    assert at == total


# strips across, block rows, by_offset, by_mul: what each shape is there for
PROJECT_SHAPES = [
    pytest.param(1, 1, 0, 1, id="1 strip"),
    pytest.param(4, 3, 0, 1, id="12 strips: 3 workgroups, five empty runs"),
    pytest.param(9, 9, 0, 1, id="81 strips: 21 workgroups, runs of 3 and 2, last workgroup one strip"),
    pytest.param(5, 2, 0, 13, id="split phase: first and last block row of 14"),
    pytest.param(5, 12, 1, 1, id="split phase: all but the first and last block row of 14"),
    pytest.param(64, 512, 0, 1, id="4096^2"),
]


@pytest.mark.parametrize("strips_x,nby,by_offset,by_mul", PROJECT_SHAPES)
def test_projection_map(hooks, strips_x, nby, by_offset, by_mul):
    strips = strips_x * nby
    seen = {}
    for order in (FORWARD, REVERSE):
        it, nwg = project_items(hooks, strips_x, nby, by_offset, by_mul, order)
        assert nwg == (strips + 3) // 4
        wg, wave, by, sx = it.T
        # a bijection from the active (workgroup, wavefront) pairs onto the launch's strips
        assert len(it) == strips and len({(a, b) for a, b in zip(wg, wave)}) == strips
        assert ((wg >= 0) & (wg < nwg) & (wave < 4) & (sx < strips_x)).all()
        assert ((by - by_offset) % by_mul == 0).all()
        lstrip = (by - by_offset) // by_mul * strips_x + sx
        assert sorted(lstrip) == list(range(strips))
        assert (lstrip % 4 == wave).all(), "a workgroup's wavefronts take four consecutive strips in either order"
        runs = runs_in_dispatch_order(wg % 8, lstrip // 4)
        assert set(runs) == set(range(min(8, nwg))), "fewer than 8 workgroups: the XCDs past them have empty runs"
        check_contiguous_tiling(runs, nwg)
        seen[order] = runs
    for q, seq in seen[FORWARD].items():
        assert seq == sorted(seq)
        assert seen[REVERSE][q] == seq[::-1], f"XCD {q} does not walk its forward run backwards"
    if nwg >= 16:
        assert max(len(s) for s in seen[FORWARD].values()) - min(len(s) for s in seen[FORWARD].values()) <= 1


def test_projection_map_refuses_what_the_kernel_has_not(hooks):
    buf = np.zeros((16, 4), np.uint32)
    n, wgs = ctypes.c_uint(), ctypes.c_uint()
    for order in (2, 3, -1):
        assert hooks.j2p_debug_project_items(4, 3, 0, 1, order, buf.ctypes.data, 16, ctypes.byref(n), ctypes.byref(wgs)) != 0


# W, rows, rows per tile, channel wavefronts, (doubles, halves, quarters in 1/256)
GRAD_SHAPES = [
    pytest.param(2000, 488, 16, 1, (64, 64, 64), id="every zone kind, short last tile row, runs of 8 and 9 units"),
    pytest.param(2000, 488, 16, 1, (0, 0, 0), id="whole items only"),
    pytest.param(4096, 4096, 16, 1, (0, 32, 10), id="4096^2"),
    pytest.param(520, 136, 16, 3, (0, 0, 0), id="joint: a unit per strip and pair of tile rows"),
    pytest.param(64, 8, 4, 1, (0, 0, 0), id="one unit: seven empty runs"),
]


@pytest.mark.parametrize("W,rows,rpw,waves,zones", GRAD_SHAPES)
def test_gradient_map(hooks, W, rows, rpw, waves, zones):
    ntx = (W - 4 + 123) // 124
    ntr = -(-rows // rpw)
    positions = ntx * ((ntr + 1) // 2)
    units = positions if waves > 1 else (positions + 3) // 4
    seen, kinds = {}, {}
    for order in (FORWARD, REVERSE):
        it, wg, nwg = grad_items(hooks, W, rows, rpw, waves, zones, order)
        strip, t0, nr, tr, kind = it.T
        cover = np.zeros((ntx, rows), np.int32)
        for s, a, b in zip(strip, t0, nr):
            cover[s, a:a + b] += 1
        assert (cover == 1).all(), f"order {order}: rows marched {np.unique(cover)} times"
        pos = (tr // 2) * ntx + strip
        unit = pos if waves > 1 else pos // 4
        runs = runs_in_dispatch_order(wg % 8, unit)
        assert set(runs) == set(range(min(8, units)))
        check_contiguous_tiling(runs, units)
        seen[order] = runs
        kinds[order] = {(int(q), int(u)): int(k) for q, u, k in zip(wg % 8, unit, kind)}
        # (kind: 0 whole, 1 half, 2 quarter, 3 double)
        assert set(kind) == {0} | {k for k, share in zip((3, 1, 2), zones) if share}, "the shape is meant to hold every kind of item it names"
    for q, seq in seen[FORWARD].items():
        assert seq == sorted(seq)
        assert seen[REVERSE][q] == seq[::-1], f"XCD {q} does not walk its forward run backwards"
        lo, hi = seq[0], seq[-1]
        # zones go by dispatch position: the unit walked i-th is of the same kind in either order, the short ones last
        for u in seq:
            assert kinds[REVERSE][(q, lo + hi - u)] == kinds[FORWARD][(q, u)]


def schedule(W, H, nch):
    """j2p_strip_schedule_of restated: strips per row, rows per strip, zone shares of a whole-canvas launch"""
    strips = (W - 4 + 123) // 124
    rpw = 16
    if strips * nch * -(-H // rpw) < 2048:
        rpw = 8
        if strips * nch * -(-H // rpw) < 2048:
            rpw = 4
    waves = strips * -(-H // rpw)
    if nch == 1 and rpw >= 8 and waves < 3 * 4096:
        zones = (0, 32, 10 if rpw >= 16 else 0)
    elif nch == 1 and rpw >= 16:
        zones = (200, 24, 8)
    else:
        zones = (0, 0, 0)
    return rpw, zones


# the sizes the orders were measured at: W, canvas rows, channels of the gradient launch, the projection launches' (ws, hs)
SWEEP = [
    pytest.param(1920, 1080, 1, [(1, 1)], id="1080p Y"),
    pytest.param(2048, 2048, 1, [(1, 1)], id="2048^2"),
    pytest.param(4096, 2048, 1, [(1, 1)], id="4096x2048"),
    pytest.param(4096, 4096, 1, [(1, 1)], id="4096^2"),
    pytest.param(4096, 4608, 1, [(1, 1)], id="4096x4608"),
    pytest.param(8192, 4096, 1, [(1, 1)], id="8192x4096"),
    pytest.param(16384, 2048, 1, [(1, 1)], id="16384x2048"),
    pytest.param(8192, 8192, 1, [(1, 1)], id="8192^2"),
    pytest.param(4096, 4096, 3, [(1, 1)], id="4096^2 4:4:4 joint"),
    pytest.param(1920, 1088, 3, [(1, 1), (2, 2)], id="1080p 4:2:0 joint"),
]


@pytest.mark.parametrize("W,rows,nch,samplings", SWEEP)
def test_regions_of_the_two_kernels_begin_on_the_same_rows(hooks, W, rows, nch, samplings):
    """XCD q's region of the gradient launch and of every projection launch begin less than one pair of tile rows (32 rows)
    apart: what an XCD's L2 holds at the end of one phase is then what the same XCD wants at the start of the next"""
    rpw, zones = schedule(W, rows, nch)
    it, wg, _ = grad_items(hooks, W, rows, rpw, nch, zones, FORWARD)
    grad_begin = {}
    for q, t0 in zip(wg % 8, it[:, 1]):
        grad_begin.setdefault(int(q), int(t0))          # (dispatch order: the first item of the XCD's first workgroup)
    for ws, hs in samplings:
        strips_x, nby = -(-W // (64 * ws)), -(-rows // (8 * hs))
        pit, _ = project_items(hooks, strips_x, nby, 0, 1, FORWARD)
        proj_begin = {}
        for b, by in zip(pit[:, 0] % 8, pit[:, 2]):
            proj_begin.setdefault(int(b), int(by) * 8 * hs)
        assert set(proj_begin) == set(grad_begin) == set(range(8))
        apart = {q: abs(grad_begin[q] - proj_begin[q]) for q in range(8)}
        assert max(apart.values()) < 32, f"sampling {ws}x{hs}: regions begin {apart} rows apart"


def policy(lib, working_set, planes, W, rows, band):
    g, p = ctypes.c_uint(), ctypes.c_uint()
    assert lib.j2p_debug_phase_order(working_set, planes, W, rows, band, ctypes.byref(g), ctypes.byref(p)) == 0
    return g.value, p.value


# W, rows, channels, band: what the policy gives (gradient, projection).  One plane = (rows + 4) x W floats; an iteration
# touches two planes, the shared gradient / prob-state buffer and a byte per coefficient (13 bytes per pixel)
POLICY = [
    (1920, 1080, 1, 0, (REVERSE, FORWARD)),          # every whole canvas: the gradient phase bottom-up
    (4096, 4096, 1, 0, (REVERSE, FORWARD)),
    (8192, 4096, 1, 0, (REVERSE, FORWARD)),          # working set past the Infinity Cache, planes within
    (8192, 8192, 1, 0, (REVERSE, FORWARD)),          # planes past it
    (4096, 4096, 3, 0, (REVERSE, FORWARD)),
    (4096, 2048, 1, 1, (FORWARD, FORWARD)),          # a band whose planes fit: as before
    (16384, 2048, 1, 1, (FORWARD, FORWARD)),
    (16384, 4096, 1, 1, (REVERSE, FORWARD)),         # a band whose planes do not
]


@pytest.mark.parametrize("W,rows,nch,band,want", POLICY)
def test_policy_table(hooks, W, rows, nch, band, want):
    planes = 2 * nch * (rows + 4) * W * 4
    working_set = planes + nch * rows * W * 5
    assert policy(hooks, working_set, planes, W, rows, band) == want


def test_policy_bound_for_bands_is_the_non_temporal_policys(hooks):
    """a band's gradient phase turns round where its two planes exceed what the non-temporal policy takes for the Infinity
    Cache (260 MiB), as before"""
    assert policy(hooks, 400 * MIB, 260 * MIB, 16384, 2048, 1) == (FORWARD, FORWARD)
    assert policy(hooks, 400 * MIB, 260 * MIB + 1, 16384, 2048, 1) == (REVERSE, FORWARD)


def test_python_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jpeg2png_amd.h")).read()
    for name in ("J2P_OPT_PHASE_ORDER", "J2P_ORDER_FORWARD", "J2P_ORDER_REVERSE"):
        assert int(re.search(r"#define %s\s+(\d+)" % name, text).group(1)) == getattr(j, name)
    assert j.phase_order(j.J2P_ORDER_REVERSE, j.J2P_ORDER_FORWARD) == 1 and j.phase_order(j.J2P_ORDER_FORWARD, j.J2P_ORDER_REVERSE) == 2
