"""Every form of the ||g|| reduction against the one restatement in tests/norm_cases.py, bit for bit.

A. The stand-alone launch of each form (j2p_norm_selftest) on injected arrays: where doubles leave the kernel (k_rowsums)
   they are compared as doubles; where only the float norm does, the arrays are norm_cases' fixtures, on which the pinned
   association and a wrong one round to different floats.
B. The chain on real gradients through the solver: strip partials (j2p_solver_debug_partials) against the gradient plane
   in march_rows' order, for every dealing of the rows and for bands against the whole canvas; the row sums against the
   partials; the float at norm_ptr against the row sums, for every norm plan.

No tolerance anywhere: both sides perform the same IEEE double additions in the same order, and the conversion to float
and sqrtf are correctly rounded on both.  The one bound (test_row_sums_are_the_sum) guards against a restatement and a
kernel that share an omission."""
import functools
import math

import numpy as np
import pytest

import norm_cases as nc
from conftest import bit_equal, make_case

pytestmark = pytest.mark.gpu

TREE_FORMS = ("fold_tree", "project_tree")                    # at most 1024 tile rows (J2P_NORM_TREE_ROWS)
LAUNCH_FORMS = ("norm_finish", "norm_bands")                  # up to 4096 (kMaxTileRows)
LEVEL2_CASES = [(f, n) for f in TREE_FORMS for n in nc.LEVEL2_SIZES] + [(f, n) for f in LAUNCH_FORMS for n in nc.LEVEL2_LAUNCH_SIZES]


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def mixed(rng, shape):
    """random doubles of mixed magnitude: uniform * 2^k, k in -30 ... 30"""
    return rng.uniform(0.0, 1.0, shape) * 2.0 ** rng.integers(-30, 31, shape)


# =====================================================================================================================
# A. forms on injected arrays
# =====================================================================================================================
@pytest.mark.parametrize("form,n", LEVEL2_CASES)
def test_level2_form_on_fixtures(lib, form, n):
    import jpeg2png_amd as j
    rng = np.random.default_rng(n)
    arrays = list(nc.fixtures(2, n).items()) + [("random", mixed(rng, n))]
    for nch in (1, 3):
        for c in range(nch):
            for k, (name, v) in enumerate(arrays):
                a = nc.in_channel(v, nch, c, seed=n + k)
                got = j.norm_selftest(form, a)
                assert bits32(got).tolist() == bits32(nc.norms_of_rows(a)).tolist(), (form, n, nch, c, name)
                assert nc.norm_bits(got[c]) == nc.norm_bits(nc.norm(v))
                if name in nc.MUTANTS[2]:
                    assert nc.norm_bits(got[c]) != nc.norm_bits(nc.to_norm(nc.MUTANTS[2][name](v)))


@pytest.mark.parametrize("form,n", LEVEL2_CASES)
def test_level2_form_on_zeros(lib, form, n):
    """all zero; one non-zero at the last index; -0.0 entries (fold_tile_row never leaves one, a reset fill might): +0.0 or
    what the restatement gives"""
    import jpeg2png_amd as j
    last = np.zeros((n, 3))
    last[n - 1] = [3.0, 0.0, 2.0 ** -40]
    some = nc.in_channel(np.full(n, 0.25), 3, 1, seed=n)
    some[::2, 1] = -0.0
    some[n - 1, 0] = -0.0
    for a in (np.zeros((n, 1)), np.zeros((n, 3)), last, np.full((n, 3), -0.0), some):
        got, want = j.norm_selftest(form, a), nc.norms_of_rows(a)
        for c in range(a.shape[1]):
            assert nc.norm_bits(got[c]) in (0, nc.norm_bits(want[c])), (form, n, c)
            if (a[:, c] > 0).any():
                assert nc.norm_bits(got[c]) == nc.norm_bits(want[c])


def band_cuts(n, nband, seed):
    """nband bands of unequal counts that tile n rows, the first of ONE row, listed from the bottom of the canvas up"""
    rng = np.random.default_rng(seed)
    inner = np.sort(rng.choice(np.arange(2, n), nband - 2, replace=False)).tolist() if nband > 2 else []
    edges = [0, 1] + inner + [n]
    return [(edges[i], edges[i + 1] - edges[i]) for i in range(nband)][::-1]


@pytest.mark.parametrize("n", [n for n in nc.LEVEL2_LAUNCH_SIZES if n >= 3])
def test_norm_bands_however_the_rows_are_cut(lib, n):
    import jpeg2png_amd as j
    for nband in (2, 3, 32):
        if n < nband + 1:
            continue
        cuts = band_cuts(n, nband, seed=n + nband)
        assert sum(c for _, c in cuts) == n and cuts[-1] == (0, 1) and len({c for _, c in cuts}) > 1
        for k, (name, v) in enumerate(nc.fixtures(2, n).items()):
            a = nc.in_channel(v, 3, k % 3, seed=n)
            one, cut = j.norm_selftest("norm_bands", a), j.norm_selftest("norm_bands", a, bands=cuts)
            assert bits32(cut).tolist() == bits32(one).tolist() == bits32(nc.norms_of_rows(a)).tolist(), (n, nband, name)


def rows_for_a_partial_last_block(ntx):
    per_block = min(256, 2048 // ntx)                         # launch_k_rowsums
    return per_block, per_block + 1


def test_rowsums_items_per_block():
    assert [rows_for_a_partial_last_block(n)[0] for n in (1, 7, 8, 9, 529)] == [256, 256, 256, 227, 3]


@pytest.mark.parametrize("ntx", [1, 7, 8, 9, 16, 17, 48, 49, 256, 257, 529])
def test_k_rowsums_doubles(lib, ntx):
    import jpeg2png_amd as j
    per_block, rows = rows_for_a_partial_last_block(ntx)
    for nch in (1, 3 if per_block != 3 else 2):
        assert nch * rows > per_block and (nch * rows) % per_block != 0          # several blocks, the last one partial
        a = mixed(np.random.default_rng(ntx + nch), (nch, rows, ntx))
        got = j.norm_selftest("rowsums", a)
        assert got.shape == (rows, nch)
        assert np.array_equal(bits64(got), bits64(nc.strip_sums(a).T))


def norm_whole_check(a, note):
    import jpeg2png_amd as j
    got = j.norm_selftest("norm_whole", a)
    want = nc.norms_of_rows(nc.strip_sums(a).T)
    assert bits32(got).tolist() == bits32(want).tolist(), note
    return got


@pytest.mark.parametrize("ntx", [n for n in nc.LEVEL1_SIZES if n >= 5])
def test_k_norm_whole_level1_on_fixtures(lib, ntx):
    """k_norm_whole lets no level-1 sum out: a level-1 fixture in ONE tile row of one channel, zeros in the channel's other
    rows — direct form up to 48 strips, staged above"""
    for nch, c, rows, r in [(1, 0, 1, 0), (3, 1, 5, 2), (3, 2, 300, 299)]:
        for name, v in nc.fixtures(1, ntx).items():
            a = mixed(np.random.default_rng(ntx), (nch, rows, ntx))
            a[c] = 0.0
            a[c, r] = v
            got = norm_whole_check(a, (ntx, nch, rows, name))
            assert nc.norm_bits(got[c]) == nc.norm_bits(nc.to_norm(nc.strip_sum(v))) != nc.norm_bits(nc.to_norm(nc.MUTANTS[1][name](v)))


@pytest.mark.parametrize("ntx,rows", [(7, 3), (48, 65), (49, 65), (33, 1024), (49, 129),
                                       (49, 512),          # staged in two rounds of 397 and 115 tile rows
                                       (529, 100),         # ... in two of 37 and one of 26
                                       (64, 160),          # a staged copy of exactly 10240 doubles: stage_copy's outer loop runs once
                                       (49, 209)])         # ... of 10241: twice
def test_k_norm_whole_level2_on_fixtures(lib, ntx, rows):
    """level-2 fixtures spread over the tile rows, one non-zero strip each; then partials everywhere"""
    P = nc._pow2(rows)
    stage = 0 if ntx <= 48 else min(rows * ntx, 156 * 1024 // 8 - P)               # launch_k_norm_whole
    if (ntx, rows) in ((49, 512), (529, 100)):
        group = stage // ntx
        assert group < rows and rows % group != 0                                  # several rounds, the last one shorter
    if (ntx, rows) in ((64, 160), (49, 209)):
        assert stage == rows * ntx == (10240 if ntx == 64 else 10241)
    rng = np.random.default_rng(rows)
    for k, (name, v) in enumerate(nc.fixtures(2, rows).items()):
        a = np.zeros((3, rows, ntx))
        a[(k + 1) % 3], a[(k + 2) % 3] = mixed(rng, (rows, ntx)), mixed(rng, (rows, ntx))
        a[k % 3, np.arange(rows), rng.integers(0, ntx, rows)] = v
        got = norm_whole_check(a, (ntx, rows, name))
        assert nc.norm_bits(got[k % 3]) == nc.norm_bits(nc.norm(v)) != nc.norm_bits(nc.to_norm(nc.MUTANTS[2][name](v)))
    norm_whole_check(mixed(rng, (3, rows, ntx)), (ntx, rows, "random"))
    norm_whole_check(mixed(rng, (1, rows, ntx)), (ntx, rows, "random, one channel"))


def test_norm_selftest_refuses_what_the_kernels_cannot_take(lib):
    import jpeg2png_amd as j
    for form, shape in [("fold_tree", (1025, 1)), ("project_tree", (1025, 3)), ("norm_finish", (4097, 1)), ("norm_finish", (4, 4)),
                        ("rowsums", (1, 4, 530)), ("norm_whole", (1, 4097, 1))]:
        with pytest.raises(j.J2PError):
            j.norm_selftest(form, np.zeros(shape))
    for bands in ([(0, 2), (1, 3)], [(0, 2), (3, 1)], [(0, 5)], [(3, 1), (0, 2)]):          # overlap, gap, too long, short
        with pytest.raises(j.J2PError):
            j.norm_selftest("norm_bands", np.zeros((4, 1)), bands=bands)


# =====================================================================================================================
# B. the chain on real gradients, through the solver
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def canvas(kind):
    if kind == "rpw16":        # the smallest one-channel canvas whose strips are 16 rows (33 strips x 65 tile rows >= 2048 wavefronts), with
        return make_case(4096, 1032, "444", 10, seed=61, y_only=True)     # zones (< 12288), an odd tile-row count and a last tile row of 8 rows
    if kind == "rpw8":         # 17 strips (the last one 62 columns) x 128 tile rows of 8
        return make_case(2048, 1024, "444", 10, seed=62, y_only=True)
    if kind == "joint":        # 4:2:0, canvas 272 x 144 of which luma covers 264 x 136: 3 strips (the last 22 columns) x 36 tile rows of 4
        return make_case(264, 136, "420", 10, seed=63)
    if kind == "tall":         # 64 x 2064: one strip x 516 tile rows of 4, an in-kernel tree of P = 1024
        return make_case(64, 2064, "444", 10, seed=64, y_only=True)
    if kind == "taller":       # 64 x 4128: 1032 tile rows, more than one in-kernel tree takes
        return make_case(64, 4128, "444", 10, seed=93, y_only=True)
    raise KeyError(kind)


def solver(kind, band=None, options=(), its=4):
    import jpeg2png_amd as j
    planes = canvas(kind)
    s = j.Solver(planes, 0.3, [0.001] * len(planes), its, band=band)
    for k, v in options:
        s.debug_option(k, v)
    return s


def device_doubles(ptr, n):
    import torch
    from jpeg2png_amd.tiled import alias_tensor
    return alias_tensor(ptr, n, torch.float64, torch.device("cuda", 0))


def read_doubles(s, ptr, n):
    s.sync()
    return device_doubles(ptr, n).cpu().numpy().copy()


def write_doubles(s, ptr, values):
    import torch
    s.sync()
    device_doubles(ptr, values.size).copy_(torch.from_numpy(np.ascontiguousarray(values, np.float64).reshape(-1)))
    torch.cuda.synchronize()


def read_partials(s):
    """(strip partials [channel, local tile row, strip] as left in memory, rows per tile row)"""
    ptr, ntx, ntr, rpw = s.debug_partials()
    assert ntx == nc.ntx_of(s.W) and ntr == -(-(s.row_end - s.row_begin) // rpw)
    return read_doubles(s, ptr, s.nch * ntr * ntx).reshape(s.nch, ntr, ntx), rpw


def read_rowsums(s, which="partials_local"):
    e = s.exchange_info()
    n = e.local_tile_rows if which == "partials_local" else e.global_tile_rows
    return read_doubles(s, getattr(e, which), n * s.nch).reshape(n, s.nch)


def read_norm(s):
    import torch
    from jpeg2png_amd.tiled import alias_tensor
    s.sync()
    return alias_tensor(s.norm_ptr(), s.nch, torch.float32, torch.device("cuda", 0)).cpu().numpy().copy()


def write_norm(s, values):
    import torch
    from jpeg2png_amd.tiled import alias_tensor
    s.sync()
    alias_tensor(s.norm_ptr(), s.nch, torch.float32, torch.device("cuda", 0)).copy_(torch.from_numpy(np.asarray(values, np.float32)))
    torch.cuda.synchronize()


def restated_partials(s, rpw):
    return np.stack([nc.strip_partials(s.download_gradient(c), rpw) for c in range(s.nch)])


def check_partials_against_gradient(s, rpw, stamped):
    """two iterations: the partials of each, sign bit cleared, are strip_partial of the gradient plane; a folding launch has
    stamped them with the iteration's parity"""
    for it in (0, 1):
        s.phase_gradient()
        part, got_rpw = read_partials(s)
        assert got_rpw == rpw
        assert np.array_equal(bits64(np.abs(part)), bits64(restated_partials(s, rpw))), f"iteration {it}"
        if stamped:
            assert (np.signbit(part) == bool(it)).all()
        else:
            assert not np.signbit(part).any()
        s.phase_project()


@pytest.mark.parametrize("fold", [0, 1])
def test_partials_of_16_row_strips_with_zones(lib, fold):
    import jpeg2png_amd as j
    with solver("rpw16", options=[(j.J2P_OPT_NORM_FOLD, fold)]) as s:
        ptr, ntx, ntr, rpw = s.debug_partials()
        assert (s.W, s.H, ntx, ntr, rpw) == (4096, 1032, 33, 65, 16)
        assert ntx * ntr >= 2048 and ntx * ntr < 3 * 4096                 # 16 rows; half and quarter items at the launch's end
        check_partials_against_gradient(s, 16, stamped=bool(fold))


def test_partials_of_8_row_strips(lib):
    with solver("rpw8") as s:
        assert s.debug_partials()[1:] == (17, 128, 8)
        assert s.launches_per_iteration() == 2               # (2 Mpixel: the solver folds by itself, the partials are stamped)
        check_partials_against_gradient(s, 8, stamped=True)


@pytest.mark.parametrize("fold", [0, 1])
def test_partials_of_a_joint_canvas(lib, fold):
    import jpeg2png_amd as j
    with solver("joint", options=[(j.J2P_OPT_NORM_FOLD, fold)]) as s:
        assert (s.W, s.H) == (272, 144) and s.debug_partials()[1:] == (3, 36, 4)
        check_partials_against_gradient(s, 4, stamped=bool(fold))


def exchange_between_bands(bands):
    """what a row-tiled run does between the phases of one-channel bands on one GPU: all-gather of the row sums before the
    projection, the edge rows into the neighbours' halo rows after it (tests/test_parity_gpu.py)"""
    import ctypes
    import jpeg2png_amd as j
    hip = j.hip_runtime()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    D2D = 3
    infos = [s.exchange_info() for s in bands]
    for s in bands:
        s.sync()
    for dst in infos:
        for src in infos:
            hip.hipMemcpy(dst.partials_all + 8 * src.first_tile_row, src.partials_local, 8 * src.local_tile_rows, D2D)
    hip.hipDeviceSynchronize()
    for s in bands:
        s.phase_project()
    for s in bands:
        s.sync()
    infos = [s.exchange_info() for s in bands]
    for up, down in zip(infos, infos[1:]):
        hip.hipMemcpy(down.recv_top[0], up.send_bottom[0], up.halo_floats * 4, D2D)
        hip.hipMemcpy(up.recv_bottom[0], down.send_top[0], up.halo_floats * 4, D2D)
    hip.hipDeviceSynchronize()


BAND_CUTS = {2: [(0, 512), (512, 1032)], 3: [(0, 336), (336, 688), (688, 1032)]}      # multiples of 16 rows


def check_bands_against_whole(iterations):
    with solver("rpw16") as whole:
        wanted = []
        for it in range(iterations):
            whole.phase_gradient()
            part, rpw = read_partials(whole)
            assert rpw == 16
            wanted.append(np.abs(part))
            whole.phase_project()
    for nband, cuts in BAND_CUTS.items():
        bands = [solver("rpw16", band=cut) for cut in cuts]
        try:
            for it in range(iterations):
                for s in bands:
                    s.phase_gradient()
                for s, (r0, r1) in zip(bands, cuts):
                    part, rpw = read_partials(s)
                    assert rpw == 16 and s.exchange_info().first_tile_row == r0 // 16
                    assert (np.signbit(part) == bool(it)).all()                    # bands fold: stamped
                    assert np.array_equal(bits64(np.abs(part)), bits64(wanted[it][:, r0 // 16:-(-r1 // 16)])), (nband, r0, it)
                exchange_between_bands(bands)
        finally:
            for s in bands:
                s.close()


def test_who_marches_a_row_never_changes_a_bit(lib):
    """the canvas of 16-row strips whole and as 2 and 3 band solvers — whose zones differ, the share of half and quarter
    items depends on the BAND's launch — over two iterations, halo rows and row sums exchanged as a row-tiled run does"""
    check_bands_against_whole(2)


@pytest.mark.parametrize("zones", [(0, 0, 0), (256, 256, 256), None, (0, 256, 0), (0, 0, 256), (100, 60, 60)])
def test_who_marches_a_row_with_every_zone_share(exp_lib, monkeypatch, zones):
    """... and with the shares of double / half / quarter items (J2P_ZONE_D / _B / _C, in 1/256 of a launch) forced: none,
    256 each (the clamps leave halves only), the solver's own, quarters only, doubles only, all four kinds"""
    if zones is not None:
        for name, v in zip(("J2P_ZONE_B", "J2P_ZONE_C", "J2P_ZONE_D"), zones):
            monkeypatch.setenv(name, str(v))
    check_bands_against_whole(1)


def test_row_sums_in_the_solver(lib):
    """level 1 where a solve runs it: fold_tile_row (tickets, J2P_OPT_NORM_FOLD 1) on the whole joint canvas, k_rowsums
    (fold 0) on a band of it — partials_local is strip_sum of the partials read back"""
    import jpeg2png_amd as j
    for band, fold in [(None, 1), ((0, 64), 0), ((64, 144), 0), ((0, 64), 1)]:
        with solver("joint", band=band, options=[(j.J2P_OPT_NORM_FOLD, fold)]) as s:
            for it in (0, 1):
                s.phase_gradient()
                part, _ = read_partials(s)
                assert (np.signbit(part) == bool(fold and it)).all()
                assert np.array_equal(bits64(read_rowsums(s)), bits64(nc.strip_sums(np.abs(part)).T)), (band, fold, it)
                if band is not None:                     # (the band's own sums stand in for the other band's: any array will do)
                    e = s.exchange_info()
                    write_doubles(s, e.partials_all, mixed(np.random.default_rng(it), e.global_tile_rows * 3))
                s.phase_project()


@pytest.mark.parametrize("kind", ["rpw16", "joint"])
def test_row_sums_are_the_sum(lib, kind):
    """the sanity bound beside the bit tests: every row sum is within N 2^-53 (relative; N = W x rows terms, all >= 0) of
    the exact sum of the terms the reference adds, float(g * g) (compute.c:203, sqf) — a restatement and a kernel that
    left the same pixels out would still agree with each other"""
    import jpeg2png_amd as j
    with solver(kind, options=[(j.J2P_OPT_NORM_FOLD, 1)]) as s:
        s.phase_gradient()
        rpw = s.debug_partials()[3]
        sums = read_rowsums(s)
        for c in range(s.nch):
            g = s.download_gradient(c)
            sq = (g * g).astype(np.float64)
            for tr in range(sums.shape[0]):
                exact = math.fsum(sq[tr * rpw:(tr + 1) * rpw].ravel().tolist())
                assert abs(sums[tr, c] - exact) <= s.W * rpw * 2.0 ** -53 * exact, (c, tr)
        s.phase_project()


def test_norm_written_by_the_gradient_launch(lib):
    """plan GRADIENT (fold on, J2P_OPT_NORM_IN_PROJECT 0): fold_tree in the solver"""
    import jpeg2png_amd as j
    for kind in ("joint", "tall"):
        with solver(kind, options=[(j.J2P_OPT_NORM_IN_PROJECT, 0), (j.J2P_OPT_NORM_FOLD, 1)]) as s:
            assert s.launches_per_iteration() == 2
            for it in (0, 1):
                s.phase_gradient()
                assert bits32(read_norm(s)).tolist() == bits32(nc.norms_of_rows(read_rowsums(s))).tolist(), (kind, it)
                s.phase_project()


def test_norm_written_by_k_norm_whole(lib):
    """plan NORM_WHOLE (fold off): no row sums in memory, restated from the partials"""
    import jpeg2png_amd as j
    for kind in ("joint", "tall", "rpw8"):
        with solver(kind, options=[(j.J2P_OPT_NORM_IN_PROJECT, 0), (j.J2P_OPT_NORM_FOLD, 0)]) as s:
            assert s.launches_per_iteration() == 3
            for it in (0, 1):
                s.phase_gradient()
                part, _ = read_partials(s)
                assert not np.signbit(part).any()
                s.phase_project()
                assert bits32(read_norm(s)).tolist() == bits32(nc.norms_of_rows(nc.strip_sums(part).T)).tolist(), (kind, it)


def test_norm_written_by_k_norm_finish(lib):
    """plan NORM_FINISH on a whole canvas: 1032 tile rows, more than an in-kernel tree takes"""
    with solver("taller") as s:
        assert s.debug_partials()[1:] == (1, 1032, 4) and s.launches_per_iteration() == 3
        for it in (0, 1):
            s.phase_gradient()
            sums = read_rowsums(s)
            s.phase_project()
            assert bits32(read_norm(s)).tolist() == bits32(nc.norms_of_rows(sums)).tolist(), it


def scaled_fixture(n, nch, like):
    """[n, nch] row sums: channel c holds the level-2 fixture of the c-th mutant, scaled by a power of FOUR — exact in
    every addition, in the conversion and in the square root — so that the norm is of the order of the one `like` gives"""
    found = list(nc.fixtures(2, n).values())
    scale = 4.0 ** round(math.log(float(np.sum(like)) / nch / nc.MIDPOINT, 4))
    a = np.stack([found[c % len(found)] for c in range(nch)], axis=1) * scale
    want = nc.norms_of_rows(a)
    for c in range(nch):        # (still fixtures: the mutant's float is another)
        name = list(nc.fixtures(2, n))[c % len(found)]
        assert nc.norm_bits(want[c]) != nc.norm_bits(nc.to_norm(nc.MUTANTS[2][name](a[:, c])))
    return a, want


def test_band_norm_finish_and_in_project_agree_on_a_fixture(exp_lib, monkeypatch):
    """NIP 2 (a band's k_project reduces partials_all itself) against J2P_BAND_NIP=0 (k_norm_finish in front of it): after
    the gradient phase the global row sums are REPLACED by a level-2 fixture; the planes must agree, and the float
    k_norm_finish left is the restatement's — so NIP 2's wiring (array, length, channel stride) is the tree's of section A"""
    planes, norms = [], []
    for kind, band in (("tall", (0, 1024)), ("joint", (64, 144))):
        for band_nip in ("1", "0"):
            monkeypatch.setenv("J2P_BAND_NIP", band_nip)
            with solver(kind, band=band) as s:
                assert s.launches_per_iteration() == (2 if band_nip == "1" else 3)
                s.phase_gradient()
                e = s.exchange_info()
                a, want = scaled_fixture(e.global_tile_rows, s.nch, read_rowsums(s) * (e.global_tile_rows / e.local_tile_rows))
                write_doubles(s, e.partials_all, a)
                s.phase_project()
                planes.append([s.download(c) for c in range(s.nch)])
                if band_nip == "0":
                    assert bits32(read_norm(s)).tolist() == bits32(want).tolist()
        assert all(bit_equal(p, q) for p, q in zip(planes[-2], planes[-1])), kind


def test_whole_norm_in_project_and_from_memory_agree_on_a_fixture(lib):
    """NIP 1 (every wavefront of k_project reduces partials_local) against J2P_OPT_NORM_IN_PROJECT 0, where the gradient
    launch has written the norm already: that float is checked first, then replaced by the fixture's"""
    import jpeg2png_amd as j
    for kind in ("tall", "joint"):
        planes = []
        for nip in (1, 0):
            with solver(kind, options=[(j.J2P_OPT_NORM_IN_PROJECT, nip), (j.J2P_OPT_NORM_FOLD, 1)]) as s:
                s.phase_gradient()
                e = s.exchange_info()
                sums = read_rowsums(s)
                a, want = scaled_fixture(e.local_tile_rows, s.nch, sums)
                if nip == 0:
                    assert bits32(read_norm(s)).tolist() == bits32(nc.norms_of_rows(sums)).tolist()
                    write_norm(s, want)
                write_doubles(s, e.partials_local, a)
                s.phase_project()
                planes.append([s.download(c) for c in range(s.nch)])
        assert all(bit_equal(p, q) for p, q in zip(*planes)), kind


def test_norm_from_bands_in_the_solver(lib):
    """plan EXTERNAL: k_norm_bands over the bands' own row sums, read in place, listed from the bottom band up"""
    import jpeg2png_amd as j
    cuts = [(0, 64), (64, 144)]
    bands = [solver("joint", band=cut) for cut in cuts]
    try:
        for s in bands:
            s.phase_gradient()
        sums = [read_rowsums(s) for s in bands]
        infos = [s.exchange_info() for s in bands]
        want = nc.norms_of_rows(np.concatenate(sums))
        for s in bands:
            s.norm_from_bands([(e.partials_local, e.first_tile_row, e.local_tile_rows) for e in infos[::-1]])
            assert bits32(read_norm(s)).tolist() == bits32(want).tolist()
        with solver("joint", options=[(j.J2P_OPT_NORM_FOLD, 1)]) as whole:          # (row sums in memory)
            whole.phase_gradient()
            assert np.array_equal(bits64(read_rowsums(whole)), bits64(np.concatenate(sums)))
            whole.phase_project()
        for s in bands:
            s.phase_project()
    finally:
        for s in bands:
            s.close()
