"""tests/norm_cases.py checked against itself, without a GPU: every fixture separates the pinned association of the ||g||
reduction from the mutant it was searched for — as FLOAT norms, which is all that most forms of the reduction let out of
the kernel — every live mutant of every size the GPU tests run has one, and the array forms of the restatement are the
scalar forms bit for bit.  Substituting any mutant for strip_sum / tree therefore fails test_fixture_separates."""
import numpy as np
import pytest

import norm_cases as nc

CASES = [(1, n) for n in nc.LEVEL1_SIZES] + [(2, n) for n in nc.LEVEL2_LAUNCH_SIZES]


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("level,n", CASES)
def test_fixture_separates(level, n):
    found = nc.fixtures(level, n)
    assert sorted(found) == sorted(nc.live(level, n))               # every live mutant has a fixture
    for name, v in found.items():
        assert v.shape == (n,) and v.dtype == np.float64 and (v > 0).all()
        want, wrong = nc.to_norm(nc.PINNED[level](v)), nc.to_norm(nc.MUTANTS[level][name](v))
        assert nc.norm_bits(want) != nc.norm_bits(wrong), (level, n, name)


def test_which_mutants_are_live():
    # fewer than three values have one association; up to four strips the eight running sums hold one element each, so
    # the mutants that keep a pairwise combine are strip_sum itself
    assert nc.live(2, 1) == [] and nc.live(2, 2) == [] and nc.live(1, 1) == [] and nc.live(1, 2) == []
    assert sorted(nc.live(2, 3)) == ["adjacent_pairs", "reversed", "sequential"]
    assert sorted(nc.live(1, 4)) == ["interleaved8_sequential_combine", "sequential"]
    assert "interleaved16" not in nc.live(1, 8) and "interleaved16" in nc.live(1, 9)
    for level, n in CASES:
        if n >= 9:
            assert sorted(nc.live(level, n)) == sorted(nc.MUTANTS[level])
    # ... and at n = 3 the adjacent-pair tree IS the sequential sum: their fixtures may coincide, both differ from tree
    x = [nc._Sym(i) for i in range(3)]
    assert nc.l2_adjacent_pairs(x).ident == nc.l2_sequential(x).ident != nc.tree(x).ident


@pytest.mark.parametrize("n", [n for n in nc.LEVEL2_LAUNCH_SIZES if n >= 3])
@pytest.mark.parametrize("nch,c", [(1, 0), (3, 0), (3, 1), (3, 2)])
def test_fixture_in_an_interleaved_channel(n, nch, c):
    for name, v in nc.fixtures(2, n).items():
        a = nc.in_channel(v, nch, c, seed=n)
        assert bits64(a[:, c]).tolist() == bits64(v).tolist()
        got = nc.norms_of_rows(a)
        assert nc.norm_bits(got[c]) == nc.norm_bits(nc.norm(v)) != nc.norm_bits(nc.to_norm(nc.MUTANTS[2][name](v)))
        for o in range(nch):
            assert nc.norm_bits(got[o]) == nc.norm_bits(nc.norm(a[:, o]))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 1023, 1024])
def test_padding_to_64_changes_nothing(n):
    """norm_tree_load pads to at least 64 rows: only +0.0 joins sums that are >= +0.0"""
    rng = np.random.default_rng(n)
    arrays = list(nc.fixtures(2, n).values()) + [rng.uniform(0, 1, n) * 2.0 ** rng.integers(-30, 31, n), np.zeros(n)]
    for v in arrays:
        assert bits64(nc.tree(v, least=64)) == bits64(nc.tree(v))
        assert bits64(nc.tree_rows(v[:, None], least=64)[0]) == bits64(nc.tree(v))


@pytest.mark.parametrize("n", [1, 4, 7, 8, 9, 17, 48, 49, 529])
def test_array_forms_are_the_scalar_forms(n):
    rng = np.random.default_rng(100 + n)
    a = rng.uniform(0, 1, (3, 5, n)) * 2.0 ** rng.integers(-30, 31, (3, 5, n))
    want = np.array([[nc.strip_sum(a[c, r]) for r in range(5)] for c in range(3)])
    assert np.array_equal(bits64(nc.strip_sums(a)), bits64(want))
    b = rng.uniform(0, 1, (n, 3)) * 2.0 ** rng.integers(-30, 31, (n, 3))
    want = np.array([nc.tree(b[:, c]) for c in range(3)])
    assert np.array_equal(bits64(nc.tree_rows(b)), bits64(want))


def test_the_pinned_sums_are_sums():
    rng = np.random.default_rng(7)
    v = rng.uniform(0, 1, 777)
    for fn in [nc.strip_sum, nc.tree] + list(nc.MUTANTS[1].values()) + list(nc.MUTANTS[2].values()):
        assert abs(float(fn(v)) - float(np.sum(v))) < 1e-10


@pytest.mark.parametrize("W,rows,rpw", [(8, 4, 4), (128, 16, 16), (136, 21, 16), (256, 19, 8), (376, 16, 4), (384, 9, 4)])
def test_strip_partials_cover_every_pixel_once(W, rows, rpw):
    """the strips' ownership rule (march_rows) tiles the canvas: with g = 1 the partials count the pixels — exact in any
    order — and a plane with ONE non-zero pixel has one non-zero partial, its square"""
    ntx, ntr = nc.ntx_of(W), (rows + rpw - 1) // rpw
    p = nc.strip_partials(np.ones((rows, W), np.float32), rpw)
    assert p.shape == (ntr, ntx) and p.sum() == rows * W
    for tr in range(ntr):
        assert p[tr].sum() == W * (min((tr + 1) * rpw, rows) - tr * rpw)
    for x, y in [(0, 0), (1, rows - 1), (W - 1, 0), (W - 2, rows - 1), (min(125, W - 1), rows // 2), (min(126, W - 1), 1), (W // 2, rows - 1)]:
        g = np.zeros((rows, W), np.float32)
        g[y, x] = 3.0
        p = nc.strip_partials(g, rpw)
        assert np.count_nonzero(p) == 1 and p[y // rpw].sum() == 9.0
        assert p[y // rpw, min(max(x - 2, 0) // nc.STRIP_COLS, ntx - 1)] == 9.0


def test_strip_partial_association():
    """lane, then pixel, then row within the group of four, then (a0 + a1) + (a2 + a3), then the lane tree — on values
    whose sum depends on the order"""
    rng = np.random.default_rng(5)
    g = (rng.uniform(0.5, 1, (16, 128)) * 2.0 ** rng.integers(-12, 12, (16, 128))).astype(np.float32)
    sq = (g * g).astype(np.float64)                      # the FLOAT product, as compute.c:203 adds it
    lanes = []
    for l in range(64):
        a = []
        for grp in range(4):
            s = 0.0
            for t in range(4 * grp, 4 * grp + 4):
                s = s + float(sq[t, 2 * l])
                s = s + float(sq[t, 2 * l + 1])
            a.append(s)
        lanes.append((a[0] + a[1]) + (a[2] + a[3]))
    for off in (32, 16, 8, 4, 2, 1):
        for l in range(64 - off):
            lanes[l] = lanes[l] + lanes[l + off]
    assert bits64(nc.strip_partial(g, 16, 0, 0)) == bits64(lanes[0])
    assert bits64(lanes[0]) != bits64(np.float64(sum(float(x) for x in sq.ravel())))        # (the order matters here)
