"""The constructions of tests/screen_cases.py, checked without a GPU: every builder finds what it aims at, the float32
restatement of the operands agrees with the oracle's own iteration-0 gradient, and the oracle is the compiled reference
bitwise on every one of these planes — which is what makes its per-iteration trace the truth that
tests/test_screens_gpu.py holds k_gradient to (the reference itself exposes no gradient)."""
import numpy as np
import pytest

import screen_cases as sc
from conftest import bit_equal
from oracle import bindings
from oracle_trace import differing

F = np.float32
SITE_IDS = [f"{kind}-{layout}-{group}-{sc.GROUPS[group][i][0]},{sc.GROUPS[group][i][1]}" for kind, layout, group, i in sc.SITES]
BOUNDARY_IDS = [f"{group}-{layout}-w{weight}" for group, layout, weight in sc.BOUNDARY_CASES]
ALL_CASES, ALL_IDS, get_case = sc.ALL_CASES, sc.ALL_IDS, sc.get_case


@pytest.mark.parametrize("kind,layout,group,i", sc.SITES, ids=SITE_IDS)
def test_every_builder_finds_its_site(kind, layout, group, i):
    """one radicand of the site is 0x407ffffe / 0x407fffff times a power of 4, a numerator divided by that norm is
    +-2^j, every value in reach passes the operand screen, and the site is the only candidate of the
    mantissa screen in its row, whose neighbours are ordinary screened rows of texture"""
    case = sc.site_case(kind, layout, group)                 # (raises LookupError where the builder finds nothing)
    site = case.sites[i]
    assert (site.x, site.y) == sc.GROUPS[group][i]
    ops = sc.site_operands(case.planes, site.x, site.y)
    rad = ops.tv if kind.startswith("tv") else ops.tgv
    nums = ops.tv_numerators if kind.startswith("tv") else ops.tgv_numerators
    assert sc.is_offending(rad) and sc.bits(rad) == site.radicand, hex(sc.bits(rad))
    assert sc.bits(rad) & 0x7fffff == sc.MANTISSAS[site.variant % 2]
    assert any(sc.is_missed_numerator(n) for ch in nums for n in ch)
    assert sc.bits(rad) & 0xffff >= 0xfffe                   # what allones_candidate looks at
    chans = sc.canvases(case.planes)
    assert all(f[site.y, site.x] == 0 for f in chans)
    assert all(sc.passes_operand_screen(f[site.y - 1:site.y + 3]).all() for f in chans)
    assert sc.candidate_rows(case.planes)[site.y] == [site.x]
    assert sc.screened_rows(case.planes)[site.y]
    # texture, not a flat plane, around the site
    row = chans[0][site.y, max(0, site.x - 40):site.x + 40]
    assert len(np.unique(row)) > 8
    # the scalar and the vectorised restatement are the same arithmetic
    r1, r2 = sc.radicand_planes(case.planes)
    assert sc.bits(r1[site.y, site.x]) == sc.bits(ops.tv) and sc.bits(r2[site.y, site.x]) == sc.bits(ops.tgv)


def test_no_two_sites_of_a_plane_share_a_row_trip():
    """a wavefront's row trip is one row of one strip: sites of one plane are in different rows or in different strips"""
    def strip(x):
        return [k for k, (a, b) in enumerate(sc.STRIPS) if a - 2 <= x <= b + 2]
    for group, positions in sc.GROUPS.items():
        for i, (x0, y0) in enumerate(positions):
            for (x1, y1) in positions[i + 1:]:
                assert y0 != y1 or not set(strip(x0)) & set(strip(x1)), (group, (x0, y0), (x1, y1))
                assert abs(y0 - y1) > 2 or abs(x0 - x1) > 4, "implanted values overlap"


def test_the_known_operand_values_are_what_the_builders_use():
    """the operand values the sites are made of: (1.0, 0x3fddb3d6) -> 0x407ffffe, (0.5, 0x3ff7def5) -> 0x407fffff, the TGV2
    pair (0x405cc470, 0xbfb988e0) -> sy = 1.0 and 0x417ffffe, and a gx0 == 1.0f for gx0 = 0x3fddb3d8 with three channels"""
    for (gx, gy), want in zip(sc.TV1_PAIRS, (0x407ffffe, 0x407fffff)):
        assert sc.bits(sc.f32(gx) * sc.f32(gx) + sc.f32(gy) * sc.f32(gy)) == want
    assert sc.tgv_pair(0x7ffffe) == (0x405cc470, 0xbfb988e0)
    rad, nums = sc._tgv_radicand(sc.f32(0x405cc470), sc.f32(0xbfb988e0))
    assert sc.bits(rad) == 0x417ffffe and nums[2] == F(1.0)
    u, v = sc.tgv_pair(0x7fffff)                              # the search, twice: deterministic
    assert (u, v) == sc.find_tgv_pair(0x7fffff)
    rad, nums = sc._tgv_radicand(sc.f32(u), sc.f32(v))
    assert sc.is_offending(rad) and sc.bits(rad) & 0x7fffff == 0x7fffff and nums[2] == F(1.0)
    assert sc.tv_scale(3) * sc.f32(sc.TV3_GX0) == F(1.0)
    with pytest.raises(LookupError):
        sc.find_tgv_pair(0x7fffff, reach=0, targets=(16.0,))


def test_the_ieee_quotient_at_the_tv_site():
    """sqrtf(0x407ffffe) = 2 - 2^-23, the all-ones norm, and 1.0 / (2 - 2^-23) rounds to 0x3f000001: the quotient the
    reference adds to the site's right neighbour, and the one the short division misses"""
    n = np.sqrt(sc.f32(0x407ffffe))
    assert sc.bits(n) == 0x3fffffff == sc.bits(F(2.0 - 2.0 ** -23))
    assert sc.bits(F(1.0) / n) == 0x3f000001
    assert sc.bits(np.sqrt(sc.f32(0x407fffff))) == 0x3fffffff          # the other radicand has the same root


@pytest.mark.parametrize("group,layout,weight", sc.BOUNDARY_CASES, ids=BOUNDARY_IDS)
def test_every_boundary_plane_holds_what_its_group_says(group, layout, weight):
    case = sc.boundary_case(group, layout, weight)
    chans = sc.canvases(case.planes)
    inside = [f[y0:y0 + h, x0 + c:x0 + c + w] for c, f in enumerate(chans) for (x0, y0, w, h) in case.patches]
    if group == "outside":
        assert all((~sc.passes_operand_screen(p)).any(axis=1).all() for p in inside)
        values = {sc.bits(abs(v)) for p in inside for v in p[~sc.passes_operand_screen(p)]}
        assert values == {sc.bits(sc.SCREEN_LO) - 1, sc.bits(sc.SCREEN_HI)}
        return
    assert all(sc.passes_operand_screen(f).all() for f in chans)
    gx = np.concatenate([np.abs(np.diff(p, axis=1)).ravel() for p in inside])
    xx = np.concatenate([np.abs(np.diff(p, n=2, axis=1)).ravel() for p in inside])
    if group in ("small", "mixed"):
        assert {sc.bits(v) for p in inside for v in p.ravel()} >= {sc.bits(v) for v in sc.SMALL}
        assert F(2.0 ** -43) in gx                           # the smallest first difference the range allows
    if group == "large":
        assert {sc.bits(abs(v)) for p in inside for v in p.ravel()} == {sc.bits(F(2.0 ** 41 - 2.0 ** 17))}
    if group in ("large", "large_plain"):
        for p in inside:
            assert (np.sign(p[:, 1:]) == -np.sign(p[:, :-1])).all() and (np.sign(p[1:]) == -np.sign(p[:-1])).all()
    if group != "small":
        assert 2.0 ** 42 <= xx.max() < 2.0 ** 43             # second differences near 2^43
    if group in ("small", "large_plain", "mixed"):
        fast = [sc.predicted_fast_rows(case.planes, x0, y0) for (x0, y0, _, _) in case.patches]
        assert min(fast) >= 1 and 2 * sum(fast) >= sc.PATCH_H * len(case.patches), fast


@pytest.mark.parametrize("name", list(sc.TABLES))
def test_the_table_planes_hold_the_steps_around_8192(name):
    case = sc.table_case(name)
    q = np.asarray(case.planes[0].quant_table).astype(np.int64)
    assert set(sc.TABLES[name]) <= set(q.tolist()) and q.max() < 32768
    assert (q.max() ** 2 > 1 << 26) == (8193 in sc.TABLES[name])
    d = np.asarray(case.planes[0].data).reshape(-1, 64)
    # the large steps carry coefficients, 8193 at position 2 included (and whether k_project's table path is on depends on
    # the table alone: one step with q * q > 2^26 switches it off for the plane)
    assert all(np.any(d[:, pos] != 0) for pos in (1, 8, 2)[:len(sc.TABLES[name])])
    assert sc.passes_operand_screen(case.planes[0].fdata).all()


@pytest.mark.parametrize("key", [k for k in ALL_CASES if k[0] in ("site", "boundary")],
                         ids=[i for k, i in zip(ALL_CASES, ALL_IDS) if k[0] in ("site", "boundary")])
def test_the_restated_operands_give_the_oracle_s_iteration_0_gradient(key):
    """the numpy float32 gather made of the radicands and numerators of screen_cases (IEEE quotients) equals the oracle's
    traced gradient of iteration 0 in every bit of every channel: the operands computed here are the ones the oracle —
    and a kernel that is bit-identical to it — divides"""
    case = get_case(key)
    trace = sc.expectation(case)["trace"]
    got = sc.restated_gradient(case.planes, case.weight)
    for c in range(len(case.planes)):
        bad = differing(got[c], trace[0, c, 0])
        assert not bad, f"channel {c}: {len(bad)} pixels differ, first {bad[0]}"
    assert np.isfinite(trace).all()


@pytest.mark.parametrize("key", ALL_CASES, ids=ALL_IDS)
def test_the_oracle_is_the_reference_on_these_planes(key):
    """3 iterations (the table planes: their 6) of the unmodified compiled reference against the oracle, bitwise"""
    if not bindings.have_ref():
        pytest.skip("oracle/_ref not built")
    case = get_case(key)
    want = sc.expectation(case)["want"]
    ref, _, _ = bindings.ref_compute(sc.fresh(case), case.weight, case.pweights, case.iterations)
    for c in range(len(case.planes)):
        assert bit_equal(ref[c], want[c]), f"channel {c}: first of {len(differing(ref[c], want[c]))} at {differing(ref[c], want[c])[0]}"
        assert bit_equal(want[c], sc.expectation(case)["trace"][case.iterations - 1, c, 1])
