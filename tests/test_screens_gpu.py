"""k_gradient's two fast-path screens, aimed at: the planes of tests/screen_cases.py hold pixels whose norm has an all-ones
mantissa TOGETHER WITH a numerator the short division is known to miss there (the mantissa screen, allones_candidate), and
patches of values at the very edges of the range the operand screen accepts.  The march is bit-identical to the reference
only if it routes these rows onto the IEEE path (or, for the in-range patches, if the exact rewritings of the screened path
hold at the ends of their range), so everything here is bitwise against the oracle — whose equality with the compiled
reference on these very planes tests/test_screen_cases_cpu.py shows — and the per-iteration gradient is compared as well:
extreme values are gone after the first projection, iteration 0's gradient is the only place they show.

The negative control builds the library with -DJ2P_EXP_NO_ALLONES_SCREEN (the one statement of the march that applies the
mantissa screen left out) and requires that the directed planes then come out WRONG, around their sites and nowhere else."""
import os

import numpy as np
import pytest

import screen_cases as sc
from conftest import band_devices, bit_equal
from oracle_trace import differing, first_difference
from screen_cases import ALL_CASES, ALL_IDS, get_case
from test_tiled_verify_gpu import _variant

pytestmark = pytest.mark.gpu

DIRECTED = [(k, i) for k, i in zip(ALL_CASES, ALL_IDS) if k[0] != "plain"]
CUT = 16                             # two bands: rows [0, 16) and the rest, so that the sites of rows 14-16 straddle the cut


def near_sites(case, x, y):
    return "; ".join(f"site {s.id} radicand {s.radicand:#x} numerator {s.numerator:#x}" for s in case.sites
                     if abs(s.x - x) <= 2 and abs(s.y - y) <= 2) or "no site within 2 pixels"


def test_this_gpu_s_short_division_misses_what_the_sites_aim_at(lib):
    """the precondition of everything below, asserted: the twice-refined reciprocal is wrong for 226 radicands, and the
    one-correction quotient is wrong at 0x407ffffe and 0x407fffff for the numerator 1.0 and for no other of the 2^23 —
    2 mismatches in the last 2^14 radicands below 4.  (The count was recorded as 4 while k_div_exhaustive compared only
    the even numerator of each pair and counted it twice: 1.0 + 2^-23 is divided correctly.)"""
    import jpeg2png_amd as j
    why = ("this GPU's v_rsq_f32 seed differs from the one the sites of tests/screen_cases.py were aimed with: "
           "the sites have to be re-aimed (tools/division_exhaustive.py lists the quotients the short form misses here)")
    bad, offenders = j.division_exhaustive(1)
    assert bad == 226, f"{bad} radicands with a wrong reciprocal, first {offenders}: {why}"
    bad, offenders = j.division_exhaustive(2, (1 << 24) - (1 << 14), 1 << 14)
    assert {int(o, 16) for o in offenders} == {0x407ffffe3f800000, 0x407fffff3f800000} and bad == 2, \
        f"{bad} wrong quotients just below 4, {offenders}: {why}"


@pytest.mark.parametrize("key", [k for k, _ in DIRECTED], ids=[i for _, i in DIRECTED])
def test_directed_operands_match_the_oracle_bit_for_bit(lib, oracle, key):
    """every site plane, boundary plane and table plane: (1) gradient and iterate of every iteration of a whole-canvas
    Solver against the oracle's trace; (2) compute() without and with logging — the logging form of the march divides by
    another sequence — against the oracle's planes, the log rows to the 1e-9 the suite holds them to everywhere (they are
    double sums taken in another order); (3) two row bands cut at row 16, final planes"""
    import jpeg2png_amd as j
    case = get_case(key)
    e = sc.expectation(case)
    n, its = len(case.planes), case.iterations
    d = first_difference(case.planes, case.weight, case.pweights, its, e["trace"])
    assert d is None, f"{case.name}: {d} ({near_sites(case, d.x, d.y)})"
    for log in (False, True):
        got = sc.fresh(case)
        rows = j.compute(got, case.weight, case.pweights, its, log=log)
        for c in range(n):
            bad = differing(got[c].fdata, e["want"][c])
            assert not bad, f"{case.name} compute(log={log}) channel {c}: {len(bad)} differ, first {bad[0]} ({near_sites(case, *bad[0])})"
        if log:
            np.testing.assert_allclose(rows, e["rows"], rtol=1e-9, atol=1e-9)
    H = e["want"][0].shape[0]
    with j.TiledSolver(case.planes, case.weight, case.pweights, its, devices=band_devices(2), cuts=[0, CUT, H]) as t:
        assert [(r0, r1) for _, r0, r1 in t.bands()] == [(0, CUT), (CUT, H)]
        t.run(its)
        for c in range(n):
            bad = differing(t.download(c), e["want"][c])
            assert not bad, f"{case.name} two bands channel {c}: {len(bad)} differ, first {bad[0]} ({near_sites(case, *bad[0])})"


@pytest.mark.timeout(900)
def test_without_the_mantissa_screen_the_sites_come_out_wrong(lib, oracle):
    """negative control.  A library built with -DJ2P_EXP_NO_ALLONES_SCREEN (tools/build_variant.py) keeps rows with an
    all-ones norm on the short division.  There the 1-channel TV site planes must differ from the oracle's iteration-0
    gradient, only within 2 pixels of a site, at a pixel that a site's own terms reach at least once per plane; a plane
    without sites must still be bit-identical through all its iterations.  Wrong bits are the expected outcome — nothing
    faults.  A variant that passes the directed comparison means that the directed test proves nothing"""
    import jpeg2png_amd as j
    lib_path = _variant("no_allones_screen", "-DJ2P_EXP_NO_ALLONES_SCREEN")
    assert os.path.exists(lib_path)
    report = []
    with j.library(lib_path):
        for kind, layout, group in sc.SITE_PLANES:
            if kind != "tv1":
                continue
            case = sc.site_case(kind, layout, group)
            trace = sc.expectation(case)["trace"]
            with j.Solver(case.planes, case.weight, case.pweights, case.iterations) as s:
                s.phase_gradient()
                got = s.download_gradient(0)
            bad = differing(got, trace[0, 0, 0])
            hit = sorted({site.id for site in case.sites for (x, y) in bad if (x, y) in site.reached()})
            report.append(f"{case.name}: {len(bad)} pixels wrong at {bad}; sites that show: {hit} of {len(case.sites)}")
            assert bad, (f"{case.name}: the library WITHOUT the mantissa screen reproduces the oracle's iteration-0 gradient — "
                         "the sites do not reach the short division's wrong quotients, the directed test is vacuous")
            for (x, y) in bad:
                assert any(abs(site.x - x) <= 2 and abs(site.y - y) <= 2 for site in case.sites), \
                    f"{case.name}: pixel ({x},{y}) differs and is not within 2 pixels of a site"
            assert hit, f"{case.name}: none of the differing pixels {bad} is reached by a site's own terms"
        plain = sc.plain_case()
        d = first_difference(plain.planes, plain.weight, plain.pweights, plain.iterations, sc.expectation(plain)["trace"])
        assert d is None, f"a plane without sites differs in the variant: {d}"
    print("\n".join(["without the mantissa screen:"] + report))
    # ... and the release library, loaded again, is right on the same planes (the directed test holds it to all of them)
    case = sc.site_case("tv1", "y", "cols")
    with j.Solver(case.planes, case.weight, case.pweights, case.iterations) as s:
        s.phase_gradient()
        assert bit_equal(s.download_gradient(0), sc.expectation(case)["trace"][0, 0, 0])
