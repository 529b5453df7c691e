"""Flat and uniformly coloured planes, the preconditions: what the reference's arithmetic (the oracle; the compiled
reference too where it is built) does with the cases of tests/degenerate_cases.py — so that tests/test_degenerate_gpu.py
cannot pass vacuously: K0 / K1 really never move and log zeros, K2 really takes the zero branch in iteration 0 and a
norm below den_ok()'s 2^-20 afterwards, K3b's chroma does both beside an ordinary luma norm.  No GPU needed."""
import numpy as np
import pytest

import degenerate_cases as dc
from conftest import bit_equal, parity_note

one_value, minus_zeros = dc.one_value, dc.minus_zeros
THREE_CHANNEL_SHAPES = [s for s, kw in dc.SHAPES.items() if not kw.get("y_only")]


@pytest.mark.parametrize("shape,kind", [c for c in dc.CASES if c[1] in ("K0", "K1")], ids=lambda v: v)
def test_zero_and_exact_dc_planes_never_move(oracle, shape, kind):
    planes, e = dc.case(shape, kind)
    for c, p in enumerate(planes):
        assert one_value(p.fdata)
        assert (p.fdata == 0).all() == (kind == "K0")                   # K1: the plane is not 0
        assert dc.restated_norm(p, dc.PWEIGHT) == 0.0
        assert bit_equal(e["want"][c], e["input"][c]), f"channel {c} after {dc.ITERATIONS} iterations"
        assert minus_zeros(e["want"][c]) == 0
    assert e["rows"].shape == (dc.ITERATIONS, 4)
    assert (e["rows"] == 0.0).all() and not np.signbit(e["rows"]).any()


@pytest.mark.parametrize("shape", [s for s in dc.SHAPES if "K2" in dc.SHAPE_KINDS[s]])
def test_inexact_dc_planes_take_the_zero_branch_and_then_a_tiny_norm(oracle, shape):
    planes, e = dc.case(shape, "K2")
    for c, p in enumerate(planes):
        assert one_value(p.fdata) and p.data[0] != 0
        assert not dc.round_trip_is_exact(p, int(p.data[0]))
        assert bit_equal(e["o1"][c], e["input"][c]), f"channel {c}: iteration 0 has ||g|| = 0"
        assert not bit_equal(e["want"][c], e["input"][c]), f"channel {c} never moved"
        norm = dc.restated_norm(p, dc.PWEIGHT)
        assert 0 < norm < dc.DEN_OK_MIN, f"channel {c}: restated ||g|| = {norm!r}"
    assert (e["rows"][0] == 0.0).all()
    uniform = dc.uniform_channels(planes, "K2")
    assert uniform
    for c in uniform:
        assert one_value(e["want"][c]), f"channel {c}"


@pytest.mark.parametrize("shape", THREE_CHANNEL_SHAPES + ["420_77x53"])
def test_tinted_chroma_beside_live_luma(oracle, shape):
    """K3b: the chroma channels stay uniform, are unchanged after 1 iteration and changed after 2, in a solve whose luma
    norm is ordinary — also at the ragged 4:2:0 77x53 the regimes were first measured on"""
    if shape in dc.SHAPES:
        planes, e = dc.case(shape, "K3b")
    else:
        planes = dc.make("K3b", 77, 53, "420", seed=7)
        e = {"input": dc.upsampled(planes)}
        for key, its in (("o1", 1), ("o2", 2), ("want", dc.ITERATIONS)):
            e[key], _ = oracle.oracle_compute(planes, dc.WEIGHT, [dc.PWEIGHT] * 3, its)
    assert int(planes[1].data[0]) > 0 > int(planes[2].data[0])
    assert not one_value(planes[0].fdata)
    assert not bit_equal(e["o1"][0], e["input"][0])                     # the luma moves from iteration 0 on
    assert dc.uniform_channels(planes, "K3b") == [1, 2]
    for c in (1, 2):
        assert bit_equal(e["o1"][c], e["input"][c]), f"channel {c}"
        assert not bit_equal(e["o2"][c], e["input"][c]), f"channel {c}"
        assert one_value(e["o2"][c]) and one_value(e["want"][c]), f"channel {c}"
        assert 0 < dc.restated_norm(planes[c], dc.PWEIGHT) < dc.DEN_OK_MIN


@pytest.mark.parametrize("shape", THREE_CHANNEL_SHAPES)
def test_grey_photograph_and_zero_luma(oracle, shape):
    """K3a / K3c: the zero channels of a joint solve never move while the live ones do"""
    for kind, zero in (("K3a", (1, 2)), ("K3c", (0,))):
        planes, e = dc.case(shape, kind)
        for c in range(3):
            if c in zero:
                assert not np.asarray(planes[c].data).any()
                assert bit_equal(e["want"][c], e["input"][c]) and not e["want"][c].any(), f"{kind} channel {c}"
            else:
                assert not bit_equal(e["o1"][c], e["input"][c]), f"{kind} channel {c}"
        assert e["rows"][0, 2] > 0                                      # tv of the live channels


@pytest.mark.parametrize("shape", list(dc.SHAPES))
def test_upper_half_zeroed_image_and_its_cuts(oracle, shape):
    """K4: the zeroed rows are a whole number of tile rows and of every channel's block rows, the input is exactly 0
    there and live below, and the cuts give one band that holds nothing else"""
    planes, e = dc.case(shape, "K4")
    n = dc.upper_rows(planes)
    H = e["input"][0].shape[0]
    assert n % 16 == 0 and 0 < n < H
    for c, p in enumerate(planes):
        assert n % (8 * p.h_samp) == 0
        assert not e["input"][c][:n].any() and minus_zeros(e["input"][c][:n]) == 0
        assert e["input"][c][n:].any()
    for nband in (2, 3):
        cuts = dc.k4_cuts(planes, nband)
        assert cuts[0] == 0 and cuts[1] == n and cuts[-1] == H and len(cuts) == nband + 1
        assert all(a < b for a, b in zip(cuts, cuts[1:]))
        assert all(v % 16 == 0 and all(v % (8 * p.h_samp) == 0 for p in planes) for v in cuts[:-1])


def test_the_search_raises_when_there_is_nothing_to_find():
    from jpeg2png_amd import synth
    plane = synth.Plane(8, 8, 1, 1, np.zeros(64, np.int16), np.full(64, 8, np.uint16))
    exact = [k for k in range(1, 64) if dc.round_trip_is_exact(plane, k)]
    assert exact                                                         # q = 8: decode(dc) = dc exactly for small dc
    assert dc.find_dc(plane, exact=True) == exact[0]
    everything = lambda *_: True                                         # noqa: E731
    saved, dc.round_trip_is_exact = dc.round_trip_is_exact, everything
    try:
        with pytest.raises(LookupError):
            dc.find_dc(plane, exact=False)
    finally:
        dc.round_trip_is_exact = saved


@pytest.mark.parametrize("shape", list(dc.SHAPES))
def test_oracle_equals_the_compiled_reference(oracle, shape):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    for kind in dc.SHAPE_KINDS[shape]:
        planes, e = dc.case(shape, kind)
        for c in range(len(planes)):
            assert bit_equal(e["want"][c], e["ref"][c]), f"{kind} channel {c}"
        np.testing.assert_allclose(e["rows"][:, 1:], e["ref_rows"][:, 1:], rtol=1e-9, atol=2e-6, err_msg=kind)
    parity_note(f"degenerate {shape} {', '.join(dc.SHAPE_KINDS[shape])}: oracle bit-identical to the reference ({dc.ITERATIONS} iterations)")
