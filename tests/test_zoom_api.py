"""jpeg2png_amd.zoomed(): the planes of an integer zoom (no GPU needed)."""
import pytest

from jpeg2png_amd import synth


def test_zoomed_scales_the_sampling_factors_of_copies():
    import jpeg2png_amd as j
    planes = synth.make_planes(40, 24, "420", 10, seed=1)
    for s in (1, 2, 3, 4):
        z = j.zoomed(planes, s)
        assert [(p.w_samp, p.h_samp) for p in z] == [(s, s), (2 * s, 2 * s), (2 * s, 2 * s)]
        assert [(p.w, p.h) for p in z] == [(p.w, p.h) for p in planes]
        assert all(a is not b and a.data is b.data for a, b in zip(z, planes))
    assert [(p.w_samp, p.h_samp) for p in planes] == [(1, 1), (2, 2), (2, 2)]       # the originals stay as they were


@pytest.mark.parametrize("s", [0, 5, -1, 2.0, True, "2", None])
def test_zoomed_refuses_factors_outside_1_to_4(s):
    import jpeg2png_amd as j
    planes = synth.make_planes(16, 16, "444", 10, seed=1, y_only=True)
    with pytest.raises(j.J2PError):
        j.zoomed(planes, s)
