"""Zooming on the GPU: the solve of planes whose sampling factors are all multiplied by s (jpeg2png_amd.zoomed) against
the UNMODIFIED reference's compute() on the same planes, bit for bit, with the wide-footprint projection path on and
off; the path actually taken where it should be; row bands equal to the whole canvas; the checked build."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import band_devices, bit_equal, make_case, parity_note

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (synth subsampling, Y only, image width): wide enough for at least one whole strip of the widest channel
SUBS = {"444": ("444", False, 150), "420": ("420", False, 150), "422": ("422", False, 150), "411": ("411", False, 270),
        "Y": ("444", True, 150)}
WIDE = (3, 4, 6, 8)


def _need_ref(oracle):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")


def solve(planes, weight, pweight, its, wide=1, mixed=1, log=False):
    """(canvas planes, log rows or None, per channel: does it take the wide-footprint path)"""
    import jpeg2png_amd as j
    with j.Solver(planes, weight, pweight, its) as s:
        s.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, wide)
        s.debug_option(j.J2P_OPT_MIXED_PROJECT, mixed)
        rows = s.run(its, log=log)
        paths = [s.wide_footprint(c) for c in range(len(planes))]
        return [s.download(c) for c in range(len(planes))], rows, paths


def check_log(got, want):
    # (the reference's CSV holds 6 decimals, logger.c:24)
    np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=1e-9, atol=2e-6)


@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("s", [2, 3, 4])
def test_zoomed_solve_is_bit_identical_to_the_reference_on_both_paths(lib, oracle, s, sub):
    import jpeg2png_amd as j
    _need_ref(oracle)
    kind, y_only, w = SUBS[sub]
    k = list(SUBS).index(sub) + s
    # ragged sizes: padded coefficient planes and edge strips take the generic path beside the new one
    planes = make_case(w + 3 * s + 1, 90 + 5 * s + 1, kind, 30, seed=100 + k, y_only=y_only)
    z = j.zoomed(planes, s)
    weight = 0.3 if k % 2 else 0.0                      # TGV / plain TV
    pw = [0.001 if k % 3 else 0.0] * len(z)
    log = k % 4 == 1
    its = 8
    want, want_log, _ = oracle.ref_compute(z, weight, pw, its, log=log)
    for wide, mixed in [(1, 1), (1, 0), (0, 1)]:
        got, rows, paths = solve(z, weight, pw, its, wide, mixed, log)
        for c in range(len(z)):
            assert bit_equal(got[c], want[c]), f"x{s} {sub} channel {c} (wide {wide}, mixed {mixed})"
        if log:
            check_log(rows, want_log)
        if wide and not mixed:
            assert paths == [p.w_samp in WIDE for p in z]
        if not wide:
            assert not any(paths)
    parity_note(f"zoom x{s} {sub} {z[0].w * z[0].w_samp}x{z[0].h * z[0].h_samp}: bit-identical to the reference, "
                f"wide-footprint path on and off")


def test_wide_footprint_path_reported_for_every_new_footprint(lib):
    """the (3,3), (4,4), (6,6) and (8,8) channels of 4:2:0 zoomed 3 and 4 times take the new path on a canvas large
    enough to have interior strips (and beyond the one-launch size of small canvases); 2x2 and 1x1 channels do not;
    J2P_OPT_WIDE_FOOTPRINT 0 turns it off, with the same bits"""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    planes = synth.make_planes(640, 480, "420", 30, seed=5)
    seen = set()
    for s in (2, 3, 4):
        z = j.zoomed(planes, s)
        with j.Solver(z, 0.3, [0.001] * 3, 3) as sv:
            assert sv.W * sv.H > 1 << 20
            paths = [sv.wide_footprint(c) for c in range(3)]
            assert paths == [p.w_samp in WIDE for p in z], (s, paths)
            seen |= {(p.w_samp, p.h_samp) for p, on in zip(z, paths) if on}
            sv.run(3)
            on = [sv.download(c) for c in range(3)]
            sv.reset()
            sv.debug_option(j.J2P_OPT_WIDE_FOOTPRINT, 0)
            assert not any(sv.wide_footprint(c) for c in range(3))
            sv.run(3)
            for c in range(3):
                assert bit_equal(sv.download(c), on[c]), (s, c)
    assert seen == {(4, 4), (3, 3), (6, 6), (8, 8)}


def test_zoomed_large_canvas_matches_the_reference(lib, oracle):
    """one canvas beyond the one-launch size (1280 x 960, x2 of 4:2:0): the per-class launches with the 4x4 path"""
    import jpeg2png_amd as j
    _need_ref(oracle)
    z = j.zoomed(make_case(640, 480, "420", 50, seed=21), 2)
    want, want_log, _ = oracle.ref_compute(z, 0.3, [0.001] * 3, 5, log=True)
    got, rows, paths = solve(z, 0.3, [0.001] * 3, 5, log=True)
    assert paths == [False, True, True]
    for c in range(3):
        assert bit_equal(got[c], want[c]), c
    check_log(rows, want_log)
    parity_note("zoom x2 420 1280x960: bit-identical to the reference")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_zoomed_row_bands_equal_the_whole_canvas(lib, s):
    """2-4 aligned row bands on one GPU (TiledSolver, and Batch with tile=True and no size gate): the band-edge rows
    the new path pushes into the neighbours' halos must make the bands equal the whole-canvas solve bitwise"""
    import jpeg2png_amd as j
    z = j.zoomed(make_case(300 + s, 200 + s, "420", 30, seed=30 + s), s)
    its = 6
    ref = copy.deepcopy(z)
    j.compute(ref, 0.3, [0.001] * 3, its)
    nb = s                                              # 2, 3, 4 bands
    with j.TiledSolver(z, 0.3, [0.001] * 3, its, devices=band_devices(nb)) as t:
        assert len(t.bands()) >= 2
        for b in range(nb):
            assert [t.band_solver(b).wide_footprint(c) for c in range(3)] == [p.w_samp in WIDE for p in z]
        t.run(its)
        for c in range(3):
            assert bit_equal(t.download(c), ref[c].fdata), f"x{s} channel {c}: {nb} bands"
    with j.Batch(devices=band_devices(2), slots_per_device=1) as b:
        out = b.wait(b.submit(z, 0.3, [0.001] * 3, its, tile=True, tile_min_band_pixels=0))
    for c in range(3):
        assert bit_equal(out[c], ref[c].fdata), f"x{s} channel {c}: Batch tile=True"


def test_zoomed_batch_round_trip_joint_and_separate(lib):
    """Batch.submit on zoomed planes: RGB of s*w x s*h, float planes of the joint canvas, and with separate=True each
    component's own zoomed canvas, equal to one-channel solves"""
    import jpeg2png_amd as j
    w, h, s, its = 150, 100, 3, 5
    z = j.zoomed(make_case(w, h, "420", 30, seed=41), s)
    ref = copy.deepcopy(z)
    j.compute(ref, 0.3, [0.001] * 3, its)
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        rgb = b.wait(b.submit(z, 0.3, [0.001] * 3, its, width=s * w, height=s * h, bits=8))
        joint = b.wait(b.submit(z, 0.3, [0.001] * 3, its))
        sep = b.wait(b.submit(z, [0.3, 0.0, 0.0], [0.001] * 3, its, separate=True))
    assert rgb.shape == (s * h, s * w, 3)
    for c in range(3):
        assert bit_equal(joint[c], ref[c].fdata)
        one = [copy.deepcopy(z[c])]
        j.compute(one, [0.3, 0.0, 0.0][c], [0.001], its)
        assert sep[c].shape == (z[c].h * z[c].h_samp, z[c].w * z[c].w_samp)
        assert bit_equal(sep[c], one[0].fdata), c


def test_zoomed_checked_build_reports_no_violations(lib):
    """the checked build (-DJ2P_DEBUG): every global access of the new path inside its range, same bits"""
    import jpeg2png_amd as j
    from jpeg2png_amd.buildlib import build_debug
    z = j.zoomed(make_case(200, 136, "420", 30, seed=51), 3)
    want, _, _ = solve(z, 0.3, [0.001] * 3, 4, mixed=0)
    with j.library(build_debug()):
        assert j.debug_build()
        for mixed in (0, 1):
            with j.Solver(z, 0.3, [0.001] * 3, 4) as sv:
                sv.debug_option(j.J2P_OPT_MIXED_PROJECT, mixed)
                assert sv.wide_footprint(1) == (not mixed)
                sv.run(4)
                assert sv.debug_violations()[0] == 0
                for c in range(3):
                    assert bit_equal(sv.download(c), want[c])


def test_randomised_zoom_sweep_matches_the_reference(lib, oracle):
    """tools/sweep_zoom.py as a test: 30 cases of the shared case stream zoomed 2-4 times, path and launch form drawn at
    random, each bit-identical to the reference"""
    _need_ref(oracle)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sweep_zoom.py"), "30", "7"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "30/30 zoomed cases bit-identical to the reference" in r.stdout
    parity_note("zoom sweep: 30/30 randomised zoomed cases bit-identical to the reference")
