"""Filtered tensor output without a GPU: the host's taps (j2p_debug_filter_taps, the text the device compiles too) against
the restatement of the header's definition (tests/filter_cases.py) bit for bit; the restatement against a float64 evaluation
of the same definition and against torch's antialiased interpolation; and what the binding refuses before it touches a
device.  The GPU tests (tests/test_filter_gpu.py) compare the kernels with the same restatement bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J2P_EINVAL = -1
BOTH = sorted(fc.FILTERS)
# the cases whose restatement costs a CPU test little: all but the 2048 x 1040 ones, which the GPU tests compute once
CPU_CASES = fc.SMALL_CASES + fc.WIDE_CASES


def source(image, seed=5):
    """a clamped float32 image of the case's size: noise that leaves [0, 255] at both ends before the clamp"""
    if image == "step":
        return fc.step_plane()
    w, h = fc.IMAGES[image]
    rng = np.random.default_rng(seed + w)
    v = np.clip(rng.normal(128., 90., (h, w)).astype(np.float32), np.float32(0), np.float32(255))
    assert (v == 0).any() and (v == 255).any()
    return v


AXES = sorted({(fc.case_box(im, box)[2], ow) for im, box, ow, _ in fc.CASES} | {(fc.case_box(im, box)[3], oh) for im, box, _, oh in fc.CASES}
              | set(fc.AXIS_PAIRS))


# ---- 1. the hook against the restatement ----

@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("box,out", AXES)
def test_the_hosts_taps_are_the_restatement_bit_for_bit(lib, name, box, out):
    filter = fc.FILTERS[name]
    want = fc.taps(filter, box, out)                    # (asserts S > 0.5 and at least one tap for every X)
    assert len(want) == out
    capacity = max(len(ws) for _, ws in want)
    buf = (ctypes.c_float * capacity)()
    first, count = ctypes.c_uint(), ctypes.c_uint()
    for X, (f, ws) in enumerate(want):
        assert lib.j2p_debug_filter_taps(filter, box, out, X, ctypes.byref(first), ctypes.byref(count), buf, capacity) == 0, X
        assert (first.value, count.value) == (f, len(ws)), (X, first.value, count.value, f, len(ws))
        got = np.frombuffer(buf, np.float32, len(ws))
        w32 = np.array(ws, np.float32)
        assert np.array_equal(got.view(np.uint32), w32.view(np.uint32)), (X, got, w32)
        assert abs(float(np.sum(w32.astype(np.float64))) - 1.) <= len(ws) * 2.0 ** -24, (X, "the weights sum to 1")
        assert 0 <= f and f + len(ws) <= box
    if out == box:
        assert all(f == X and len(ws) == 1 and ws[0] == 1 for X, (f, ws) in enumerate(want))
    # windows never move backwards: what lets a tile take its source segment from its first and last column
    firsts = [f for f, _ in want]
    ends = [f + len(ws) for f, ws in want]
    assert firsts == sorted(firsts) and ends == sorted(ends)


def test_the_hook_refuses(lib):
    buf = (ctypes.c_float * 8)()
    first, count = ctypes.c_uint(7), ctypes.c_uint(7)
    args = (ctypes.byref(first), ctypes.byref(count), buf, 8)
    assert lib.j2p_debug_filter_taps(0, 8, 4, 0, *args) == J2P_EINVAL               # area is no filter of this form
    assert lib.j2p_debug_filter_taps(3, 8, 4, 0, *args) == J2P_EINVAL
    assert lib.j2p_debug_filter_taps(fc.TRIANGLE, 0, 4, 0, *args) == J2P_EINVAL
    assert lib.j2p_debug_filter_taps(fc.TRIANGLE, 8, 0, 0, *args) == J2P_EINVAL
    assert lib.j2p_debug_filter_taps(fc.TRIANGLE, 8, 4, 4, *args) == J2P_EINVAL
    assert lib.j2p_debug_filter_taps(fc.TRIANGLE, 8, 4, 0, None, ctypes.byref(count), buf, 8) == J2P_EINVAL
    assert (first.value, count.value) == (7, 7)
    # more taps than room: refused, the count is reported and nothing beyond the room is written
    small = (ctypes.c_float * 3)(9., 9., 9.)
    assert lib.j2p_debug_filter_taps(fc.CUBIC, 64, 4, 1, ctypes.byref(first), ctypes.byref(count), small, 2) == J2P_EINVAL
    assert count.value == len(fc.taps(fc.CUBIC, 64, 4)[1][1]) > 2 and small[2] == 9.


# ---- 2. the restatement against a float64 evaluation of the same definition ----

@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_restatement_is_the_definition_in_float64(case, name):
    image, box, ow, oh = case
    box = fc.case_box(image, box)
    v = source(image)
    got = fc.resample(v, box, ow, oh, fc.FILTERS[name])
    want = fc.evaluate64(v, box, ow, oh, fc.FILTERS[name])
    assert got.shape == (oh, ow) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    limit = fc.bound(box, ow, oh, fc.FILTERS[name])
    print(case, name, "max error", err, "bound", limit, "spare", limit / err if err else float("inf"))
    assert err <= limit
    if ow == box[2] and oh == box[3]:
        assert np.array_equal(got, v[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]), "out == box on both axes is the slice"


# ---- 3. torch's antialiased interpolation: a yardstick for the formula, not the contract ----
# torch forms centres and weights in f32, so it cannot agree bit for bit.  The bounds are twice the largest difference of the
# RESTATEMENT from torch 2.10 over the cases below, per direction (DESIGN.md section 17 has the figures); the margin is there
# because torch's f32 weights may move between versions.  Seen: shrinking 8.46e-3 (1040 -> 1039 columns), enlarging 9.44e-3
# (1040 -> 1041).  Both come from the 1040-wide rows at ratios next to 1: torch's centre (X + 0.5) * scale is an f32, whose last
# place near 1000 is 6e-5 of a pixel, on weights that change by 1 per pixel and values up to 255.  The cases below 64 outputs a
# side stay within 1.7e-4 shrinking (5.2e-4 at 45 x 37 -> 44 x 36) and 1.0e-3 enlarging.  A formula that differed would be off
# by units.
TORCH_BOUND = {"shrinking": 2 * 8.47e-3, "enlarging": 2 * 9.44e-3}


def torch_antialias(crop, oh, ow, mode):
    """F.interpolate(antialias=True) of a float32 [h, w] array.  A one-column output with BOTH axes resized is asked for one
    axis after the other, rows first: for 1040 x 24 -> 1 x 5 torch 2.10 gives, in float32 and float64 alike, values 2.2 away from
    its own one-axis answers applied in that order (which agree with the definition to 1e-4) — it resizes the rows of a tensor
    that is one column wide wrongly — so that form is not used as a yardstick."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(crop))[None, None]
    h, w = crop.shape

    def call(x, size):
        return torch.nn.functional.interpolate(x, size=size, mode=mode, antialias=True, align_corners=False)

    if ow == 1 and w != 1 and oh != h:
        return call(call(t, (oh, w)), (oh, 1))[0, 0].numpy()
    return call(t, (oh, ow))[0, 0].numpy()


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("case", CPU_CASES + [("wide", (0, 0, 33, 17), 50, 29), ("padded_420", (0, 0, 8, 8), 1, 1)],
                         ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_restatement_agrees_with_torch_antialias(case, name):
    image, box, ow, oh = case
    bx, by, bw, bh = fc.case_box(image, box)
    v = source(image)
    got = fc.resample(v, (bx, by, bw, bh), ow, oh, fc.FILTERS[name])
    want = torch_antialias(v[by:by + bh, bx:bx + bw], oh, ow, {"triangle": "bilinear", "cubic": "bicubic"}[name])
    want = np.clip(want, 0, 255)                                   # (torch does not clamp the cubic's overshoot)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    direction = "enlarging" if ow > bw or oh > bh else "shrinking"
    print(case, name, direction, "max difference from torch", err)
    assert err <= TORCH_BOUND[direction]


# ---- 4. properties of the definition ----

def test_negative_zero_becomes_positive_zero_where_nothing_is_resized():
    v = np.full((4, 6), -0.0, np.float32)
    v[2, 3] = 5.
    for filter in fc.FILTERS.values():
        got = fc.resample(v, (1, 1, 4, 2), 4, 2, filter)
        assert np.array_equal(got, v[1:3, 1:5]) and (got.view(np.uint32)[got == 0] == 0).all()


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("value,box,ow,oh", [(0., (0, 0, 45, 37), 7, 5), (255., (0, 0, 45, 37), 7, 5), (37., (3, 2, 40, 30), 9, 7),
                                            (200., (0, 0, 1040, 24), 65, 5), (16., (0, 0, 45, 37), 90, 74), (255., (2, 1, 16, 16), 37, 41),
                                            (101., (0, 0, 5, 3), 64, 40)])
def test_a_flat_integer_plane_resamples_to_itself(value, box, ow, oh, name):
    """To itself as an 8-bit sample, and as a float within the rounding of its sums: the normalised f32 weights of an output
    sum to 1 only within count * 2^-24 (255.0000153 under the triangle from 48 to 77 columns), so bit-exactness of the float is
    not a property of this form — which is why the definition clamps at 255 too.  0 is exact."""
    filter = fc.FILTERS[name]
    v = np.full((box[1] + box[3], box[0] + box[2]), value, np.float32)
    acc = fc.accumulate(v, box, ow, oh, filter)
    off = float(np.abs(acc.astype(np.float64) - value).max())
    print(name, value, box, ow, oh, "largest distance from the value", off)
    assert off <= fc.bound(box, ow, oh, filter) * (value / 255.)
    if value == 0.:
        assert (acc.view(np.uint32) == 0).all()
    m = fc.resample(v, box, ow, oh, filter)
    assert (np.rint(m) == value).all() and m.max() <= 255.


def test_the_clamp_case_needs_both_clamps():
    """a 0 / 255 step at column 24 of 48: the cubic leaves [0, 255] at both ends, the triangle exceeds 255 by rounding alone"""
    v = fc.step_plane()
    box = (0, 0, 48, 40)
    for ow, low, high in ((19, -11.35, 266.35), (77, -12.09, 267.09)):
        acc = fc.accumulate(v, box, ow, 40, fc.CUBIC)
        assert abs(float(acc.min()) - low) < 0.01 and abs(float(acc.max()) - high) < 0.01, (ow, acc.min(), acc.max())
        m = fc.resample(v, box, ow, 40, fc.CUBIC)
        assert m.min() == 0. and m.max() == 255.
    acc = fc.accumulate(v, box, 77, 40, fc.TRIANGLE)
    assert float(acc.max()) > 255. and float(acc.max()) - 255. < 1e-4 and acc.min() >= 0., acc.max()
    assert fc.resample(v, box, 77, 40, fc.TRIANGLE).max() == 255.


# ---- 5. the binding ----

def test_python_refusals_need_no_gpu():
    import jpeg2png_amd as j
    for bad in (dict(out_width=0), dict(out_height=0), dict(out_width=65537), dict(out_height=65537), dict(box=(0, 0, 49, 40)),
                dict(box=(40, 0, 9, 40)), dict(box=(0, 39, 48, 2)), dict(box=(-1, 0, 4, 4)), dict(box=(0, 0, 0, 4)), dict(box=(0, 0, 8))):
        with pytest.raises(j.J2PError):
            j._c_resample(48, 40, bad.get("out_width"), bad.get("out_height"), bad.get("box"), fc.TRIANGLE)
    with pytest.raises(j.J2PError):
        j._c_resample(None, 40, 4, 4, None, fc.CUBIC)
    r = j._c_resample(48, 40, None, None, None, fc.CUBIC)
    assert (r.box_x, r.box_y, r.box_w, r.box_h, r.out_w, r.out_h, r.filter) == (0, 0, 48, 40, 48, 40, 2)
    r = j._c_resample(48, 40, 65536, None, (1, 2, 30, 20), fc.TRIANGLE)           # larger than the box: allowed
    assert (r.box_x, r.box_y, r.box_w, r.box_h, r.out_w, r.out_h, r.filter) == (1, 2, 30, 20, 65536, 20, 1)
    for bad in ("lanczos", "nearest", 1, "Triangle"):
        with pytest.raises(j.J2PError, match="filter"):
            j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=7, filter=bad)
    # Batch.submit refuses a filter without tensor= before it looks at anything else
    with pytest.raises(j.J2PError, match="tensor"):
        j.Batch.submit(object.__new__(j.Batch), [None] * 3, 0.3, [0.001] * 3, 2, width=48, height=40, filter="cubic")
    # Solver.to_tensor refuses a bad resample before it needs torch or the solver
    with pytest.raises(j.J2PError, match="65536"):
        j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=65537, filter="triangle")


def test_no_filter_and_area_make_the_calls_they_made(monkeypatch):
    """filter=None and filter="area" build the same j2p_resize, refuse the same, and never come near the new calls; "triangle"
    builds a j2p_resample from the same keywords"""
    import jpeg2png_amd as j

    class Stop(Exception):
        pass

    calls = []
    real_resize, real_resample = j._c_resize, j._c_resample

    def spy_resize(*a):
        r = real_resize(*a)
        calls.append(("resize", a, bytes(r)))
        return r

    def spy_resample(*a):
        r = real_resample(*a)
        calls.append(("resample", a, bytes(r)))
        return r

    def stop(*_a, **_k):
        raise Stop()

    monkeypatch.setattr(j, "_c_resize", spy_resize)
    monkeypatch.setattr(j, "_c_resample", spy_resample)
    monkeypatch.setattr(j, "_torch", stop)              # what Solver.to_tensor does next
    monkeypatch.setattr(j, "_c_planes", stop)           # what Batch.submit does next
    kw = dict(out_width=7, out_height=5, box=(1, 2, 30, 20))
    want = ("resize", (48, 40, 7, 5, (1, 2, 30, 20)), bytes(j._CResize(1, 2, 30, 20, 7, 5)))
    for extra in ({}, {"filter": None}, {"filter": "area"}):
        calls.clear()
        with pytest.raises(Stop):
            j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, **kw, **extra)
        with pytest.raises(Stop):
            j.Batch.submit(object.__new__(j.Batch), [None] * 3, 0.3, [0.001] * 3, 2, width=48, height=40, tensor=object(), **kw, **extra)
        assert calls == [want, want], extra
        # enlarging stays refused, in the words it was refused in
        with pytest.raises(j.J2PError, match="enlarging is what zooming is for"):
            j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=49, **extra)
        with pytest.raises(j.J2PError, match="enlarging is what zooming is for"):
            j.Batch.submit(object.__new__(j.Batch), [None] * 3, 0.3, [0.001] * 3, 2, width=48, height=40, tensor=object(), out_height=41, **extra)
        # and without any of the keywords nothing is built at all
        calls.clear()
        with pytest.raises(Stop):
            j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, **extra)
        assert calls == []
    calls.clear()
    with pytest.raises(Stop):
        j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, filter="triangle", **kw)
    with pytest.raises(Stop):
        j.Batch.submit(object.__new__(j.Batch), [None] * 3, 0.3, [0.001] * 3, 2, width=48, height=40, tensor=object(), filter="cubic",
                       out_width=96, out_height=80)
    assert calls == [("resample", (48, 40, 7, 5, (1, 2, 30, 20), 1), bytes(j._CResample(1, 2, 30, 20, 7, 5, 1))),
                     ("resample", (48, 40, 96, 80, None, 2), bytes(j._CResample(0, 0, 48, 40, 96, 80, 2)))]


def test_symbols_and_structs(lib):
    import jpeg2png_amd as j
    for name in ("j2p_planes_to_tensor_resampled", "j2p_batch_submit_resampled", "j2p_debug_filter_taps"):
        assert name in j.C_ABI_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(j._CResample) == 28
    # the structs that may not grow did not
    assert ctypes.sizeof(j._CResize) == 24 and ctypes.sizeof(j._CTensor) == 64
    size, off = j.job_layout()
    assert size == ctypes.sizeof(j._CJob) and off + ctypes.sizeof(j._CTensor) == size
    # NULL arguments are refused without a device
    assert lib.j2p_planes_to_tensor_resampled(None, 3, 8, 8, None, None) == J2P_EINVAL
    assert lib.j2p_batch_submit_resampled(None, None, None, None) == J2P_EINVAL


def test_the_package_still_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import jpeg2png_amd as j\n"
            "r = j._c_resample(48, 40, 77, 5, None, 2)\n"
            "assert (r.out_w, r.filter) == (77, 2)\n"
            "try:\n"
            "    j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=77, filter='cubic')\n"
            "except j.J2PError as e:\n"
            "    assert 'PyTorch' in str(e), e\n"
            "else:\n"
            "    raise SystemExit('no error')\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-800:]
