"""Resized tensor output without a GPU: the integer taps, the numpy restatement of the definition (tests/resize_cases.py)
against the float64 area integral and against torch's own area interpolation, and what the binding refuses before it touches a
device.  The GPU tests (tests/test_resize_gpu.py) compare the kernel with the same restatement bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(image, seed=5):
    """a clamped float32 image of the case's size: noise that leaves [0, 255] at both ends before the clamp"""
    w, h = rc.IMAGES[image]
    rng = np.random.default_rng(seed + w)
    v = rng.normal(128., 90., (h, w)).astype(np.float32)
    v = np.clip(v, np.float32(0), np.float32(255))
    assert (v == 0).any() and (v == 255).any()
    return v


AXES = sorted({(rc.case_box(im, box)[2], ow) for im, box, ow, _ in rc.CASES} | {(rc.case_box(im, box)[3], oh) for im, box, _, oh in rc.CASES})


@pytest.mark.parametrize("box,out", AXES)
def test_taps_partition_the_box(box, out):
    t = rc.taps(box, out)
    assert len(t) == out
    if out == box:
        assert t == [(X, [1]) for X in range(box)]
        return
    for first, ws in t:
        assert sum(ws) == box and all(1 <= a <= out for a in ws)
    assert t[0][0] == 0 and t[-1][0] + len(t[-1][1]) == box
    for (f0, w0), (f1, _) in zip(t, t[1:]):
        last0 = f0 + len(w0) - 1
        assert f1 in (last0, last0 + 1), "consecutive outputs share at most one source index and leave no gap"
    # every source index is covered with total weight `out`
    cover = np.zeros(box, np.int64)
    for first, ws in t:
        cover[first:first + len(ws)] += ws
    assert (cover == out).all()
    # and the padded arrays say the same
    idx, wts = rc.tap_arrays(box, out)
    assert (wts.sum(axis=1) == box).all() and idx.max() == box - 1


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_restatement_is_the_area_integral(case):
    image, box, ow, oh = case
    box = rc.case_box(image, box)
    v = source(image)
    got = rc.resample(v, box, ow, oh)
    want = rc.integral(v, box, ow, oh)
    assert got.shape == (oh, ow) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(case, "max error", err, "bound", rc.bound(box, ow, oh))
    assert err <= rc.bound(box, ow, oh)
    if ow == box[2] and oh == box[3]:
        assert np.array_equal(got, v[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]), "a pure crop is the slice"


@pytest.mark.parametrize("w,h,ow,oh", [(64, 48, 16, 16), (48, 40, 12, 10), (45, 37, 45, 37), (1040, 24, 65, 6)])
def test_integer_ratios_agree_with_torch_area_interpolation(w, h, ow, oh):
    import torch
    rng = np.random.default_rng(w * h)
    v = np.clip(rng.normal(128., 90., (h, w)), 0, 255).astype(np.float32)
    got = rc.resample(v, (0, 0, w, h), ow, oh)
    want = torch.nn.functional.interpolate(torch.from_numpy(v)[None, None], size=(oh, ow), mode="area")[0, 0].numpy()
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print((w, h, ow, oh), "max difference from torch", err)
    assert err <= 2 * rc.bound((0, 0, w, h), ow, oh)


@pytest.mark.parametrize("value,box,ow,oh", [(0., (0, 0, 45, 37), 7, 5), (255., (0, 0, 45, 37), 7, 5), (37., (3, 2, 40, 30), 9, 7),
                                            (200., (0, 0, 1040, 24), 65, 5), (16., (0, 0, 1040, 24), 1039, 23)])
def test_a_flat_integer_plane_resamples_to_itself(value, box, ow, oh):
    assert value * box[2] * box[3] < 2 ** 24             # every product and partial sum is an integer below 2^24: exact
    v = np.full((box[1] + box[3], box[0] + box[2]), value, np.float32)
    assert (rc.resample(v, box, ow, oh) == np.float32(value)).all()


def test_negative_zero_becomes_positive_zero_in_a_crop():
    v = np.full((4, 6), -0.0, np.float32)
    got = rc.resample(v, (1, 1, 4, 2), 4, 2)
    assert (got.view(np.uint32) == 0).all()


def test_python_refusals_need_no_gpu():
    import jpeg2png_amd as j
    for bad in (dict(out_width=49), dict(out_height=41), dict(out_width=0), dict(box=(0, 0, 49, 40)), dict(box=(40, 0, 9, 40)),
                dict(box=(0, 39, 48, 2)), dict(box=(-1, 0, 4, 4)), dict(box=(0, 0, 0, 4)), dict(box=(0, 0, 8)), dict(box=(4, 4, 8, 8), out_width=9)):
        with pytest.raises(j.J2PError):
            j._c_resize(48, 40, bad.get("out_width"), bad.get("out_height"), bad.get("box"))
    with pytest.raises(j.J2PError):
        j._c_resize(None, 40, 4, 4, None)
    r = j._c_resize(48, 40, None, None, None)
    assert (r.box_x, r.box_y, r.box_w, r.box_h, r.out_w, r.out_h) == (0, 0, 48, 40, 48, 40)
    r = j._c_resize(48, 40, 7, None, (1, 2, 30, 20))
    assert (r.box_x, r.box_y, r.box_w, r.box_h, r.out_w, r.out_h) == (1, 2, 30, 20, 7, 20)
    # Batch.submit refuses the keywords without tensor= before it looks at anything else (no batch, no device: the unbound
    # method on a bare object)
    for kw in (dict(out_width=8), dict(out_height=8), dict(box=(0, 0, 8, 8))):
        with pytest.raises(j.J2PError, match="tensor"):
            j.Batch.submit(object.__new__(j.Batch), [None] * 3, 0.3, [0.001] * 3, 2, width=48, height=40, **kw)
    # Solver.to_tensor refuses a bad resize before it needs torch or the solver
    with pytest.raises(j.J2PError, match="larger than the box"):
        j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=49)


def test_symbols_and_struct(lib):
    import jpeg2png_amd as j
    for name in ("j2p_planes_to_tensor_resized", "j2p_batch_submit_resized"):
        assert name in j.C_ABI_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(j._CResize) == 24
    # the structs that may not grow did not
    assert ctypes.sizeof(j._CTensor) == 64
    size, off = j.job_layout()
    assert size == ctypes.sizeof(j._CJob) and off + ctypes.sizeof(j._CTensor) == size
    # NULL arguments are refused without a device
    assert lib.j2p_planes_to_tensor_resized(None, 3, 8, 8, None, None) == -1
    assert lib.j2p_batch_submit_resized(None, None, None, None) == -1


def test_the_package_still_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import jpeg2png_amd as j\n"
            "r = j._c_resize(48, 40, 7, 5, None)\n"
            "assert r.out_w == 7\n"
            "try:\n"
            "    j.Solver.to_tensor(object.__new__(j.Solver), 48, 40, out_width=7)\n"
            "except j.J2PError as e:\n"
            "    assert 'PyTorch' in str(e), e\n"
            "else:\n"
            "    raise SystemExit('no error')\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-800:]
