"""Filtered tensor output on the GPU (j2p_planes_to_tensor_resampled, j2p_batch_submit_resampled, the filter= keyword of
Solver.to_tensor and Batch.submit).  Every comparison is of BIT PATTERNS, tolerance zero, against the restatement of the header's
definition (tests/filter_cases.py) applied to Solver.download(c) of the same solver.  Every destination is a window of a larger
tensor pre-filled with a sentinel, and every byte outside the window is checked afterwards (the helpers of
tests/test_resize_gpu.py).  The kernel stages 512 source columns at a time: the rows of the 1040 wide image are two chunks and a
tail.  Solves are 2 iterations, shared by module fixtures and left unchanged."""
import ctypes

import numpy as np
import pytest

import filter_cases as fc
from conftest import make_case
from test_resize_gpu import BIAS, SCALE, Image, bits, c_tensor, check_window, sentinel, torch_dtype, window

J2P_EINVAL, J2P_ESTATE = -1, -4
BOTH = sorted(fc.FILTERS)


class Filtered(Image):
    """test_resize_gpu's solved image, with the filtered form's expectation and C entry point"""

    def want(self, box, ow, oh, name, dtype, layout, scale=None, bias=None):
        return fc.expected(self.planes, self.w, self.h, self.box(box), ow, oh, fc.FILTERS[name], dtype, layout, scale, bias)

    def resampled(self, ct, box, ow, oh, filter, w=None, h=None, refs=None, nplane=None):
        """the C entry point; synchronises afterwards"""
        r = self.j._CResample(*self.box(box), ow, oh, filter)
        rcode = self.lib.j2p_planes_to_tensor_resampled(self.refs if refs is None else refs, self.n if nplane is None else nplane,
                                                        self.w if w is None else w, self.h if h is None else h, ctypes.byref(r), ctypes.byref(ct))
        for s in self.solvers:
            s.sync()
        return rcode


def step_planes():
    """one luma plane of 48 x 40 whose blocks hold a DC coefficient alone, 200 below zero in the left three block columns and 200
    above in the right three (quantisation steps of 1: the solver may move a coefficient by half a unit): far outside [0, 255]
    after the +128 on both sides, so the clamped image is the 0 / 255 step of filter_cases.step_plane"""
    from jpeg2png_amd import synth
    from oracle import bindings
    data = np.zeros((5, 6, 64), np.int16)
    data[:, :3, 0] = -1600
    data[:, 3:, 0] = 1600
    p = synth.Plane(48, 40, 1, 1, data.reshape(-1), np.ones(64, np.uint16))
    p.fdata = bindings.decode_plane(p)
    return [p]


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def images(lib):
    import jpeg2png_amd as j
    made = {
        "clamping_444": Filtered(j, make_case(48, 40, "444", 3, seed=18), 48, 40),
        "padded_420": Filtered(j, make_case(45, 37, "420", 10, seed=5), 45, 37),
        "padded_420_s": Filtered(j, make_case(45, 37, "420", 10, seed=5), 45, 37, separate=True),
        "grey": Filtered(j, make_case(45, 37, "420", 25, seed=11, y_only=True), 45, 37),
        "wide": Filtered(j, make_case(1040, 24, "420", 10, seed=3), 1040, 24),
        "large_grey": Filtered(j, make_case(2048, 1040, "420", 10, seed=9, y_only=True), 2048, 1040, its=1),
        "step": Filtered(j, step_planes(), 48, 40),
    }
    assert (made["padded_420"].s.W, made["padded_420"].s.H) == (48, 48) and made["grey"].n == 1 and made["step"].n == 1
    assert {(k, (m.w, m.h)) for k, m in made.items() if k in fc.IMAGES} == set(fc.IMAGES.items())
    yield made
    for m in made.values():
        m.close()


# ---- 1. the definition, case by case ----

@pytest.mark.gpu
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_every_case_is_the_definition(torch_cuda, images, case):
    """both filters; f32 CHW (m itself, after * 1 + 0) and u8 HWC, through Solver.to_tensor; the 4:2:0 image also from the three
    solvers of `-s`, through the C entry point.  The 2048 x 1040 image: f32 only."""
    import jpeg2png_amd as j
    torch = torch_cuda
    image, box, ow, oh = case
    for name in BOTH:
        for key in [image] + (["padded_420_s"] if image == "padded_420" else []):
            c = images[key]
            kw = {} if box is None else {"box": box}
            means = [fc.resample(v, c.box(box), ow, oh, fc.FILTERS[name]) for v in fc.clamped(c.planes, c.w, c.h)]
            for dtype, layout in (("f32", "chw"),) + (() if image == "large_grey" else (("u8", "hwc"),)):
                buf, win, idx = window(torch, c.n, ow, oh, dtype, layout)
                want = fc.elements(means, dtype, layout)
                if key.endswith("_s"):
                    torch.cuda.synchronize()
                    assert c.resampled(c_tensor(j, win, layout, dtype), box, ow, oh, fc.FILTERS[name]) == 0
                else:
                    assert c.s.to_tensor(c.w, c.h, layout=layout, out=win, out_width=ow, out_height=oh, filter=name, **kw) is win
                check_window(buf, idx, want, dtype, (key, case, name, dtype, layout))
    if image == "padded_420":
        assert not np.array_equal(images["padded_420"].planes[1], images["padded_420_s"].planes[1])   # (two different solves)


@pytest.mark.gpu
def test_the_clamp_case_clamps_at_both_ends(torch_cuda, images):
    """the solved step image IS the 0 / 255 step, the restatement leaves [0, 255] on it before the clamp — below and above under
    the cubic, above by rounding alone under the triangle — and the kernel's u8 and f32 elements are the clamped ones"""
    torch = torch_cuda
    c = images["step"]
    v = fc.clamped(c.planes, c.w, c.h)[0]
    assert np.array_equal(v, fc.step_plane())
    box = (0, 0, 48, 40)
    for name, ow in (("cubic", 19), ("cubic", 77), ("triangle", 77)):
        acc = fc.accumulate(v, box, ow, 40, fc.FILTERS[name])
        assert (acc > 255.).any() and ((acc < 0.).any() or name == "triangle"), (name, ow, acc.min(), acc.max())
        for dtype in ("u8", "f32"):
            buf, win, idx = window(torch, 1, ow, 40, dtype, "chw")
            c.s.to_tensor(48, 40, out=win, out_width=ow, out_height=40, filter=name)
            want = c.want(None, ow, 40, name, dtype, "chw")
            assert want.min() == 0 and want.max() == (255 if dtype == "u8" else 0x437f0000)
            check_window(buf, idx, want, dtype, (name, ow, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", ["u8", "f16", "bf16", "f32"])
def test_every_dtype_and_layout(torch_cuda, images, dtype, layout):
    torch = torch_cuda
    kw = {} if dtype == "u8" else {"scale": SCALE, "bias": BIAS}
    for name, (ow, oh) in (("triangle", (7, 5)), ("cubic", (53, 41))):
        for key in ("clamping_444", "padded_420"):
            c = images[key]
            buf, win, idx = window(torch, 3, ow, oh, dtype, layout)
            c.s.to_tensor(c.w, c.h, layout=layout, out=win, out_width=ow, out_height=oh, filter=name, **kw)
            want = c.want(None, ow, oh, name, dtype, layout, **kw)
            assert len(np.unique(want)) > 16
            check_window(buf, idx, want, dtype, (key, name, dtype, layout))
    # allocated by the call: the shape is the output's, larger than the image
    g = images["grey"]
    t = g.s.to_tensor(45, 37, dtype=torch_dtype(dtype), layout=layout, out_width=50, out_height=40, filter="cubic")
    assert tuple(t.shape) == ((1, 40, 50) if layout == "chw" else (40, 50, 1)) and t.is_contiguous()
    assert np.array_equal(bits(t), g.want(None, 50, 40, "cubic", dtype, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH)
def test_nothing_resized_is_the_slice_of_to_tensor(torch_cuda, images, name):
    c = images["padded_420"]
    whole = bits(c.s.to_tensor(c.w, c.h, scale=SCALE, bias=BIAS))
    source = np.stack(fc.clamped(c.planes, c.w, c.h))
    for bx in (1, 2, 3, 5):
        t = c.s.to_tensor(c.w, c.h, box=(bx, 2, 40, 30), filter=name, scale=SCALE, bias=BIAS)     # no out_*: the box's size
        assert tuple(t.shape) == (3, 30, 40)
        want = whole[:, 2:32, bx:bx + 40]
        same = (bits(t) == want) | (source[:, 2:32, bx:bx + 40].view(np.uint32) == 0x80000000)   # identical wherever the source is not -0
        assert same.all(), (name, bx)


# ---- 2. strided destinations ----

@pytest.mark.gpu
def test_a_padded_slot_of_a_batch_tensor_and_a_transposed_view(torch_cuda, images):
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f16")
    batch = torch.full((2, 3, 12, 16), fill, dtype=torch.float16, device="cuda:0")
    slot = batch[1, :, 2:10, 4:12]
    c.s.to_tensor(c.w, c.h, out=slot, out_width=8, out_height=8, scale=SCALE, bias=BIAS, filter="triangle")
    want = np.full((2, 3, 12, 16), fill_bits, np.uint16)
    want[1, :, 2:10, 4:12] = c.want(None, 8, 8, "triangle", "f16", "chw", SCALE, BIAS)
    assert np.array_equal(bits(batch), want)
    # transposed, and larger than the box: x steps over whole columns
    store = torch.full((3, 61, 50), fill, dtype=torch.float32, device="cuda:0")
    view = store.transpose(1, 2)
    assert tuple(view.shape) == (3, 50, 61) and view.stride(2) == 50
    c.s.to_tensor(c.w, c.h, out=view, out_width=61, out_height=50, filter="cubic")
    assert np.array_equal(bits(store), c.want(None, 61, 50, "cubic", "f32", "chw").transpose(0, 2, 1))


@pytest.mark.gpu
def test_calls_of_different_sizes_reuse_the_scratch(torch_cuda, images):
    """a small call, one whose taps need more scratch, the small one again — queued back to back on one stream, each reading the
    taps the call before it has overwritten"""
    torch = torch_cuda
    c = images["wide"]
    fill, fill_bits = sentinel("f32")
    shapes = [(7, 5, "triangle"), (1041, 30, "cubic"), (7, 5, "triangle"), (3, 2, "cubic")]
    outs = [torch.full((3, oh, ow), fill, dtype=torch.float32, device="cuda:0") for ow, oh, _ in shapes]
    for t, (ow, oh, name) in zip(outs, shapes):
        c.s.to_tensor(c.w, c.h, out=t, out_width=ow, out_height=oh, filter=name)
    for t, (ow, oh, name) in zip(outs, shapes):
        assert np.array_equal(bits(t), c.want(None, ow, oh, name, "f32", "chw")), (ow, oh, name)


# ---- 3. refusals ----

@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f32")
    t = torch.full((3, 60, 70), fill, dtype=torch.float32, device="cuda:0")
    t8 = torch.full((3, 60, 70), 201, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ok = c_tensor(j, t, "chw", "f32")
    T = fc.TRIANGLE
    refused = {
        "filter 0 (area)": c.resampled(ok, None, 7, 5, 0),
        "filter 3": c.resampled(ok, None, 7, 5, 3),
        "filter -1": c.resampled(ok, None, 7, 5, -1),
        "empty box": c.resampled(ok, (0, 0, 0, 5), 1, 1, T),
        "empty box rows": c.resampled(ok, (0, 0, 5, 0), 1, 1, T),
        "box leaves the image right": c.resampled(ok, (40, 0, 6, 5), 3, 3, T),
        "box leaves the image below": c.resampled(ok, (0, 30, 5, 8), 3, 3, T),
        "box inside the canvas, outside the image": c.resampled(ok, (0, 0, 48, 37), 8, 8, T),
        "box_x beyond": c.resampled(ok, (45, 0, 1, 1), 1, 1, T),
        "box wraps around": c.resampled(ok, (2, 0, 0xffffffff, 5), 3, 3, T),
        "out_w 0": c.resampled(ok, None, 0, 5, T),
        "out_h 0": c.resampled(ok, None, 7, 0, fc.CUBIC),
        "out_w 65537": c.resampled(ok, None, 65537, 5, T),
        "out_h 65537": c.resampled(ok, None, 7, 65537, fc.CUBIC),
        "image beyond the canvas": c.resampled(ok, (0, 0, 49, 37), 7, 5, T, w=49),
        "two planes": c.resampled(ok, None, 7, 5, T, nplane=2),
        "u8 with a scale": c.resampled(c_tensor(j, t8, "chw", "u8", scale=(1, 2, 1)), None, 7, 5, T),
        "unknown dtype": c.resampled(c_tensor(j, t, "chw", 4), None, 7, 5, T),
        "stride 0": c.resampled(c_tensor(j, t, "chw", "f32", strides=(60 * 70, 0, 1)), None, 7, 5, T),
        "NULL data": c.resampled(c_tensor(j, t, "chw", "f32", data=0), None, 7, 5, T),
        "misaligned": c.resampled(c_tensor(j, t, "chw", "f32", data=t.data_ptr() + 2), None, 7, 5, T),
        "NULL resample": c.lib.j2p_planes_to_tensor_resampled(c.refs, 3, 45, 37, None, ctypes.byref(ok)),
        "NULL tensor": c.lib.j2p_planes_to_tensor_resampled(c.refs, 3, 45, 37, ctypes.byref(j._CResample(0, 0, 45, 37, 7, 5, T)), None),
    }
    assert {k: v for k, v in refused.items() if v != J2P_EINVAL} == {}
    # a band solver: a state error from the C entry point, J2PError from the binding
    planes = make_case(48, 32, "420", 25, seed=11)
    with j.TiledSolver(planes, 0.3, [0.001] * 3, 2, devices=[0, 0]) as tiled:
        tiled.run(2)
        tiled.sync()
        band = tiled.band_solver(0)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(band._h, ch) for ch in range(3)])
        r = j._CResample(0, 0, 48, 16, 7, 5, T)
        assert band._lib.j2p_planes_to_tensor_resampled(refs, 3, 48, 16, ctypes.byref(r), ctypes.byref(ok)) == J2P_ESTATE
        with pytest.raises(j.J2PError):
            band.to_tensor(48, 16, out=t[:, :5, :7], out_width=7, out_height=5, filter="triangle")
    for bad in (lambda: c.s.to_tensor(45, 37, out_width=65537, filter="cubic"),
                lambda: c.s.to_tensor(45, 37, box=(0, 0, 46, 37), filter="cubic"),
                lambda: c.s.to_tensor(45, 37, out_width=46, filter="lanczos"),
                lambda: c.s.to_tensor(45, 37, out_width=46),                                        # the area form still refuses to enlarge
                lambda: c.s.to_tensor(45, 37, out_width=46, filter="area"),
                lambda: c.s.to_tensor(45, 37, out=t, out_width=7, out_height=5, filter="triangle"),  # the shape is the output's
                lambda: c.s.to_tensor(45, 37, dtype=torch.uint8, out_width=7, scale=[2.0, 1.0, 1.0], filter="triangle")):
        with pytest.raises(j.J2PError):
            bad()
    torch.cuda.synchronize()
    assert (bits(t) == fill_bits).all() and (bits(t8) == 201).all()
    # and after all that the call still works, larger than the image
    assert c.resampled(ok, None, 70, 60, T) == 0
    assert not (bits(t) == fill_bits).any()


# ---- 4. the batch engine ----

@pytest.mark.gpu
def test_batch_jobs_of_different_sizes_fill_the_slots_of_one_tensor(torch_cuda, images):
    """four images into the 8 x 8 slots of one tensor under the triangle filter: two larger than the slot, two smaller"""
    import jpeg2png_amd as j
    torch = torch_cuda
    jobs = [("clamping_444", lambda: make_case(48, 40, "444", 3, seed=18), 48, 40), ("padded_420", lambda: make_case(45, 37, "420", 10, seed=5), 45, 37),
            ("small_a", lambda: make_case(7, 5, "444", 10, seed=21), 7, 5), ("small_b", lambda: make_case(4, 6, "444", 10, seed=22), 4, 6)]
    small = {name: Filtered(j, make(), w, h) for name, make, w, h in jobs[2:]}
    fill, fill_bits = sentinel("f16")
    batch = torch.full((4, 3, 8, 8), fill, dtype=torch.float16, device="cuda:0")
    try:
        with j.Batch(devices=[0], slots_per_device=2) as b:
            with pytest.raises(j.J2PError):
                b.submit(jobs[0][1](), 0.3, [0.001] * 3, 2, width=48, height=40, out_width=8, filter="triangle")        # no tensor=
            with pytest.raises(j.J2PError):
                b.submit(jobs[0][1](), 0.3, [0.001] * 3, 2, width=48, height=40, tensor=batch[0], out_width=8, out_height=8, tile=True,
                         tile_min_band_pixels=0, filter="triangle")
            with pytest.raises(j.J2PError):                                                                              # area: no enlarging
                b.submit(jobs[2][1](), 0.3, [0.001] * 3, 2, width=7, height=5, tensor=batch[2], out_width=8, out_height=8)
            torch.cuda.synchronize()
            assert (bits(batch) == fill_bits).all()
            tickets = [b.submit(make(), 0.3, [0.001] * 3, 2, width=w, height=h, tensor=batch[i], scale=SCALE, bias=BIAS, out_width=8,
                                out_height=8, filter="triangle") for i, (_, make, w, h) in enumerate(jobs)]
            for i, ticket in enumerate(tickets):
                assert b.wait(ticket).data_ptr() == batch[i].data_ptr()
        got = bits(batch)
        for i, (name, _, _, _) in enumerate(jobs):
            c = small[name] if name in small else images[name]
            assert np.array_equal(got[i], c.want(None, 8, 8, "triangle", "f16", "chw", SCALE, BIAS)), name
        assert len({got[i].tobytes() for i in range(4)}) == 4
    finally:
        for c in small.values():
            c.close()


@pytest.mark.gpu
def test_submit_resampled_with_null_is_submit_and_needs_a_tensor(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    planes = make_case(45, 37, "420", 10, seed=5)
    out = [torch.full((3, 37, 45), -7.0, dtype=torch.float16, device="cuda:0") for _ in range(2)]
    big = torch.full((3, 50, 61), -7.0, dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    with j.Batch(devices=[0], slots_per_device=1) as b:
        def job_for(t):
            job = j._CJob()
            job.nchannel = 3
            cpl, keep = j._c_planes(planes)
            for ch in range(3):
                job.planes[ch] = cpl[ch]
                job.weight[ch], job.pweight[ch], job.iterations[ch] = 0.3, 0.001, 2
            job.out_w, job.out_h = 45, 37
            if t is not None:
                job.out_tensor = c_tensor(j, t, "chw", "f16")
            return job, keep

        ticket = ctypes.c_int(-1)
        job, keep = job_for(out[0])
        assert b._lib.j2p_batch_submit(b._h, ctypes.byref(job), ctypes.byref(ticket)) == 0
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        job, keep2 = job_for(out[1])
        assert b._lib.j2p_batch_submit_resampled(b._h, ctypes.byref(job), None, ctypes.byref(ticket)) == 0
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        assert np.array_equal(bits(out[0]), bits(out[1]))
        # a resample without tensor output, and bad resamples: refused at submit
        r = j._CResample(0, 0, 45, 37, 61, 50, fc.CUBIC)
        host = np.zeros((3, 37, 45), np.float32)
        job, keep3 = job_for(None)
        for c in range(3):
            job.out_planes[c] = host[c].ctypes.data
        assert b._lib.j2p_batch_submit_resampled(b._h, ctypes.byref(job), ctypes.byref(r), ctypes.byref(ticket)) == J2P_EINVAL
        job, keep4 = job_for(big)
        for bad in (j._CResample(0, 0, 46, 37, 7, 5, 1), j._CResample(0, 0, 45, 37, 65537, 5, 1), j._CResample(0, 0, 45, 37, 0, 5, 1),
                    j._CResample(0, 0, 45, 37, 7, 5, 0), j._CResample(0, 0, 45, 37, 7, 5, 3)):
            assert b._lib.j2p_batch_submit_resampled(b._h, ctypes.byref(job), ctypes.byref(bad), ctypes.byref(ticket)) == J2P_EINVAL
        job.tile = 1
        assert b._lib.j2p_batch_submit_resampled(b._h, ctypes.byref(job), ctypes.byref(r), ctypes.byref(ticket)) == J2P_EINVAL
        torch.cuda.synchronize()
        assert (bits(big) == 0xc700).all()
        # and a good one: the cubic, larger than the image
        job.tile = 0
        assert b._lib.j2p_batch_submit_resampled(b._h, ctypes.byref(job), ctypes.byref(r), ctypes.byref(ticket)) == 0
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0
    assert np.array_equal(bits(out[0]), bits(out[1])) and not host.any()
    assert np.array_equal(bits(big), images["padded_420"].want(None, 61, 50, "cubic", "f16", "chw"))


# ---- 5. stream order ----

@pytest.mark.gpu
def test_torch_work_queued_behind_a_filtered_to_tensor_sees_the_finished_tensor(torch_cuda, images):
    torch = torch_cuda
    c = images["wide"]
    want = c.want(None, 65, 30, "triangle", "f32", "chw", SCALE, BIAS)
    t = c.s.to_tensor(c.w, c.h, scale=SCALE, bias=BIAS, out_width=65, out_height=30, filter="triangle")
    copy = t.clone()                                    # no synchronisation in between
    assert np.array_equal(bits(copy), want)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((3, 30, 65), -7.0, device="cuda:0")         # the fill is queued on the side stream, the kernels behind it
        t = c.s.to_tensor(c.w, c.h, scale=SCALE, bias=BIAS, out=out, out_width=65, out_height=30, filter="triangle")
        copy = t.clone()
    side.synchronize()
    assert np.array_equal(bits(copy), want)
