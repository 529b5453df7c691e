"""Resized tensor output on the GPU (j2p_planes_to_tensor_resized, j2p_batch_submit_resized, the out_width / out_height / box
keywords of Solver.to_tensor and Batch.submit).  Every comparison is of BIT PATTERNS, tolerance zero, against the numpy
restatement of the header's definition (tests/resize_cases.py) applied to Solver.download(c) of the same solver.  Every
destination is a window of a larger tensor pre-filled with a sentinel, and every byte outside the window is checked
afterwards.  The kernel stages kResizeChunk = 512 source columns at a time (resize_cases.KERNEL_CHUNK): the rows of the 1040
wide case span three chunks.  Solves are 2 iterations, shared by module fixtures and left unchanged."""
import ctypes

import numpy as np
import pytest

import resize_cases as rc
from conftest import make_case

J2P_EINVAL, J2P_ESTATE = -1, -4
_M, _S = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [float(np.float32(1.0 / (255.0 * s))) for s in _S]
BIAS = [float(np.float32(-m / s)) for m, s in zip(_M, _S)]


def torch_dtype(name):
    import torch
    return {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def bits(t):
    """bit patterns of a torch tensor as numpy unsigned integers"""
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.uint8:
        return t.numpy()
    if t.dtype == torch.float32:
        return t.numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def sentinel(dtype):
    """(fill value, its bit pattern); the float one is negative beyond anything the scales and biases used here give"""
    return (201, 201) if dtype == "u8" else (-7.0, {"f32": 0xc0e00000, "f16": 0xc700, "bf16": 0xc0e0}[dtype])


class Image:
    """one solved image: solvers (one joint, or one per component as `-s`), the downloaded planes, the plane references"""

    def __init__(self, j, planes, w, h, separate=False, its=2):
        self.j, self.n, self.w, self.h = j, len(planes), w, h
        groups = [[p] for p in planes] if separate else [planes]
        self.solvers = [j.Solver(g, 0.3, [0.001] * len(g), its) for g in groups]
        for s in self.solvers:
            s.run(its)
        self.s = self.solvers[0]
        if separate:
            self.planes = [s.download(0) for s in self.solvers]
            self.refs = (j._CPlaneRef * self.n)(*[j._CPlaneRef(s._h, 0) for s in self.solvers])
        else:
            self.planes = [self.s.download(c) for c in range(self.n)]
            self.refs = (j._CPlaneRef * self.n)(*[j._CPlaneRef(self.s._h, c) for c in range(self.n)])
        self.lib = self.s._lib

    def close(self):
        for s in self.solvers:
            s.close()

    def box(self, box):
        return (0, 0, self.w, self.h) if box is None else box

    def expected(self, box, ow, oh, dtype, layout, scale=None, bias=None):
        return rc.expected(self.planes, self.w, self.h, self.box(box), ow, oh, dtype, layout, scale, bias)

    def call(self, ct, box, ow, oh, w=None, h=None, refs=None, nplane=None):
        """the C entry point; synchronises afterwards"""
        r = self.j._CResize(*self.box(box), ow, oh)
        rcode = self.lib.j2p_planes_to_tensor_resized(self.refs if refs is None else refs, self.n if nplane is None else nplane,
                                                      self.w if w is None else w, self.h if h is None else h, ctypes.byref(r), ctypes.byref(ct))
        for s in self.solvers:
            s.sync()
        return rcode


def c_tensor(j, t, layout, dtype, scale=(1, 1, 1), bias=(0, 0, 0), data=None, strides=None):
    sc, sy, sx = strides or (t.stride() if layout == "chw" else (t.stride(2), t.stride(0), t.stride(1)))
    code = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}.get(dtype, dtype)
    return j._CTensor(t.data_ptr() if data is None else data, code, sc, sy, sx, (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias))


def window(torch, n, ow, oh, dtype, layout):
    """(the padded tensor full of the sentinel, the ow x oh window inside it, the window's index)"""
    fill, _ = sentinel(dtype)
    if layout == "chw":
        buf = torch.full((n, oh + 2, ow + 3), fill, dtype=torch_dtype(dtype), device="cuda:0")
        idx = (slice(None), slice(1, 1 + oh), slice(2, 2 + ow))
    else:
        buf = torch.full((oh + 2, ow + 3, n), fill, dtype=torch_dtype(dtype), device="cuda:0")
        idx = (slice(1, 1 + oh), slice(2, 2 + ow), slice(None))
    return buf, buf[idx], idx


def check_window(buf, idx, want, dtype, what):
    got = bits(buf)
    full = np.full(got.shape, sentinel(dtype)[1], got.dtype)
    full[idx] = want
    bad = np.argwhere(got != full)
    assert bad.size == 0, (what, len(bad), "first at", tuple(bad[0]), "got", got[tuple(bad[0])], "want", full[tuple(bad[0])])


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def images(lib):
    import jpeg2png_amd as j
    made = {
        "clamping_444": Image(j, make_case(48, 40, "444", 3, seed=18), 48, 40),
        "padded_420": Image(j, make_case(45, 37, "420", 10, seed=5), 45, 37),
        "padded_420_s": Image(j, make_case(45, 37, "420", 10, seed=5), 45, 37, separate=True),
        "grey": Image(j, make_case(45, 37, "420", 25, seed=11, y_only=True), 45, 37),
        "wide": Image(j, make_case(1040, 24, "420", 10, seed=3), 1040, 24),
        "large_grey": Image(j, make_case(2048, 1040, "420", 10, seed=9, y_only=True), 2048, 1040, its=1),
    }
    assert (made["padded_420"].s.W, made["padded_420"].s.H) == (48, 48) and made["grey"].n == 1
    assert {(k, (m.w, m.h)) for k, m in made.items() if k in rc.IMAGES} == set(rc.IMAGES.items())
    yield made
    for m in made.values():
        m.close()


# ---- 1. the definition, case by case ----

@pytest.mark.gpu
def test_the_clamping_case_clamps_at_both_ends(images):
    c = images["clamping_444"]
    v = np.stack(rc.unclamped(c.planes, c.w, c.h)).astype(np.float64)
    assert (v < 0.).any() and (v > 255.).any() and ((v > 0.) & (v < 255.)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_every_case_is_the_definition(torch_cuda, images, case):
    """f32 CHW (the mean itself, after * 1 + 0) and u8 HWC, through Solver.to_tensor; the 4:2:0 image also from the three
    solvers of `-s`, through the C entry point"""
    import jpeg2png_amd as j
    torch = torch_cuda
    image, box, ow, oh = case
    for name in [image] + (["padded_420_s"] if image == "padded_420" else []):
        c = images[name]
        kw = {} if box is None else {"box": box}
        for dtype, layout in (("f32", "chw"), ("u8", "hwc")):
            buf, win, idx = window(torch, c.n, ow, oh, dtype, layout)
            want = c.expected(box, ow, oh, dtype, layout)
            if name.endswith("_s"):
                torch.cuda.synchronize()
                assert c.call(c_tensor(j, win, layout, dtype), box, ow, oh) == 0
            else:
                assert c.s.to_tensor(c.w, c.h, layout=layout, out=win, out_width=ow, out_height=oh, **kw) is win
            check_window(buf, idx, want, dtype, (name, case, dtype, layout))
    if image == "padded_420":
        assert not np.array_equal(images["padded_420"].planes[1], images["padded_420_s"].planes[1])   # (two different solves)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", ["u8", "f16", "bf16", "f32"])
def test_every_dtype_and_layout(torch_cuda, images, dtype, layout):
    torch = torch_cuda
    kw = {} if dtype == "u8" else {"scale": SCALE, "bias": BIAS}
    for name in ("clamping_444", "padded_420"):
        c = images[name]
        buf, win, idx = window(torch, 3, 7, 5, dtype, layout)
        c.s.to_tensor(c.w, c.h, layout=layout, out=win, out_width=7, out_height=5, **kw)
        want = c.expected(None, 7, 5, dtype, layout, **kw)
        assert len(np.unique(want)) > 16
        check_window(buf, idx, want, dtype, (name, dtype, layout))
    # allocated by the call: the shape is the output's
    t = images["grey"].s.to_tensor(45, 37, dtype=torch_dtype(dtype), layout=layout, out_width=7, out_height=5)
    assert tuple(t.shape) == ((1, 5, 7) if layout == "chw" else (5, 7, 1)) and t.is_contiguous()
    assert np.array_equal(bits(t), images["grey"].expected(None, 7, 5, dtype, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["u8", "f32", "f16"])
def test_a_pure_crop_is_the_slice_of_to_tensor(torch_cuda, images, dtype):
    c = images["padded_420"]
    kw = {} if dtype == "u8" else {"scale": SCALE, "bias": BIAS}
    whole = bits(c.s.to_tensor(c.w, c.h, dtype=torch_dtype(dtype), **kw))
    source = np.stack(rc.clamped(c.planes, c.w, c.h))
    for bx in (1, 2, 3, 5):
        box = (bx, 2, 40, 30)
        t = c.s.to_tensor(c.w, c.h, dtype=torch_dtype(dtype), box=box, **kw)             # no out_*: the box's size
        assert tuple(t.shape) == (3, 30, 40)
        want = whole[:, 2:32, bx:bx + 40]
        same = bits(t) == want
        if dtype != "u8":
            same |= source[:, 2:32, bx:bx + 40].view(np.uint32) == 0x80000000                # identical wherever the source is not -0
        assert same.all(), (dtype, bx)


# ---- 2. strided destinations ----

@pytest.mark.gpu
def test_a_padded_slot_of_a_batch_tensor_and_a_transposed_view(torch_cuda, images):
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f16")
    batch = torch.full((2, 3, 12, 16), fill, dtype=torch.float16, device="cuda:0")
    slot = batch[1, :, 2:10, 4:12]
    c.s.to_tensor(c.w, c.h, out=slot, out_width=8, out_height=8, scale=SCALE, bias=BIAS)
    want = np.full((2, 3, 12, 16), fill_bits, np.uint16)
    want[1, :, 2:10, 4:12] = c.expected(None, 8, 8, "f16", "chw", SCALE, BIAS)
    assert np.array_equal(bits(batch), want)
    # transposed: x steps over whole columns
    store = torch.full((3, 7, 5), fill, dtype=torch.float32, device="cuda:0")
    view = store.transpose(1, 2)
    assert tuple(view.shape) == (3, 5, 7) and view.stride(2) == 5
    c.s.to_tensor(c.w, c.h, out=view, out_width=7, out_height=5)
    assert np.array_equal(bits(store), c.expected(None, 7, 5, "f32", "chw").transpose(0, 2, 1))


@pytest.mark.gpu
def test_two_calls_with_different_boxes_into_one_tensor(torch_cuda, images):
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f32")
    t = torch.full((3, 6, 20), fill, dtype=torch.float32, device="cuda:0")
    boxes = ((0, 0, 22, 37), (23, 5, 22, 30))
    for i, box in enumerate(boxes):
        c.s.to_tensor(c.w, c.h, out=t[:, :5, 10 * i:10 * i + 7], box=box, out_width=7, out_height=5)
    want = np.full((3, 6, 20), fill_bits, np.uint32)
    for i, box in enumerate(boxes):
        want[:, :5, 10 * i:10 * i + 7] = c.expected(box, 7, 5, "f32", "chw")
    assert np.array_equal(bits(t), want)
    assert not np.array_equal(want[:, :5, 0:7], want[:, :5, 10:17])


# ---- 3. refusals ----

@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f32")
    t = torch.full((3, 37, 45), fill, dtype=torch.float32, device="cuda:0")
    t8 = torch.full((3, 37, 45), 201, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ok = c_tensor(j, t, "chw", "f32")
    refused = {
        "empty box": c.call(ok, (0, 0, 0, 5), 1, 1),
        "empty box rows": c.call(ok, (0, 0, 5, 0), 1, 1),
        "box leaves the image right": c.call(ok, (40, 0, 6, 5), 3, 3),
        "box leaves the image below": c.call(ok, (0, 30, 5, 8), 3, 3),
        "box inside the canvas, outside the image": c.call(ok, (0, 0, 48, 37), 8, 8),
        "box_x beyond": c.call(ok, (45, 0, 1, 1), 1, 1),
        "box wraps around": c.call(ok, (2, 0, 0xffffffff, 5), 3, 3),
        "out_w 0": c.call(ok, None, 0, 5),
        "out_h 0": c.call(ok, None, 7, 0),
        "out_w > box_w": c.call(ok, (0, 0, 20, 20), 21, 5),
        "out_h > box_h": c.call(ok, (0, 0, 20, 20), 5, 21),
        "image beyond the canvas": c.call(ok, (0, 0, 49, 37), 7, 5, w=49),
        "two planes": c.call(ok, None, 7, 5, nplane=2),
        "u8 with a scale": c.call(c_tensor(j, t8, "chw", "u8", scale=(1, 2, 1)), None, 7, 5),
        "unknown dtype": c.call(c_tensor(j, t, "chw", 4), None, 7, 5),
        "stride 0": c.call(c_tensor(j, t, "chw", "f32", strides=(37 * 45, 0, 1)), None, 7, 5),
        "NULL data": c.call(c_tensor(j, t, "chw", "f32", data=0), None, 7, 5),
        "misaligned": c.call(c_tensor(j, t, "chw", "f32", data=t.data_ptr() + 2), None, 7, 5),
        "NULL resize": c.lib.j2p_planes_to_tensor_resized(c.refs, 3, 45, 37, None, ctypes.byref(ok)),
        "NULL tensor": c.lib.j2p_planes_to_tensor_resized(c.refs, 3, 45, 37, ctypes.byref(j._CResize(0, 0, 45, 37, 7, 5)), None),
    }
    assert {k: v for k, v in refused.items() if v != J2P_EINVAL} == {}
    # a band solver: a state error from the C entry point, J2PError from the binding
    planes = make_case(48, 32, "420", 25, seed=11)
    with j.TiledSolver(planes, 0.3, [0.001] * 3, 2, devices=[0, 0]) as tiled:
        tiled.run(2)
        tiled.sync()
        band = tiled.band_solver(0)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(band._h, ch) for ch in range(3)])
        r = j._CResize(0, 0, 48, 16, 7, 5)
        assert band._lib.j2p_planes_to_tensor_resized(refs, 3, 48, 16, ctypes.byref(r), ctypes.byref(ok)) == J2P_ESTATE
        with pytest.raises(j.J2PError):
            band.to_tensor(48, 16, out=t[:, :5, :7], out_width=7, out_height=5)
    for bad in (lambda: c.s.to_tensor(45, 37, out_width=46),
                lambda: c.s.to_tensor(45, 37, box=(0, 0, 46, 37)),
                lambda: c.s.to_tensor(45, 37, out=t, out_width=7, out_height=5),                  # the shape is the output's
                lambda: c.s.to_tensor(45, 37, dtype=torch.uint8, out_width=7, scale=[2.0, 1.0, 1.0])):
        with pytest.raises(j.J2PError):
            bad()
    torch.cuda.synchronize()
    assert (bits(t) == fill_bits).all() and (bits(t8) == 201).all()
    # and after all that the call still works
    assert c.call(ok, None, 45, 37) == 0
    assert not (bits(t) == fill_bits).any()


# ---- 4. the batch engine ----

@pytest.mark.gpu
def test_batch_jobs_of_different_sizes_fill_the_slots_of_one_tensor(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    jobs = [("clamping_444", make_case(48, 40, "444", 3, seed=18), False), ("padded_420", make_case(45, 37, "420", 10, seed=5), False),
            ("padded_420_s", make_case(45, 37, "420", 10, seed=5), True), ("wide", make_case(1040, 24, "420", 10, seed=3), False)]
    fill, fill_bits = sentinel("f16")
    batch = torch.full((4, 3, 8, 8), fill, dtype=torch.float16, device="cuda:0")
    with j.Batch(devices=[0], slots_per_device=2) as b:
        with pytest.raises(j.J2PError):
            b.submit(jobs[0][1], 0.3, [0.001] * 3, 2, width=48, height=40, out_width=8)         # no tensor=
        with pytest.raises(j.J2PError):
            b.submit(jobs[0][1], 0.3, [0.001] * 3, 2, width=48, height=40, tensor=batch[0], out_width=8, out_height=8, tile=True,
                     tile_min_band_pixels=0)
        torch.cuda.synchronize()
        assert (bits(batch) == fill_bits).all()
        tickets = [b.submit(planes, 0.3, [0.001] * 3, 2, separate=sep, width=images[name].w, height=images[name].h, tensor=batch[i],
                            scale=SCALE, bias=BIAS, out_width=8, out_height=8) for i, (name, planes, sep) in enumerate(jobs)]
        for i, ticket in enumerate(tickets):
            assert b.wait(ticket).data_ptr() == batch[i].data_ptr()
    got = bits(batch)
    for i, (name, _, _) in enumerate(jobs):
        assert np.array_equal(got[i], images[name].expected(None, 8, 8, "f16", "chw", SCALE, BIAS)), name
    assert len({got[i].tobytes() for i in range(4)}) == 4


@pytest.mark.gpu
def test_submit_resized_with_null_is_submit_and_needs_a_tensor(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    planes = make_case(45, 37, "420", 10, seed=5)
    out = [torch.full((3, 37, 45), -7.0, dtype=torch.float16, device="cuda:0") for _ in range(2)]
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
        assert b._lib.j2p_batch_submit_resized(b._h, ctypes.byref(job), None, ctypes.byref(ticket)) == 0
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        assert np.array_equal(bits(out[0]), bits(out[1]))
        assert np.array_equal(bits(out[0]), rc.elements(rc.clamped(images["padded_420"].planes, 45, 37), "f16", "chw"))
        # a resize without tensor output, and a bad resize: refused at submit
        r = j._CResize(0, 0, 45, 37, 7, 5)
        host = np.zeros((3, 37, 45), np.float32)
        job, keep3 = job_for(None)
        for c in range(3):
            job.out_planes[c] = host[c].ctypes.data
        assert b._lib.j2p_batch_submit_resized(b._h, ctypes.byref(job), ctypes.byref(r), ctypes.byref(ticket)) == J2P_EINVAL
        job, keep4 = job_for(out[1])
        for bad in (j._CResize(0, 0, 46, 37, 7, 5), j._CResize(0, 0, 45, 37, 46, 5), j._CResize(0, 0, 45, 37, 0, 5)):
            assert b._lib.j2p_batch_submit_resized(b._h, ctypes.byref(job), ctypes.byref(bad), ctypes.byref(ticket)) == J2P_EINVAL
        job.tile = 1
        assert b._lib.j2p_batch_submit_resized(b._h, ctypes.byref(job), ctypes.byref(r), ctypes.byref(ticket)) == J2P_EINVAL
    assert np.array_equal(bits(out[0]), bits(out[1])) and not host.any()


# ---- 5. stream order ----

@pytest.mark.gpu
def test_torch_work_queued_behind_a_resized_to_tensor_sees_the_finished_tensor(torch_cuda, images):
    torch = torch_cuda
    c = images["wide"]
    want = c.expected(None, 65, 5, "f32", "chw", SCALE, BIAS)
    t = c.s.to_tensor(c.w, c.h, scale=SCALE, bias=BIAS, out_width=65, out_height=5)
    copy = t.clone()                                    # no synchronisation in between
    assert np.array_equal(bits(copy), want)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((3, 5, 65), -7.0, device="cuda:0")         # the fill is queued on the side stream, the kernel behind it
        t = c.s.to_tensor(c.w, c.h, scale=SCALE, bias=BIAS, out=out, out_width=65, out_height=5)
        copy = t.clone()
    side.synchronize()
    assert np.array_equal(bits(copy), want)
