"""Multi-output tensor resampling on the GPU (j2p_planes_to_tensors_resampled, j2p_batch_submit_outputs, Solver.to_tensors and
the outputs= keyword of Batch.submit).  The call defines no arithmetic of its own: the truth of every output is the single call
Solver.to_tensor(filter=...) on the same solver, compared as raw bits with tolerance zero — and, since that costs little on
images this small, also the restatement of the header's definition (tests/filter_cases.py).  Destinations are windows of larger
tensors pre-filled with a sentinel, and every byte outside the windows is checked (the helpers of tests/test_resize_gpu.py).
Solves are 2 iterations, shared by a module fixture and left unchanged."""
import ctypes

import numpy as np
import pytest

import filter_cases as fc
import outputs_cases as oc
from conftest import make_case
from test_resize_gpu import BIAS, SCALE, Image, bits, c_tensor, check_window, sentinel, torch_dtype, window

J2P_EINVAL, J2P_ESTATE = -1, -4


class Solved(Image):
    """test_resize_gpu's solved image with the single filtered call, the definition, and the C entry point of the list"""

    def norm(self, dtype):
        return {} if dtype == "u8" else {"scale": SCALE[:self.n], "bias": BIAS[:self.n]}

    def item(self, o, **more):
        """the dict of Solver.to_tensors / Batch.submit of an output of outputs_cases"""
        box, ow, oh, name, dtype, layout = o
        return {"out_width": ow, "out_height": oh, "filter": name, "layout": layout, **({} if box is None else {"box": box}), **self.norm(dtype), **more}

    def single(self, o):
        """the bits the single call gives for that output, in a tensor of its own"""
        box, ow, oh, name, dtype, layout = o
        return bits(self.s.to_tensor(self.w, self.h, dtype=torch_dtype(dtype), **self.item(o)))

    def want(self, o):
        box, ow, oh, name, dtype, layout = o
        return fc.expected(self.planes, self.w, self.h, self.box(box), ow, oh, fc.FILTERS[name], dtype, layout, **self.norm(dtype))

    def c_output(self, o, t, **tensor_kw):
        box, ow, oh, name, dtype, layout = o
        norm = self.norm(dtype)
        pad = lambda v, d: tuple(v) + (d,) * (3 - len(v))      # noqa: E731
        kw = {"scale": pad(norm["scale"], 1), "bias": pad(norm["bias"], 0)} if norm else {}
        return self.j._COutput(self.j._CResample(*self.box(box), ow, oh, fc.FILTERS[name]), c_tensor(self.j, t, layout, dtype, **{**kw, **tensor_kw}))

    def call(self, items, n=None, refs=None):
        """the C entry point; synchronises afterwards"""
        arr = (self.j._COutput * max(len(items), 1))(*items)
        rcode = self.lib.j2p_planes_to_tensors_resampled(self.refs if refs is None else refs, self.n, self.w, self.h, len(items) if n is None else n, arr)
        for s in self.solvers:
            s.sync()
        return rcode


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def images(lib):
    import jpeg2png_amd as j
    made = {
        "clamping_444": Solved(j, make_case(48, 40, "444", 3, seed=18), 48, 40),
        "padded_420": Solved(j, make_case(45, 37, "420", 10, seed=5), 45, 37),
        "grey": Solved(j, make_case(45, 37, "420", 25, seed=11, y_only=True), 45, 37),
        "wide": Solved(j, make_case(1040, 24, "420", 10, seed=3), 1040, 24),
    }
    assert all((m.w, m.h) == fc.IMAGES[k] for k, m in made.items()) and made["grey"].n == 1
    yield made
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def truths(torch_cuda, images):
    """per output set: the single call's bits of every output, computed once and left unchanged"""
    return {name: [images[image].single(o) for o in outs] for name, (image, outs) in oc.SETS.items()}


def fill_windows(torch, c, outs):
    made = [window(torch, c.n, o[1], o[2], o[4], o[5]) for o in outs]
    return made, [c.item(o, out=win) for o, (_, win, _) in zip(outs, made)]


# ---- 1. one output is the single call ----

@pytest.mark.gpu
def test_one_output_is_the_single_call(torch_cuda, images):
    torch = torch_cuda
    for image, o in (("padded_420", oc.K3[0]), ("grey", oc.K16[8]), ("wide", oc.WIDE[1]), ("clamping_444", oc.MIXED[1])):
        c = images[image]
        want = c.single(o)
        got = c.s.to_tensors(c.w, c.h, [c.item(o, dtype=torch_dtype(o[4]))])
        assert len(got) == 1 and got[0].dtype == torch_dtype(o[4]) and np.array_equal(bits(got[0]), want), (image, o)
        buf, win, idx = window(torch, c.n, o[1], o[2], o[4], o[5])
        torch.cuda.synchronize()
        assert c.call([c.c_output(o, win)]) == 0
        check_window(buf, idx, want, o[4], (image, o))


# ---- 2 to 5. the output sets: three outputs and their reversal, sixteen on the tiles' edges, very unequal grids, every dtype ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(oc.SETS))
def test_every_output_of_a_call_is_its_single_call(torch_cuda, images, truths, name):
    torch = torch_cuda
    image, outs = oc.SETS[name]
    c = images[image]
    made, items = fill_windows(torch, c, outs)
    got = c.s.to_tensors(c.w, c.h, items)
    assert len(got) == len(outs) and all(g is win for g, (_, win, _) in zip(got, made))
    for i, (o, (buf, win, idx)) in enumerate(zip(outs, made)):
        raw = win.cpu().contiguous().view(torch.uint8)                              # the raw bits, byte for byte
        assert torch.equal(raw, torch.from_numpy(np.ascontiguousarray(truths[name][i]).view(np.uint8)).reshape(raw.shape)), (name, i, o)
        check_window(buf, idx, truths[name][i], o[4], (name, i, o))                # ... and nothing outside the window
        assert np.array_equal(truths[name][i], c.want(o)), (name, i, o)             # the single call is the definition
    if name == "k3":
        assert c.box(outs[0][0])[2] > outs[0][1] and outs[1][0][2] < outs[1][1] and outs[2][0][2:] == outs[2][1:3]   # shrinks, enlarges, identity
    # allocated by the call: shapes, dtypes and bits
    got = c.s.to_tensors(c.w, c.h, [c.item(o, dtype=torch_dtype(o[4])) for o in outs])
    for i, (o, t) in enumerate(zip(outs, got)):
        assert tuple(t.shape) == ((c.n, o[2], o[1]) if o[5] == "chw" else (o[2], o[1], c.n)) and t.is_contiguous()
        assert np.array_equal(bits(t), truths[name][i]), (name, i, o)


# ---- 6. strided destinations ----

@pytest.mark.gpu
def test_slots_of_a_padded_batch_tensor_and_of_a_transposed_view(torch_cuda, images):
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f16")
    batch = torch.full((3, 3, 12, 16), fill, dtype=torch.float16, device="cuda:0")
    store = torch.full((2, 3, 21, 19), fill, dtype=torch.float16, device="cuda:0")
    view = store.transpose(2, 3)                       # (2, 3, 19, 21): x steps over whole rows of the store
    outs = [(None, 8, 8, "triangle", "f16", "chw"), (oc.BOX, 8, 8, "cubic", "f16", "chw"), ((5, 3, 16, 16), 8, 8, "cubic", "f16", "chw"),
            (None, 21, 19, "cubic", "f16", "chw"), (oc.BOX, 20, 17, "triangle", "f16", "chw")]
    dest = [batch[0, :, 2:10, 4:12], batch[2, :, 2:10, 4:12], batch[1, :, 4:12, 8:16], view[1], view[0, :, 1:18, 1:21]]
    assert view.stride(3) == 19
    single = [c.single(o) for o in outs]
    c.s.to_tensors(c.w, c.h, [c.item(o, out=d) for o, d in zip(outs, dest)])
    want = np.full((3, 3, 12, 16), fill_bits, np.uint16)
    want[0, :, 2:10, 4:12], want[2, :, 2:10, 4:12], want[1, :, 4:12, 8:16] = single[0], single[1], single[2]
    assert np.array_equal(bits(batch), want)
    want = np.full((2, 3, 19, 21), fill_bits, np.uint16)
    want[1] = single[3]
    want[0, :, 1:18, 1:21] = single[4]
    assert np.array_equal(bits(store), want.transpose(0, 1, 3, 2))


# ---- 7. refusals ----

@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = images["padded_420"]
    fill, fill_bits = sentinel("f32")
    good = [(None, 7, 5, "cubic", "f32", "chw"), (oc.BOX, 64, 33, "triangle", "f32", "chw")]
    ts = [torch.full((3, o[2], o[1]), fill, dtype=torch.float32, device="cuda:0") for o in good]
    last = torch.full((3, 5, 7), fill, dtype=torch.float32, device="cuda:0")
    t8 = torch.full((3, 5, 7), 201, dtype=torch.uint8, device="cuda:0")
    host = np.full((3, 5, 7), fill, np.float32)
    torch.cuda.synchronize()
    items = [c.c_output(o, t) for o, t in zip(good, ts)]
    o7 = (None, 7, 5, "triangle", "f32", "chw")
    bad_last = {
        "an empty box": c.c_output(((0, 0, 0, 5), 7, 5, "triangle", "f32", "chw"), last),
        "a box that leaves the image": c.c_output(((40, 0, 6, 5), 7, 5, "triangle", "f32", "chw"), last),
        "a host pointer": c.c_output(o7, last, data=host.ctypes.data),
        "NULL data": c.c_output(o7, last, data=0),
        "u8 with a scale": c.c_output((None, 7, 5, "triangle", "u8", "chw"), t8, scale=(1, 2, 1)),
        "a stride of 0": c.c_output(o7, last, strides=(35, 0, 1)),
        "an unknown dtype": j._COutput(j._CResample(0, 0, 45, 37, 7, 5, 1), c_tensor(j, last, "chw", 4)),
    }
    for code in (0, 3, -1):                             # the area form's code and unknown ones
        bad_last[f"filter {code}"] = j._COutput(j._CResample(0, 0, 45, 37, 7, 5, code), c_tensor(j, last, "chw", "f32"))
    refused = {what: c.call(items + [bad]) for what, bad in bad_last.items()}
    refused["no output"] = c.call(items, n=0)
    refused["17 outputs"] = c.call(items * 9, n=17)
    refused["NULL outputs"] = c.lib.j2p_planes_to_tensors_resampled(c.refs, 3, 45, 37, 2, None)
    assert {k: v for k, v in refused.items() if v != J2P_EINVAL} == {}
    planes = make_case(48, 32, "420", 25, seed=11)
    with j.TiledSolver(planes, 0.3, [0.001] * 3, 2, devices=[0, 0]) as tiled:
        tiled.run(2)
        tiled.sync()
        band = tiled.band_solver(0)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(band._h, ch) for ch in range(3)])
        arr = (j._COutput * 2)(*[j._COutput(j._CResample(0, 0, 48, 16, o[1], o[2], 1), c_tensor(j, t, "chw", "f32")) for o, t in zip(good, ts)])
        assert band._lib.j2p_planes_to_tensors_resampled(refs, 3, 48, 16, 2, arr) == J2P_ESTATE
        with pytest.raises(j.J2PError):
            band.to_tensors(48, 16, [{"out_width": 7, "out_height": 5, "filter": "triangle"}] * 2)
    for bad in (lambda: c.s.to_tensors(45, 37, [c.item(good[0]), c.item(good[1], out=ts[0])]),          # the shape is the output's
                lambda: c.s.to_tensors(45, 37, [c.item(good[0], out=ts[0]), c.item(good[1], out=ts[1], dtype=torch.float16)]),
                lambda: c.s.to_tensors(45, 37, [c.item(good[0], out=ts[0]), {"out_width": 7, "filter": "triangle", "dtype": torch.uint8, "scale": 2.0}])):
        with pytest.raises(j.J2PError):
            bad()
    torch.cuda.synchronize()
    assert all((bits(t) == fill_bits).all() for t in ts + [last]) and (bits(t8) == 201).all() and (host == fill).all()
    # and after all that the call still works
    assert c.call(items) == 0
    assert all(np.array_equal(bits(t), c.single(o)) for o, t in zip(good, ts))


# ---- 8. the scratch is shared by the outputs of a call and reused by the next ----

@pytest.mark.gpu
def test_calls_of_different_sizes_reuse_the_scratch(torch_cuda, images, truths):
    """a large call, a small one, the large one again — queued back to back on one stream, each reading taps where the call
    before it had other outputs' — and a single call in between, whose taps start where the list's first output's do"""
    torch = torch_cuda
    c = images["wide"]
    large, small = oc.WIDE, oc.WIDE[2:4][::-1]
    first = c.s.to_tensors(c.w, c.h, [c.item(o) for o in large])
    little = c.s.to_tensors(c.w, c.h, [c.item(o) for o in small])
    alone = c.s.to_tensor(c.w, c.h, **c.item(large[0]))
    again = c.s.to_tensors(c.w, c.h, [c.item(o) for o in large])
    for i, o in enumerate(large):
        assert np.array_equal(bits(first[i]), truths["wide"][i]) and np.array_equal(bits(again[i]), truths["wide"][i]), (i, o)
    assert np.array_equal(bits(little[0]), truths["wide"][3]) and np.array_equal(bits(little[1]), truths["wide"][2])
    assert np.array_equal(bits(alone), truths["wide"][0])


# ---- 9. the batch engine ----

BATCH_VIEWS = [(None, 24, 20, "triangle", "f16", "chw"), (oc.BOX, 64, 33, "cubic", "f16", "chw"), (oc.BOX, 20, 17, "triangle", "f32", "hwc"),
               ((5, 3, 16, 16), 8, 8, "cubic", "u8", "chw"), (None, 7, 5, "cubic", "bf16", "chw")]


def empty_like(torch, c, o):
    fill, _ = sentinel(o[4])
    return torch.full((c.n, o[2], o[1]) if o[5] == "chw" else (o[2], o[1], c.n), fill, dtype=torch_dtype(o[4]), device="cuda:0")


@pytest.mark.gpu
def test_a_job_with_five_outputs_equals_five_jobs_with_one(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = images["padded_420"]
    planes = make_case(45, 37, "420", 10, seed=5)
    multi = [empty_like(torch, c, o) for o in BATCH_VIEWS]
    ones = [empty_like(torch, c, o) for o in BATCH_VIEWS]
    host = None
    with j.Batch(devices=[0], slots_per_device=2) as b:
        t = b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=37, outputs=[c.item(o, tensor=m) for o, m in zip(BATCH_VIEWS, multi)])
        tickets = [b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=37, tensor=one, **c.item(o)) for o, one in zip(BATCH_VIEWS, ones)]
        got = b.wait(t)
        assert isinstance(got, list) and [g.data_ptr() for g in got] == [m.data_ptr() for m in multi]
        for ticket in tickets:
            b.wait(ticket)
        host = b.wait(b.submit(planes, 0.3, [0.001] * 3, 2))
    for o, m, one in zip(BATCH_VIEWS, multi, ones):
        assert np.array_equal(bits(m), bits(one)) and np.array_equal(bits(m), c.single(o)), o
    assert all(np.array_equal(host[ch], c.planes[ch]) for ch in range(3))              # (the batch's solve is the fixture's)


@pytest.mark.gpu
def test_jobs_of_different_images_in_flight_fill_the_right_tensors(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    jobs = [("padded_420", lambda: make_case(45, 37, "420", 10, seed=5), BATCH_VIEWS), ("clamping_444", lambda: make_case(48, 40, "444", 3, seed=18), oc.MIXED),
            ("grey", lambda: make_case(45, 37, "420", 25, seed=11, y_only=True), oc.K16), ("clamping_444", lambda: make_case(48, 40, "444", 3, seed=18), oc.MIXED[1:2]),
            ("padded_420", lambda: make_case(45, 37, "420", 10, seed=5), oc.K3)]
    dest = [[empty_like(torch, images[image], o) for o in outs] for image, _, outs in jobs]
    with j.Batch(devices=[0], slots_per_device=3) as b:
        tickets = []
        for (image, make, outs), ts in zip(jobs, dest):
            c, planes = images[image], make()
            if len(outs) == 1:                          # a single-output job of the existing kind among them
                tickets.append(b.submit(planes, 0.3, [0.001] * c.n, 2, width=c.w, height=c.h, tensor=ts[0], **c.item(outs[0])))
            else:
                tickets.append(b.submit(planes, 0.3, [0.001] * c.n, 2, width=c.w, height=c.h, outputs=[c.item(o, tensor=t) for o, t in zip(outs, ts)]))
        for ticket in tickets[::-1]:
            b.wait(ticket)
    for (image, _, outs), ts in zip(jobs, dest):
        for o, t in zip(outs, ts):
            assert np.array_equal(bits(t), images[image].single(o)), (image, o)


@pytest.mark.gpu
def test_submit_outputs_refusals_and_none_is_submit(torch_cuda, images):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = images["padded_420"]
    planes = make_case(45, 37, "420", 10, seed=5)
    outs = BATCH_VIEWS[:2]
    ts = [empty_like(torch, c, o) for o in outs]
    whole = [torch.full((3, 37, 45), -7.0, dtype=torch.float16, device="cuda:0") for _ in range(2)]
    host = np.zeros((3, 5, 7), np.float32)
    torch.cuda.synchronize()
    arr = (j._COutput * 17)(*([c.c_output(o, t) for o, t in zip(outs, ts)] * 8 + [c.c_output(outs[0], ts[0])]))
    with j.Batch(devices=[0], slots_per_device=1) as b:
        def job_for(t=None, tile=0, bits_=0):
            job = j._CJob()
            job.nchannel = 3
            cpl, keep = j._c_planes(planes)
            for ch in range(3):
                job.planes[ch] = cpl[ch]
                job.weight[ch], job.pweight[ch], job.iterations[ch] = 0.3, 0.001, 2
            job.out_w, job.out_h, job.tile, job.out_bits = 45, 37, tile, bits_
            if t is not None:
                job.out_tensor = c_tensor(j, t, "chw", "f16")
            return job, keep

        ticket = ctypes.c_int(-1)
        submit = lambda job, n, a: b._lib.j2p_batch_submit_outputs(b._h, ctypes.byref(job), n, a, ctypes.byref(ticket))    # noqa: E731
        refused = {}
        job, k1 = job_for(whole[0])
        refused["out_tensor set"] = submit(job, 2, arr)
        job, k2 = job_for(tile=1)
        refused["tile set"] = submit(job, 2, arr)
        job, k3 = job_for(bits_=8)
        refused["out_bits set"] = submit(job, 2, arr)
        job, k4 = job_for()
        refused["17 outputs"] = submit(job, 17, arr)
        bad = (j._COutput * 2)(arr[0], c.c_output(((40, 0, 6, 5), 7, 5, "triangle", "f16", "chw"), ts[1]))
        refused["a box outside the job's crop"] = submit(job, 2, bad)
        bad = (j._COutput * 2)(arr[0], j._COutput(j._CResample(0, 0, 45, 37, 7, 5, 0), arr[1].t))
        refused["filter 0"] = submit(job, 2, bad)
        bad = (j._COutput * 2)(arr[0], c.c_output((None, 7, 5, "triangle", "f32", "chw"), ts[1], data=host.ctypes.data))
        refused["a host pointer"] = submit(job, 2, bad)
        assert {k: v for k, v in refused.items() if v != J2P_EINVAL} == {}
        with pytest.raises(j.J2PError):
            b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=37, outputs=[c.item(outs[0], tensor=ts[0])], tile=True)
        with pytest.raises(j.J2PError):
            b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=37, outputs=[c.item(outs[0], tensor=ts[0])], tensor=ts[1])
        # no outputs: j2p_batch_submit, here of a plain tensor job
        job, k5 = job_for(whole[0])
        assert b._lib.j2p_batch_submit(b._h, ctypes.byref(job), ctypes.byref(ticket)) == 0 and b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        job, k6 = job_for(whole[1])
        assert submit(job, 0, arr) == 0 and b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        job, k7 = job_for(whole[1])
        assert submit(job, 2, None) == 0 and b._lib.j2p_batch_wait(b._h, ticket.value) == 0
        torch.cuda.synchronize()
        assert all((bits(t) == sentinel(o[4])[1]).all() for o, t in zip(outs, ts)) and not host.any()
        # and a good one, whose float planes are still delivered (out_planes is honoured)
        job, k8 = job_for()
        canvas = np.zeros((3, 48, 48), np.float32)
        for ch in range(3):
            job.out_planes[ch] = canvas[ch].ctypes.data
        assert submit(job, 2, arr) == 0 and b._lib.j2p_batch_wait(b._h, ticket.value) == 0
    assert np.array_equal(bits(whole[0]), bits(whole[1])) and not (bits(whole[0]) == 0xc700).all()
    assert all(np.array_equal(bits(t), c.single(o)) for o, t in zip(outs, ts))
    assert all(np.array_equal(canvas[ch], c.planes[ch]) for ch in range(3))


# ---- 10. stream order ----

@pytest.mark.gpu
def test_torch_work_queued_behind_to_tensors_sees_the_finished_tensors(torch_cuda, images, truths):
    torch = torch_cuda
    c = images["wide"]
    outs = oc.WIDE
    ts = c.s.to_tensors(c.w, c.h, [c.item(o) for o in outs])
    copies = [t.clone() for t in ts]                    # no synchronisation in between
    assert all(np.array_equal(bits(cp), truths["wide"][i]) for i, cp in enumerate(copies))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dest = [torch.full((3, o[2], o[1]), -7.0, device="cuda:0") for o in outs]       # the fills are queued on the side stream, the kernels behind them
        ts = c.s.to_tensors(c.w, c.h, [c.item(o, out=d) for o, d in zip(outs, dest)])
        copies = [t.clone() for t in ts]
    side.synchronize()
    assert all(np.array_equal(bits(cp), truths["wide"][i]) for i, cp in enumerate(copies))
