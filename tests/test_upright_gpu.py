"""Upright output on the GPU (k_upright_rows, k_upright_transpose; j2p_solver_set_orientation, Solver.set_orientation,
Solver.from_jpeg(upright=), Batch.submit(orientation=)).  The permutation touches no value, so every comparison is an equality:
a pointwise form of an oriented solver is the restatement's permutation (tests/upright_cases.py) of the same form unoriented; a
resampled form, the coefficients and the files are the project's existing restatements fed the permuted, replicated planes that
upright_cases makes from the solver's downloaded float planes.

Sizes.  The transposing kernel moves tiles of 64 x 64 destination elements through LDS (kUprightTile), the row-wise one 4 rows x
256 columns per workgroup, and both write the upright canvas, the upright image rounded up to 16.  45x38 and 17x9 have partial
8x8 blocks and a partial 16 on both axes, 1x1 is all replication, and 129x70 gives a transposed canvas of 80 x 144: two tiles
across with the second partial, three down with the third partial, and source rows that start at 64 and 128 — while 129 columns
unturned are more than one wavefront's 64 with a ragged end.  One case is zoomed 2x (the source size is the file's times the zoom).
Solves are 2 iterations, shared by a module fixture and left unchanged."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import filter_cases as fc
import resize_cases as rc
import upright_cases as uc
from conftest import make_case
from test_jpeg_out_gpu import _need_ref
from test_jpeg_sub_gpu import expected_sub
from test_tensor_gpu import bits, torch_dtype

J2P_EINVAL, J2P_ESTATE = -1, -4
SCALE, BIAS = [0.5, 0.25, 2.0], [-3.0, 1.5, 0.125]


class Case:
    """one solved image: the solver, its downloaded planes (unoriented: downloads never are) and the image's size"""

    def __init__(self, j, planes, w, h, its=2):
        self.j, self.n, self.w, self.h = j, len(planes), w, h
        self.s = j.Solver(planes, 0.3, [0.001] * self.n, its)
        self.s.run(its)
        self.planes = [self.s.download(c) for c in range(self.n)]
        self.lib = self.s._lib
        self.refs = (j._CPlaneRef * self.n)(*[j._CPlaneRef(self.s._h, c) for c in range(self.n)])
        u, p, ref = ctypes.c_uint, ctypes.c_void_p, ctypes.POINTER(j._CPlaneRef)
        self.lib.j2p_planes_to_rgb.argtypes = self.lib.j2p_planes_to_grey.argtypes = [ref, u, u, u, p]
        self.lib.j2p_planes_rows_to_rgb.argtypes = self.lib.j2p_planes_rows_to_grey.argtypes = [ref, u, u, u, u, p]

    def close(self):
        self.s.close()

    @contextlib.contextmanager
    def oriented(self, o):
        self.s.set_orientation(o, self.w, self.h)
        try:
            yield uc.upright_size(o, self.w, self.h)
        finally:
            self.s.set_orientation(1, self.w, self.h)

    def samples_rc(self, w, h, bits_):
        out = np.zeros(h * w * self.n * (bits_ // 8), np.uint8)
        code = getattr(self.lib, "j2p_planes_to_rgb" if self.n == 3 else "j2p_planes_to_grey")(self.refs, w, h, bits_, out.ctypes.data)
        return code, (out.reshape(h, w, self.n) if bits_ == 8 else out.view(">u2").reshape(h, w, self.n))

    def samples(self, w, h, bits_):
        code, out = self.samples_rc(w, h, bits_)
        assert code == 0, self.lib.j2p_last_error()
        return out

    def upright_planes(self, o):
        """what an output form reads: the permuted, replicated planes — for orientation 1 the canvas itself, solved padding included
        (today's path, which replicates nothing)"""
        return self.planes if o == 1 else uc.upright_planes(self.planes, o, self.w, self.h)


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def cases(lib):
    import jpeg2png_amd as j
    made = {
        "45x38_420": Case(j, make_case(45, 38, "420", 25, seed=7), 45, 38),
        "17x9_444": Case(j, make_case(17, 9, "444", 25, seed=8), 17, 9),
        "1x1_444": Case(j, make_case(1, 1, "444", 25, seed=9), 1, 1),
        "129x70_420": Case(j, make_case(129, 70, "420", 25, seed=10), 129, 70),
        "45x38_420_zoom2": Case(j, j.zoomed(make_case(45, 38, "420", 25, seed=7), 2), 90, 76, its=3),
        "45x38_grey": Case(j, make_case(45, 38, "420", 25, seed=11, y_only=True), 45, 38),
    }
    yield made
    for c in made.values():
        c.close()


def ceil_div(a, b):
    return -(-a // b)


def moved(a, layout):
    """[rows, columns, channels] of a tensor's bits"""
    return np.moveaxis(a, 0, 2) if layout == "chw" else a


# ---- the pointwise forms: samples and tensors, all eight orientations ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x38_420", "17x9_444", "1x1_444", "129x70_420", "45x38_420_zoom2", "45x38_grey"])
def test_samples_and_tensors_are_the_permuted_unoriented_ones(torch_cuda, cases, name):
    c = cases[name]
    plain = {b: c.samples(c.w, c.h, b) for b in (8, 16)}
    plain_t = {(d, lay): bits(c.s.to_tensor(c.w, c.h, dtype=torch_dtype(d), layout=lay, **({} if d == "u8" else {"scale": SCALE[:c.n], "bias": BIAS[:c.n]})))
               for d in ("u8", "f16", "bf16", "f32") for lay in ("chw", "hwc")}
    for o in uc.ORIENTATIONS:
        with c.oriented(o) as (uw, uh):
            assert c.s.orientation == o
            for b in (8, 16):
                assert np.array_equal(c.samples(uw, uh, b), uc.upright(plain[b], o)), (o, b)
            for (d, lay), want in plain_t.items():
                got = bits(c.s.to_tensor(uw, uh, dtype=torch_dtype(d), layout=lay, **({} if d == "u8" else {"scale": SCALE[:c.n], "bias": BIAS[:c.n]})))
                assert np.array_equal(moved(got, lay), uc.upright(moved(want, lay), o)), (o, d, lay)
            # a crop of the upright image from its top left corner is the crop of the permuted image
            if uw > 1 and uh > 1:
                assert np.array_equal(c.samples(uw - 1, uh - 1, 8), uc.upright(plain[8], o)[:uh - 1, :uw - 1]), o
    assert all(np.array_equal(c.s.download(k).view(np.uint32), c.planes[k].view(np.uint32)) for k in range(c.n)), "the planes changed"


# ---- the resampled forms ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x38_420", "129x70_420", "45x38_grey"])
def test_resampled_forms_are_the_restatements_of_the_permuted_planes(torch_cuda, cases, name):
    c = cases[name]
    for o in uc.HEAVY:
        planes = c.upright_planes(o)
        with c.oriented(o) as (uw, uh):
            # boxes that touch the upright image's far edges
            far = (uw // 3, uh // 4, uw - uw // 3, uh - uh // 4)
            for box, ow, oh in ((far, max(1, far[2] // 2), max(1, far[3] // 3)), ((0, 0, uw, uh), max(1, uw // 2), uh)):
                got = bits(c.s.to_tensor(uw, uh, dtype=torch_dtype("f32"), out_width=ow, out_height=oh, box=box))
                assert np.array_equal(got, rc.expected(planes, uw, uh, box, ow, oh, "f32", "chw")), (o, "area", box)
            for filt, dtype, ow, oh in (("triangle", "f32", 24, 20), ("cubic", "f16", uw + 3, max(1, uh // 2))):
                got = bits(c.s.to_tensor(uw, uh, dtype=torch_dtype(dtype), out_width=ow, out_height=oh, box=far, filter=filt))
                assert np.array_equal(got, fc.expected(planes, uw, uh, far, ow, oh, fc.FILTERS[filt], dtype, "chw")), (o, filt)
            # a mixed list from one call
            outs = [{"out_width": 16, "out_height": 12, "filter": "triangle", "dtype": torch_dtype("f32")},
                    {"out_width": 9, "out_height": 11, "filter": "cubic", "box": far, "dtype": torch_dtype("u8"), "layout": "hwc"},
                    {"out_width": uw, "out_height": uh + 2, "filter": "cubic", "dtype": torch_dtype("bf16")}]
            got = c.s.to_tensors(uw, uh, outs)
            for t, spec, dtype in zip(got, outs, ("f32", "u8", "bf16")):
                want = fc.expected(planes, uw, uh, spec.get("box", (0, 0, uw, uh)), spec["out_width"], spec["out_height"], fc.FILTERS[spec["filter"]],
                                   dtype, spec.get("layout", "chw"))
                assert np.array_equal(bits(t), want), (o, spec)


# ---- coefficients, and the files ----

def oriented_coefficients(c, tables, sub, uw, uh):
    """Solver.coefficients of every channel for a JPEG of the upright image"""
    bw, bh = ceil_div(uw, 8), ceil_div(uh, 8)
    out = []
    for k in range(c.n):
        sx, sy = (1, 1) if k == 0 else sub
        out.append(c.s.coefficients(k, tables[k], blocks_w=ceil_div(bw, sx), blocks_h=ceil_div(bh, sy), subsampling=(sx, sy)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x38_420", "17x9_444", "129x70_420"])
def test_coefficients_are_the_restatement_on_the_permuted_replicated_planes(lib, oracle, cases, name):
    """the last blocks (45, 17, 129 and 38, 9, 70 are no multiples of 8) and the overhanging chroma grid read replicated samples: a
    mirror taken about the canvas instead of the image would show there"""
    import jpeg2png_amd as j
    _need_ref(oracle)
    c = cases[name]
    tables = j.quality_tables(90, 3)
    for o in uc.HEAVY:
        planes = c.upright_planes(o)
        with c.oriented(o) as (uw, uh):
            for sub in ((1, 1), (2, 2)):
                got = oriented_coefficients(c, tables, sub, uw, uh)
                for k in range(c.n):
                    sx, sy = (1, 1) if k == 0 else sub
                    bh, bw = got[k].shape[:2]
                    assert (bw, bh) == (ceil_div(ceil_div(uw, 8), sx), ceil_div(ceil_div(uh, 8), sy))
                    want = expected_sub(oracle, planes[k], tables[k], (sx, sy), bw, bh)
                    assert np.array_equal(got[k], want), f"orientation {o}, channel {k}, sampling {sub}: {int((got[k] != want).sum())} coefficients differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x38_420", "129x70_420", "45x38_grey"])
def test_files_are_the_coders_of_the_oriented_coefficients_and_samples(lib, cases, name):
    import jpeg2png_amd as j
    c = cases[name]
    tables = j.quality_tables(85, c.n)
    for o in uc.HEAVY:
        with c.oriented(o) as (uw, uh):
            for sub in ((1, 1), (2, 2)) if c.n == 3 else ((1, 1),):
                coef = oriented_coefficients(c, tables, sub, uw, uh)
                for optimize in (False, True):
                    got = c.s.to_jpeg(uw, uh, quality=85, subsampling=sub, optimize=optimize)
                    assert got == j.entropy_encode(coef, uw, uh, tables, sub, optimize=optimize), (o, sub, optimize)
            for b in (8, 16):
                samples = c.samples(uw, uh, b)
                samples = samples[:, :, 0] if c.n == 1 else samples
                assert c.s.to_png(uw, uh, bits=b) == j.png_encode(samples.astype(np.uint8 if b == 8 else np.uint16), bits=b), (o, b)


# ---- identity and steady state ----

@pytest.mark.gpu
def test_orientation_1_is_never_having_set_it(lib):
    import jpeg2png_amd as j
    with j.Solver(make_case(45, 38, "420", 25, seed=7), 0.3, [0.001] * 3, 2) as s:
        s.run(2)
        assert s.orientation == 1 and s.upright_bytes() == 0
        never = (s.to_png(45, 38), s.to_jpeg(45, 38, quality=90, subsampling=(2, 2)), s.coefficients(0, np.full(64, 3, np.uint16)))
        s.set_orientation(1, 45, 38)
        one = (s.to_png(45, 38), s.to_jpeg(45, 38, quality=90, subsampling=(2, 2)), s.coefficients(0, np.full(64, 3, np.uint16)))
        assert never[0] == one[0] and never[1] == one[1] and np.array_equal(never[2], one[2])
        assert s.upright_bytes() == 0, "an unoriented call allocated upright planes"
        s.set_orientation(6, 45, 38)
        turned = s.to_png(38, 45)
        assert turned != never[0] and s.upright_bytes() > 0
        s.set_orientation(1, 45, 38)
        assert s.to_png(45, 38) == never[0] and s.to_jpeg(45, 38, quality=90, subsampling=(2, 2)) == never[1]


@pytest.mark.gpu
def test_a_second_oriented_call_allocates_nothing(torch_cuda, cases):
    c = cases["129x70_420"]
    with c.oriented(7) as (uw, uh):
        first = (c.s.to_png(uw, uh), bits(c.s.to_tensor(uw, uh, out_width=40, out_height=30, filter="cubic")), c.s.to_jpeg(uw, uh, quality=80))
        sizes = (c.s.upright_bytes(), c.s.output_scratch_bytes())
        assert sizes[0] >= 3 * 80 * 144 * 4 and sizes[1] > 0
        again = (c.s.to_png(uw, uh), bits(c.s.to_tensor(uw, uh, out_width=40, out_height=30, filter="cubic")), c.s.to_jpeg(uw, uh, quality=80))
        assert (c.s.upright_bytes(), c.s.output_scratch_bytes()) == sizes
        assert first[0] == again[0] and np.array_equal(first[1], again[1]) and first[2] == again[2]


# ---- separate solvers ----

@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(45, 38), (17, 9)])
def test_separate_solvers_oriented_alike_and_not(lib, cases, w, h):
    """three solvers of one channel each (`-s`).  At 17x9 4:2:0 their canvases differ in width — 24 columns for Y, 32 for Cb and Cr —
    so every plane is permuted with its own source stride; at 45x38 all three are 48 wide."""
    import jpeg2png_amd as j
    clib = cases["45x38_420"].lib           # (with the sample forms' argtypes set)
    planes = make_case(w, h, "420", 25, seed=7)
    solvers = [j.Solver([p], 0.3, [0.001], 2) for p in planes]
    try:
        assert (solvers[0].W != solvers[1].W) == ((w, h) == (17, 9)), [s.W for s in solvers]
        for s in solvers:
            s.run(2)
        down = [s.download(0) for s in solvers]
        tables = j.quality_tables(90, 3)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, 0) for s in solvers])
        for o in uc.HEAVY:
            uw, uh = uc.upright_size(o, w, h)
            for s in solvers:
                s.set_orientation(o, w, h)
            # each solver's own coefficients (a call of one plane), then the file of all three from one call
            coef = [s.coefficients(0, tables[k], blocks_w=ceil_div(ceil_div(uw, 8), 2 if k else 1), blocks_h=ceil_div(ceil_div(uh, 8), 2 if k else 1),
                                   subsampling=(2, 2) if k else (1, 1)) for k, s in enumerate(solvers)]
            for optimize in (False, True):
                got = solvers[0].to_jpeg(uw, uh, quality=90, subsampling=(2, 2), others=solvers[1:], optimize=optimize)
                assert got == j.entropy_encode(coef, uw, uh, tables, (2, 2), optimize=optimize), (o, optimize)
            for b in (8, 16):
                out = np.zeros(uh * uw * 3 * (b // 8), np.uint8)
                assert clib.j2p_planes_to_rgb(refs, uw, uh, b, out.ctypes.data) == 0
                out = out.reshape(uh, uw, 3) if b == 8 else out.view(">u2").reshape(uh, uw, 3)
                # the restatement of the sample form on the three permuted planes (tests/test_tensor_gpu.py: clamped, then
                # the truncation of x * 2^(bits - 8))
                want = np.stack([(v * np.float32(1 << (b - 8))).astype(np.uint32) for v in rc.clamped(uc.upright_planes(down, o, w, h), uw, uh)], axis=2)
                assert np.array_equal(out.astype(np.uint32), want), (o, b)
                assert solvers[0].to_png(uw, uh, bits=b, others=solvers[1:]) == j.png_encode(out.astype(np.uint8 if b == 8 else np.uint16), bits=b), (o, b)
        # one of them oriented differently, or for another source size, or not at all
        for odd in ((3, w, h), (6, w - 1, h), (1, w, h)):
            for s in solvers:
                s.set_orientation(6, w, h)
            solvers[1].set_orientation(*odd)
            out = np.zeros((w, h, 3), np.uint8)
            assert clib.j2p_planes_to_rgb(refs, h, w, 8, out.ctypes.data) == J2P_EINVAL, odd
            with pytest.raises(j.J2PError) as e:
                solvers[0].to_jpeg(h, w, quality=90, others=solvers[1:])
            assert e.value.code == J2P_EINVAL
            with pytest.raises(j.J2PError) as e:
                solvers[0].to_png(h, w, others=solvers[1:])
            assert e.value.code == J2P_EINVAL
        for s in solvers:
            s.set_orientation(6, w, h)
        assert clib.j2p_planes_to_rgb(refs, h, w, 8, out.ctypes.data) == 0
    finally:
        for s in solvers:
            s.close()


# ---- refusals ----

@pytest.mark.gpu
def test_refusals_leave_the_solver_usable(torch_cuda, cases):
    import jpeg2png_amd as j
    c = cases["45x38_420"]
    before = c.s.to_png(c.w, c.h)
    for bad in ((0, 45, 38), (9, 45, 38), (6, 49, 38), (6, 45, 49), (6, 0, 38), (6, 45, 0)):
        with pytest.raises(j.J2PError) as e:
            c.s.set_orientation(*bad)
        assert e.value.code == J2P_EINVAL, bad
        assert c.s.orientation == 1
        assert c.s.to_png(c.w, c.h) == before
    with c.oriented(6) as (uw, uh):
        want = c.samples(uw, uh, 8)
        # the upright image is 38 x 45 on a canvas of 48 x 48: extents beyond it are refused as they are for any canvas
        assert c.samples_rc(49, uh, 8)[0] == J2P_EINVAL and c.samples_rc(uw, 49, 8)[0] == J2P_EINVAL
        # the rows forms
        out = np.zeros(uh * uw * 3, np.uint8)
        assert c.lib.j2p_planes_rows_to_rgb(c.refs, uw, 0, uh, 8, out.ctypes.data) == J2P_ESTATE
        ct = j._CTensor(1, 0, 1, 1, 1, (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0))
        assert c.lib.j2p_planes_rows_to_tensor(c.refs, 3, uw, 0, uh, ctypes.byref(ct)) == J2P_ESTATE
        q = np.ones(64, np.uint16)
        room = np.zeros(6 * 6 * 64, np.int16)
        assert c.lib.j2p_planes_rows_to_coefficients_sub(c.refs, 1, 1, 5, 0, 6, q.ctypes.data, room.ctypes.data) == J2P_ESTATE
        assert np.array_equal(c.samples(uw, uh, 8), want)
    assert c.s.to_png(c.w, c.h) == before
    # a band solver takes no orientation but 1
    with j.Solver(make_case(48, 48, "420", 25, seed=2), 0.3, [0.001] * 3, 0, band=(0, 16)) as band:
        band.set_orientation(1, 48, 16)
        with pytest.raises(j.J2PError) as e:
            band.set_orientation(6, 48, 16)
        assert e.value.code == J2P_ESTATE and band.orientation == 1


# ---- the batch engine ----

ITS = 2


def solver_path(j, file, o, make):
    """what a Solver made from `file` and oriented o gives: make(solver, upright width, upright height)"""
    with j.Solver.from_jpeg(file, 0.3, [0.001] * 3, ITS) as s:
        s.set_orientation(o, s.jpeg["width"], s.jpeg["height"])
        s.run(ITS)
        return make(s, *uc.upright_size(o, s.jpeg["width"], s.jpeg["height"]))


@pytest.mark.gpu
def test_batch_file_jobs_follow_the_tag(torch_cuda, lib):
    import jpeg2png_amd as j
    torch = torch_cuda
    tagged = uc.pil_jpeg(45, 38, seed=5, orientation=6)
    assert j.jpeg_orientation(tagged) == 6
    untagged = uc.strip_app_segments(tagged)
    assert j.jpeg_orientation(untagged) == 1
    slot = {"out_width": 224, "out_height": 189, "filter": "triangle"}
    want_png = solver_path(j, tagged, 6, lambda s, w, h: s.to_png(w, h))
    want_jpeg = solver_path(j, tagged, 6, lambda s, w, h: s.to_jpeg(w, h, quality=90, subsampling=(2, 2)))
    want_slot = solver_path(j, tagged, 6, lambda s, w, h: bits(s.to_tensors(w, h, [dict(slot, dtype=torch.float16)])[0]))
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        t = torch.zeros((3, 189, 224), dtype=torch.float16, device="cuda")
        tickets = [b.submit(None, 0.3, [0.001] * 3, ITS, file=tagged, orientation="exif", png={}),
                   b.submit(None, 0.3, [0.001] * 3, ITS, file=tagged, orientation="exif", jpeg={"quality": 90, "subsampling": (2, 2)}),
                   b.submit(None, 0.3, [0.001] * 3, ITS, file=tagged, orientation="exif", outputs=[dict(slot, tensor=t)])]
        got = [b.wait(k) for k in tickets]
        assert got[0] == want_png and got[1] == want_jpeg and np.array_equal(bits(got[2][0]), want_slot)
        # the samples of the job's own form, and with the orientation given as a number
        samples = b.wait(b.submit(None, 0.3, [0.001] * 3, ITS, file=tagged, orientation=6, bits=8))
        assert samples.shape == (45, 38, 3) and j.png_encode(samples) == want_png
        # a file without the tag: the unoriented job, byte for byte
        plain = b.wait(b.submit(None, 0.3, [0.001] * 3, ITS, file=untagged, png={}))
        assert b.wait(b.submit(None, 0.3, [0.001] * 3, ITS, file=untagged, orientation="exif", png={})) == plain
        # refusals at submit, and the batch goes on
        with pytest.raises(j.J2PError) as e:
            b.submit(make_case(45, 38, "420", 25, seed=7), 0.3, [0.001] * 3, ITS, width=45, height=38, orientation="exif", png={})
        assert e.value.code == J2P_EINVAL
        with pytest.raises(j.J2PError) as e:
            b.submit(make_case(45, 38, "420", 25, seed=7), 0.3, [0.001] * 3, ITS, width=45, height=38, bits=8, orientation=3, tile=True)
        assert e.value.code == J2P_EINVAL
        with pytest.raises(j.J2PError):
            b.submit(None, 0.3, [0.001] * 3, ITS, file=tagged, orientation=9, png={})
        assert b.wait(b.submit(None, 0.3, [0.001] * 3, ITS, file=untagged, png={})) == plain


@pytest.mark.gpu
def test_batch_job_from_coefficients_with_orientation_3(lib, cases):
    import jpeg2png_amd as j
    c = cases["45x38_420"]
    tables = j.quality_tables(90, 3)
    with c.oriented(3) as (uw, uh):
        want_samples = c.samples(uw, uh, 16)
        want_png = c.s.to_png(uw, uh)
        want_coef = oriented_coefficients(c, tables, (2, 2), uw, uh)
    planes = make_case(45, 38, "420", 25, seed=7)
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        tickets = [b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=38, bits=16, orientation=3),
                   b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=38, orientation=3, png={}),
                   b.submit(planes, 0.3, [0.001] * 3, 2, width=45, height=38, orientation=3, quant_tables=tables, subsampling=[(1, 1), (2, 2), (2, 2)])]
        got = [b.wait(k) for k in tickets]
    assert np.array_equal(got[0], want_samples[:, :, :].reshape(got[0].shape)) and got[1] == want_png
    assert all(np.array_equal(a, w) for a, w in zip(got[2], want_coef))


# ---- end to end against PIL ----

@pytest.mark.gpu
def test_upright_png_is_exif_transpose_of_the_plain_png(lib):
    import jpeg2png_amd as j
    from PIL import Image, ImageOps
    files = {o: uc.pil_jpeg(45, 38, seed=6, orientation=o) for o in uc.ORIENTATIONS}
    with j.Solver.from_jpeg(files[1], 0.3, [0.001] * 3, ITS) as s:
        assert s.orientation == 1
        s.run(ITS)
        plain = Image.open(io.BytesIO(s.to_png(45, 38)))
        plain.load()
    for o, file in files.items():
        with j.Solver.from_jpeg(file, 0.3, [0.001] * 3, ITS, upright=True) as s:
            assert s.orientation == o
            s.run(ITS)
            uw, uh = uc.upright_size(o, 45, 38)
            got = Image.open(io.BytesIO(s.to_png(uw, uh)))
            assert "exif" not in got.info
        tagged = plain.copy()
        tagged.getexif()[uc.TAG] = o
        want = ImageOps.exif_transpose(tagged)
        assert got.size == want.size == (uw, uh) and np.array_equal(np.asarray(got), np.asarray(want)), o
