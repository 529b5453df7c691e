"""Tensor output: the solved image as a torch tensor left on the GPU (j2p_planes[_rows]_to_tensor, Solver.to_tensor,
Batch.submit(tensor=...)).  Every comparison is of BIT PATTERNS, tolerance zero: include/jpeg2png_amd.h defines every bit of
an element, and `expected()` below restates that definition in numpy — float64 for the colour matrix, astype(float32) for
the narrowings, a float32 multiply and then a float32 add, astype(float16) for f16 and round-to-nearest-even on the f32 bits
for bf16 — applied to Solver.download(c) of the same solver.  The anchor to the reference program is the sample path
(j2p_planes_to_rgb / _grey), whose PNG bytes the CLI tests hold to the reference's: the u8 tensor must equal its 8-bit
samples and the f32 tensor its 16-bit ones.  Solves are 2 iterations on 48x32 canvases, shared by module fixtures and left
unchanged."""
import ctypes

import numpy as np
import pytest

from conftest import band_devices, make_case

J2P_EINVAL, J2P_ESTATE = -1, -4
W, H = 48, 32

# the usual ImageNet normalisation of a [0, 255] image: (v / 255 - m) / s = v * (1 / (255 s)) + (-m / s), computed in float64
# and rounded to f32 ONCE, here; the same f32 values go to the library and to numpy
_M, _S = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [float(np.float32(1.0 / (255.0 * s))) for s in _S]
BIAS = [float(np.float32(-m / s)) for m, s in zip(_M, _S)]


def unclamped(planes, w, h):
    """the float32 values the clamp sees (png.c:37-45 after jpeg2png.c:156-159): one array per output channel"""
    yi = (planes[0][:h, :w].astype(np.float64) + 128.).astype(np.float32)
    if len(planes) == 1:
        return [yi]
    y, cb, cr = yi.astype(np.float64), planes[1][:h, :w].astype(np.float64), planes[2][:h, :w].astype(np.float64)
    return [(y + 1.402 * cr).astype(np.float32), (y - 0.34414 * cb - 0.71414 * cr).astype(np.float32), (y + 1.772 * cb).astype(np.float32)]


def bf16_bits(t):
    u = np.ascontiguousarray(t, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def clamped(planes, w, h):
    """the float32 values after the clamp (png.c:15-17), one array per output channel"""
    return [np.where(v.astype(np.float64) > 255., np.float32(255), np.where(v.astype(np.float64) < 0., np.float32(0), v)).astype(np.float32)
            for v in unclamped(planes, w, h)]


def expected(planes, w, h, dtype, layout, scale=None, bias=None):
    """the tensor's bit patterns (uint8 / uint16 / uint32) from the downloaded planes: the header's definition, restated"""
    out = []
    for k, v in enumerate(clamped(planes, w, h)):
        if dtype == "u8":
            out.append(v.astype(np.uint32).astype(np.uint8))
            continue
        t = (v * np.float32(1.0 if scale is None else scale[k])).astype(np.float32)
        t = (t + np.float32(0.0 if bias is None else bias[k])).astype(np.float32)
        out.append({"f32": lambda: t.view(np.uint32), "f16": lambda: t.astype(np.float16).view(np.uint16), "bf16": lambda: bf16_bits(t)}[dtype]())
    return np.stack(out, axis=0 if layout == "chw" else 2)


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


class Case:
    """one solved image: the solver, its downloaded planes and the C entry points"""

    def __init__(self, j, planes, its=2, weight=0.3):
        self.j, self.n = j, len(planes)
        self.s = j.Solver(planes, weight, [0.001] * self.n, its)
        self.s.run(its)
        self.planes = [self.s.download(c) for c in range(self.n)]
        self.lib = self.s._lib
        self.refs = (j._CPlaneRef * self.n)(*[j._CPlaneRef(self.s._h, c) for c in range(self.n)])

    def close(self):
        self.s.close()

    def samples(self, bits_, w=W, h=H):
        u, p = ctypes.c_uint, ctypes.c_void_p
        ref = ctypes.POINTER(self.j._CPlaneRef)
        self.lib.j2p_planes_to_rgb.argtypes = self.lib.j2p_planes_to_grey.argtypes = [ref, u, u, u, p]
        out = np.zeros(h * w * self.n * (bits_ // 8), np.uint8)
        assert getattr(self.lib, "j2p_planes_to_rgb" if self.n == 3 else "j2p_planes_to_grey")(self.refs, w, h, bits_, out.ctypes.data) == 0
        return out.reshape(h, w, self.n) if bits_ == 8 else out.view(">u2").reshape(h, w, self.n)


def c_tensor(j, t, layout, dtype=None, scale=(1, 1, 1), bias=(0, 0, 0), data=None, strides=None):
    """a j2p_tensor for the C entry points, field by field"""
    sc, sy, sx = strides or (t.stride() if layout == "chw" else (t.stride(2), t.stride(0), t.stride(1)))
    code = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}.get(dtype, dtype)
    return j._CTensor(t.data_ptr() if data is None else data, code, sc, sy, sx, (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias))


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def joint_420(lib):
    import jpeg2png_amd as j
    c = Case(j, make_case(W, H, "420", 25, seed=11))
    assert (c.s.W, c.s.H) == (W, H)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grey(lib):
    import jpeg2png_amd as j
    c = Case(j, make_case(W, H, "420", 25, seed=11, y_only=True))
    assert (c.s.W, c.s.H, c.n) == (W, H, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def clamping_444(lib):
    """quality 10: the blue channel leaves [0, 255] at both ends before the clamp"""
    import jpeg2png_amd as j
    c = Case(j, make_case(W, H, "444", 10, seed=7))
    yield c
    c.close()


@pytest.fixture(scope="module")
def padded_420(lib):
    """a 40x20 image inside a 48x32 canvas"""
    import jpeg2png_amd as j
    c = Case(j, make_case(40, 20, "420", 10, seed=5))
    assert (c.s.W, c.s.H) == (W, H)
    yield c
    c.close()


# ---- 1. anchor: the sample path ----

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rgb", "grey"])
def test_u8_and_f32_tensors_are_the_8_and_16_bit_samples(torch_cuda, joint_420, grey, which):
    torch = torch_cuda
    c = joint_420 if which == "rgb" else grey
    s8, s16 = c.samples(8), c.samples(16)
    assert s8.any() and s8.min() < s8.max()
    t8 = c.s.to_tensor(W, H, dtype=torch.uint8, layout="hwc")
    assert t8.shape == (H, W, c.n) and t8.dtype == torch.uint8 and t8.device == torch.device("cuda", 0)
    assert np.array_equal(bits(t8), s8)
    t32 = c.s.to_tensor(W, H, dtype=torch.float32, layout="hwc", scale=[1.0] * c.n, bias=[0.0] * c.n)
    f = t32.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.floor(f * 256.).astype(np.uint16), s16.astype(np.uint16))
    # and both agree with the restatement
    assert np.array_equal(bits(t8), expected(c.planes, W, H, "u8", "hwc"))
    assert np.array_equal(bits(t32), expected(c.planes, W, H, "f32", "hwc"))


def expected_sample_bytes(planes, w, h, bits_):
    """the sample forms' bytes from the downloaded planes (png.c:44-62): interleaved, one byte per sample or two, big-endian.
    The float32 multiply by 256 is exact (a power of two, nothing near overflow)"""
    if bits_ == 8:
        return expected(planes, w, h, "u8", "hwc").tobytes()
    return np.stack([(v * np.float32(256)).astype(np.float32).astype(np.uint32) for v in clamped(planes, w, h)], axis=2).astype(">u2").tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bits_", [8, 16])
@pytest.mark.parametrize("which", ["rgb", "grey"])
def test_sample_bytes_are_the_restatement(clamping_444, grey, which, bits_):
    """The sample forms against numpy, so that the anchor above has an anchor of its own in this file: RGB with the clamp at
    work and greyscale, 8 and 16 bits, widths with and without a w % 4 tail and narrower than 4, one row and more, and a
    rows form that does not start at row 0.  64 sentinel bytes behind every output stay as they were."""
    c = clamping_444 if which == "rgb" else grey
    u, p, ref = ctypes.c_uint, ctypes.c_void_p, ctypes.POINTER(c.j._CPlaneRef)
    name = "j2p_planes_to_rgb" if c.n == 3 else "j2p_planes_to_grey"
    whole_form, rows_form = getattr(c.lib, name), getattr(c.lib, name.replace("planes_", "planes_rows_"))
    whole_form.argtypes, rows_form.argtypes = [ref, u, u, u, p], [ref, u, u, u, u, p]

    def check(w, y0, y1, call):
        n = (y1 - y0) * w * c.n * (bits_ // 8)
        out = np.full(n + 64, 0xa5, np.uint8)
        assert call(out.ctypes.data) == 0, (w, y0, y1)
        want = expected_sample_bytes(c.planes, w, y1, bits_)
        assert out[:n].tobytes() == want[len(want) - n:], (w, y0, y1)
        assert (out[n:] == 0xa5).all(), (w, y0, y1)

    for w in (1, 3, 4, 5, 47, 48):
        for h in (1, 31, 32):
            check(w, 0, h, lambda data: whole_form(c.refs, w, h, bits_, data))
    for w in (47, 48):
        check(w, 16, 31, lambda data: rows_form(c.refs, w, 16, 31, bits_, data))
    if which == "rgb" and bits_ == 8:
        v = np.frombuffer(expected_sample_bytes(c.planes, W, H, 8), np.uint8)
        assert (v == 0).any() and (v == 255).any() and len(np.unique(v)) > 16        # the clamp is at work in what was compared


# ---- 2. the definition, with the clamp at work ----

@pytest.mark.gpu
def test_the_clamping_case_clamps_at_both_ends(clamping_444):
    v = np.stack(unclamped(clamping_444.planes, W, H)).astype(np.float64)
    assert (v < 0.).any() and (v > 255.).any() and ((v > 0.) & (v < 255.)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", ["u8", "f16", "bf16", "f32"])
def test_every_dtype_and_layout_is_the_definition(torch_cuda, clamping_444, dtype, layout):
    c = clamping_444
    kw = {} if dtype == "u8" else {"scale": SCALE, "bias": BIAS}
    t = c.s.to_tensor(W, H, dtype=torch_dtype(dtype), layout=layout, **kw)
    assert tuple(t.shape) == ((3, H, W) if layout == "chw" else (H, W, 3)) and t.is_contiguous()
    want = expected(c.planes, W, H, dtype, layout, **kw)
    assert len(np.unique(want)) > 16
    assert np.array_equal(bits(t), want)


@pytest.mark.gpu
def test_scale_one_bias_zero_is_still_two_operations(torch_cuda, clamping_444):
    """default scale / bias: the product and the sum are formed all the same"""
    c = clamping_444
    for dtype in ("f32", "f16", "bf16"):
        t = c.s.to_tensor(W, H, dtype=torch_dtype(dtype))
        assert np.array_equal(bits(t), expected(c.planes, W, H, dtype, "chw"))
    # a bias that cancels: clamped 255 * 1 + (-255) is +0, and a negative scale gives -0 + 0 = +0 for clamped zeros
    t = c.s.to_tensor(W, H, scale=[-1.0, -1.0, -1.0], bias=[0.0, 0.0, 0.0])
    want = expected(c.planes, W, H, "f32", "chw", scale=[-1.0] * 3, bias=[0.0] * 3)
    assert np.array_equal(bits(t), want) and not (want == 0x80000000).any() and (want == 0).any()


# ---- 3. crops, tails and the three destination paths ----

@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_crops_and_row_tails(torch_cuda, clamping_444, padded_420, dtype, layout):
    c = clamping_444
    for w in (1, 3, 4, 5, 47, 48):
        for h in (1, 31, 32):
            t = c.s.to_tensor(w, h, dtype=torch_dtype(dtype), layout=layout)
            assert np.array_equal(bits(t), expected(c.planes, w, h, dtype, layout)), (w, h)
    t = padded_420.s.to_tensor(40, 20, dtype=torch_dtype(dtype), layout=layout)
    assert np.array_equal(bits(t), expected(padded_420.planes, 40, 20, dtype, layout))


def path_of(j, t, layout, dtype, w=W):
    ct = c_tensor(j, t, layout, dtype)
    return j.tensor_path(w, 3, ct.dtype, ct.stride_c, ct.stride_y, ct.stride_x, ct.data)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["u8", "f16", "bf16", "f32"])
def test_each_destination_path_is_reached_and_right(torch_cuda, clamping_444, dtype):
    import jpeg2png_amd as j
    torch = torch_cuda
    c, td = clamping_444, torch_dtype(dtype)
    fill, fill_bits = sentinel(dtype)
    dev = torch.device("cuda", 0)
    # contiguous chw: planar; contiguous hwc: interleaved
    for layout, path in (("chw", "planar"), ("hwc", "interleaved")):
        shape = (3, H, W) if layout == "chw" else (H, W, 3)
        t = torch.empty(shape, dtype=td, device=dev)
        assert path_of(j, t, layout, dtype) == path
        assert c.s.to_tensor(W, H, layout=layout, out=t) is t
        assert np.array_equal(bits(t), expected(c.planes, W, H, dtype, layout)), path
    # the same two, one element into a larger buffer: misaligned for every store wider than an element -> generic
    for layout in ("chw", "hwc"):
        shape = (3, H, W) if layout == "chw" else (H, W, 3)
        buf = torch.full((3 * H * W + 2,), fill, dtype=td, device=dev)
        t = buf[1:-1].view(shape)
        assert path_of(j, t, layout, dtype) == "generic"
        c.s.to_tensor(W, H, layout=layout, out=t)
        assert np.array_equal(bits(t), expected(c.planes, W, H, dtype, layout)), ("misaligned", layout)
        assert bits(buf)[0] == fill_bits and bits(buf)[-1] == fill_bits
    # transposed strides: x steps over whole columns
    t = torch.empty((3, W, H), dtype=td, device=dev).transpose(1, 2)
    assert tuple(t.shape) == (3, H, W) and t.stride(2) == H and path_of(j, t, "chw", dtype) == "generic"
    c.s.to_tensor(W, H, out=t)
    assert np.array_equal(bits(t), expected(c.planes, W, H, dtype, "chw")), "transposed"
    # rows of 47 elements: every second row would be misaligned -> generic, whatever the layout
    wide = torch.full((3, H, 47), fill, dtype=td, device=dev)
    assert path_of(j, wide, "chw", dtype, w=47) == "generic"
    c.s.to_tensor(47, H, out=wide)
    assert np.array_equal(bits(wide), expected(c.planes, 47, H, dtype, "chw"))


# ---- 4. strided destinations leave the rest alone ----

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "u8"])
def test_a_slot_of_a_padded_batch_tensor(torch_cuda, clamping_444, dtype):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = clamping_444
    fill, fill_bits = sentinel(dtype)
    batch = torch.full((2, 3, 40, 64), fill, dtype=torch_dtype(dtype), device="cuda:0")
    slot = batch[1, :, 4:36, 8:56]
    assert path_of(j, slot, "chw", dtype) == "planar"            # rows 64 elements apart, 8 elements in: vector stores
    kw = {} if dtype == "u8" else {"scale": SCALE, "bias": BIAS}
    c.s.to_tensor(W, H, out=slot, **kw)
    got = bits(batch)
    want = np.full(got.shape, fill_bits, got.dtype)
    want[1, :, 4:36, 8:56] = expected(c.planes, W, H, dtype, "chw", **kw)
    assert dtype == "u8" or not (want[1, :, 4:36, 8:56] == fill_bits).any()
    assert np.array_equal(got, want)


# ---- 5. the rows form is the whole form ----

@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("f32", "chw"), ("u8", "hwc"), ("bf16", "hwc")])
def test_whole_rows_and_halves_are_the_same_bytes(torch_cuda, joint_420, dtype, layout):
    import jpeg2png_amd as j
    torch = torch_cuda
    c = joint_420
    shape = (3, H, W) if layout == "chw" else (H, W, 3)
    got = []
    for rows in (None, [(0, H)], [(0, 16), (16, H)]):
        t = torch.zeros(shape, dtype=torch_dtype(dtype), device="cuda:0")
        torch.cuda.synchronize()
        if rows is None:
            assert c.lib.j2p_planes_to_tensor(c.refs, 3, W, H, ctypes.byref(c_tensor(j, t, layout, dtype))) == 0
        for y0, y1 in rows or []:
            part = t[:, y0:y1] if layout == "chw" else t[y0:y1]
            strides = (t.stride() if layout == "chw" else (t.stride(2), t.stride(0), t.stride(1)))
            assert c.lib.j2p_planes_rows_to_tensor(c.refs, 3, W, y0, y1, ctypes.byref(c_tensor(j, part, layout, dtype, strides=strides))) == 0
        c.s.sync()
        got.append(bits(t))
    assert np.array_equal(got[0], expected(c.planes, W, H, dtype, layout))
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])


@pytest.mark.gpu
def test_band_solvers_write_their_own_rows_into_one_tensor(torch_cuda, joint_420):
    """two bands on the tensor's GPU: each writes its rows; the planes of a row-tiled solve are the whole-canvas solve's"""
    import jpeg2png_amd as j
    torch = torch_cuda
    devices = band_devices(2)
    if len(set(devices)) > 1:
        devices = [devices[0]] * 2              # the tensor lives on ONE device: both bands there
    planes = make_case(W, H, "420", 25, seed=11)
    t = torch.zeros((3, H, W), dtype=torch.float16, device=f"cuda:{devices[0]}")
    with j.TiledSolver(planes, 0.3, [0.001] * 3, 2, devices=devices) as tiled:
        assert tiled.nband == 2
        tiled.run(2)
        tiled.sync()
        for b in range(2):
            band = tiled.band_solver(b)
            assert (band.row_begin, band.row_end) == (16 * b, 16 * b + 16)
            refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(band._h, ch) for ch in range(3)])
            whole = c_tensor(j, t, "chw", "f16", scale=SCALE, bias=BIAS)
            assert band._lib.j2p_planes_to_tensor(refs, 3, W, 16, ctypes.byref(whole)) == J2P_ESTATE
            rows = t[:, band.row_begin:band.row_end]
            assert band.to_tensor(W, 16, layout="chw", scale=SCALE, bias=BIAS, out=rows) is rows
        torch.cuda.synchronize()
    assert np.array_equal(bits(t), expected(joint_420.planes, W, H, "f16", "chw", scale=SCALE, bias=BIAS))


# ---- 6. refusals ----

@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(torch_cuda, lib):
    import jpeg2png_amd as j
    torch = torch_cuda
    planes = make_case(W, H, "420", 25, seed=11)
    fill, fill_bits = sentinel("f32")
    t = torch.full((3, H, W), fill, dtype=torch.float32, device="cuda:0")
    t8 = torch.full((3, H, W), 201, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    hip = j.hip_runtime()
    with j.Solver(planes, 0.3, [0.001] * 3, 2) as s, j.Solver(planes[:2], 0.3, [0.001] * 2, 2) as s2:
        s.run(1)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, c) for c in range(3)])

        def call(ct, nplane=3, w=W, rows=(0, H), r=refs):
            return s._lib.j2p_planes_rows_to_tensor(r, nplane, w, rows[0], rows[1], ctypes.byref(ct))

        ok = c_tensor(j, t, "chw", "f32")
        host = np.zeros(3 * H * W, np.float32)
        inf, nan = float("inf"), float("nan")
        refused = {
            "unknown dtype": call(c_tensor(j, t, "chw", 4)),
            "negative dtype": call(c_tensor(j, t, "chw", -1)),
            "stride_c 0": call(c_tensor(j, t, "chw", "f32", strides=(0, W, 1))),
            "stride_y 0": call(c_tensor(j, t, "chw", "f32", strides=(H * W, 0, 1))),
            "stride_x -1": call(c_tensor(j, t, "chw", "f32", strides=(H * W, W, -1))),
            "NULL data": call(c_tensor(j, t, "chw", "f32", data=0)),
            "misaligned f32": call(c_tensor(j, t, "chw", "f32", data=t.data_ptr() + 2)),
            "misaligned f16": call(c_tensor(j, t, "chw", "f16", data=t.data_ptr() + 1)),
            "host memory": call(c_tensor(j, t, "chw", "f32", data=host.ctypes.data)),
            "scale inf": call(c_tensor(j, t, "chw", "f32", scale=(1, inf, 1))),
            "scale nan": call(c_tensor(j, t, "chw", "f32", scale=(nan, 1, 1))),
            "bias nan": call(c_tensor(j, t, "chw", "f32", bias=(0, 0, nan))),
            "bias -inf": call(c_tensor(j, t, "chw", "f32", bias=(-inf, 0, 0))),
            "u8 scale": call(c_tensor(j, t8, "chw", "u8", scale=(1, 2, 1))),
            "u8 bias": call(c_tensor(j, t8, "chw", "u8", bias=(0, 0, 1))),
            "two planes": call(ok, nplane=2),
            "wider than the canvas": call(ok, w=W + 1),
            "rows beyond the canvas": call(ok, rows=(0, H + 1)),
            "empty row range": call(ok, rows=(5, 5)),
            "empty width": call(ok, w=0),
            "NULL tensor": s._lib.j2p_planes_rows_to_tensor(refs, 3, W, 0, H, None),
            "bad channel": call(ok, r=(j._CPlaneRef * 3)(j._CPlaneRef(s._h, 0), j._CPlaneRef(s._h, 1), j._CPlaneRef(s._h, 3))),
        }
        managed = ctypes.c_void_p()
        hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
        if hip.hipMallocManaged(ctypes.byref(managed), host.nbytes, 1) == 0 and managed.value:
            refused["managed memory"] = call(c_tensor(j, t, "chw", "f32", data=managed.value))
            hip.hipFree.argtypes = [ctypes.c_void_p]
            hip.hipFree(managed)
        if j.device_count() > 1:
            other = torch.full((3, H, W), fill, dtype=torch.float32, device="cuda:1")
            torch.cuda.synchronize(1)
            refused["another GPU's memory"] = call(c_tensor(j, other, "chw", "f32"))
        assert {k: v for k, v in refused.items() if v != J2P_EINVAL} == {}
        # between the two phases of an iteration: a state error, as for the samples
        s.phase_gradient()
        assert call(ok) == J2P_ESTATE
        s.phase_project()
        # the binding's own refusals
        for bad in (lambda: s2.to_tensor(W, H),                                                  # two channels
                    lambda: s.to_tensor(W, H, out=t[:, :, :1].expand(3, H, W)),                   # a zero stride
                    lambda: s.to_tensor(W, H, out=t[:, :H - 1]),                                  # wrong shape
                    lambda: s.to_tensor(W, H, dtype=torch.float64),
                    lambda: s.to_tensor(W, H, dtype=torch.uint8, scale=[2.0, 1.0, 1.0]),
                    lambda: s.to_tensor(W, H, layout="nhwc"),
                    lambda: s.to_tensor(W, H, out=torch.zeros((3, H, W))),                        # a CPU tensor
                    lambda: s.to_tensor(W, H, scale=[1.0, 1.0])):
            with pytest.raises(j.J2PError):
                bad()
        s.sync()
        torch.cuda.synchronize()
        assert (bits(t) == fill_bits).all() and (bits(t8) == 201).all() and not host.any()
        # and after all that the call still works
        assert call(ok) == 0
        s.sync()
        assert not (bits(t) == fill_bits).any()


@pytest.mark.gpu
def test_batch_refusals(torch_cuda, lib):
    import jpeg2png_amd as j
    torch = torch_cuda
    planes = make_case(W, H, "420", 25, seed=11)
    fill, fill_bits = sentinel("f16")
    t = torch.full((3, H, W), fill, dtype=torch.float16, device="cuda:0")
    t2 = torch.full((2, H, W), fill, dtype=torch.float16, device="cuda:0")
    common = dict(width=W, height=H)
    with j.Batch(devices=[0], slots_per_device=1) as b:
        def refused(pl, **kw):
            with pytest.raises(j.J2PError):
                b.wait(b.submit(pl, 0.3, [0.001] * len(pl), 2, **common, **kw))
        refused(planes, tensor=t, tile=True, tile_min_band_pixels=0)
        refused(planes[:2], tensor=t2)                                             # two channels
        refused(planes, tensor=t, bits=8)
        refused(planes, tensor=t, quant_tables=[np.ones(64, np.uint16)] * 3)
        refused(planes, tensor=t.cpu())
        refused(planes, tensor=t, layout="whc")
        refused(planes, tensor=t[:, :, :W - 1])                                    # wrong shape
        refused(planes, tensor=t.double())
        refused(planes, scale=[1.0] * 3)                                           # scale without a tensor
        with pytest.raises(j.J2PError):
            b.submit(planes, 0.3, [0.001] * 3, 2, tensor=t)                        # no width / height
        # the C interface refuses the same at submit: tile, two channels, a host pointer
        for change in ({"tile": 1}, {"nchannel": 2}, {"out_bits": 8}, {"host": True}):
            job, keep = j._CJob(), []
            job.nchannel = 3
            cpl, keep = j._c_planes(planes)
            for c in range(3):
                job.planes[c] = cpl[c]
                job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 2
            job.out_w, job.out_h = W, H
            job.out_tensor = c_tensor(j, t, "chw", "f16")
            host = np.zeros(3 * H * W, np.float16)
            for k, v in change.items():
                if k == "host":
                    job.out_tensor.data = host.ctypes.data
                else:
                    setattr(job, k, v)
            ticket = ctypes.c_int(-1)
            assert b._lib.j2p_batch_submit(b._h, ctypes.byref(job), ctypes.byref(ticket)) == J2P_EINVAL, change
            assert not host.any()
        if j.device_count() > 1:
            other = torch.full((3, H, W), fill, dtype=torch.float16, device="cuda:1")
            refused(planes, tensor=other)                                          # a GPU this batch does not drive
        # the batch still works, and nothing was written meanwhile
        torch.cuda.synchronize()
        assert (bits(t) == fill_bits).all()
        assert b.wait(b.submit(planes, 0.3, [0.001] * 3, 2, tensor=t, **common)) is t
        assert not (bits(t) == fill_bits).any()


# ---- 7. asynchrony and stream order ----

@pytest.mark.gpu
def test_torch_work_queued_behind_to_tensor_sees_the_finished_tensor(torch_cuda, clamping_444):
    torch = torch_cuda
    c = clamping_444
    want = expected(c.planes, W, H, "f32", "chw", scale=SCALE, bias=BIAS)
    t = c.s.to_tensor(W, H, scale=SCALE, bias=BIAS)
    copy = t.clone()                                    # no synchronisation in between
    assert np.array_equal(bits(copy), want)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((3, H, W), -7.0, device="cuda:0")          # the fill is queued on the side stream, the kernel behind it
        t = c.s.to_tensor(W, H, scale=SCALE, bias=BIAS, out=out)
        copy = t.clone()
    side.synchronize()
    assert np.array_equal(bits(copy), want)


# ---- 8. the batch engine ----

def solve_to_tensor(j, torch, planes, separate, scale, bias):
    """Solver + to_tensor of the same inputs: one joint solve, or one solve per component as `-s` (jpeg2png.c:147-152)"""
    t = torch.zeros((3, H, W), dtype=torch.float16, device="cuda:0")
    if not separate:
        with j.Solver(planes, 0.3, [0.001] * 3, 2) as s:
            s.run(2)
            s.to_tensor(W, H, scale=scale, bias=bias, out=t)
            torch.cuda.synchronize()
        return t
    solvers = [j.Solver([p], 0.3, [0.001], 2) for p in planes]
    try:
        for s in solvers:
            s.run(2)
        refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, 0) for s in solvers])
        torch.cuda.synchronize()
        assert solvers[0]._lib.j2p_planes_to_tensor(refs, 3, W, H, ctypes.byref(c_tensor(j, t, "chw", "f16", scale=scale, bias=bias))) == 0
        solvers[0].sync()
    finally:
        for s in solvers:
            s.close()
    return t


@pytest.mark.gpu
def test_batch_tensor_jobs_fill_the_slots_of_one_tensor(torch_cuda, lib):
    import jpeg2png_amd as j
    torch = torch_cuda
    cases = [(make_case(W, H, "420", 25, seed=11), False), (make_case(W, H, "420", 25, seed=11), True),
             (make_case(W, H, "420", 10, seed=12), False), (make_case(W, H, "420", 10, seed=12), True)]
    fill, fill_bits = sentinel("f16")
    batch = torch.full((4, 3, H, W), fill, dtype=torch.float16, device="cuda:0")
    with j.Batch(devices=[0], slots_per_device=2) as b:
        tickets = [b.submit(planes, 0.3, [0.001] * 3, 2, separate=separate, width=W, height=H, tensor=batch[i], scale=SCALE, bias=BIAS)
                   for i, (planes, separate) in enumerate(cases)]
        # jobs without a tensor in the same batch: samples and planes
        rgb = b.submit(cases[0][0], 0.3, [0.001] * 3, 2, width=W, height=H, bits=8)
        flo = b.submit(cases[0][0], 0.3, [0.001] * 3, 2)
        u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        u8_ticket = b.submit(cases[0][0], 0.3, [0.001] * 3, 2, width=W, height=H, tensor=u8, layout="hwc")
        for i, ticket in enumerate(tickets):
            assert b.wait(ticket).data_ptr() == batch[i].data_ptr()
        rgb, flo = b.wait(rgb), b.wait(flo)
        assert b.wait(u8_ticket) is u8
    got = bits(batch)                                   # (after wait the tensor is complete for any stream)
    assert not (got == fill_bits).any()
    for i, (planes, separate) in enumerate(cases):
        want = bits(solve_to_tensor(j, torch, planes, separate, SCALE, BIAS))
        assert np.array_equal(got[i], want), (i, separate)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    assert np.array_equal(bits(u8), rgb) and rgb.any()
    assert np.array_equal(got[0], expected(flo, W, H, "f16", "chw", scale=SCALE, bias=BIAS))
