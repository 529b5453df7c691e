"""Every way a batch job is refused, as a table: how to build the bad job, the stage that reports it ("submit": the
j2p_batch_submit* call / Batch.submit itself; "wait": j2p_batch_wait), the return code and the full message, copied as literals
from the source.  RAW goes through _CJob and the eight C entry points, so that Python's own checks shadow nothing
(test_job_refusals_gpu.py); PYTHON holds every J2PError that Batch.submit itself raises before it needs a device
(test_job_refusals_cpu.py).

The job is the smallest that takes every path: 4:2:0, luma 32x16 coefficients, chroma 16x8, image 30x13 (a crop, and a block row
that overhangs it), 2 iterations."""
import ctypes
from collections import namedtuple

import numpy as np

import decode_cases as dc
from jpeg2png_amd import synth

J2P_EINVAL, J2P_EFORMAT = -1, -6
WIDTH, HEIGHT, ITERATIONS, WEIGHT, PWEIGHT = 30, 13, 2, 0.3, [0.001, 0.002, 0.003]


def planes():
    return synth.make_planes(WIDTH, HEIGHT, "420", 10, seed=7)


def bare_planes():
    """the same without coefficients: what a job made from samples or from a file takes"""
    return [synth.Plane(p.w, p.h, p.w_samp, p.h_samp, None, p.quant_table) for p in planes()]


def samples():
    """decoded 8-bit planes of the image: luma 13x30, chroma 7x15"""
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (HEIGHT, WIDTH), dtype=np.uint8)] + [rng.integers(0, 256, (7, 15), dtype=np.uint8) for _ in range(2)]


def jpeg_file():
    """the planes' coefficients as a baseline JPEG file, written on the host"""
    p = planes()
    return dc.write([q.data for q in p], WIDTH, HEIGHT, [p[0].quant_table, p[1].quant_table], (2, 2))


# ---- the C entry points ----

Raw = namedtuple("Raw", "name stage rc message build gpus", defaults=(1,))


class Kit:
    """what the builders of RAW take their parts from; everything a job points into lives as long as the kit"""

    def __init__(self, j, torch):
        self.j, self.torch, self.keep = j, torch, []
        self.file_bytes = np.frombuffer(jpeg_file(), dtype=np.uint8)
        self.file = (self.file_bytes.ctypes.data, self.file_bytes.size)
        self.garbage = np.frombuffer(b"not a JPEG file at all", dtype=np.uint8)
        self.rgb = np.zeros((HEIGHT, WIDTH, 3), np.uint8)
        self.float_planes = [np.zeros((16, 32), np.float32) for _ in range(3)]

    def hold(self, x):
        self.keep.append(x)
        return x

    def job(self, bare=False, **fields):
        """a good job that hands its float planes back, with `fields` set on top: a value, or {index: value} for an array member"""
        j = self.j
        job = j._CJob()
        cpl, keep = j._c_planes(bare_planes() if bare else planes())
        self.hold(keep)
        job.nchannel = 3
        for c in range(3):
            job.planes[c] = cpl[c]
            job.weight[c], job.pweight[c], job.iterations[c] = WEIGHT, PWEIGHT[c], ITERATIONS
            job.out_planes[c] = self.float_planes[c].ctypes.data
        for name, v in fields.items():
            if isinstance(v, dict):
                for i, x in v.items():
                    getattr(job, name)[i] = x
            else:
                setattr(job, name, v)
        return ctypes.byref(self.hold(job))

    def image(self, **fields):
        """... that knows its image's size"""
        return dict(dict(out_w=WIDTH, out_h=HEIGHT), **fields)

    def rgb_out(self, **fields):
        return self.image(out_bits=8, out_rgb=self.rgb.ctypes.data, **fields)

    def coef_out(self, **fields):
        """quantised coefficients of every channel at full resolution"""
        tables = self.hold([np.ascontiguousarray(p.quant_table, np.uint16) for p in planes()])
        grids = self.hold([np.zeros((2, 4, 64), np.int16) for _ in range(3)])
        return dict(dict(out_blocks_w=4, out_blocks_h=2, out_quant={c: tables[c].ctypes.data for c in range(3)},
                         out_coef={c: grids[c].ctypes.data for c in range(3)}), **fields)

    def table_with_zero(self):
        q = self.hold(np.ascontiguousarray(planes()[0].quant_table, np.uint16).copy())
        q[5] = 0
        return q.ctypes.data

    def tensor(self, shape=(3, HEIGHT, WIDTH), device=0):
        t = self.hold(self.torch.zeros(shape, dtype=self.torch.float32, device=f"cuda:{device}"))
        self.torch.cuda.synchronize(device)
        return self.j._c_tensor(t, 3, shape[2], shape[1], "chw", None, None)

    def host_tensor(self):
        a = self.hold(np.zeros((3, HEIGHT, WIDTH), np.float32))
        one = (ctypes.c_float * 3)(1, 1, 1)
        return self.j._CTensor(a.ctypes.data, self.j.J2P_DTYPE_F32, HEIGHT * WIDTH, WIDTH, 1, one, (ctypes.c_float * 3)())

    def resize(self, *spec):
        return ctypes.byref(self.hold(self.j._CResize(*spec)))

    def resample(self, *spec):
        return ctypes.byref(self.hold(self.j._CResample(*spec)))

    def outputs(self, n=2, second_filter=1, second=None):
        """n outputs of 8x6, triangle-filtered; the second one with that filter code, or that tensor"""
        items = self.hold((self.j._COutput * n)())
        for i in range(n):
            items[i].r = self.j._CResample(0, 0, WIDTH, HEIGHT, 8, 6, second_filter if i == 1 else 1)
            items[i].t = second if i == 1 and second is not None else self.tensor((3, 6, 8))
        return n, items

    def samples(self, device=None, **fields):
        """the j2p_samples of the three channels, in host memory or on that GPU; fields: {member: {channel: value}}"""
        arr = self.hold((self.j._CSamples * 3)())
        for c, a in enumerate(samples()):
            if device is None:
                ptr = self.hold(a).ctypes.data
            else:
                ptr = self.hold(self.torch.from_numpy(a).to(f"cuda:{device}")).data_ptr()
                self.torch.cuda.synchronize(device)
            arr[c] = self.j._CSamples(ptr, a.shape[1], a.shape[0], a.shape[1], 1)
        for name, per_channel in fields.items():
            for c, v in per_channel.items():
                setattr(arr[c], name, v)
        return arr

    def managed(self):
        """256 bytes of managed memory, or None where the runtime has none to give"""
        hip = self.j.hip_runtime()
        p = ctypes.c_void_p()
        hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
        if hip.hipMallocManaged(ctypes.byref(p), 256, 1) != 0 or not p.value:
            return None
        return p.value

    def file_on(self, device):
        t = self.hold(self.torch.from_numpy(self.file_bytes.copy()).to(f"cuda:{device}"))
        self.torch.cuda.synchronize(device)
        return t.data_ptr(), int(t.numel())

    def jpeg(self, spec=True, width=WIDTH, sub_w=2, out=True, size=True, capacity=65536):
        """(spec, out, capacity, size) of a JPEG job: quality 90, 4:2:0"""
        j = self.j
        cj, held = j._c_jpeg(width, HEIGHT, 3, 90, None, (2, 2))
        cj.sub_w = sub_w
        buf = self.hold(np.zeros(65536, np.uint8))
        self.hold((cj, held))
        return (ctypes.byref(cj) if spec else None, buf.ctypes.data if out else None, capacity, ctypes.byref(self.hold(ctypes.c_size_t(0))) if size else None)


RESIZE_OK, RESAMPLE_OK = (0, 0, WIDTH, HEIGHT, 10, 5), (0, 0, WIDTH, HEIGHT, 40, 9, 2)
TENSOR_NEEDS = "job: tensor output needs three channels (RGB) or one (greyscale)"

RAW = [
    # validate_job, on the worker: a job without tensor output is refused when it is waited for
    Raw("nchannel 0", "wait", J2P_EINVAL, "job: nchannel must be 1..3", lambda k: ("j2p_batch_submit", [k.job(nchannel=0)])),
    Raw("out_bits 12", "wait", J2P_EINVAL, "job: out_bits must be 0, 8 or 16", lambda k: ("j2p_batch_submit", [k.job(**k.image(out_bits=12))])),
    Raw("sample output with two channels", "wait", J2P_EINVAL, "job: sample output needs out_rgb and three channels (RGB) or one (greyscale)",
        lambda k: ("j2p_batch_submit", [k.job(**k.rgb_out(nchannel=2))])),
    Raw("sample output without out_rgb", "wait", J2P_EINVAL, "job: sample output needs out_rgb and three channels (RGB) or one (greyscale)",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_bits=8))])),
    Raw("sample output of an empty image", "wait", J2P_EINVAL, "job: sample output of an empty image",
        lambda k: ("j2p_batch_submit", [k.job(**k.rgb_out(out_w=0))])),
    Raw("coefficient output with out_bits", "wait", J2P_EINVAL, "job: coefficient output (out_coef) needs out_bits 0",
        lambda k: ("j2p_batch_submit", [k.job(**k.rgb_out(**k.coef_out()))])),
    Raw("coefficient output without out_blocks_w", "wait", J2P_EINVAL, "job: coefficient output needs out_blocks_w and out_blocks_h",
        lambda k: ("j2p_batch_submit", [k.job(**k.coef_out(out_blocks_w=0))])),
    Raw("coefficient output without out_coef[1]", "wait", J2P_EINVAL, "job: coefficient output needs out_coef and out_quant for channel 1",
        lambda k: ("j2p_batch_submit", [_without_coef_1(k)])),
    Raw("a zero quantisation step", "wait", J2P_EINVAL, "job: channel 0: output quantisation table entry 5 is zero",
        lambda k: ("j2p_batch_submit", [_with_zero_step(k)])),
    Raw("output sampling factor 3", "wait", J2P_EINVAL, "job: channel 1: output sampling factors 3x1 (1 and 2 are supported)",
        lambda k: ("j2p_batch_submit", [k.job(**k.coef_out(out_sub_w={1: 3}, out_sub_h={1: 1}))])),
    Raw("tile devices outside the batch", "wait", J2P_EINVAL, "job: tile devices [5, 6) of 1", lambda k: ("j2p_batch_submit", [k.job(tile=1, tile_first=5)])),
    # ... and at submit when it has a tensor
    Raw("tensor with out_bits", "submit", J2P_EINVAL, "job: tensor output (out_tensor) needs out_bits 0 and no out_coef",
        lambda k: ("j2p_batch_submit", [k.job(**k.rgb_out(out_tensor=k.tensor()))])),
    Raw("tensor with out_coef", "submit", J2P_EINVAL, "job: tensor output (out_tensor) needs out_bits 0 and no out_coef",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.tensor(), **k.coef_out()))])),
    Raw("tensor with two channels", "submit", J2P_EINVAL, TENSOR_NEEDS, lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.tensor(), nchannel=2))])),
    Raw("tensor without out_w", "submit", J2P_EINVAL, "job: tensor output needs out_w and out_h",
        lambda k: ("j2p_batch_submit", [k.job(out_tensor=k.tensor(), out_h=HEIGHT)])),
    Raw("tensor with tile", "submit", J2P_EINVAL, "job: tensor output of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.tensor(), tile=1))])),
    Raw("a tensor in host memory", "submit", J2P_EINVAL, "job: out_tensor.data is not device memory (managed and host memory are refused)",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.host_tensor()))])),
    Raw("a tensor in host memory, nchannel 0: the job's own rules first", "submit", J2P_EINVAL, "job: nchannel must be 1..3",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.host_tensor(), nchannel=0))])),
    Raw("a tensor job from samples with out_bits", "submit", J2P_EINVAL, "job: tensor output (out_tensor) needs out_bits 0 and no out_coef",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True, **k.rgb_out(out_tensor=k.tensor())), k.samples(), 0, None])),
    # resized and resampled jobs
    Raw("resized without out_tensor", "submit", J2P_EINVAL, "job: a resized job needs tensor output (out_tensor)",
        lambda k: ("j2p_batch_submit_resized", [k.job(**k.image()), k.resize(*RESIZE_OK)])),
    Raw("resampled without out_tensor", "submit", J2P_EINVAL, "job: a resampled job needs tensor output (out_tensor)",
        lambda k: ("j2p_batch_submit_resampled", [k.job(**k.image()), k.resample(*RESAMPLE_OK)])),
    Raw("resized to more than the box", "submit", J2P_EINVAL, "job: resize: the output is larger than the box (enlarging is what zooming is for)",
        lambda k: ("j2p_batch_submit_resized", [k.job(**k.image(out_tensor=k.tensor((3, 5, 31)))), k.resize(0, 0, WIDTH, HEIGHT, 31, 5)])),
    Raw("resampled with an unknown filter", "submit", J2P_EINVAL, "job: resample: unknown filter",
        lambda k: ("j2p_batch_submit_resampled", [k.job(**k.image(out_tensor=k.tensor((3, 9, 40)))), k.resample(0, 0, WIDTH, HEIGHT, 40, 9, 0)])),
    Raw("resized with out_bits: the resize first, then the job's own rules", "submit", J2P_EINVAL, "job: resize: the box leaves the image",
        lambda k: ("j2p_batch_submit_resized", [k.job(**k.rgb_out(out_tensor=k.tensor((3, 5, 10)))), k.resize(1, 0, WIDTH, HEIGHT, 10, 5)])),
    # outputs
    Raw("17 outputs", "submit", J2P_EINVAL, "job: 17 outputs (at most 16)", lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image()), *k.outputs(17)])),
    Raw("outputs with out_bits", "submit", J2P_EINVAL, "job: a job with outputs needs out_tensor.data NULL, out_bits 0 and no out_coef",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.rgb_out()), *k.outputs()])),
    Raw("outputs with out_tensor", "submit", J2P_EINVAL, "job: a job with outputs needs out_tensor.data NULL, out_bits 0 and no out_coef",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image(out_tensor=k.tensor())), *k.outputs()])),
    Raw("outputs with two channels", "submit", J2P_EINVAL, TENSOR_NEEDS, lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image(nchannel=2)), *k.outputs()])),
    Raw("outputs with nchannel 0", "submit", J2P_EINVAL, TENSOR_NEEDS, lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image(nchannel=0)), *k.outputs()])),
    Raw("outputs without out_h", "submit", J2P_EINVAL, "job: tensor output needs out_w and out_h",
        lambda k: ("j2p_batch_submit_outputs", [k.job(out_w=WIDTH), *k.outputs()])),
    Raw("outputs with tile", "submit", J2P_EINVAL, "job: tensor output of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image(tile=1)), *k.outputs()])),
    Raw("outputs with a bad second spec", "submit", J2P_EINVAL, "job: output 1: resample: unknown filter",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image()), *k.outputs(second_filter=0)])),
    Raw("outputs with the second tensor in host memory", "submit", J2P_EINVAL,
        "job: output 1: the tensor's data is not device memory (managed and host memory are refused)",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image()), *k.outputs(second=k.host_tensor())])),
    Raw("outputs on two GPUs", "submit", J2P_EINVAL, "job: output 1 lives on device 1, output 0 on device 0",
        lambda k: ("j2p_batch_submit_outputs", [k.job(**k.image()), *k.outputs(second=k.tensor((3, 6, 8), device=1))]), 2),
    Raw("17 outputs of a file job", "submit", J2P_EINVAL, "job: 17 outputs (at most 16)",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True), *k.file, *k.outputs(17)])),
    # samples
    Raw("samples with nchannel 0", "submit", J2P_EINVAL, "job: nchannel must be 1..3",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True, nchannel=0), k.samples(), 0, None])),
    Raw("samples with tile", "submit", J2P_EINVAL, "job: sample input of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True, tile=1), k.samples(), 0, None])),
    Raw("samples with plane data set", "submit", J2P_EINVAL, "job: channel 0: a job with samples takes no data / fdata (both must be NULL)",
        lambda k: ("j2p_batch_submit_samples", [k.job(), k.samples(), 0, None])),
    Raw("samples with NULL data", "submit", J2P_EINVAL, "job: channel 1: samples: data is NULL",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(data={1: None}), 0, None])),
    Raw("samples wider than the plane", "submit", J2P_EINVAL, "job: channel 0: samples: 40x13 samples for a coefficient plane of 32x16",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(w={0: 40}), 0, None])),
    Raw("samples with stride 0", "submit", J2P_EINVAL, "job: channel 2: samples: strides must be at least 1",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(stride_x={2: 0}), 0, None])),
    Raw("samples in managed memory", "submit", J2P_EINVAL, "job: channel 0: samples: data is neither host nor plain device memory (managed memory is refused)",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(data={0: k.managed()}, w={0: 8}, h={0: 8}, stride_y={0: 8}), 0, None])),
    Raw("samples on two GPUs", "submit", J2P_EINVAL, "job: channel 1: samples live on device 1, others on device 0",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(device=0, data={1: k.samples(device=1)[1].data}), 0, None]), 2),
    Raw("samples with NULL data and 17 outputs: the samples first", "submit", J2P_EINVAL, "job: channel 1: samples: data is NULL",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True, **k.image()), k.samples(data={1: None}), *k.outputs(17)])),
    # JPEG output
    Raw("JPEG without a spec", "submit", J2P_EINVAL, "job: jpeg: spec is NULL",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image()), None, *k.jpeg(spec=False)])),
    Raw("JPEG from a file without a spec", "submit", J2P_EINVAL, "job: jpeg: spec is NULL",
        lambda k: ("j2p_batch_submit_file_jpeg", [k.job(bare=True), *k.file, *k.jpeg(spec=False)])),
    Raw("JPEG with out_bits", "submit", J2P_EINVAL, "job: a JPEG job needs out_bits 0, no out_coef and out_tensor.data NULL",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.rgb_out()), None, *k.jpeg()])),
    Raw("JPEG with tile", "submit", J2P_EINVAL, "job: JPEG output of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image(tile=1)), None, *k.jpeg()])),
    Raw("JPEG with sampling factor 3", "submit", J2P_EINVAL, "job: jpeg: sampling factors must be 1 or 2",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image()), None, *k.jpeg(sub_w=3)])),
    Raw("JPEG of two channels", "submit", J2P_EINVAL, "job: jpeg: three components or one",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image(nchannel=2)), None, *k.jpeg()])),
    Raw("JPEG whose size is not the image's", "submit", J2P_EINVAL, "job: the JPEG is 31x13, the job's image (out_w x out_h) 30x13",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image()), None, *k.jpeg(width=31)])),
    Raw("JPEG with size NULL", "submit", J2P_EINVAL, "job: JPEG output needs out and size",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(**k.image()), None, *k.jpeg(size=False)])),
    Raw("JPEG with out NULL and a capacity", "submit", J2P_EINVAL, "job: JPEG output needs out and size",
        lambda k: ("j2p_batch_submit_file_jpeg", [k.job(bare=True), *k.file, *k.jpeg(out=False)])),
    Raw("JPEG with out_bits from samples with NULL data: the JPEG first", "submit", J2P_EINVAL,
        "job: a JPEG job needs out_bits 0, no out_coef and out_tensor.data NULL",
        lambda k: ("j2p_batch_submit_jpeg", [k.job(bare=True, **k.rgb_out()), k.samples(data={1: None}), *k.jpeg()])),
    # file input
    Raw("a NULL file", "submit", J2P_EINVAL, "job: file is NULL or empty", lambda k: ("j2p_batch_submit_file", [k.job(bare=True), None, 100, 0, None])),
    Raw("an empty file", "submit", J2P_EINVAL, "job: file is NULL or empty", lambda k: ("j2p_batch_submit_file", [k.job(bare=True), k.file[0], 0, 0, None])),
    Raw("a NULL file and no spec: the file first", "submit", J2P_EINVAL, "job: file is NULL or empty",
        lambda k: ("j2p_batch_submit_file_jpeg", [k.job(bare=True), None, 100, *k.jpeg(spec=False)])),
    Raw("an empty file to a JPEG", "submit", J2P_EINVAL, "job: file is NULL or empty",
        lambda k: ("j2p_batch_submit_file_jpeg", [k.job(bare=True), k.file[0], 0, *k.jpeg()])),
    Raw("file with tile", "submit", J2P_EINVAL, "job: file input of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True, tile=1), *k.file, 0, None])),
    Raw("file with tile to a JPEG with out_bits: the file first", "submit", J2P_EINVAL, "job: file input of a row-tiled job is not supported",
        lambda k: ("j2p_batch_submit_file_jpeg", [k.job(bare=True, **k.rgb_out(tile=1)), *k.file, *k.jpeg()])),
    Raw("a file that is no JPEG", "submit", J2P_EFORMAT, "jpeg: not a JPEG file (no SOI marker)",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True), k.garbage.ctypes.data, k.garbage.size, 0, None])),
    Raw("two channels for a three-component file", "submit", J2P_EINVAL, "job: 2 channels for a file of 3 components (all of them, or 1 for component 0 alone)",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True, nchannel=2), *k.file, 0, None])),
    Raw("file with plane data set", "submit", J2P_EINVAL, "job: channel 0: a job with a file takes no data / fdata (both must be NULL)",
        lambda k: ("j2p_batch_submit_file", [k.job(), *k.file, 0, None])),
    Raw("a plane size that is not the file's", "submit", J2P_EINVAL, "job: channel 0: the plane is 40x16, the file's component 32x16",
        lambda k: ("j2p_batch_submit_file", [_wide_plane(k), *k.file, 0, None])),
    # NULL arguments
    Raw("a NULL job", "submit", J2P_EINVAL, "NULL argument", lambda k: ("j2p_batch_submit", [None])),
    Raw("a NULL job with samples", "submit", J2P_EINVAL, "NULL argument", lambda k: ("j2p_batch_submit_samples", [None, k.samples(), 0, None])),
    # pins: the batch drives device 0 only
    Raw("a tensor on a GPU the batch does not drive", "submit", J2P_EINVAL, "job: the tensor lives on device 1, which this batch does not drive",
        lambda k: ("j2p_batch_submit", [k.job(**k.image(out_tensor=k.tensor(device=1)))]), 2),
    Raw("samples on a GPU the batch does not drive", "submit", J2P_EINVAL, "job: the samples live on device 1, which this batch does not drive",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True), k.samples(device=1), 0, None]), 2),
    Raw("a file on a GPU the batch does not drive", "submit", J2P_EINVAL, "job: the file lives on device 1, which this batch does not drive",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True), *k.file_on(1), 0, None]), 2),
    Raw("samples on one GPU, the tensor on another", "submit", J2P_EINVAL, "job: the samples live on device 1, the output tensor on device 0",
        lambda k: ("j2p_batch_submit_samples", [k.job(bare=True, **k.image(out_tensor=k.tensor())), k.samples(device=1), 0, None]), 2),
    Raw("the file on one GPU, the tensor on another", "submit", J2P_EINVAL, "job: the file lives on device 1, the output tensor on device 0",
        lambda k: ("j2p_batch_submit_file", [k.job(bare=True, **k.image(out_tensor=k.tensor())), *k.file_on(1), 0, None]), 2),
]


def _without_coef_1(k):
    out = k.coef_out()
    out["out_coef"][1] = None
    return k.job(**out)


def _with_zero_step(k):
    out = k.coef_out()
    out["out_quant"][0] = k.table_with_zero()
    return k.job(**out)


def _wide_plane(k):
    job = k.job(bare=True)
    job._obj.planes[0].w = 40
    return job


# ---- Batch.submit's own refusals: the keywords on top of a three-plane job of WIDTH x HEIGHT ----

Python = namedtuple("Python", "name message keywords planes", defaults=("coefficients",))
GOOD_OUTPUT = {"out_width": 7, "out_height": 5, "filter": "triangle"}
TABLES = [np.ones(64, np.uint16)] * 3

PYTHON = [
    Python("file with samples", "job: file= excludes samples= and tile", dict(file=b"x", samples=[None] * 3)),
    Python("file with tile", "job: file= excludes samples= and tile", dict(file=b"x", tile=True)),
    Python("file with a resized tensor", "job: with file= a resized tensor is an output of outputs=", dict(file=b"x", box=(0, 0, 8, 8))),
    Python("file with planes that carry data", "job: with file= the planes carry neither data nor fdata", dict(file=jpeg_file())),
    Python("samples with tile", "job: samples= excludes tile", dict(samples=[None] * 3, tile=True)),
    Python("samples with a resized tensor", "job: with samples= a resized tensor is an output of outputs=", dict(samples=[None] * 3, filter="cubic")),
    Python("two sample arrays", "job: 2 sample arrays for 3 planes", dict(samples=[None] * 2)),
    Python("samples with planes that carry data", "job: with samples= the planes carry neither data nor fdata", dict(samples=[None] * 3)),
    Python("jpeg with bits", "job: jpeg= excludes bits, quant_tables, subsampling, tensor=, outputs=, out and tile", dict(jpeg={"quality": 90}, bits=8)),
    Python("jpeg with out", "job: jpeg= excludes bits, quant_tables, subsampling, tensor=, outputs=, out and tile", dict(jpeg={"quality": 90}, out=object())),
    Python("jpeg that is no dict", "job: jpeg= is a dict of quality or quant_tables, subsampling and capacity", dict(jpeg=90)),
    Python("jpeg with an unknown key", "job: jpeg= is a dict of quality or quant_tables, subsampling and capacity", dict(jpeg={"quality": 90, "size": 1})),
    Python("jpeg of two planes", "jpeg: three components or one", dict(jpeg={"quality": 90}), "two"),
    Python("outputs with tensor", "job: outputs= excludes tensor=, bits, quant_tables and tile", dict(outputs=[dict(GOOD_OUTPUT, tensor=object())], tensor=object())),
    Python("outputs with subsampling", "job: outputs= excludes tensor=, bits, quant_tables and tile",
           dict(outputs=[dict(GOOD_OUTPUT, tensor=object())], subsampling=[(1, 1)] * 3)),
    Python("outputs with a keyword of one output", "job: with outputs= every output carries its own keywords (out_width, out_height, box, filter, layout, scale, bias)",
           dict(outputs=[dict(GOOD_OUTPUT, tensor=object())], bias=1.0)),
    Python("outputs without a tensor", "job: every output of outputs= needs its tensor=", dict(outputs=[dict(GOOD_OUTPUT)])),
    Python("outputs whose dtype is not the tensor's", "tensor output: tensor is None, dtype says float32",
           dict(outputs=[dict(GOOD_OUTPUT, tensor=object(), dtype="float32")])),
    Python("filter without tensor", "job: filter belongs to tensor output (tensor=)", dict(filter="cubic")),
    Python("out_width without tensor", "job: out_width, out_height and box belong to tensor output (tensor=)", dict(out_width=8)),
    Python("tensor with quant_tables", "job: tensor output and coefficient output (quant_tables) exclude each other", dict(tensor=object(), quant_tables=TABLES)),
    Python("tensor with bits", "job: tensor output needs bits = 0", dict(tensor=object(), bits=8)),
    Python("tensor with out", "job: tensor output is written into `tensor`; out is for host arrays", dict(tensor=object(), out=object())),
    Python("layout without tensor", "job: layout, scale and bias belong to tensor output (tensor=)", dict(layout="hwc")),
    Python("scale with quant_tables", "job: layout, scale and bias belong to tensor output (tensor=)", dict(scale=2.0, quant_tables=TABLES)),
    Python("quant_tables with bits", "job: coefficient output (quant_tables) needs bits = 0", dict(quant_tables=TABLES, bits=8)),
    Python("two quant_tables", "job: one quantisation table per plane", dict(quant_tables=TABLES[:2])),
    Python("quant_tables without width", "job: coefficient output needs width and height", dict(quant_tables=TABLES, width=None)),
    Python("two subsampling pairs", "job: one (sx, sy) pair per plane", dict(quant_tables=TABLES, subsampling=[(1, 1)] * 2)),
    Python("a quant table of 63 entries", "job: a quantisation table has 64 entries", dict(quant_tables=[np.ones(64, np.uint16)] * 2 + [np.ones(63, np.uint16)])),
    Python("coefficient out of the wrong kind", "out must be a list of 3 writeable C-contiguous int16 arrays of shapes [(2, 4, 64), (1, 2, 64), (1, 2, 64)]",
           dict(quant_tables=TABLES, subsampling=[(1, 1), (2, 2), (2, 2)], out=[np.zeros((2, 4, 64), np.int16)] * 3)),
    Python("subsampling without quant_tables", "job: subsampling needs coefficient output (quant_tables)", dict(subsampling=[(1, 1)] * 3)),
    Python("bits 12", "job: out_bits must be 0, 8 or 16", dict(bits=12)),
    Python("bits of two planes", "job: sample output needs three planes (RGB) or one (greyscale)", dict(bits=8), "two"),
    Python("sample out of the wrong shape", "out must be a writeable C-contiguous (13, 30, 3) array of 1-byte integers for bits = 8",
           dict(bits=8, out=np.zeros((13, 30), np.uint8))),
]
