"""Every legal (input kind, output kind) pair that Batch.submit offers, joint and separate, on the smallest job that takes every path
(job_refusal_cases: 4:2:0, luma 32x16, chroma 16x8, image 30x13, 2 iterations): each result is bit-equal to what the corresponding
Solver / Solver.from_samples / Solver.from_jpeg instances give after the same iterations, read with download / coefficients /
to_tensor / to_tensors / to_jpeg.  A separate job is three one-plane solvers; where a Solver method reads one solver only (the
tensor forms), the library call behind that method is made with one plane of each."""
import ctypes

import numpy as np
import pytest

import job_refusal_cases as rc

W, H, N = rc.WIDTH, rc.HEIGHT, rc.ITERATIONS
INPUTS = ("planes", "samples", "file")
BOX = dict(out_width=10, out_height=5, box=(3, 2, 20, 10))                  # area form
CUBIC = dict(out_width=40, out_height=9, filter="cubic")                    # filtered, enlarging in x
SUBS = [(1, 1), (2, 2), (2, 2)]
JPEG = dict(quality=90, subsampling=(2, 2))


def output_specs(torch):
    return [dict(out_width=8, out_height=6, filter="triangle"),
            dict(out_width=40, out_height=20, filter="cubic", box=(3, 2, 20, 10), layout="hwc", dtype=torch.float16)]


def tables():
    return [p.quant_table for p in rc.planes()]


def grid(sub):
    """(blocks_w, blocks_h) of a channel's coefficient output at that subsampling"""
    return -(-4 // sub[0]), -(-2 // sub[1])


class Source:
    """one input kind: the planes and keywords of its jobs, and the solvers that are those jobs' solves"""

    def __init__(self, j, torch, kind):
        self.j, self.kind = j, kind
        full = rc.planes()
        self.planes, self.keywords = (full, {}) if kind == "planes" else (rc.bare_planes(), None)
        if kind == "samples":
            self.samples = [torch.from_numpy(a).cuda() for a in rc.samples()]
            torch.cuda.synchronize()
            self.keywords = dict(samples=self.samples)
        if kind == "file":
            # the project's own encoder makes the file
            self.file = j.entropy_encode([p.data.reshape(p.h // 8, p.w // 8, 64) for p in full], W, H, tables(), (2, 2))
            self.keywords = dict(file=self.file)

    def solvers(self, separate):
        """run: the one joint solver, or one per plane"""
        j = self.j
        if not separate:
            if self.kind == "planes":
                ss = [j.Solver(self.planes, rc.WEIGHT, rc.PWEIGHT, N)]
            elif self.kind == "samples":
                ss = [j.Solver.from_samples(self.samples, self.planes, rc.WEIGHT, rc.PWEIGHT, N)]
            else:
                ss = [j.Solver.from_jpeg(self.file, rc.WEIGHT, rc.PWEIGHT, N)]
        elif self.kind == "samples":
            ss = [j.Solver.from_samples([self.samples[c]], [p], rc.WEIGHT, [rc.PWEIGHT[c]], N) for c, p in enumerate(self.planes)]
        else:
            # (a file's one-plane solver is the solver of that component's decoded coefficients: from_jpeg always takes them all)
            data = [p.data for p in self.planes] if self.kind == "planes" else [a.reshape(-1) for a in j.entropy_decode(self.file)]
            ss = [j.Solver([j.Plane(p.w, p.h, p.w_samp, p.h_samp, data[c], p.quant_table)], rc.WEIGHT, [rc.PWEIGHT[c]], N)
                  for c, p in enumerate(self.planes)]
        for s in ss:
            s.run(N)
            s.sync()
        return ss


def tensors_of_three(j, torch, ss, specs=None, eight_bit=False):
    """the tensor(s) of specs — None (the image; eight_bit: as uint8 "hwc" samples), a j2p_resize, a j2p_resample, or a list of
    output dicts (one call) — from channel 0 of three solvers: the calls behind Solver.to_tensor / to_tensors with one plane of each"""
    lib = j.load_library()
    refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(s._h, 0) for s in ss])

    def new(w, h, layout="chw", dtype=torch.float32):
        return torch.zeros((3, h, w) if layout == "chw" else (h, w, 3), dtype=dtype, device="cuda")

    if isinstance(specs, list):
        rs = [j._output_spec(W, H, o, "out") for o in specs]
        out = [new(r.out_w, r.out_h, o.get("layout", "chw"), o.get("dtype", torch.float32)) for o, r in zip(specs, rs)]
        items = (j._COutput * len(specs))()
        for i, (o, r) in enumerate(zip(specs, rs)):
            items[i].r, items[i].t = r, j._c_tensor(out[i], 3, r.out_w, r.out_h, o.get("layout", "chw"), None, None)
        torch.cuda.synchronize()
        j._check(lib.j2p_planes_to_tensors_resampled(refs, 3, W, H, len(specs), items))
    elif specs is None:
        dtype, layout = (torch.uint8, "hwc") if eight_bit else (torch.float32, "chw")
        out = new(W, H, layout, dtype)
        ct = j._c_tensor(out, 3, W, H, layout, None, None)
        torch.cuda.synchronize()
        j._check(lib.j2p_planes_rows_to_tensor(refs, 3, W, 0, H, ctypes.byref(ct)))
    else:
        out = new(specs.out_w, specs.out_h)
        ct = j._c_tensor(out, 3, specs.out_w, specs.out_h, "chw", None, None)
        call = lib.j2p_planes_to_tensor_resampled if isinstance(specs, j._CResample) else lib.j2p_planes_to_tensor_resized
        torch.cuda.synchronize()
        j._check(call(refs, 3, W, H, ctypes.byref(specs), ctypes.byref(ct)))
    ss[0].sync()
    return out


def reference(j, torch, source, separate):
    """{output form: what the Solver instances give}"""
    ss = source.solvers(separate)
    one = ss[0]
    at = (lambda c: (ss[c], 0)) if separate else (lambda c: (one, c))
    want = {"float planes": [at(c)[0].download(at(c)[1]) for c in range(3)],
            "coefficients": [at(c)[0].coefficients(at(c)[1], tables()[c], *grid((1, 1))) for c in range(3)],
            "subsampled coefficients": [at(c)[0].coefficients(at(c)[1], tables()[c], *grid(SUBS[c]), subsampling=SUBS[c]) for c in range(3)],
            "jpeg": one.to_jpeg(W, H, others=ss[1:], **JPEG)}
    if separate:
        want["8-bit samples"] = tensors_of_three(j, torch, ss, eight_bit=True)
        want["tensor"] = tensors_of_three(j, torch, ss)
        want["tensor, box and area"] = tensors_of_three(j, torch, ss, j._c_resize(W, H, BOX["out_width"], BOX["out_height"], BOX["box"]))
        want["tensor, cubic"] = tensors_of_three(j, torch, ss, j._c_resample(W, H, CUBIC["out_width"], CUBIC["out_height"], None, j.FILTERS["cubic"]))
        want["two outputs"] = tensors_of_three(j, torch, ss, output_specs(torch))
    else:
        want["8-bit samples"] = one.to_tensor(W, H, dtype=torch.uint8, layout="hwc")
        want["tensor"] = one.to_tensor(W, H)
        want["tensor, box and area"] = one.to_tensor(W, H, **BOX)
        want["tensor, cubic"] = one.to_tensor(W, H, **CUBIC)
        want["two outputs"] = one.to_tensors(W, H, output_specs(torch))
    torch.cuda.synchronize()
    want = {k: flat(v) for k, v in want.items()}
    for s in ss:
        s.close()
    return want


def flat(v):
    """a result as a list of (shape, dtype, bytes)"""
    items = v if isinstance(v, list) else [v]
    out = []
    for a in items:
        if isinstance(a, bytes):
            out.append(((len(a),), "bytes", a))
            continue
        a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
        out.append((a.shape, str(a.dtype), np.ascontiguousarray(a).tobytes()))
    return out


def jobs(j, torch, b, source, separate):
    """{output form: what wait() returns}, every form of the input kind in flight together; and what each job was given to fill"""
    args = (source.planes, rc.WEIGHT, rc.PWEIGHT, N)
    kw = dict(source.keywords, separate=separate, width=W, height=H)
    given = {"tensor": torch.zeros((3, H, W), device="cuda"),
             "two outputs": [torch.zeros((3, 6, 8), device="cuda"), torch.zeros((20, 40, 3), dtype=torch.float16, device="cuda")],
             "8-bit samples": np.zeros((H, W, 3), np.uint8)}
    tickets = {"float planes": b.submit(*args, **dict(source.keywords, separate=separate)),
               "8-bit samples": b.submit(*args, bits=8, out=given["8-bit samples"], **kw),
               "coefficients": b.submit(*args, quant_tables=tables(), **kw),
               "subsampled coefficients": b.submit(*args, quant_tables=tables(), subsampling=SUBS, **kw),
               "tensor": b.submit(*args, tensor=given["tensor"], **kw),
               "two outputs": b.submit(*args, outputs=[dict(o, tensor=t) for o, t in zip(output_specs(torch), given["two outputs"])], **kw),
               "jpeg": b.submit(*args, jpeg=JPEG, **kw)}
    if source.kind == "planes":
        # (samples= and file= refuse a resized tensor outside outputs=)
        given["tensor, box and area"] = torch.zeros((3, 5, 10), device="cuda")
        given["tensor, cubic"] = torch.zeros((3, 9, 40), device="cuda")
        tickets["tensor, box and area"] = b.submit(*args, tensor=given["tensor, box and area"], **BOX, **kw)
        tickets["tensor, cubic"] = b.submit(*args, tensor=given["tensor, cubic"], **CUBIC, **kw)
    return {k: b.wait(t) for k, t in tickets.items()}, given


@pytest.fixture(scope="module")
def batch(lib):
    import jpeg2png_amd as j
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        yield b


@pytest.mark.gpu
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
@pytest.mark.parametrize("kind", INPUTS)
def test_every_output_form_equals_the_solvers(lib, batch, kind, separate):
    import torch
    import jpeg2png_amd as j
    source = Source(j, torch, kind)
    got, given = jobs(j, torch, batch, source, separate)
    want = reference(j, torch, source, separate)
    assert len(got) == (9 if kind == "planes" else 7)
    for form, result in got.items():
        have = flat(result)
        assert [(s, d) for s, d, _ in have] == [(s, d) for s, d, _ in want[form]], f"{kind}, {form}"
        assert [x for _, _, x in have] == [x for _, _, x in want[form]], f"{kind}, {form}: not bit-equal"
    # wait() hands back the caller's own array and tensors
    for form, mine in given.items():
        if isinstance(mine, list):
            assert len(got[form]) == len(mine) and all(a is b for a, b in zip(got[form], mine)), form
        else:
            assert got[form] is mine, form
    assert got["jpeg"][:2] == b"\xff\xd8" and bool(got["tensor"].any())
