"""Sample input on the GPU (k_samples_to_coefficients, j2p_solver_create_from_samples, Solver.from_samples, the samples= keyword of
Batch.submit).  The shared cases (tests/samples_cases.py) recover their own coefficients on the CPU (tests/test_samples_cpu.py), so
the coefficients a solver made from their 8-bit samples holds must EQUAL the cases' `data`, from every memory and stride form; and
the solve of such a solver must equal, as raw bits, the solve of the solver made from those coefficients.  Where the samples are
not a decoded file's (cropped, random, saturated) the truth is the restated definition.  Every case is a few blocks."""
import ctypes

import numpy as np
import pytest

import samples_cases as sc
from conftest import bit_equal

J2P_EINVAL = -1
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda(lib):
    import torch
    assert torch.cuda.is_available()
    return torch


def on_device(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def windowed(torch, a):
    """a as a window of a larger sentinel-filled tensor: odd base address, row stride w + 5 (never a multiple of 8 for the cases'
    widths, which are) — every lane takes the element loads.  Returns (buffer, view)."""
    h, w = a.shape
    pitch = w + 5
    buf = torch.full((h * pitch + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = 1 if buf.data_ptr() % 2 == 0 else 2
    view = buf[start:start + h * pitch].view(h, pitch)[:, :w]
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 2 == 1 and view.stride() == (pitch, 1) and pitch % 8
    return buf, view


def interleaved(torch, cb, cr):
    """the two chroma planes as the halves of one interleaved UV tensor (NV12's second plane): stride_x == 2"""
    uv = torch.from_numpy(np.ascontiguousarray(np.stack([cb, cr], axis=-1))).cuda()
    assert uv[:, :, 0].stride() == (2 * cb.shape[1], 2)
    return uv, uv[:, :, 0], uv[:, :, 1]


FORMS = ("device", "host", "window", "interleaved_uv", "cpu_tensor")
# an interleaved UV plane needs two chroma planes of one size: every colour case has them, the luma-only fixtures have none
COLOUR = [n for n in sc.NAMES if len(sc.case(n).planes) == 3 and (sc.case(n).planes[1].w, sc.case(n).planes[1].h) == (sc.case(n).planes[2].w, sc.case(n).planes[2].h)]
COEFFICIENT_CASES = [(n, f) for n in sc.NAMES for f in FORMS if f != "interleaved_uv" or n in COLOUR]


def inputs(torch, case, form):
    """(what must stay alive, the samples argument) of a case in one of the forms"""
    s = case.samples
    if form == "device":
        t = [on_device(torch, a) for a in s]
        return t, t
    if form == "host":
        return None, [np.array(a) for a in s]
    if form == "cpu_tensor":
        t = [torch.from_numpy(np.array(a)) for a in s]
        return t, t
    if form == "window":
        made = [windowed(torch, a) for a in s]
        return made, [v for _, v in made]
    uv, cb, cr = interleaved(torch, s[1], s[2])
    return uv, [on_device(torch, s[0]), cb, cr]


def data_of(p):
    return np.asarray(p.data, np.int16).reshape(p.h // 8, p.w // 8, 64)


# ---- 1. the coefficients ----

@pytest.mark.gpu
@pytest.mark.parametrize("name,form", COEFFICIENT_CASES, ids=[f"{n}-{f}" for n, f in COEFFICIENT_CASES])
def test_coefficients_equal_the_cases_own(torch_cuda, name, form):
    import jpeg2png_amd as j
    torch = torch_cuda
    case = sc.case(name)
    keep, samples = inputs(torch, case, form)
    before = [buf.clone() for buf, _ in keep] if form == "window" else None
    with j.Solver.from_samples(samples, case.bare_planes(), case.weight, case.pweight[:len(case.planes)], case.iterations) as s:
        for c, p in enumerate(case.planes):
            got = s.download_coefficients(c)
            assert got.shape == data_of(p).shape and got.dtype == np.int16
            assert np.array_equal(got, data_of(p)), f"{name}, {form}, channel {c}: {int((got != data_of(p)).sum())} coefficients differ"
            assert s.clipped_samples(c) == 0
    if form == "window":
        torch.cuda.synchronize()
        for (buf, view), was in zip(keep, before):                  # the samples and what surrounds them were only read
            assert torch.equal(buf, was)


def test_every_colour_case_takes_the_interleaved_form():
    assert len(COLOUR) == 8 and len(COEFFICIENT_CASES) == 4 * len(sc.NAMES) + len(COLOUR)


# ---- 2. the solve ----

@pytest.fixture(scope="module")
def coefficient_solves(lib):
    """per SOLVED fixture what the coefficient-built solver gives: planes after the fixture's iterations and what it reports —
    computed once, left unchanged"""
    import jpeg2png_amd as j
    out = {}
    for name in sc.SOLVED:
        case = sc.case(name)
        n = len(case.planes)
        with j.Solver(case.coefficient_planes(), case.weight, case.pweight[:n], case.iterations) as s:
            s.run(case.iterations)
            planes = [s.download(c) for c in range(n)]
            for a in planes:
                a.setflags(write=False)
            out[name] = (planes, [(s.coefficient_bytes(c), s.shares_state(c), s.wide_footprint(c)) for c in range(n)], (s.W, s.H))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("device", "host"))
@pytest.mark.parametrize("name", sc.SOLVED)
def test_solve_equals_the_coefficient_built_solvers_bit_for_bit(torch_cuda, coefficient_solves, name, form):
    import jpeg2png_amd as j
    case = sc.case(name)
    n = len(case.planes)
    want, reports, canvas = coefficient_solves[name]
    keep, samples = inputs(torch_cuda, case, form)
    with j.Solver.from_samples(samples, case.bare_planes(), case.weight, case.pweight[:n], case.iterations) as s:
        assert (s.W, s.H) == canvas
        assert [(s.coefficient_bytes(c), s.shares_state(c), s.wide_footprint(c)) for c in range(n)] == reports
        for again in range(2):
            s.run(case.iterations)
            for c in range(n):
                assert bit_equal(s.download(c), want[c]), f"{name}, {form}, channel {c}, {'after reset' if again else 'first run'}"
            s.reset()
        # the planes of iteration 0 are the library's own decode of the recovered coefficients
        with j.Solver(case.coefficient_planes(), case.weight, case.pweight[:n], case.iterations) as ref:
            for c in range(n):
                assert bit_equal(s.download(c), ref.download(c))


# ---- 3. replication, widths, clipped counts: against the restatement ----

def check_against_restatement(j, samples_arg, host_samples, planes, label):
    with j.Solver.from_samples(samples_arg, planes, 0.3, [0.001] * len(planes), 2) as s:
        for c, (p, a) in enumerate(zip(planes, host_samples)):
            got = s.download_coefficients(c)
            want = sc.expected_coefficients(a, p.w, p.h, p.quant_table)
            assert np.array_equal(got, want), f"{label}, channel {c}: {int((got != want).sum())} of {want.size} coefficients differ"
            assert s.clipped_samples(c) == sc.clipped(a), f"{label}, channel {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("device", "host", "window"))
@pytest.mark.parametrize("crop", ("w-3_h-5", "1x1"))
def test_missing_columns_and_rows_are_replicated(torch_cuda, crop, form):
    """compared with the restatement, not with the case: the encoder's padding is not the decoder's"""
    import jpeg2png_amd as j
    torch = torch_cuda
    case = sc.case("synth_420_72x40_q30")                     # luma 72x40: 9 blocks per row, so the wavefront's spare lanes too
    planes = case.bare_planes()
    host = [np.array(a[:1, :1] if crop == "1x1" else a[:a.shape[0] - 5, :a.shape[1] - 3]) for a in case.samples]
    if form == "device":
        arg = [on_device(torch, a) for a in host]
    elif form == "window":
        keep = [windowed(torch, a) for a in host]
        arg = [v for _, v in keep]
    else:
        arg = host
    check_against_restatement(j, arg, host, planes, f"{crop}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", (8, 9, 56, 64, 72))
def test_widths_around_a_wavefronts_and_a_workgroups_blocks(torch_cuda, blocks):
    """below, at and across the 8 blocks of a wavefront and the 32 of a workgroup; two block rows; random samples over the whole
    byte range, so the clipped count is checked too — also with the last 3 columns and 5 rows missing, where the replicated
    samples must not be counted"""
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    torch = torch_cuda
    rng = np.random.default_rng(blocks)
    w, h = blocks * 8, 16
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    a[rng.random((h, w)) < 0.1] = 255
    a[rng.random((h, w)) < 0.1] = 0
    q = rng.integers(1, 64, 64).astype(np.uint16)
    planes = [Plane(w, h, 1, 1, None, q)]
    assert sc.clipped(a) > 0
    for label, host in (("whole", a), ("cropped", np.array(a[:h - 5, :w - 3]))):
        check_against_restatement(j, [on_device(torch, host)], [host], planes, f"{blocks} blocks, {label}, device")
        check_against_restatement(j, [host], [host], planes, f"{blocks} blocks, {label}, host")
        keep, view = windowed(torch, host)
        check_against_restatement(j, [view], [host], planes, f"{blocks} blocks, {label}, window")


@pytest.mark.gpu
@pytest.mark.parametrize("value,dc", [(0, -1024), (255, 1016)])
def test_saturated_planes_reach_the_ends_of_the_range(torch_cuda, value, dc):
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    w, h = 72, 24
    a = np.full((h, w), value, np.uint8)
    for arg in ([on_device(torch_cuda, a)], [a]):
        with j.Solver.from_samples(arg, [Plane(w, h, 1, 1, None, np.ones(64, np.uint16))], 0.3, [0.001], 1) as s:
            got = s.download_coefficients(0)
            assert (got[..., 0] == dc).all() and not got[..., 1:].any()
            assert s.clipped_samples(0) == w * h
            assert s.coefficient_bytes(0) == 2                # beyond a byte: not narrowed


# ---- 4. refusals ----

@pytest.mark.gpu
def test_refusals_leave_no_solver(torch_cuda):
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    torch = torch_cuda
    lib = j.load_library()
    case = sc.case("y_48x40_tgv")
    p = case.planes[0]
    a = case.samples[0]
    bare = case.bare_planes()
    t = on_device(torch, a)
    torch.cuda.synchronize()
    with pytest.raises(j.J2PError, match="data / fdata"):
        j.Solver.from_samples([t], [Plane(p.w, p.h, 1, 1, p.data, p.quant_table)], 0.3, [0.001], 2)
    with pytest.raises(j.J2PError, match="at least 1"):
        j.Solver.from_samples([t[:, :1].expand(p.h, p.w)], bare, 0.3, [0.001], 2)                       # stride_x 0
    with pytest.raises(j.J2PError, match="at least 1"):
        j.Solver.from_samples([np.broadcast_to(a[:1], a.shape)], bare, 0.3, [0.001], 2)                  # stride_y 0
    with pytest.raises(j.J2PError, match="samples for a coefficient plane"):
        j.Solver.from_samples([on_device(torch, np.zeros((p.h, p.w + 1), np.uint8))], bare, 0.3, [0.001], 2)
    with pytest.raises(j.J2PError, match="samples for a coefficient plane"):
        j.Solver.from_samples([np.zeros((p.h + 1, p.w), np.uint8)], bare, 0.3, [0.001], 2)
    with pytest.raises(j.J2PError):
        j.Solver.from_samples([t.to(torch.float32)], bare, 0.3, [0.001], 2)
    with pytest.raises(j.J2PError):
        j.Solver.from_samples([t, t], bare, 0.3, [0.001], 2)

    # the C entry point: data set on the plane, and managed memory
    q = np.ascontiguousarray(p.quant_table, np.uint16)
    d = np.ascontiguousarray(p.data, np.int16)
    pw = (ctypes.c_float * 1)(0.001)

    def create(plane_data, ptr):
        cpl = (j._CPlane * 1)(j._CPlane(p.w, p.h, 1, 1, plane_data, None, q.ctypes.data))
        csm = (j._CSamples * 1)(j._CSamples(ptr, p.w, p.h, p.w, 1))
        h = ctypes.c_void_p(0xDEAD)
        return lib.j2p_solver_create_from_samples(ctypes.byref(h), 0, None, 1, cpl, csm, 0.3, pw, 2), h.value

    assert create(d.ctypes.data, t.data_ptr()) == (J2P_EINVAL, None)
    hip = j.hip_runtime()
    managed = ctypes.c_void_p()
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    if hip.hipMallocManaged(ctypes.byref(managed), a.nbytes, 1) == 0 and managed.value:
        assert create(None, managed.value) == (J2P_EINVAL, None)
        assert "managed" in lib.j2p_last_error().decode()
        hip.hipFree.argtypes = [ctypes.c_void_p]
        hip.hipFree(managed)
    if j.device_count() > 1:
        other = on_device(torch, a).to("cuda:1")
        torch.cuda.synchronize(1)
        assert create(None, other.data_ptr()) == (J2P_EINVAL, None)
    rc, h = create(None, t.data_ptr())                        # ... and the same call with nothing wrong
    assert rc == 0 and h
    lib.j2p_solver_destroy(h)
    with j.Solver(case.coefficient_planes(), 0.3, [0.001], 2) as s:
        with pytest.raises(j.J2PError, match="not made from samples"):
            s.clipped_samples(0)
        assert np.array_equal(s.download_coefficients(0), data_of(p))      # any solver's coefficients can be read


# ---- 5. the batch engine ----

@pytest.mark.gpu
def test_batch_sample_jobs_and_coefficient_jobs_in_flight_together(torch_cuda):
    import jpeg2png_amd as j
    torch = torch_cuda
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = []
        for name in sc.SOLVED:
            case = sc.case(name)
            n = len(case.planes)
            args = (case.weight, case.pweight[:n], case.iterations)
            dev = [on_device(torch, a) for a in case.samples]
            tickets.append((name, "coefficients", b.submit(case.coefficient_planes(), *args, samples=None), None))
            tickets.append((name, "device samples", b.submit(case.bare_planes(), *args, samples=dev), dev))
            tickets.append((name, "host samples", b.submit(case.bare_planes(), *args, samples=[np.array(a) for a in case.samples]), None))
            tickets.append((name, "separate", b.submit(case.coefficient_planes(), *args, separate=True), None))
            tickets.append((name, "separate, device samples", b.submit(case.bare_planes(), *args, separate=True, samples=dev), dev))
        got = {(name, kind): b.wait(t) for name, kind, t, _ in tickets}
    for name in sc.SOLVED:
        for kind, truth in (("device samples", "coefficients"), ("host samples", "coefficients"), ("separate, device samples", "separate")):
            want, have = got[(name, truth)], got[(name, kind)]
            assert len(want) == len(have) == len(sc.case(name).planes)
            for c in range(len(want)):
                assert bit_equal(have[c], want[c]), f"{name}: {kind}, channel {c}"


@pytest.mark.gpu
def test_batch_sample_jobs_fill_the_same_tensors_and_samples(torch_cuda):
    import jpeg2png_amd as j
    torch = torch_cuda
    case = sc.case("rgb420_padded_40x20")
    W, H = 40, 20
    args = (case.weight, case.pweight, case.iterations)
    specs = [{"out_width": 24, "out_height": 16, "filter": "triangle"}, {"out_width": 50, "out_height": 30, "filter": "cubic", "box": (3, 2, 30, 15), "layout": "hwc"}]

    def tensors():
        return [torch.full((3, 16, 24), 7.0, device="cuda"), torch.full((30, 50, 3), 7.0, device="cuda")]

    dev = [on_device(torch, a) for a in case.samples]
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        jobs = {
            "coefficients": b.submit(case.coefficient_planes(), *args, width=W, height=H, outputs=[dict(o, tensor=t) for o, t in zip(specs, tensors())]),
            "device samples": b.submit(case.bare_planes(), *args, width=W, height=H, outputs=[dict(o, tensor=t) for o, t in zip(specs, tensors())], samples=dev),
            "host samples": b.submit(case.bare_planes(), *args, width=W, height=H, outputs=[dict(o, tensor=t) for o, t in zip(specs, tensors())],
                                     samples=[np.array(a) for a in case.samples]),
        }
        one = {"coefficients": b.submit(case.coefficient_planes(), *args, width=W, height=H, tensor=torch.zeros((3, H, W), device="cuda")),
               "device samples": b.submit(case.bare_planes(), *args, width=W, height=H, tensor=torch.zeros((3, H, W), device="cuda"), samples=dev)}
        rgb = {"coefficients": b.submit(case.coefficient_planes(), *args, width=W, height=H, bits=8),
               "host samples": b.submit(case.bare_planes(), *args, width=W, height=H, bits=8, samples=[np.array(a) for a in case.samples])}
        got = {k: [t.cpu().numpy() for t in b.wait(v)] for k, v in jobs.items()}
        got_one = {k: b.wait(v).cpu().numpy() for k, v in one.items()}
        got_rgb = {k: b.wait(v) for k, v in rgb.items()}
        # refused at submit
        with pytest.raises(j.J2PError, match="tile"):
            b.submit(case.bare_planes(), *args, samples=dev, tile=True)
        job = j._CJob()
        job.nchannel, job.tile = 3, 1
        csm, held, _ = j._c_samples(dev)
        cpl, keep = j._c_planes(case.bare_planes())
        for c in range(3):
            job.planes[c] = cpl[c]
        ticket = ctypes.c_int(-5)
        assert b._lib.j2p_batch_submit_samples(b._h, ctypes.byref(job), csm, 0, None, ctypes.byref(ticket)) == J2P_EINVAL and ticket.value == -5
        assert "row-tiled" in b._lib.j2p_last_error().decode()
        with pytest.raises(j.J2PError, match="data / fdata|neither data nor fdata"):
            b.submit(case.coefficient_planes(), *args, samples=dev)
        with pytest.raises(j.J2PError, match="at least 1"):
            b.submit(case.bare_planes(), *args, samples=[dev[0], dev[1], dev[2][:, :1].expand(dev[2].shape)])
    for k in ("device samples", "host samples"):
        for i in range(2):
            assert bit_equal(got[k][i], got["coefficients"][i]), f"{k}, output {i}"
            assert not (got[k][i] == 7.0).all()
    assert bit_equal(got_one["device samples"], got_one["coefficients"]) and got_one["coefficients"].any()
    assert np.array_equal(got_rgb["host samples"], got_rgb["coefficients"]) and got_rgb["coefficients"].shape == (H, W, 3)


# ---- 6. stream order ----

@pytest.mark.gpu
def test_samples_written_on_torchs_stream_just_before_the_call(torch_cuda):
    """the producer is queued on torch's current stream — behind enough work that it has not run when from_samples is called — and
    nothing synchronises: the solver's stream has to wait for it"""
    import jpeg2png_amd as j
    torch = torch_cuda
    case = sc.case("rgb422_48x32")
    src = [on_device(torch, a) for a in case.samples]
    dst = [torch.zeros_like(t) for t in src]
    big = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    for _ in range(6):
        big = big @ big * 1e-4
    for d, s in zip(dst, src):
        d.copy_(s)
    with j.Solver.from_samples(dst, case.bare_planes(), case.weight, case.pweight, case.iterations) as s:
        for c, p in enumerate(case.planes):
            assert np.array_equal(s.download_coefficients(c), data_of(p)), f"channel {c}"
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                              # ... and the same from a stream that is not the default one
        for _ in range(6):
            big = big @ big * 1e-4
        for d in dst:
            d.zero_()
        for d, s in zip(dst, src):
            d.copy_(s)
        with j.Solver.from_samples(dst, case.bare_planes(), case.weight, case.pweight, case.iterations) as s:
            for c, p in enumerate(case.planes):
                assert np.array_equal(s.download_coefficients(c), data_of(p)), f"channel {c}, side stream"
    torch.cuda.synchronize()


# ---- 7. the header of a file the command-line driver wrote ----

@pytest.mark.gpu
def test_header_of_a_file_the_driver_wrote(tmp_path, tmp_path_factory):
    """`-j 90 -S 420`: jpeg_header against libjpeg's reading of the file (the driver needs the GPU for its solve, hence here)"""
    import os
    import subprocess
    from test_jpeg_out_cli import PREFIX, ROOT, load_coefficients, make_jpeg, pil_tables, run
    from jpeg2png_amd.buildlib import build_cli
    import jpeg2png_amd as j
    exe = build_cli()
    if exe is None or not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        pytest.skip("libjpeg / libpng headers not available: the command-line driver was not built")
    rc_exe = str(tmp_path_factory.mktemp("rc") / "read_coefficients")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(PREFIX, "include"), os.path.join(ROOT, "tests", "c", "read_coefficients.c"),
                    "-o", rc_exe, os.path.join(PREFIX, "lib", "libjpeg.so"), "-Wl,-rpath," + os.path.join(PREFIX, "lib")], check=True)
    jpg, out = str(tmp_path / "in.jpg"), str(tmp_path / "out.jpg")
    make_jpeg(jpg, 101, 67, 30, 2, seed=4)
    r = run(exe, jpg, "-o", out, "-q", "-i", "4", "-j", "90", "-S", "420")
    assert r.returncode == 0, r.stderr
    w, h, planes = load_coefficients(rc_exe, out)
    got = j.jpeg_header(open(out, "rb").read())
    tables = pil_tables(rc_exe, tmp_path, 90, 3)
    assert (got["width"], got["height"]) == (w, h) == (101, 67)
    for c, (p, g) in enumerate(zip(planes, got["planes"])):
        assert (g.w, g.h, g.w_samp, g.h_samp) == (p.w, p.h, p.w_samp, p.h_samp), f"component {c}"
        assert np.array_equal(g.quant_table, tables[c]) and np.array_equal(g.quant_table, p.quant_table), f"component {c}"
    assert [(g.w_samp, g.h_samp) for g in got["planes"]] == [(1, 1), (2, 2), (2, 2)]
