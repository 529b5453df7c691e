"""Estimated tables on the GPU: the histogram kernel (k_samples_dct_histogram, j2p_samples_histogram) must EQUAL the restatement of
tests/estimate_cases.py — every bin, `blocks` and `excluded` — at the plane sizes where its work is divided (a wavefront's 8
blocks, a workgroup's 4 wavefronts, more groups than one launch's workgroups take in one turn), from every memory and stride form,
and where a counter could wrap or a bin could be missed; and a solver or a batch job made with quant="estimate" must be, bit for
bit, the one made with the tables the estimate returned."""
import ctypes

import numpy as np
import pytest

import estimate_cases as es
from conftest import bit_equal

J2P_EINVAL = -1


@pytest.fixture(scope="module")
def torch_cuda(lib, oracle):
    import torch
    assert torch.cuda.is_available()
    return torch


def noisy(w, h, seed):
    """bytes over the whole range — AC values on both sides of the LDS bins' bound — with some 0 and 255 for the exclusion"""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 255, (h, w)).astype(np.uint8)
    a[rng.random((h, w)) < 0.004] = 0
    a[rng.random((h, w)) < 0.004] = 255
    return a


def check(got, samples, label):
    hist, blocks, excluded = got
    want, want_blocks, want_excluded = es.histogram(samples)
    assert hist.shape == (64, 1024) and hist.dtype == np.uint32
    assert (blocks, excluded) == (want_blocks, want_excluded), label
    assert np.array_equal(hist, want), f"{label}: {int((hist != want).sum())} bins differ"
    assert (hist.sum(axis=1) == blocks).all(), label


# w x h: 7, 8 and 9 blocks across a wavefront's 8; 4 and 5 groups against a workgroup's 4; no complete block; odd edges
SIZES = [(1, 1), (7, 7), (8, 8), (9, 9), (15, 17), (63, 8), (64, 8), (72, 8), (8, 32), (8, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_histogram_equals_the_restatement_at_the_divisions_of_the_work(torch_cuda, w, h):
    import jpeg2png_amd as j
    a = noisy(w, h, 100 * w + h)
    check(j.samples_histogram(a), a, f"{w}x{h}, host")
    check(j.samples_histogram(torch_cuda.from_numpy(a).cuda()), a, f"{w}x{h}, device")


def test_complete_blocks_exist_in_the_small_cases_that_should_have_them(oracle):
    assert [es.histogram(noisy(w, h, 1))[1:] == (0, 0) for w, h in SIZES[:2]] == [True, True]
    assert es.histogram(np.full((17, 15), 9, np.uint8))[1] == 2 and es.histogram(np.full((40, 8), 9, np.uint8))[1] == 5


@pytest.mark.gpu
def test_strides_views_and_the_turns_of_the_grid(torch_cuda):
    import jpeg2png_amd as j
    torch = torch_cuda
    cb, cr = noisy(72, 24, 5), noisy(72, 24, 6)
    uv = torch.from_numpy(np.ascontiguousarray(np.stack([cb, cr], axis=-1))).cuda()              # NV12's second plane
    assert uv[:, :, 1].stride() == (144, 2)
    check(j.samples_histogram(uv[:, :, 0]), cb, "stride_x 2, device, first half")
    check(j.samples_histogram(uv[:, :, 1]), cr, "stride_x 2, device, second half")
    host_uv = np.ascontiguousarray(np.stack([cb, cr], axis=-1))
    check(j.samples_histogram(host_uv[:, :, 1]), cr, "stride_x 2, host")
    # a window of a larger tensor at an odd address with a row stride that is no multiple of 8: the element loads
    buf = torch.full((24 * 77 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    start = 1 if buf.data_ptr() % 2 == 0 else 2
    view = buf[start:start + 24 * 77].view(24, 77)[:, :72]
    view.copy_(torch.from_numpy(cb))
    before = buf.clone()
    check(j.samples_histogram(view), cb, "window, device")
    assert torch.equal(buf, before)
    check(j.samples_histogram(np.asfortranarray(cb)), cb, "column-major, host")                 # stride_y 1, stride_x 24
    check(j.samples_histogram(cb[::2, ::3]), np.ascontiguousarray(cb[::2, ::3]), "strided view, host")
    check(j.samples_histogram(torch.from_numpy(cb)), cb, "cpu tensor")
    # 16 x 130 = 2080 groups of 8 blocks: more than the 2048 a launch's 512 workgroups take in one turn
    big = noisy(1024, 1040, 7)
    check(j.samples_histogram(torch.from_numpy(big).cuda()), big, "1024x1040, device")


@pytest.mark.gpu
def test_flat_planes(torch_cuda):
    import jpeg2png_amd as j
    torch = torch_cuda
    # all 0: every block excluded, the histogram empty
    z = np.zeros((24, 72), np.uint8)
    for arg in (z, torch.from_numpy(z).cuda()):
        hist, blocks, excluded = j.samples_histogram(arg)
        assert (blocks, excluded) == (0, 27) and not hist.any()
    # value 1: the DC's last reachable bin
    one = np.full((16, 40), 1, np.uint8)
    hist, blocks, excluded = j.samples_histogram(torch.from_numpy(one).cuda())
    assert (blocks, excluded) == (10, 0) and hist[0, 1016] == 10 and (hist[1:, 0] == 10).all() and hist.sum() == 640
    check((hist, blocks, excluded), one, "flat 1")
    # 65536 and 262144 equal blocks (2048x2048, 4096x4096): a counter narrower than 32 bits anywhere on the way would wrap
    for side in (2048, 4096):
        n = (side // 8) ** 2
        flat = torch.full((side, side), 100, dtype=torch.uint8, device="cuda")
        hist, blocks, excluded = j.samples_histogram(flat)
        assert (blocks, excluded) == (n, 0)
        assert hist[0, 224] == n and (hist[1:, 0] == n).all() and int(hist.sum(dtype=np.uint64)) == 64 * n


@pytest.mark.gpu
def test_a_corpus_file_and_its_estimate(torch_cuda):
    import jpeg2png_amd as j
    for ch in es.corpus_file(200, 120, 75, "444")[1]:
        got = j.samples_histogram(torch_cuda.from_numpy(np.array(ch.samples)).cuda())
        check(got, ch.samples, ch.name)
        table, det, quality = j.estimate_quant_table(got[0], chroma=ch.chroma)
        assert det.any() and np.array_equal(table[det], ch.table[det]), ch.name


@pytest.mark.gpu
def test_histogram_refusals(torch_cuda):
    import jpeg2png_amd as j
    torch = torch_cuda
    lib = j.load_library()
    a = noisy(16, 16, 3)
    hist = np.empty((64, 1024), np.uint32)
    n, x = ctypes.c_ulonglong(), ctypes.c_ulonglong()

    def call(ptr, w=16, h=16, sy=16, sx=1, samples=True, out=hist.ctypes.data):
        csm = (j._CSamples * 1)(j._CSamples(ptr, w, h, sy, sx))
        return lib.j2p_samples_histogram(0, None, csm if samples else None, out, ctypes.byref(n), ctypes.byref(x))

    assert call(a.ctypes.data) == 0 and n.value + x.value == 4
    for kw in ({"samples": False}, {"out": None}, {"w": 0}, {"h": 0}, {"sy": 0}, {"sx": 0}, {"sx": -1}):
        assert call(a.ctypes.data, **kw) == J2P_EINVAL, kw
    assert call(None) == J2P_EINVAL
    hip = j.hip_runtime()
    managed = ctypes.c_void_p()
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    if hip.hipMallocManaged(ctypes.byref(managed), a.nbytes, 1) == 0 and managed.value:
        assert call(managed.value) == J2P_EINVAL and "managed" in lib.j2p_last_error().decode()
        hip.hipFree.argtypes = [ctypes.c_void_p]
        hip.hipFree(managed)
    with pytest.raises(j.J2PError):
        j.samples_histogram(torch.from_numpy(a).cuda().to(torch.float32))


# ---- the solver and the batch ----

@pytest.fixture(scope="module")
def case_420(torch_cuda):
    """64x48 4:2:0 at quality 50: planes without arrays or tables, and the samples a decoder would hand over"""
    import samples_cases as sc
    from jpeg2png_amd import synth
    from jpeg2png_amd.synth import Plane
    planes = synth.make_planes(64, 48, "420", 50, seed=21)
    samples = [sc.plane_samples(p) for p in planes]
    bare = [Plane(p.w, p.h, p.w_samp, p.h_samp, None, None) for p in planes]
    return bare, samples


def with_tables(bare, tables):
    from jpeg2png_amd.synth import Plane
    return [Plane(p.w, p.h, p.w_samp, p.h_samp, None, t) for p, t in zip(bare, tables)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("device", "host"))
def test_estimating_solver_equals_the_solver_given_its_tables(torch_cuda, case_420, form):
    import jpeg2png_amd as j
    bare, samples = case_420
    arg = [torch_cuda.from_numpy(a).cuda() for a in samples] if form == "device" else samples
    with j.Solver.from_samples(arg, bare, 0.3, [0.001] * 3, 10, quant="estimate") as s:
        triples = s.estimated_tables
        assert len(triples) == 3
        for c, (table, det, quality) in enumerate(triples):
            want = es.estimate(es.histogram(samples[c])[0], chroma=c > 0)
            assert np.array_equal(table, want[0]) and np.array_equal(det, want[1]) and quality == want[2], f"channel {c}"
        s.run(10)
        got = [s.download(c) for c in range(3)]
    with j.Solver.from_samples(arg, with_tables(bare, [t for t, _, _ in triples]), 0.3, [0.001] * 3, 10) as s:
        assert s.estimated_tables is None
        s.run(10)
        for c in range(3):
            assert bit_equal(got[c], s.download(c)), f"channel {c}"
    # tables given in every plane are ignored; in some planes only, refused
    ones = [np.ones(64, np.uint16)] * 3
    with j.Solver.from_samples(arg, with_tables(bare, ones), 0.3, [0.001] * 3, 10, quant="estimate") as s:
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(s.estimated_tables, triples))
    with pytest.raises(j.J2PError, match="some planes"):
        j.Solver.from_samples(arg, with_tables(bare, [ones[0], None, None]), 0.3, [0.001] * 3, 10, quant="estimate")
    with pytest.raises(j.J2PError, match="quant="):
        j.Solver.from_samples(arg, bare, 0.3, [0.001] * 3, 10, quant="guess")


@pytest.mark.gpu
def test_estimating_batch_job_equals_the_job_given_its_tables(torch_cuda, case_420):
    import jpeg2png_amd as j
    bare, samples = case_420
    dev = [torch_cuda.from_numpy(a).cuda() for a in samples]
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        t_host = b.submit(bare, 0.3, [0.001] * 3, 10, samples=samples, quant="estimate")
        t_dev = b.submit(bare, 0.3, [0.001] * 3, 10, samples=dev, quant="estimate")
        got_host, got_dev = b.wait(t_host), b.wait(t_dev)
        triples = b.estimated_tables(t_host)
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(triples, b.estimated_tables(t_dev)))
        want = b.wait(b.submit(with_tables(bare, [t for t, _, _ in triples]), 0.3, [0.001] * 3, 10, samples=samples))
    for c in range(3):
        assert np.array_equal(triples[c][0], es.estimate(es.histogram(samples[c])[0], chroma=c > 0)[0]), f"channel {c}"
        assert bit_equal(got_host[c], want[c]) and bit_equal(got_dev[c], want[c]), f"channel {c}"


@pytest.mark.gpu
def test_batch_refusals_queue_nothing(torch_cuda, case_420):
    import jpeg2png_amd as j
    bare, samples = case_420
    ones = np.ones(64, np.uint16)
    alive = []
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        def submit(planes, tile=0, with_samples=True):
            job = j._CJob()
            job.nchannel, job.tile = 3, tile
            cpl, keep = j._c_planes(planes)
            for c in range(3):
                job.planes[c] = cpl[c]
                job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 2
            out = [np.empty((48, 64), np.float32) for _ in range(3)]
            for c in range(3):
                job.out_planes[c] = out[c].ctypes.data
            csm, held, _ = j._c_samples(samples)
            ticket = ctypes.c_int(-5)
            rc = b._lib.j2p_batch_submit_samples_estimated(b._h, ctypes.byref(job), csm if with_samples else None, 0, None, None, ctypes.byref(ticket))
            # (what an accepted job points into has to outlive the call: the worker fills `out` until j2p_batch_wait)
            alive.append((job, cpl, keep, out, csm, held))
            return rc, ticket.value, b._lib.j2p_last_error().decode()

        rc, ticket, err = submit(bare, tile=1)
        assert (rc, ticket) == (J2P_EINVAL, -5) and "row-tiled" in err
        rc, ticket, err = submit(bare, with_samples=False)
        assert (rc, ticket) == (J2P_EINVAL, -5) and "need samples" in err
        rc, ticket, err = submit(with_tables(bare, [ones, None, ones]))
        assert (rc, ticket) == (J2P_EINVAL, -5) and "2 of 3 planes" in err
        # ... and through Python
        for kw in ({"samples": samples, "tile": True}, {"samples": None}, {"samples": samples, "jpeg": {"quality": 90}}):
            with pytest.raises(j.J2PError) as e:
                b.submit(bare, 0.3, [0.001] * 3, 2, quant="estimate", width=64, height=48, **kw)
            assert e.value.code == J2P_EINVAL
        with pytest.raises(j.J2PError, match="some planes"):
            b.submit(with_tables(bare, [ones, None, ones]), 0.3, [0.001] * 3, 2, samples=samples, quant="estimate")
        assert not b._pending and not b._estimates
        # the same call with nothing wrong
        rc, ticket, _ = submit(bare)
        assert rc == 0 and ticket > 0 and b._lib.j2p_batch_wait(b._h, ticket) == 0
        assert all(np.isfinite(a).all() for a in alive[-1][3])
