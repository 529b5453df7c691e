"""Greyscale output of the batch engine (one-plane jobs with out_bits 8 / 16, j2p_planes_to_grey /
j2p_planes_rows_to_grey): the samples are the UNMODIFIED reference's compute(1, ...) on the plane, written as png.c:37-45
writes R (= G = B) when Cb = Cr = 0 — whole canvas, zoomed, row-tiled — and the same bytes as the RGB writer's on a
plane with zero chroma beside it."""
import ctypes

import numpy as np
import pytest

from conftest import band_devices, make_case, parity_note


def grey_samples(canvas, w, h, bits):
    """png.c:37-45 with Cb = Cr = 0 after jpeg2png.c:156-159: y = (float)(Y + 128.), clamp in double, times
    (1 << bits) / 256 in float, truncated; 16 bits big-endian"""
    y = (canvas[:h, :w].astype(np.float64) + 128.0).astype(np.float32)
    y64 = y.astype(np.float64)
    y = np.where(y64 > 255.0, np.float32(255.0), np.where(y64 < 0.0, np.float32(0.0), y)).astype(np.float32)
    bitfactor = np.float32((1 << bits) / 256.0)
    s = (y * bitfactor).astype(np.uint32)
    return s.astype(np.uint8) if bits == 8 else s.astype(">u2")


def _need_ref(oracle):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference sources)")


CASES = [  # (zoom, separate, bits)
    (1, False, 8), (1, True, 16), (2, False, 16), (2, True, 8), (3, False, 8), (3, True, 16), (4, False, 16), (4, True, 8),
]


@pytest.mark.gpu
@pytest.mark.parametrize("zoom,separate,bits", CASES)
def test_one_plane_job_writes_the_reference_luma_as_grey(lib, oracle, zoom, separate, bits):
    import jpeg2png_amd as j
    _need_ref(oracle)
    w, h, its = 61 + 4 * zoom, 45 + 3 * zoom, 6 + zoom
    planes = j.zoomed(make_case(w, h, "444", 20 + 10 * zoom, seed=300 + zoom, y_only=True), zoom)
    planes[0].fdata = oracle.decode_plane(planes[0])
    weight, pw = (0.3, [0.001]) if zoom % 2 else (0.0, [0.002])
    want, _, _ = oracle.ref_compute(planes, weight, pw, its)
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        got = b.wait(b.submit(planes, weight, pw, its, separate=separate, width=w * zoom, height=h * zoom, bits=bits))
    assert got.shape == (h * zoom, w * zoom) and got.dtype == (np.uint8 if bits == 8 else np.dtype(">u2"))
    assert np.array_equal(got, grey_samples(want[0], w * zoom, h * zoom, bits))
    parity_note(f"grey x{zoom} {w}x{h} bits {bits} separate {separate}: samples of the reference's compute(1) bit-identical")


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16])
def test_row_tiled_grey_job_equals_the_reference(lib, oracle, capfd, bits):
    """tile=True over three bands (device 0 three times where there is one GPU; a 200-row canvas makes three bands of
    at least 48 rows): every band writes its own rows through j2p_planes_rows_to_grey"""
    import jpeg2png_amd as j
    _need_ref(oracle)
    w, h, its = 90, 197, 7
    planes = make_case(w, h, "444", 30, seed=41 + bits, y_only=True)
    want, _, _ = oracle.ref_compute(planes, 0.3, [0.001], its)
    with j.Batch(devices=band_devices(3), slots_per_device=1) as b:
        tiled = b.wait(b.submit(planes, 0.3, [0.001], its, width=w, height=h, bits=bits, tile=True, tile_min_band_pixels=0))
    assert "not row-tiling" not in capfd.readouterr().err          # (the single-solver fallback says so)
    assert np.array_equal(tiled, grey_samples(want[0], w, h, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16])
def test_grey_equals_each_channel_of_the_rgb_writer_with_zero_chroma(lib, bits):
    """the grey writer pinned to the RGB one: Y with large coefficients (both clamps hit) and all-zero chroma
    coefficients, 0 iterations: R, G and B of the three-channel job each equal the one-plane job's grey"""
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    w, h = 70, 53
    rng = np.random.default_rng(7 + bits)
    y = make_case(w, h, "444", 50, seed=5, y_only=True)[0]
    data = rng.integers(-60, 61, size=y.data.shape).astype(np.int16)
    data.reshape(-1, 64)[:, 0] = rng.integers(-120, 121, size=data.size // 64)
    q = np.full(64, 4, np.uint16)
    q[0] = 16
    yp = Plane(y.w, y.h, 1, 1, data, q)
    zero = [Plane(y.w, y.h, 1, 1, np.zeros_like(data), np.full(64, 9, np.uint16)) for _ in range(2)]
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        grey = b.wait(b.submit([yp], 0.3, [0.001], 0, width=w, height=h, bits=bits))
        rgb = b.wait(b.submit([yp] + zero, 0.3, [0.001] * 3, 0, width=w, height=h, bits=bits))
    top = 255 * (1 << bits) // 256
    assert (grey == 0).any() and (grey == top).any() and ((grey > 0) & (grey < top)).any()
    for c in range(3):
        assert np.array_equal(rgb[:, :, c], grey), f"channel {c}"


@pytest.mark.gpu
def test_colour_jobs_are_unchanged_beside_grey_jobs(lib):
    import jpeg2png_amd as j
    colour = make_case(120, 80, "420", 20, seed=9)
    greys = [make_case(96 + 8 * k, 64, "444", 30, seed=20 + k, y_only=True) for k in range(3)]
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        alone = b.wait(b.submit(colour, 0.3, [0.001] * 3, 8, width=120, height=80, bits=8))
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = [b.submit(greys[0], 0.3, [0.001], 8, width=96, height=64, bits=16),
                   b.submit(colour, 0.3, [0.001] * 3, 8, width=120, height=80, bits=8),
                   b.submit(greys[1], 0.3, [0.001], 8, width=104, height=64, bits=8),
                   b.submit(greys[2], 0.3, [0.001], 8, separate=True, width=112, height=64, bits=8)]
        outs = [b.wait(t) for t in tickets]
    assert np.array_equal(outs[1], alone)
    assert [o.shape for o in outs] == [(64, 96), (80, 120, 3), (64, 104), (64, 112)]


def test_submit_refuses_wrong_sample_shapes(lib):
    """refused in Python before anything is submitted (no device needed)"""
    import jpeg2png_amd as j
    b = j.Batch.__new__(j.Batch)            # (no j2p_batch: a refusal must come before the submit)
    b._lib, b._h, b._pending = j.load_library(), None, {}
    grey = make_case(64, 48, "444", 30, seed=1, y_only=True)
    colour = make_case(64, 48, "420", 30, seed=1)
    with pytest.raises(j.J2PError, match=r"\(48, 64\)"):
        b.submit(grey, 0.3, [0.001], 4, width=64, height=48, bits=8, out=np.empty((48, 64, 3), np.uint8))
    with pytest.raises(j.J2PError, match="2-byte"):
        b.submit(grey, 0.3, [0.001], 4, width=64, height=48, bits=16, out=np.empty((48, 64), np.uint8))
    with pytest.raises(j.J2PError, match="three planes"):
        b.submit(colour[:2], 0.3, [0.001] * 2, 4, width=64, height=48, bits=8)
    assert not b._pending


@pytest.mark.gpu
def test_batch_refuses_two_channel_sample_output_in_c(lib):
    """the C side of the same rule: a j2p_job with nchannel 2 and out_bits fails at j2p_batch_wait, before any work"""
    import jpeg2png_amd as j
    planes = make_case(64, 48, "420", 30, seed=2)[:2]
    cpl, keep = j._c_planes(planes)
    job = j._CJob()
    job.nchannel = 2
    for c in range(2):
        job.planes[c] = cpl[c]
        job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 4
    buf = np.empty(64 * 48 * 3, np.uint8)
    job.out_bits, job.out_w, job.out_h, job.out_rgb = 8, 64, 48, buf.ctypes.data
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        t = ctypes.c_int()
        assert b._lib.j2p_batch_submit(b._h, ctypes.byref(job), ctypes.byref(t)) == 0
        rc = b._lib.j2p_batch_wait(b._h, t.value)
        assert rc == -1 and b"greyscale" in b._lib.j2p_last_error()
    del keep
