"""The entropy coder on the GPU (k_entropy_lengths, k_scan_*, k_entropy_pack, k_stuff_count, k_stuff_copy; j2p_entropy_encode,
j2p_planes_to_jpeg, j2p_batch_submit_jpeg; jpeg2png_amd.entropy_encode, Solver.to_jpeg, Batch.submit(jpeg=)): every file is,
byte for byte, the restatement of tests/entropy_cases.py — which tests/test_entropy_cpu.py holds against libjpeg — of the same
coefficients.  The directed cases are a few blocks each; the two 368x368 ones (3174 scan positions, about 600 KB dense) cross
the 1024 positions of one workgroup of the scans, the 64 of one workgroup of the coding kernels and, dense, the 1024 chunks
of one workgroup of the stuffing pass's scan."""
import ctypes

import numpy as np
import pytest

import entropy_cases as ec
import samples_cases as sc

J2P_EINVAL, J2P_ESTATE, J2P_ESPACE = -1, -4, -5


@pytest.fixture(scope="module")
def directed():
    cases = ec.directed_cases()
    return {name: (case, ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])) for name, case in cases.items()}


NAMES = sorted(ec.directed_cases())


def c_call(lib, case, room, fill=0xA5):
    """j2p_entropy_encode into a buffer of `room` bytes pre-filled with `fill` -> (rc, size, buffer)"""
    import jpeg2png_amd as j
    n = len(case["coefficients"])
    tables = [np.ascontiguousarray(t, dtype=np.uint16) for t in case["quant"]]
    spec = j._CJpeg(case["width"], case["height"], *case["sub"])
    for c in range(n):
        spec.quant[c] = tables[c].ctypes.data
    arrays = [np.ascontiguousarray(a, dtype=np.int16) for a in case["coefficients"]]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    buf = np.full(room, fill, dtype=np.uint8)
    size = ctypes.c_size_t(0)
    rc = lib.j2p_entropy_encode(0, ctypes.byref(spec), ptrs, n, buf.ctypes.data, room, ctypes.byref(size))
    return rc, size.value, buf


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_entropy_encode_is_the_restatement(lib, directed, name):
    case, want = directed[name]
    rc, size, buf = c_call(lib, case, len(want) + 64)
    assert rc == 0, lib.j2p_last_error().decode()
    assert size == len(want)
    got = buf[:size].tobytes()
    if got != want:
        first = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        raise AssertionError(f"{name}: byte {first} of {len(want)} differs: {got[first - 2:first + 6].hex()} for {want[first - 2:first + 6].hex()}")
    assert (buf[size:] == 0xA5).all(), "bytes behind the file were touched"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stuffed_end", "sparse_41x23_420", "dense_24x40_444"])
def test_one_byte_short_writes_nothing_and_reports_the_size(lib, directed, name):
    case, want = directed[name]
    rc, size, buf = c_call(lib, case, len(want) - 1)
    assert rc == J2P_ESPACE and size == len(want) and (buf == 0xA5).all()
    assert str(len(want)) in lib.j2p_last_error().decode()
    rc, size, buf = c_call(lib, case, len(want))                # exactly enough
    assert rc == 0 and buf.tobytes() == want


@pytest.mark.gpu
def test_python_entropy_encode_and_refusals(lib, directed):
    import jpeg2png_amd as j
    for name in ("sparse_40x24_422", "grey_17x9_dense", "dense_368x368_420"):       # (the last: larger than the first guess)
        case, want = directed[name]
        assert j.entropy_encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"]) == want, name
    case, _ = directed["sparse_41x23_420"]
    bad = [a.copy() for a in case["coefficients"]]
    bad[2][0, 1, 9] = 1024
    with pytest.raises(j.J2PError, match="1024"):
        j.entropy_encode(bad, 41, 23, case["quant"], (2, 2))
    with pytest.raises(j.J2PError, match="grid"):
        j.entropy_encode(case["coefficients"], 41, 23, case["quant"], (1, 1))


SOLVER_CASES = [  # (fixture, width, height, subsampling, quality)
    ("rgb444_48x32_q50", 48, 32, (1, 1), 90),
    ("rgb420_padded_40x20", 40, 20, (2, 2), 75),
    ("rgb420_padded_40x20", 37, 19, (2, 1), 95),
    ("rgb422_48x32", 41, 27, (1, 2), 50),
    ("y_48x40_tgv", 48, 40, (1, 1), 90),
    ("y_48x40_tgv", 43, 33, (2, 2), 75),           # (one component: the sampling is taken as 1)
]


def restated_from(solvers_channels, width, height, tables, sub):
    """the restatement applied to what Solver.coefficients() returns for the same tables and subsampling"""
    n = len(solvers_channels)
    sub = sub if n == 3 else (1, 1)
    bw, bh = -(-width // 8), -(-height // 8)
    coefficients = []
    for c, (s, ch) in enumerate(solvers_channels):
        sx, sy = (1, 1) if c == 0 else sub
        coefficients.append(s.coefficients(ch, tables[c], blocks_w=-(-bw // sx), blocks_h=-(-bh // sy), subsampling=(sx, sy)))
    return ec.encode(coefficients, width, height, tables, sub)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,width,height,sub,quality", SOLVER_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_{c[3][0]}{c[3][1]}" for c in SOLVER_CASES])
def test_solver_to_jpeg_is_the_restatement_of_its_coefficients(lib, fixture, width, height, sub, quality):
    import jpeg2png_amd as j
    case = sc.case(fixture)
    n = len(case.planes)
    tables = j.quality_tables(quality, n)
    with j.Solver(case.coefficient_planes(), case.weight, case.pweight[:n], case.iterations) as s:
        s.run(case.iterations)
        before = [s.download(c) for c in range(n)]
        got = s.to_jpeg(width, height, quality=quality, subsampling=sub)
        again = s.to_jpeg(width, height, quant_tables=tables, subsampling=sub)         # (the scratch is there now: no growth)
        want = restated_from([(s, c) for c in range(n)], width, height, tables, sub)
        assert all(np.array_equal(s.download(c).view(np.uint32), before[c].view(np.uint32)) for c in range(n))
    assert got == want and again == want


@pytest.mark.gpu
def test_three_separate_solvers_make_one_file(lib):
    import jpeg2png_amd as j
    case = sc.case("rgb420_padded_40x20")
    tables = j.quality_tables(90, 3)
    solvers = [j.Solver([p], 0.3 if c == 0 else 0.0, [0.001], 4 + c) for c, p in enumerate(case.coefficient_planes())]
    try:
        for c, s in enumerate(solvers):
            s.run(4 + c)
        for sub in ((2, 2), (1, 1)):
            got = solvers[0].to_jpeg(40, 20, quality=90, subsampling=sub, others=solvers[1:])
            assert got == restated_from([(s, 0) for s in solvers], 40, 20, tables, sub), sub
    finally:
        for s in solvers:
            s.close()


@pytest.mark.gpu
def test_batch_jpeg_jobs_with_coefficient_jobs_and_sample_jobs_in_flight(lib):
    import jpeg2png_amd as j
    jobs = [("rgb444_48x32_q50", 48, 32, (1, 1), False), ("rgb420_padded_40x20", 40, 20, (2, 2), False), ("rgb422_48x32", 45, 30, (2, 1), True),
            ("y_48x40_tgv", 48, 40, (1, 1), False), ("rgb420_padded_40x20", 33, 17, (1, 2), True)]
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = []
        for name, w, h, sub, separate in jobs:
            case = sc.case(name)
            n = len(case.planes)
            args = (case.weight, case.pweight[:n], case.iterations)
            tables = j.quality_tables(85, n)
            subs = [(1, 1)] + [sub] * (n - 1)
            tickets.append((
                b.submit(case.coefficient_planes(), *args, separate=separate, width=w, height=h, jpeg={"quality": 85, "subsampling": sub}),
                b.submit(case.coefficient_planes(), *args, separate=separate, width=w, height=h, quant_tables=tables, subsampling=subs),
                b.submit(case.bare_planes(), *args, separate=separate, width=w, height=h, jpeg={"quant_tables": tables, "subsampling": sub},
                         samples=[np.array(a) for a in case.samples]),
                b.submit(case.bare_planes(), *args, separate=separate, width=w, height=h, quant_tables=tables, subsampling=subs,
                         samples=[np.array(a) for a in case.samples])))
        for (name, w, h, sub, separate), (t_file, t_coef, t_sfile, t_scoef) in zip(jobs, tickets):
            n = len(sc.case(name).planes)
            tables = j.quality_tables(85, n)
            for kind, file, coefficients in (("coefficients", b.wait(t_file), b.wait(t_coef)), ("samples", b.wait(t_sfile), b.wait(t_scoef))):
                assert isinstance(file, bytes)
                assert file == ec.encode(coefficients, w, h, tables, sub if n == 3 else (1, 1)), f"{name}, {kind}"
        # a buffer that is too small fails the job with the size it needs
        case = sc.case("rgb444_48x32_q50")
        t = b.submit(case.coefficient_planes(), case.weight, case.pweight, 1, width=48, height=32, jpeg={"quality": 85, "capacity": 700})
        with pytest.raises(j.J2PError, match=r"error -5: .*the file has \d+ bytes, the buffer 700"):
            b.wait(t)
        # refused at submit
        planes = case.coefficient_planes()
        with pytest.raises(j.J2PError, match="tile"):
            b.submit(planes, case.weight, case.pweight, 1, width=48, height=32, jpeg={"quality": 85}, tile=True)
        job = j._CJob()
        job.nchannel, job.out_w, job.out_h = 3, 48, 32
        cpl, keep = j._c_planes(planes)
        for c in range(3):
            job.planes[c] = cpl[c]
            job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 1
        spec, held = j._c_jpeg(48, 32, 3, 85, None, (1, 1))
        buf, size, ticket = np.zeros(65536, np.uint8), ctypes.c_size_t(0), ctypes.c_int(-7)

        def refused(what):
            rc = b._lib.j2p_batch_submit_jpeg(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), ctypes.byref(ticket))
            assert rc == J2P_EINVAL and ticket.value == -7 and what in b._lib.j2p_last_error().decode(), b._lib.j2p_last_error().decode()

        job.tile = 1
        refused("row-tiled")
        job.tile, job.out_bits = 0, 8
        refused("out_bits 0")
        job.out_bits, job.out_w = 0, 47
        refused("48x32")
        job.out_w = 48
        spec.sub_w = 3
        refused("sampling factors")
        spec.sub_w = 1
        assert b._lib.j2p_batch_submit_jpeg(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size),
                                            ctypes.byref(ticket)) == 0
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0 and buf[:2].tobytes() == b"\xff\xd8" and buf[size.value - 2:size.value].tobytes() == b"\xff\xd9"


@pytest.mark.gpu
def test_solver_refusals(lib):
    import jpeg2png_amd as j
    case = sc.case("y_48x40_tgv")
    q = j.quality_tables(75, 3)
    with j.Solver(case.coefficient_planes(), 0.3, [0.001], 0, band=(0, 16)) as s:
        ref = j._CPlaneRef(s._h, 0)
        spec, held = j._c_jpeg(48, 16, 1, 75, None, (1, 1))
        size = ctypes.c_size_t(0)
        assert lib.j2p_planes_to_jpeg(ctypes.byref(ref), 1, ctypes.byref(spec), None, 0, ctypes.byref(size)) == J2P_ESTATE
        assert "whole-canvas" in lib.j2p_last_error().decode()
    with j.Solver(case.coefficient_planes(), 0.3, [0.001], 0) as s:
        big = q[0].astype(np.uint16).copy()
        big[3] = 256
        spec = j._CJpeg(48, 40, 1, 1)
        spec.quant[0] = big.ctypes.data
        ref = j._CPlaneRef(s._h, 0)
        size = ctypes.c_size_t(0)
        buf = np.zeros(65536, np.uint8)
        assert lib.j2p_planes_to_jpeg(ctypes.byref(ref), 1, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)) == J2P_EINVAL
        assert "above 255" in lib.j2p_last_error().decode()
        with pytest.raises(j.J2PError, match="1..255"):
            s.to_jpeg(48, 40, quant_tables=[big])
        spec, held = j._c_jpeg(56, 40, 1, 75, None, (1, 1))                           # wider than the canvas
        assert lib.j2p_planes_to_jpeg(ctypes.byref(ref), 1, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size)) == J2P_EINVAL
        assert s.to_jpeg(48, 40, quality=75)[:2] == b"\xff\xd8"
    case = sc.case("rgb444_48x32_q50")
    with j.Solver(case.coefficient_planes(), case.weight, case.pweight, 0) as s:
        other = q[1].copy()
        other[0] += 1
        with pytest.raises(j.J2PError, match="quant\\[2\\] differs"):
            s.to_jpeg(48, 32, quant_tables=[q[0], q[1], other])
        with pytest.raises(j.J2PError, match="one of them"):
            s.to_jpeg(48, 32)
