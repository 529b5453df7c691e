"""Optimised Huffman tables on the GPU (k_entropy_histogram; j2p_entropy_encode_ex, j2p_planes_to_jpeg_ex, j2p_batch_submit_jpeg_ex;
entropy_encode(optimize=, stats=), Solver.to_jpeg(optimize=), Batch.submit(jpeg={"optimize": True})): the device's symbol counts
are, per table and symbol, the restatement's of tests/huffman_cases.py, and every file is, byte for byte, the restatement's —
which tests/test_huffman_cpu.py holds against libjpeg's optimize_coding — of the same coefficients.  The counts are compared
themselves: a wrong count that happens not to move a code length would pass a comparison of files."""
import ctypes

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
import samples_cases as sc

J2P_EINVAL, J2P_ESPACE = -1, -5
NAMES = sorted(hc.directed_cases())


@pytest.fixture(scope="module")
def directed():
    """{name: (case, the restatement's file, its report)}, computed once"""
    return {name: (case,) + hc.encode_case(case) for name, case in hc.directed_cases().items()}


def encode(case, **keywords):
    import jpeg2png_amd as j
    return j.entropy_encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], **keywords)


def same_counts(stats, report, name):
    for key, want in zip(hc.TABLE_NAMES, report["counts"]):
        got = stats[key]
        assert got == want, f"{name}: {key}: " + ", ".join(f"symbol {s:#04x}: {g} for {w}" for s, (g, w) in enumerate(zip(got, want)) if g != w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_counts_and_file_are_the_restatements(lib, directed, name):
    case, want, report = directed[name]
    got, stats = encode(case, optimize=True, stats=True)
    same_counts(stats, report, name)
    assert stats["scan_bits"] == report["bits"] and stats["stuffed_bytes"] == report["stuffed"]
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(f"{name}: {len(got)} bytes for {len(want)}; byte {first} differs: {got[first - 2:first + 6].hex()} for {want[first - 2:first + 6].hex()}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_41x23_420", "grey_17x9_dense", "limited", "ties", "dense_368x368_420"])
def test_the_decoder_reads_the_optimised_file_back(lib, directed, name):
    import jpeg2png_amd as j
    case, want, _report = directed[name]
    arrays = j.entropy_decode(want)
    assert len(arrays) == len(case["coefficients"])
    for c, (a, b) in enumerate(zip(arrays, case["coefficients"])):
        assert np.array_equal(a, b), f"{name}: component {c}"
    parsed = j.jpeg_parse(want)
    assert (parsed["width"], parsed["height"]) == (case["width"], case["height"])
    for c, k in enumerate(parsed["components"]):
        assert np.array_equal(k["quant_table"], case["quant"][c]), f"{name}: component {c}"
        assert (k["dc_slot"], k["ac_slot"]) == ((0, 0) if c == 0 else (1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_41x23_420", "two_tiles", "dense_24x40_444"])
def test_without_the_flag_the_file_is_the_plain_one(lib, directed, name):
    """optimize=False, flags 0 and the entry points without flags: entropy_cases.encode, as before — and the counts are there
    for the asking all the same"""
    import jpeg2png_amd as j
    import test_entropy_gpu as teg
    case, _want, report = directed[name]
    plain = ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])
    assert encode(case) == plain and encode(case, optimize=False) == plain
    got, stats = encode(case, stats=True)
    assert got == plain
    same_counts(stats, report, name)
    rc, size, buf = teg.c_call(lib, case, len(plain) + 64)              # j2p_entropy_encode itself
    assert rc == 0 and buf[:size].tobytes() == plain and (buf[size:] == 0xA5).all()


def c_call_ex(lib, case, room, flags, fill=0xA5):
    """j2p_entropy_encode_ex into a buffer of `room` bytes pre-filled with `fill` -> (rc, size, buffer)"""
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
    rc = lib.j2p_entropy_encode_ex(0, ctypes.byref(spec), ptrs, n, buf.ctypes.data, room, ctypes.byref(size), flags, None)
    return rc, size.value, buf


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stuffed_end", "sparse_41x23_420", "zrl_heavy"])
def test_one_byte_short_reports_the_optimised_size(lib, directed, name):
    case, want, _report = directed[name]
    plain = ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"])
    assert len(want) < len(plain)
    rc, size, buf = c_call_ex(lib, case, len(want) - 1, 1)
    assert rc == J2P_ESPACE and size == len(want) and (buf == 0xA5).all()
    assert str(len(want)) in lib.j2p_last_error().decode()
    rc, size, buf = c_call_ex(lib, case, len(want), 1)                  # exactly enough
    assert rc == 0 and buf.tobytes() == want


@pytest.mark.gpu
def test_unknown_flag_bits_are_refused(lib, directed):
    import jpeg2png_amd as j
    case, _want, _report = directed["sparse_41x23_420"]
    for flags in (2, 3, 0x80000000):
        rc, size, buf = c_call_ex(lib, case, 4096, flags)
        assert rc == J2P_EINVAL and size == 0 and (buf == 0xA5).all() and "flag" in lib.j2p_last_error().decode()
    fixture = sc.case("y_48x40_tgv")
    with j.Solver(fixture.coefficient_planes(), 0.3, [0.001], 0) as s:
        ref = j._CPlaneRef(s._h, 0)
        spec, _held = j._c_jpeg(48, 40, 1, 75, None, (1, 1))
        size, buf = ctypes.c_size_t(0), np.zeros(65536, np.uint8)
        assert lib.j2p_planes_to_jpeg_ex(ctypes.byref(ref), 1, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), 2) == J2P_EINVAL
        assert "flag" in lib.j2p_last_error().decode() and size.value == 0
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        job = j._CJob()
        job.nchannel, job.out_w, job.out_h = 1, 48, 40
        cpl, _keep = j._c_planes(fixture.coefficient_planes())
        job.planes[0] = cpl[0]
        job.weight[0], job.pweight[0], job.iterations[0] = 0.3, 0.001, 1
        ticket = ctypes.c_int(-7)
        rc = b._lib.j2p_batch_submit_jpeg_ex(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), 4, ctypes.byref(ticket))
        assert rc == J2P_EINVAL and ticket.value == -7 and "flag" in b._lib.j2p_last_error().decode()


SOLVES = [(41, 23, "420", (2, 2), 75, False), (17, 9, "444", (1, 1), 90, True)]


def solver_coefficients(s, n, width, height, tables, sub):
    bw, bh = -(-width // 8), -(-height // 8)
    out = []
    for c in range(n):
        sx, sy = (1, 1) if c == 0 else sub
        out.append(s.coefficients(c, tables[c], blocks_w=-(-bw // sx), blocks_h=-(-bh // sy), subsampling=(sx, sy)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,sampling,sub,quality,grey", SOLVES, ids=["41x23_420", "17x9_grey"])
def test_solver_to_jpeg_is_entropy_encode_of_its_coefficients(lib, width, height, sampling, sub, quality, grey):
    """... which is the restatement of them; and the second call of the same size finds the solver's scratch large enough"""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    planes = synth.make_planes(width, height, sampling, 30, seed=width * height, y_only=grey)
    n = len(planes)
    tables = j.quality_tables(quality, n)
    with j.Solver(planes, 0.3, [0.001] * n, 3) as s:
        s.run(3)
        got = s.to_jpeg(width, height, quality=quality, subsampling=sub, optimize=True)
        room = s.output_scratch_bytes()
        again = s.to_jpeg(width, height, quant_tables=tables, subsampling=sub, optimize=True)
        assert s.output_scratch_bytes() == room > 0, "the second call of the same size grew the scratch"
        plain = s.to_jpeg(width, height, quality=quality, subsampling=sub)
        assert s.output_scratch_bytes() == room
        coefficients = solver_coefficients(s, n, width, height, tables, sub)
    assert got == j.entropy_encode(coefficients, width, height, tables, sub, optimize=True)
    assert got == hc.encode(coefficients, width, height, tables, sub) and again == got
    assert plain == ec.encode(coefficients, width, height, tables, sub) and len(got) < len(plain)


@pytest.mark.gpu
def test_batch_jobs_with_the_flag(lib):
    """coefficient, sample and file jobs with jpeg={"optimize": True}, a job without it in between: each is entropy_encode of the
    coefficients the same job delivers"""
    import jpeg2png_amd as j
    case = sc.case("rgb420_padded_40x20")
    tables = j.quality_tables(85, 3)
    args = (case.weight, case.pweight, case.iterations)
    subs = [(1, 1), (2, 2), (2, 2)]
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        t_opt = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg={"quality": 85, "subsampling": (2, 2), "optimize": True})
        t_plain = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg={"quality": 85, "subsampling": (2, 2), "optimize": False})
        t_coef = b.submit(case.coefficient_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs)
        t_samples = b.submit(case.bare_planes(), *args, width=37, height=19, jpeg={"quant_tables": tables, "subsampling": (2, 2), "optimize": True},
                             samples=[np.array(a) for a in case.samples])
        t_scoef = b.submit(case.bare_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs,
                           samples=[np.array(a) for a in case.samples])
        coefficients, scoefficients = b.wait(t_coef), b.wait(t_scoef)
        optimised, plain, from_samples = b.wait(t_opt), b.wait(t_plain), b.wait(t_samples)
        assert optimised == hc.encode(coefficients, 37, 19, tables, (2, 2)) == j.entropy_encode(coefficients, 37, 19, tables, (2, 2), optimize=True)
        assert plain == ec.encode(coefficients, 37, 19, tables, (2, 2))
        assert from_samples == hc.encode(scoefficients, 37, 19, tables, (2, 2))
        # file in, optimised file out
        t_file = b.submit(None, *args, file=plain, jpeg={"quality": 85, "subsampling": (2, 2), "optimize": True})
        t_fcoef = b.submit(None, *args, file=plain, quant_tables=tables, subsampling=subs)
        assert b.wait(t_file) == hc.encode(b.wait(t_fcoef), 37, 19, tables, (2, 2))
        # a buffer that is too small fails the job with the optimised size
        t = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg={"quality": 85, "subsampling": (2, 2), "optimize": True, "capacity": 100})
        with pytest.raises(j.J2PError, match=rf"error -5: .*the file has {len(optimised)} bytes, the buffer 100"):
            b.wait(t)
