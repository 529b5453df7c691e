"""The progressive JPEG file on the GPU (k_prog_*; j2p_entropy_encode_progressive, j2p_planes_to_jpeg_progressive,
j2p_batch_submit_jpeg_progressive, j2p_batch_submit_file_jpeg_progressive; entropy_encode(progressive=), Solver.to_jpeg(progressive=),
Batch.submit(jpeg={"progressive": True})): every file is, byte for byte, the restatement's of tests/progressive_cases.py — which
tests/test_progressive_cpu.py holds against libjpeg's jpeg_simple_progression() — of the same coefficients, and the device's
per-scan symbol counts, bits, stuffed bytes and EOB runs are the restatement's.  The counts are compared themselves: a wrong
count that happens not to move a code length would pass a comparison of files.  What each case of progressive_cases.gpu_cases() is
there for — where k_prog_runs cuts a run and from which block, the loops of its walk, how a scan's stream ends — is asserted from
the restatement's report by tests/test_progressive_cpu.py::test_case_preconditions."""
import ctypes

import numpy as np
import pytest

import entropy_cases as ec
import huffman_cases as hc
import progressive_cases as pc
import samples_cases as sc
from test_huffman_gpu import solver_coefficients
from test_jpeg_out_cli import _helper, load_component, load_coefficients, read_component, read_coefficients  # noqa: F401

J2P_ESPACE = -5
NAMES = sorted(pc.gpu_cases())


@pytest.fixture(scope="module")
def directed():
    """{name: (case, the restatement's file, its per-scan report)}, computed once"""
    return {name: (case,) + pc.encode_case(case) for name, case in pc.gpu_cases().items()}


def encode(case, **keywords):
    import jpeg2png_amd as j
    return j.entropy_encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], progressive=True, **keywords)


def same_file(got, want, name):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(f"{name}: {len(got)} bytes for {len(want)}; byte {first} differs: {got[first - 2:first + 6].hex()} for {want[first - 2:first + 6].hex()}")


def same_scans(stats, report, name):
    assert len(stats) == len(report), name
    for k, (got, want) in enumerate(zip(stats, report)):
        comps, ss, se, ah, al = want["scan"]
        where = f"{name}: scan {k + 1} {want['scan']}"
        assert (got["components"], got["ss"], got["se"], got["ah"], got["al"]) == (comps, ss, se, ah, al), where
        tables = {((t[0] == "ac") << 4) | t[1]: c for t, c in want["counts"].items()}
        assert list(got["tables"]) == list(tables), where
        for t, count in tables.items():
            assert got["tables"][t] == count, f"{where}: table {t:#04x}: " + ", ".join(
                f"symbol {s:#04x}: {g} for {w}" for s, (g, w) in enumerate(zip(got["tables"][t], count)) if g != w)
        assert got["eob_runs"] == sum(want["flushes"].values()), where
        assert (got["bits"], got["stuffed_bytes"]) == (want["bits"], want["stuffed"]), where


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_counts_and_file_are_the_restatements(lib, directed, name):
    case, want, report = directed[name]
    got, stats = encode(case, stats=True)
    same_scans(stats, report, name)
    same_file(got, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_41x23_420", "refine_zrl"])
def test_optimize_changes_nothing_and_no_stats_is_the_same_file(lib, directed, name):
    case, want, _report = directed[name]
    assert encode(case) == want and encode(case, optimize=True) == want and encode(case, optimize=False) == want


def c_call(lib, case, room, fill=0xA5, behind=64):
    """j2p_entropy_encode_progressive into `room` bytes of a buffer of room + behind, pre-filled with `fill` -> (rc, size, buffer)"""
    import jpeg2png_amd as j
    n = len(case["coefficients"])
    tables = [np.ascontiguousarray(t, dtype=np.uint16) for t in case["quant"]]
    spec = j._CJpeg(case["width"], case["height"], *case["sub"])
    for c in range(n):
        spec.quant[c] = tables[c].ctypes.data
    arrays = [np.ascontiguousarray(a, dtype=np.int16) for a in case["coefficients"]]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    buf = np.full(room + behind, fill, dtype=np.uint8)
    size = ctypes.c_size_t(0)
    rc = lib.j2p_entropy_encode_progressive(0, ctypes.byref(spec), ptrs, n, buf.ctypes.data, room, ctypes.byref(size), None)
    return rc, size.value, buf


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stuffed_end", "sparse_41x23_420", "refine_zrl"] + pc.STREAM_END_NAMES)
def test_one_byte_short_reports_the_size_and_touches_nothing(lib, directed, name):
    """... the end_<...> cases among them: scans that end on a byte, on a word, and on an FF whose 00 is the scan's final byte"""
    case, want, _report = directed[name]
    rc, size, buf = c_call(lib, case, len(want) - 1)
    assert rc == J2P_ESPACE and size == len(want) and (buf == 0xA5).all()
    assert str(len(want)) in lib.j2p_last_error().decode()
    rc, size, buf = c_call(lib, case, len(want))                # exactly enough, sentinels behind
    assert rc == 0 and size == len(want) and buf[:size].tobytes() == want and (buf[size:] == 0xA5).all()


SOLVES = [(41, 23, "444", (1, 1), 90, False, 1), (41, 23, "420", (2, 2), 75, False, 1), (17, 9, "444", (1, 1), 90, True, 1),
          (45, 38, "420", (2, 2), 85, False, 6)]


@pytest.fixture(scope="module")
def readers(tmp_path_factory):
    """libjpeg's readers (tests/c/read_coefficients.c, read_component.c), or None where the helpers do not build"""
    import os
    from test_jpeg_out_cli import PREFIX
    if not os.path.exists(os.path.join(PREFIX, "include", "jpeglib.h")):
        return None
    return _helper(tmp_path_factory, "read_coefficients"), _helper(tmp_path_factory, "read_component")


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,sampling,sub,quality,grey,orientation", SOLVES, ids=["41x23_444", "41x23_420", "17x9_grey", "45x38_420_o6"])
def test_solver_to_jpeg_is_the_restatement_of_its_coefficients(lib, readers, tmp_path, width, height, sampling, sub, quality, grey, orientation):
    """... and the second call of the same size finds the solver's scratch large enough; libjpeg reads the file back to them"""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    planes = synth.make_planes(width, height, sampling, 30, seed=width * height, y_only=grey)
    n = len(planes)
    tables = j.quality_tables(quality, n)
    with j.Solver(planes, 0.3, [0.001] * n, 3) as s:
        s.run(3)
        uw, uh = width, height
        if orientation != 1:
            s.set_orientation(orientation, width, height)
            uw, uh = height, width
        got = s.to_jpeg(uw, uh, quality=quality, subsampling=sub, progressive=True)
        room = s.output_scratch_bytes()
        again = s.to_jpeg(uw, uh, quant_tables=tables, subsampling=sub, progressive=True, optimize=True)
        assert s.output_scratch_bytes() == room > 0, "the second call of the same size grew the scratch"
        optimised = s.to_jpeg(uw, uh, quality=quality, subsampling=sub, optimize=True)
        coefficients = solver_coefficients(s, n, uw, uh, tables, sub)
    same_file(got, pc.encode(coefficients, uw, uh, tables, sub), "to_jpeg")
    assert again == got and got == j.entropy_encode(coefficients, uw, uh, tables, sub, progressive=True)
    assert optimised == hc.encode(coefficients, uw, uh, tables, sub)
    if readers is not None and (sub != (1, 1) or grey):
        path = str(tmp_path / "progressive.jpg")
        open(path, "wb").write(got)
        if grey:
            w, h, k, plane = load_component(readers[1], path)
            back = [plane]
        else:
            w, h, back = load_coefficients(readers[0], path)
        assert (w, h) == (uw, uh)
        for c, (plane, (gh, gw)) in enumerate(zip(back, ec.grids(uw, uh, n, sub))):
            assert np.array_equal(plane.data.reshape(gh, gw, 64), coefficients[c]), f"component {c}"


@pytest.mark.gpu
def test_batch_jobs_progressive_optimised_and_plain_together(lib):
    """coefficient, sample and file jobs in flight together: each is the restatement of the coefficients the same job delivers"""
    import jpeg2png_amd as j
    case = sc.case("rgb420_padded_40x20")
    tables = j.quality_tables(85, 3)
    args = (case.weight, case.pweight, case.iterations)
    subs = [(1, 1), (2, 2), (2, 2)]
    keys = {"quality": 85, "subsampling": (2, 2)}
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        t_prog = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, progressive=True))
        t_opt = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, optimize=True))
        t_plain = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys))
        t_both = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, progressive=True, optimize=True))
        t_coef = b.submit(case.coefficient_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs)
        t_samples = b.submit(case.bare_planes(), *args, width=37, height=19, jpeg={"quant_tables": tables, "subsampling": (2, 2), "progressive": True},
                             samples=[np.array(a) for a in case.samples])
        t_scoef = b.submit(case.bare_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs,
                           samples=[np.array(a) for a in case.samples])
        coefficients, scoefficients = b.wait(t_coef), b.wait(t_scoef)
        progressive, optimised, plain, both, from_samples = b.wait(t_prog), b.wait(t_opt), b.wait(t_plain), b.wait(t_both), b.wait(t_samples)
        same_file(progressive, pc.encode(coefficients, 37, 19, tables, (2, 2)), "batch")
        assert both == progressive
        assert optimised == hc.encode(coefficients, 37, 19, tables, (2, 2)) and plain == ec.encode(coefficients, 37, 19, tables, (2, 2))
        same_file(from_samples, pc.encode(scoefficients, 37, 19, tables, (2, 2)), "batch, samples")
        # file in, progressive file out
        t_file = b.submit(None, *args, file=plain, jpeg=dict(keys, progressive=True))
        t_fcoef = b.submit(None, *args, file=plain, quant_tables=tables, subsampling=subs)
        same_file(b.wait(t_file), pc.encode(b.wait(t_fcoef), 37, 19, tables, (2, 2)), "batch, file")
        # a buffer that is too small fails the job with the progressive size
        t = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, progressive=True, capacity=100))
        with pytest.raises(j.J2PError, match=rf"error -5: .*the file has {len(progressive)} bytes, the buffer 100"):
            b.wait(t)


@pytest.mark.gpu
def test_tile_jobs_are_refused_at_submit(lib):
    import jpeg2png_amd as j
    case = sc.case("rgb444_48x32_q50")
    planes = case.coefficient_planes()
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        with pytest.raises(j.J2PError, match="tile"):
            b.submit(planes, case.weight, case.pweight, 1, width=48, height=32, jpeg={"quality": 85, "progressive": True}, tile=True)
        job = j._CJob()
        job.nchannel, job.out_w, job.out_h, job.tile = 3, 48, 32, 1
        cpl, _keep = j._c_planes(planes)
        for c in range(3):
            job.planes[c] = cpl[c]
            job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 1
        spec, _held = j._c_jpeg(48, 32, 3, 85, None, (1, 1))
        buf, size, ticket = np.zeros(65536, np.uint8), ctypes.c_size_t(0), ctypes.c_int(-7)
        rc = b._lib.j2p_batch_submit_jpeg_progressive(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size),
                                                      ctypes.byref(ticket))
        assert rc == -1 and ticket.value == -7 and "row-tiled" in b._lib.j2p_last_error().decode()
