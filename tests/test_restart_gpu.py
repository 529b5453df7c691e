"""Restart intervals on the GPU (k_*_restart, k_restart_pad, k_restart_ends, k_stuff_*_restart; j2p_entropy_encode_opt,
j2p_planes_to_jpeg_opt, j2p_batch_submit_jpeg_opt, j2p_batch_submit_file_jpeg_opt; entropy_encode(restart_rows=, restart_interval=),
Solver.to_jpeg(...), Batch.submit(jpeg={"restart_rows": ...})): every file of the three coders is, byte for byte, the restatement's of
tests/restart_cases.py — which tests/test_restart_cpu.py holds against libjpeg with restart_interval / restart_in_rows — and the
device's per-scan counts, bits, stuffed bytes, EOB runs, intervals, padding bits and markers are the restatement's.  Every file goes
back through the library's own decoders, which must return the coefficients value for value.  What each directed case is there for
is asserted from the restatement's report by tests/test_restart_cpu.py::test_case_preconditions."""
import ctypes

import numpy as np
import pytest

import entropy_cases as ec
import restart_cases as rc
import samples_cases as sc
from test_huffman_gpu import solver_coefficients
from test_progressive_gpu import same_file

CASES = rc.gpu_cases()
NAMES = sorted(CASES)
TABLE_KEYS = {("dc", 0): "dc0", ("ac", 0): "ac0", ("dc", 1): "dc1", ("ac", 1): "ac1"}


def test_the_cases_are_all_there():
    """the sweep at one N and one R each, three coders x six settings x four shapes, the directed cases and the large ones: nothing
    is skipped silently"""
    assert len(rc.sweep_cases()) == 2 * 160 and len(rc.shape_cases()) == 3 * 6 * 4 and len(rc.directed_cases()) == 14 and len(rc.large_cases()) == 3
    assert len(NAMES) == 320 + 72 + 14 + 2


@pytest.fixture(scope="module")
def restated():
    """{name: (file, per-scan report)}, each computed once when first asked for"""
    done = {}

    def get(name):
        if name not in done:
            case, coder, n, r = CASES[name]
            done[name] = rc.encode_case(case, coder, n, r)
        return done[name]
    return get


def encode(case, coder, n, r, **keywords):
    import jpeg2png_amd as j
    return j.entropy_encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"], optimize=coder == "optimized",
                            progressive=coder == "progressive", restart_interval=n, restart_rows=r, **keywords)


def same_restart(got, want, where):
    entry = want["plan"]
    assert (got["interval"], got["intervals"], got["markers"], got["padding_bits"]) == (entry["interval"], entry["intervals"], want["markers"],
                                                                                      want["padding"]), where


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_file_and_statistics_are_the_restatements_and_decode_back(lib, restated, name):
    import jpeg2png_amd as j
    case, coder, n, r = CASES[name]
    want, report = restated(name)
    got, stats = encode(case, coder, n, r, stats=True)
    if coder == "progressive":
        assert len(stats) == len(report), name
        for k, (g, w) in enumerate(zip(stats, report)):
            where = f"{name}: scan {k + 1} {w['scan']}"
            tables = {((t[0] == "ac") << 4) | t[1]: c for t, c in w["counts"].items()}
            assert g["tables"] == tables, where
            assert (g["bits"], g["stuffed_bytes"], g["eob_runs"]) == (w["bits"], w["stuffed"], w["eob_runs"]), where
            same_restart(g["restart"], w, where)
    else:
        w = report[0]
        for t, key in TABLE_KEYS.items():
            assert stats[key] == w["counts"].get(t, [0] * 256), f"{name}: {key}"
        assert (stats["scan_bits"], stats["stuffed_bytes"]) == (w["bits"], w["stuffed"]), name
        same_restart(stats["restart"], w, name)
    same_file(got, want, name)
    assert encode(case, coder, n, r) == want, f"{name}: without stats"
    back = j.entropy_decode(got, progressive=coder == "progressive")
    assert len(back) == len(case["coefficients"])
    for c, (a, b) in enumerate(zip(back, case["coefficients"])):
        assert np.array_equal(a, b), f"{name}: component {c}"


# the twelve older entry points are shorthands: each coder's record, and what its entry points' names end in
RECORD = {"baseline": (0, 0, 0, 0), "optimized": (1, 0, 0, 0), "progressive": (0, 1, 0, 0)}
SHORTHAND = {"baseline": "", "optimized": "_ex", "progressive": "_progressive"}


def c_call(lib, case, options, room, fill=0xA5, behind=64, shorthand=None, stats=False):
    """j2p_entropy_encode_opt — or, with shorthand=coder, the older entry point whose record `options` is — into `room` bytes of a
    buffer of room + behind, pre-filled with `fill` -> (rc, size, buffer), and with stats the coder's own record behind them"""
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
    record = (j._CProgressiveStats if options[1] else j._CEncodeStats)() if stats else None
    ref = None if record is None else ctypes.byref(record)
    head = (0, ctypes.byref(spec), ptrs, n, buf.ctypes.data, room, ctypes.byref(size))
    if shorthand is None:
        opt = j._CJpegOptions(*options)
        rc_ = lib.j2p_entropy_encode_opt(*head, ctypes.byref(opt), None if options[1] else ref, ref if options[1] else None, None)
    else:
        assert tuple(options) == RECORD[shorthand] and not (stats and shorthand == "baseline")
        tail = {"baseline": (), "optimized": (options[0], ref), "progressive": (ref,)}[shorthand]
        rc_ = getattr(lib, "j2p_entropy_encode" + SHORTHAND[shorthand])(*head, *tail)
    return (rc_, size.value, buf) + ((record,) if stats else ())


def planes_call(lib, solver, n, spec, options=None, shorthand=None):
    """j2p_planes_to_jpeg_opt with `options` — or the older entry point of shorthand=coder — on the solver's n planes -> the file"""
    import jpeg2png_amd as j
    refs = (j._CPlaneRef * 3)(*[j._CPlaneRef(solver._h, c) for c in range(n)])
    buf, size = np.empty(1 << 16, dtype=np.uint8), ctypes.c_size_t(0)
    head = (refs, n, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size))
    if shorthand is None:
        opt = j._CJpegOptions(*options)
        rc_ = lib.j2p_planes_to_jpeg_opt(*head, ctypes.byref(opt))
    else:
        rc_ = getattr(lib, "j2p_planes_to_jpeg" + SHORTHAND[shorthand])(*head, *((RECORD[shorthand][0],) if shorthand == "optimized" else ()))
    assert rc_ == 0, lib.j2p_last_error().decode()
    return buf[:size.value].tobytes()


def shorthand_entry(coder, called):
    """a stand-in for jpeg2png_amd._entry_point: the job Batch.submit has built goes, as it is, to the older C entry point of `coder`
    in the place of the _opt one — the record, which must be that shorthand's, leaves the arguments and _ex gets its flags"""
    import jpeg2png_amd as j
    real = j._entry_point

    def entry(source, source_args, kind, output_args):
        name, args = real(source, source_args, kind, output_args)
        record = args[-1]._obj
        assert name.endswith("_jpeg_opt") and (record.flags, record.progressive, record.restart_interval, record.restart_in_rows) == RECORD[coder]
        called.append(name[:-len("_opt")] + SHORTHAND[coder])
        return called[-1], args[:-1] + ((record.flags,) if coder == "optimized" else ())
    return entry


@pytest.mark.gpu
@pytest.mark.parametrize("coder", rc.CODERS)
def test_without_restarts_the_opt_call_is_the_old_call(lib, coder):
    """entropy_encode makes the _opt call: its file is j2p_entropy_encode's, _ex's and _progressive's byte for byte, called as C
    calls them, for a buffer of exactly the file's size with sentinels behind"""
    import jpeg2png_amd as j
    case = ec.make(41, 23, 3, (2, 2), "sparse", seed=4123)
    new = j.entropy_encode(case["coefficients"], 41, 23, case["quant"], (2, 2), optimize=coder == "optimized", progressive=coder == "progressive")
    rc_, size, buf = c_call(lib, case, RECORD[coder], len(new), shorthand=coder)
    assert rc_ == 0 and size == len(new) and buf[:size].tobytes() == new and (buf[size:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("coder", rc.CODERS)
def test_without_restarts_the_planes_and_batch_opt_calls_are_the_old_calls(lib, monkeypatch, coder):
    """Solver.to_jpeg and Batch.submit (planes, samples and file=) make the _opt calls with both restart fields 0: their files are,
    byte for byte, those of j2p_planes_to_jpeg, _ex and _progressive, of j2p_batch_submit_jpeg, _ex and _progressive and of the
    three j2p_batch_submit_file_jpeg calls, which get the same solver and the same jobs through ctypes"""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    keys = {"optimize": coder == "optimized", "progressive": coder == "progressive"}
    planes = synth.make_planes(45, 38, "420", 30, seed=4538)
    case = sc.case("rgb420_padded_40x20")
    args = (case.weight, case.pweight, case.iterations)
    jpeg = dict(keys, quality=85, subsampling=(2, 2))

    def files(old):
        with j.Solver(planes, 0.3, [0.001] * 3, 3) as s:
            s.run(3)
            if old:
                spec, _held = j._c_jpeg(45, 38, 3, 80, None, (2, 2))
                out = [planes_call(lib, s, 3, spec, shorthand=coder)]
            else:
                out = [s.to_jpeg(45, 38, quality=80, subsampling=(2, 2), **keys)]
        with j.Batch(devices=(0,), slots_per_device=2) as b:
            tickets = [b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=jpeg),
                       b.submit(case.bare_planes(), *args, width=37, height=19, jpeg=jpeg, samples=[np.array(a) for a in case.samples])]
            out += [b.wait(t) for t in tickets]
            out.append(b.wait(b.submit(None, *args, file=plain_file, jpeg=jpeg)))
        return out
    plain_file = j.entropy_encode(ec.make(37, 19, 3, (2, 2), "sparse", seed=3719)["coefficients"], 37, 19, j.quality_tables(85, 3), (2, 2))
    new = files(False)
    called = []
    with monkeypatch.context() as m:
        m.setattr(j, "_entry_point", shorthand_entry(coder, called))
        old = files(True)
    assert called == ["j2p_batch_submit_jpeg" + SHORTHAND[coder]] * 2 + ["j2p_batch_submit_file_jpeg" + SHORTHAND[coder]]
    assert len(new) == 4 and len(old) == 4 and all(len(f) > 100 for f in old)
    for k, (a, b) in enumerate(zip(new, old)):
        same_file(a, b, f"{coder}: file {k}")


def fields(x):
    """a ctypes record as plain Python values, member for member"""
    if isinstance(x, ctypes.Structure):
        return {name: fields(getattr(x, name)) for name, *_ in x._fields_}
    return [fields(v) for v in x] if isinstance(x, ctypes.Array) else x


SHORTHAND_SHAPES = {"420_41x23": (41, 23, 3, (2, 2), 4123), "grey_17x9": (17, 9, 1, (1, 1), 179)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHORTHAND_SHAPES))
def test_every_shorthand_writes_its_records_file(lib, monkeypatch, shape):
    """each of the twelve older entry points against the _opt call of its family with the shorthand's record — {0,0,0,0}, {flags,0,0,0},
    {0,1,0,0} — on the smallest shapes with an MCU walk, dummy blocks on both edges (41x23 4:2:0: 3x2 MCUs) and a scan of one
    component (17x9): the same file byte for byte, and for j2p_entropy_encode_ex / _progressive the same statistics"""
    import jpeg2png_amd as j
    from jpeg2png_amd.synth import Plane
    width, height, n, sub, seed = SHORTHAND_SHAPES[shape]
    case = ec.make(width, height, n, sub, "sparse", seed=seed)
    sizes = {}
    for coder in rc.CODERS:
        stats = coder != "baseline"
        new = c_call(lib, case, RECORD[coder], 1 << 16, stats=stats)
        old = c_call(lib, case, RECORD[coder], 1 << 16, shorthand=coder, stats=stats)
        assert new[0] == 0 and old[0] == 0 and new[1] == old[1] > 100, coder
        assert np.array_equal(new[2], old[2]) and (new[2][new[1]:] == 0xA5).all(), coder
        sizes[coder] = new[1]
        if stats:
            got, want = fields(old[3]), fields(new[3])
            assert got == want, coder
            assert want["nscans"] == (10 if n == 3 else 6) if coder == "progressive" else want["scan_bits"] > 0
    assert sizes["optimized"] < sizes["baseline"] and len(set(sizes.values())) == 3      # (three different files)
    grids = ec.grids(width, height, n, case["sub"])
    planes = [Plane(gw * 8, gh * 8, *((1, 1) if c == 0 else case["sub"]), np.ascontiguousarray(case["coefficients"][c], np.int16).reshape(-1),
                    np.asarray(case["quant"][c], np.uint16)) for c, (gh, gw) in enumerate(grids)]
    bare = [Plane(p.w, p.h, p.w_samp, p.h_samp, None, p.quant_table) for p in planes]
    rng = np.random.default_rng(seed)
    samples = [rng.integers(0, 256, (-(-height // (p.h_samp if c else 1)), -(-width // (p.w_samp if c else 1))), dtype=np.uint8)
               for c, p in enumerate(planes)]
    file = c_call(lib, case, RECORD["baseline"], 1 << 16)
    file = file[2][:file[1]].tobytes()
    spec, _held = j._c_jpeg(width, height, n, 80, None, case["sub"])
    args = (0.3, [0.001] * n, 2)
    with j.Solver(planes, *args) as s:
        s.run(2)
        for coder in rc.CODERS:
            same_file(planes_call(lib, s, n, spec, shorthand=coder), planes_call(lib, s, n, spec, options=RECORD[coder]), f"planes, {coder}")
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        def submit(coder):
            jpeg = {"quality": 80, "subsampling": case["sub"], "optimize": coder == "optimized", "progressive": coder == "progressive"}
            return [b.submit(planes, *args, width=width, height=height, jpeg=jpeg),
                    b.submit(bare, *args, width=width, height=height, jpeg=jpeg, samples=samples),
                    b.submit(None, *args, file=file, jpeg=jpeg)]
        called = []
        for coder in rc.CODERS:
            new = submit(coder)
            with monkeypatch.context() as m:
                m.setattr(j, "_entry_point", shorthand_entry(coder, called))
                old = submit(coder)
            for k, (a, o) in enumerate(zip(new, old)):
                got, want = b.wait(o), b.wait(a)
                assert len(want) > 100
                same_file(got, want, f"batch, {coder}: job {k}")
    assert sorted(set(called)) == sorted(f + SHORTHAND[c] for f in ("j2p_batch_submit_jpeg", "j2p_batch_submit_file_jpeg") for c in rc.CODERS)


@pytest.mark.gpu
def test_a_batch_record_is_refused_for_what_is_wrong_with_it(lib):
    """progressive = 2 is refused as that, not as unknown flag bits; restart fields as everywhere"""
    import jpeg2png_amd as j
    case = sc.case("rgb420_padded_40x20")
    planes = case.coefficient_planes()
    with j.Batch(devices=(0,), slots_per_device=1) as b:
        job = j._CJob()
        job.nchannel, job.out_w, job.out_h = 3, 37, 19
        cpl, _keep = j._c_planes(planes)
        for c in range(3):
            job.planes[c] = cpl[c]
            job.weight[c], job.pweight[c], job.iterations[c] = 0.3, 0.001, 1
        spec, _held = j._c_jpeg(37, 19, 3, 85, None, (2, 2))
        buf, size, ticket = np.zeros(65536, np.uint8), ctypes.c_size_t(0), ctypes.c_int(-7)
        for options, message in (((0, 2, 0, 0), "progressive is 0 or 1"), ((2, 0, 0, 0), "unknown flag bits"), ((0, 0, 65536, 0), "restart_interval is above 65535"),
                                 ((0, 1, 1, 1), "both set")):
            opt = j._CJpegOptions(*options)
            rc_ = b._lib.j2p_batch_submit_jpeg_opt(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size),
                                                   ctypes.byref(opt), ctypes.byref(ticket))
            assert rc_ == -1 and ticket.value == -7 and message in b._lib.j2p_last_error().decode(), options
        rc_ = b._lib.j2p_batch_submit_jpeg_opt(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), None,
                                               ctypes.byref(ticket))
        assert rc_ == -1 and "options is NULL" in b._lib.j2p_last_error().decode()
        # (the flags of an _ex call are its record's: refused in the same words, as they were when they travelled alone)
        rc_ = b._lib.j2p_batch_submit_jpeg_ex(b._h, ctypes.byref(job), None, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size), 2,
                                              ctypes.byref(ticket))
        assert rc_ == -1 and ticket.value == -7 and b._lib.j2p_last_error().decode() == "job: jpeg: unknown flag bits"
        # ... and the same of a file job, whose two entry points hand their record to the same check
        data = np.frombuffer(j.entropy_encode(ec.make(37, 19, 3, (2, 2), "sparse", seed=3719)["coefficients"], 37, 19, j.quality_tables(85, 3), (2, 2)),
                             dtype=np.uint8)
        fjob = j._CJob()
        fjob.nchannel = 3
        bare, _fkeep = j._c_planes(case.bare_planes())
        for c in range(3):
            fjob.planes[c] = bare[c]
            fjob.weight[c], fjob.pweight[c], fjob.iterations[c] = 0.3, 0.001, 1
        head = (b._h, ctypes.byref(fjob), data.ctypes.data, data.size, ctypes.byref(spec), buf.ctypes.data, buf.size, ctypes.byref(size))
        for options, message in (((0, 2, 0, 0), "job: jpeg: progressive is 0 or 1"), ((2, 0, 0, 0), "job: jpeg: unknown flag bits"),
                                 ((0, 1, 1, 1), "job: jpeg: restart_interval and restart_in_rows are both set")):
            opt = j._CJpegOptions(*options)
            rc_ = b._lib.j2p_batch_submit_file_jpeg_opt(*head, ctypes.byref(opt), ctypes.byref(ticket))
            assert rc_ == -1 and ticket.value == -7 and b._lib.j2p_last_error().decode() == message, options
        rc_ = b._lib.j2p_batch_submit_file_jpeg_ex(*head, 2, ctypes.byref(ticket))
        assert rc_ == -1 and ticket.value == -7 and b._lib.j2p_last_error().decode() == "job: jpeg: unknown flag bits"
        # (a good record: the job is taken, so what was refused above was refused for the record alone)
        opt = j._CJpegOptions(1, 0, 0, 1)
        assert b._lib.j2p_batch_submit_file_jpeg_opt(*head, ctypes.byref(opt), ctypes.byref(ticket)) == 0, b._lib.j2p_last_error().decode()
        assert b._lib.j2p_batch_wait(b._h, ticket.value) == 0 and size.value > 100 and bytes(buf[:2]) == b"\xff\xd8"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["420_41x23_baseline_r1", "420_41x23_progressive_n3", "ff_by_padding"])
def test_one_byte_short_reports_the_size_and_touches_nothing(lib, restated, name):
    case, coder, n, r = CASES[name]
    want = restated(name)[0]
    options = (1 if coder == "optimized" else 0, 1 if coder == "progressive" else 0, n, r)
    rc_, size, buf = c_call(lib, case, options, len(want) - 1)
    assert rc_ == -5 and size == len(want) and (buf == 0xA5).all()
    rc_, size, buf = c_call(lib, case, options, len(want))
    assert rc_ == 0 and size == len(want) and buf[:size].tobytes() == want and (buf[size:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("coder", rc.CODERS)
def test_solver_to_jpeg_is_entropy_encode_of_its_coefficients(lib, coder):
    """... with the same options, which is the restatement; and the second call of a size takes no block"""
    import jpeg2png_amd as j
    from jpeg2png_amd import synth
    width, height, sub = 45, 38, (2, 2)
    planes = synth.make_planes(width, height, "420", 30, seed=4538)
    tables = j.quality_tables(80, 3)
    keys = {"optimize": coder == "optimized", "progressive": coder == "progressive"}
    with j.Solver(planes, 0.3, [0.001] * 3, 3) as s:
        s.run(3)
        rows = s.to_jpeg(width, height, quality=80, subsampling=sub, restart_rows=1, **keys)
        takes = lib.j2p_pool_thread_takes()
        again = s.to_jpeg(width, height, quant_tables=tables, subsampling=sub, restart_rows=1, **keys)
        assert lib.j2p_pool_thread_takes() == takes, "the second call of the same size took a block"
        mcus = s.to_jpeg(width, height, quality=80, subsampling=sub, restart_interval=2, **keys)
        coefficients = solver_coefficients(s, 3, width, height, tables, sub)
    assert again == rows
    same_file(rows, rc.encode_report(coefficients, width, height, tables, sub, coder, 0, 1)[0], "to_jpeg, rows")
    same_file(mcus, rc.encode_report(coefficients, width, height, tables, sub, coder, 2, 0)[0], "to_jpeg, MCUs")
    assert rows == j.entropy_encode(coefficients, width, height, tables, sub, restart_rows=1, **keys)
    assert mcus == j.entropy_encode(coefficients, width, height, tables, sub, restart_interval=2, **keys)


@pytest.mark.gpu
def test_batch_jobs_of_the_three_coders(lib):
    """a coefficient job per coder, a sample job and a file job: each is entropy_encode, with the same options, of the coefficients
    the same job delivers"""
    import jpeg2png_amd as j
    case = sc.case("rgb420_padded_40x20")
    tables = j.quality_tables(85, 3)
    args = (case.weight, case.pweight, case.iterations)
    subs = [(1, 1), (2, 2), (2, 2)]
    keys = {"quality": 85, "subsampling": (2, 2)}
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        t_base = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, restart_rows=1))
        t_opt = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, optimize=True, restart_interval=2))
        t_prog = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, progressive=True, restart_rows=1))
        t_plain = b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys))
        t_coef = b.submit(case.coefficient_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs)
        t_samples = b.submit(case.bare_planes(), *args, width=37, height=19,
                             jpeg={"quant_tables": tables, "subsampling": (2, 2), "progressive": True, "restart_interval": 3},
                             samples=[np.array(a) for a in case.samples])
        t_scoef = b.submit(case.bare_planes(), *args, width=37, height=19, quant_tables=tables, subsampling=subs,
                           samples=[np.array(a) for a in case.samples])
        coefficients, scoefficients = b.wait(t_coef), b.wait(t_scoef)
        base, optimised, progressive, plain, from_samples = b.wait(t_base), b.wait(t_opt), b.wait(t_prog), b.wait(t_plain), b.wait(t_samples)
        same_file(base, rc.encode_report(coefficients, 37, 19, tables, (2, 2), "baseline", 0, 1)[0], "batch, baseline")
        same_file(optimised, rc.encode_report(coefficients, 37, 19, tables, (2, 2), "optimized", 2, 0)[0], "batch, optimised")
        same_file(progressive, rc.encode_report(coefficients, 37, 19, tables, (2, 2), "progressive", 0, 1)[0], "batch, progressive")
        assert base == j.entropy_encode(coefficients, 37, 19, tables, (2, 2), restart_rows=1)
        assert optimised == j.entropy_encode(coefficients, 37, 19, tables, (2, 2), optimize=True, restart_interval=2)
        assert progressive == j.entropy_encode(coefficients, 37, 19, tables, (2, 2), progressive=True, restart_rows=1)
        assert plain == ec.encode(coefficients, 37, 19, tables, (2, 2))
        same_file(from_samples, rc.encode_report(scoefficients, 37, 19, tables, (2, 2), "progressive", 3, 0)[0], "batch, samples")
        t_file = b.submit(None, *args, file=plain, jpeg=dict(keys, optimize=True, restart_rows=2))
        t_fcoef = b.submit(None, *args, file=plain, quant_tables=tables, subsampling=subs)
        same_file(b.wait(t_file), rc.encode_report(b.wait(t_fcoef), 37, 19, tables, (2, 2), "optimized", 0, 2)[0], "batch, file")
        with pytest.raises(j.J2PError, match="both set"):
            b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, restart_rows=1, restart_interval=1))
        with pytest.raises(j.J2PError, match="65535"):
            b.submit(case.coefficient_planes(), *args, width=37, height=19, jpeg=dict(keys, restart_rows=65536))
