"""Reading a JPEG file on the GPU (k_unstuff_*, k_decode_*; j2p_entropy_decode, j2p_entropy_decode_ex,
j2p_solver_create_from_jpeg, j2p_batch_submit_file, j2p_batch_submit_file_jpeg; jpeg2png_amd.entropy_decode, Solver.from_jpeg,
Batch.submit(file=)): every comparison is exact, with the arrays of
the plain-Python restatement in tests/decode_cases.py — which tests/test_decode_cpu.py holds against libjpeg, and which
returns the coefficients the cases' files were written from.  The directed cases are a few blocks each; the two 368x368 ones
(about 600 KB dense) are the only ones that cross a workgroup of the scans at the default subsequence length.  At the
smallest length (32 bits) and an odd one (75) a 16x8 image has dozens of subsequences, and blocks and single symbols straddle them.
decode_cases.boundary_cases() put restart markers, stuffed bytes and fill bytes on the unstuffing kernels' lane, chunk and
workgroup edges, and have more restart intervals than a workgroup of k_decode_intervals (256) and a tile of the scans (1024)
hold; the periodic file has more blocks, and at 32 bits more subsequences, than the 256 tiles k_scan_tiles takes in one trip."""
import ctypes

import numpy as np
import pytest

import decode_cases as dc
import entropy_cases as ec
import samples_cases as sc
from conftest import bit_equal

J2P_EFORMAT = -6
SMALL = (32, 75)                        # J2P_DECODE_SUBSEQUENCE_MIN, and a length no power of two divides


@pytest.fixture(scope="module")
def good():
    """{name: (file, [arrays of the restated decoder])}; the arrays are the coefficients the files were written from (test_decode_cpu)"""
    out = {}
    for name, case in ec.directed_cases().items():
        out[name] = (ec.encode(case["coefficients"], case["width"], case["height"], case["quant"], case["sub"]), case["coefficients"])
    for name, (case, data) in {**dc.framing_cases(), **dc.boundary_cases()}.items():
        out[name] = (data, case["coefficients"])
    for _data, arrays in out.values():
        for a in arrays:
            a.setflags(write=False)
    return out


DIRECTED = sorted(ec.directed_cases())
FRAMING = sorted(dc.framing_cases())
BOUNDARY = sorted(dc.BOUNDARY)          # aimed at the kernels' lanes, chunks, workgroups and tiles: decode_cases.boundary_cases()
DAMAGED = ("cut_mid_block", "cut_between_blocks", "rst_number_changed", "rst_removed", "code_in_no_table", "run_past_63",
           # refused by the kernels alone (kDecodeBadDc, the bytes-left-over arm of kDecodeBadEnd, the marker count of kDecodeBadMarker)
           "dc_above_int16", "dc_below_int16", "leftover_byte", "leftover_many", "rst_doubled", "rst_before_eoi",
           "rst_empty_interval")


def c_decode(lib, data, shapes, bits=None, fill=0x5A5A):
    """j2p_entropy_decode (bits None) or _ex into arrays pre-filled with `fill` -> (rc, arrays, stats)"""
    import jpeg2png_amd as j
    raw = np.frombuffer(data, dtype=np.uint8)
    arrays = [np.full(s, fill, dtype=np.int16) for s in shapes]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    stats = j._CDecodeStats()
    if bits is None:
        rc = lib.j2p_entropy_decode(0, raw.ctypes.data, raw.size, ptrs, None, None)
    else:
        rc = lib.j2p_entropy_decode_ex(0, raw.ctypes.data, raw.size, ptrs, None, None, bits, ctypes.byref(stats))
    return rc, arrays, stats


def check(name, got, want):
    assert len(got) == len(want), name
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, f"{name}: component {c}: {a.shape} for {b.shape}"
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{name}: component {c}: {len(bad)} of {b.size} values differ, the first at {bad[0].tolist()}: {a[tuple(bad[0])]} for {b[tuple(bad[0])]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", DIRECTED + FRAMING + BOUNDARY)
def test_entropy_decode_is_the_restatement(lib, good, name):
    data, want = good[name]
    rc, got, _ = c_decode(lib, data, [a.shape for a in want])
    assert rc == 0, lib.j2p_last_error().decode()
    check(name, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", SMALL)
@pytest.mark.parametrize("name", DIRECTED + FRAMING + BOUNDARY)
def test_small_subsequences(lib, good, name, bits):
    data, want = good[name]
    rc, got, stats = c_decode(lib, data, [a.shape for a in want], bits=bits)
    assert rc == 0, lib.j2p_last_error().decode()
    check(f"{name} at {bits} bits", got, want)
    frame = dc.parse(data)
    assert stats.intervals == len(dc._intervals(data[frame["scan_begin"]:frame["scan_end"]])[0])
    assert stats.subsequences >= stats.data_bytes * 8 // bits
    assert 1 <= stats.rounds <= stats.subsequences
    print(f"{name}: {bits} bits: {stats.subsequences} subsequences in {stats.intervals} intervals, {stats.rounds} rounds, recomputed {list(stats.recomputed)[:stats.rounds]}")


@pytest.fixture(scope="module")
def periodic():
    """decode_cases.periodic_case(513, 512): (file, coefficients), 262 656 grey blocks"""
    data, want = dc.periodic_case(513, 512)
    want.setflags(write=False)
    return data, want


@pytest.mark.gpu
def test_decode_across_257_scan_tiles(lib, periodic):
    """4104 x 4096 grey, one 22-byte period 65 664 times: the 262 656 DC differences are 257 tiles of the scan in front of
    k_decode_dc, so k_scan_tiles goes round its carry loop twice, and the sums of difference + 32768 pass 2^32; at 32 bits the
    subsequences (more than the blocks: a block is 44 bits) are more than 256 tiles too, for the scan of done[]"""
    import jpeg2png_amd as j
    data, want = periodic
    assert want.shape[0] * want.shape[1] == 262656 > 256 * 1024 and 262656 * 32768 > 1 << 32
    got, stats = j.entropy_decode(data, stats=True)
    check("periodic", got, [want])
    assert stats["intervals"] == 1 and 1 <= stats["rounds"] <= stats["subsequences"]
    got, stats = j.entropy_decode(data, subsequence_bits=32, stats=True)
    check("periodic at 32 bits", got, [want])
    assert stats["subsequences"] > 256 * 1024 and stats["subsequences"] >= stats["data_bytes"] * 8 // 32
    assert stats["data_bytes"] == 262656 // 4 * len(dc.periodic_period()[1])
    assert 1 <= stats["rounds"] <= stats["subsequences"]
    print(f"periodic 513x512 blocks: 32 bits: {stats['subsequences']} subsequences, {stats['rounds']} rounds, recomputed {stats['recomputed']}")


@pytest.mark.gpu
def test_encode_across_257_scan_tiles(lib, periodic):
    """the same coefficients through the device's coder: 257 tiles of len[] for its scan, and the file byte for byte"""
    import jpeg2png_amd as j
    data, want = periodic
    got = j.entropy_encode([want], 4104, 4096, ec.quant_tables(75, 1))
    assert len(got) == len(data)
    if got != data:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(data, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError(f"{len(bad)} of {len(data)} bytes differ, the first at {bad[0]}: {a[bad[0]]:02x} for {b[bad[0]]:02x}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("zero", "dense"))
def test_all_zero_and_dense_converge(lib, kind):
    """16x8 grey: the all-zero file is two symbols a block; the dense one has symbols of up to 26 bits, most of a 32-bit subsequence"""
    case = ec.make(16, 8, 1, (1, 1), kind, seed=9)
    data = ec.encode(case["coefficients"], 16, 8, case["quant"])
    for bits in SMALL + (0,):
        rc, got, stats = c_decode(lib, data, [(1, 2, 64)], bits=bits)
        assert rc == 0, lib.j2p_last_error().decode()
        check(kind, got, case["coefficients"])
        assert 1 <= stats.rounds <= stats.subsequences
        assert stats.recomputed[0] == stats.subsequences          # the first round decodes everything
        print(f"{kind} 16x8: {bits or 1024} bits: {stats.subsequences} subsequences, {stats.rounds} rounds, recomputed {list(stats.recomputed)[:stats.rounds]}")


@pytest.mark.gpu
def test_python_entropy_decode_and_stats(lib, good):
    import jpeg2png_amd as j
    data, want = good["restart_4_of_6"]
    check("python", j.entropy_decode(data), want)
    got, stats = j.entropy_decode(data, subsequence_bits=75, stats=True)
    check("python, 75 bits", got, want)
    assert stats["intervals"] == 5 and stats["rounds"] == len(stats["recomputed"]) <= stats["subsequences"]
    info = j.jpeg_parse(data)
    assert [(k["blocks_h"], k["blocks_w"]) for k in info["components"]] == [a.shape[:2] for a in want]


@pytest.mark.gpu
def test_a_file_in_device_memory_gives_the_same(lib, good):
    import torch
    import jpeg2png_amd as j
    for name in ("dense_368x368_420", "restart_1", "fill_bytes"):
        data, want = good[name]
        # (one byte into an allocation: the scan is read in place at whatever address it has)
        buf = torch.zeros(len(data) + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        check(name, j.entropy_decode(buf[1:]), want)


@pytest.mark.gpu
def test_damaged_files_in_device_memory_are_refused(lib, good):
    """the failure exits of a file that was opened from device memory: one whose headers are refused (the parse of its host copy
    fails: nothing is opened) and one whose scan is (the decode into the pooled grids fails), then a good decode of the same kind"""
    import torch
    import jpeg2png_amd as j
    ok, want = good["sparse_41x23_420"]
    rst_removed, _why = dc.damaged_cases()["rst_removed"]
    comps, _, _ = dc.geometry(dc.parse(rst_removed))

    def decode(data, shapes):
        # (the C entry point: jpeg2png_amd.entropy_decode reads the headers of a host copy itself first)
        buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        arrays = [np.full(s, 0x5A5A, dtype=np.int16) for s in shapes]
        ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
        return lib.j2p_entropy_decode(0, buf.data_ptr(), buf.numel(), ptrs, None, None), arrays

    for name, bad, shapes, code in (("progressive", bytes(ok).replace(b"\xff\xc0", b"\xff\xc2", 1), [a.shape for a in want], j.J2P_ENOTSUP),
                                    ("rst_removed", rst_removed, [(gh, gw, 64) for gh, gw, _, _ in comps], J2P_EFORMAT)):
        rc, got = decode(bad, shapes)
        assert rc == code, f"{name}: {rc} {lib.j2p_last_error().decode()}"
        assert all((a == 0x5A5A).all() for a in got), name
    rc, got = decode(ok, [a.shape for a in want])
    assert rc == 0, lib.j2p_last_error().decode()
    check("after the refusals", got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_files_are_refused(lib, good, name):
    """J2P_EFORMAT, the pre-filled output untouched, and a good decode afterwards in the same process"""
    data, _why = dc.damaged_cases()[name]
    frame = dc.parse(data)
    comps, _, _ = dc.geometry(frame)
    for bits in (None,) + SMALL:
        rc, got, _ = c_decode(lib, data, [(gh, gw, 64) for gh, gw, _, _ in comps], bits=bits)
        assert rc == J2P_EFORMAT, f"{name} at {bits} bits: {rc} {lib.j2p_last_error().decode()}"
        assert all((a == 0x5A5A).all() for a in got), name
    ok, want = good["sparse_41x23_420"]
    rc, got, _ = c_decode(lib, ok, [a.shape for a in want])
    assert rc == 0, lib.j2p_last_error().decode()
    check("after " + name, got, want)


# ---- solvers ----
def file_of(case):
    """a solver fixture's coefficients written as a file -> (file, planes as Solver takes them)"""
    planes = case.coefficient_planes()
    n = len(planes)
    sub = (planes[1].w_samp, planes[1].h_samp) if n == 3 else (1, 1)
    arrays = [np.asarray(p.data).reshape(p.h // 8, p.w // 8, 64) for p in planes]
    # the image size that gives exactly these grids
    width, height = planes[0].w, planes[0].h
    assert [a.shape[:2] for a in arrays] == ec.grids(width, height, n, sub)
    quant = [np.asarray(p.quant_table) for p in planes]
    if n == 3:
        assert np.array_equal(quant[1], quant[2])
    return dc.write(arrays, width, height, quant, sub, restart=3, tables="own"), planes


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("rgb420_64x48", "rgb444_48x32_q50", "y_48x40_tgv"))
def test_solver_from_jpeg_is_the_coefficient_built_solver(lib, name):
    import jpeg2png_amd as j
    case = sc.case(name)
    data, planes = file_of(case)
    n = len(planes)
    iterations = 50
    with j.Solver(planes, case.weight, case.pweight[:n], iterations) as ref, j.Solver.from_jpeg(data, case.weight, case.pweight[:n], iterations) as s:
        assert (s.W, s.H, s.nch) == (ref.W, ref.H, n)
        for c in range(n):
            assert np.array_equal(s.download_coefficients(c), np.asarray(planes[c].data).reshape(planes[c].h // 8, planes[c].w // 8, 64)), f"channel {c}"
            assert (s.coefficient_bytes(c), s.shares_state(c), s.wide_footprint(c)) == (ref.coefficient_bytes(c), ref.shares_state(c), ref.wide_footprint(c))
            assert bit_equal(s.download(c), ref.download(c)), f"{name}: channel {c} at iteration 0"
        ref.run(iterations)
        for again in range(2):
            s.run(iterations)
            for c in range(n):
                assert bit_equal(s.download(c), ref.download(c)), f"{name}: channel {c}, {'after reset' if again else 'first run'}"
            s.reset()


@pytest.mark.gpu
def test_solver_from_a_file_in_device_memory(lib):
    import torch
    import jpeg2png_amd as j
    case = sc.case("rgb420_64x48")
    data, planes = file_of(case)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    with j.Solver.from_jpeg(buf, case.weight, case.pweight, 4) as s, j.Solver.from_jpeg(data, case.weight, case.pweight, 4) as host:
        s.run(4)
        host.run(4)
        for c in range(3):
            assert np.array_equal(s.download_coefficients(c), host.download_coefficients(c))
            assert bit_equal(s.download(c), host.download(c))


@pytest.mark.gpu
def test_a_damaged_file_makes_no_solver_and_spoils_nothing(lib):
    import jpeg2png_amd as j
    bad, _ = dc.damaged_cases()["rst_removed"]
    with pytest.raises(j.J2PError) as e:
        j.Solver.from_jpeg(bad, 0.3, [0.001] * 3, 4)
    assert e.value.code == j.J2P_EFORMAT
    case = sc.case("rgb444_48x32_q50")
    data, planes = file_of(case)
    with j.Solver.from_jpeg(data, case.weight, case.pweight, 2) as s:
        assert np.array_equal(s.download_coefficients(0), np.asarray(planes[0].data).reshape(planes[0].h // 8, planes[0].w // 8, 64))


# ---- batch jobs ----
def _device_file(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.mark.gpu
def test_batch_file_jobs_equal_coefficient_jobs(lib):
    """Batch.submit(file=) against Batch.submit(planes): float planes (joint and separate), bits=8 samples, a tensor, and a job that
    also delivers a file (jpeg=: file in, file out), the file in host memory and in device memory, all in flight together"""
    import torch
    import jpeg2png_amd as j
    want, got = {}, {}
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets, held = [], []
        for name in ("rgb420_64x48", "rgb444_48x32_q50", "y_48x40_tgv"):
            case = sc.case(name)
            data, planes = file_of(case)
            n = len(planes)
            W, H = planes[0].w, planes[0].h
            args = (case.weight, case.pweight[:n], 50)
            dev = _device_file(torch, data)
            held.append(dev)
            jpeg = {"quality": 90, "subsampling": (2, 2) if n == 3 else (1, 1)}
            for kind, kw in (("planes", {}), ("separate", {"separate": True}), ("rgb", {"bits": 8, "width": W, "height": H}),
                             ("jpeg", {"jpeg": jpeg, "width": W, "height": H})):
                tickets.append((want, (name, kind), b.submit(planes, *args, **kw)))
                tickets.append((got, (name, kind, "host"), b.submit(None, *args, file=data, **kw)))
                tickets.append((got, (name, kind, "device"), b.submit(None, *args, file=dev, **kw)))
            for where, key, f in ((want, (name, "tensor"), None), (got, (name, "tensor", "host"), data), (got, (name, "tensor", "device"), dev)):
                t = torch.zeros((n, H, W), device="cuda")
                tickets.append((where, key, b.submit(planes if f is None else None, *args, width=W, height=H, tensor=t, file=f)))
        for where, key, t in tickets:
            where[key] = b.wait(t)
    assert len(got) == 2 * len(want) == 30
    for (name, kind, form), have in got.items():
        ref = want[(name, kind)]
        label = f"{name}: {kind}, {form} file"
        if kind in ("planes", "separate"):
            assert len(have) == len(ref) and all(bit_equal(a, r) for a, r in zip(have, ref)), label
        elif kind == "rgb":
            assert have.shape == ref.shape and np.array_equal(have, ref) and ref.any(), label
        elif kind == "jpeg":
            assert len(ref) > 300 and have == ref, label
        else:
            assert bit_equal(have.cpu().numpy(), ref.cpu().numpy()) and ref.any().item(), label


@pytest.mark.gpu
def test_batch_file_job_with_outputs_sizes_left_to_the_file_and_component_0_alone(lib):
    import torch
    import jpeg2png_amd as j
    case = sc.case("rgb420_64x48")
    data, planes = file_of(case)
    specs = [{"out_width": 24, "out_height": 16, "filter": "triangle"}, {"out_width": 80, "out_height": 50, "filter": "cubic", "layout": "hwc"}]

    def outputs():
        return [dict(o, tensor=t) for o, t in zip(specs, (torch.full((3, 16, 24), 7.0, device="cuda"), torch.full((50, 80, 3), 7.0, device="cuda")))]

    args = (case.weight, case.pweight, 6)
    with j.Batch(devices=(0,), slots_per_device=2) as b:
        a = b.submit(planes, *args, width=64, height=48, outputs=outputs())
        f = b.submit(None, *args, outputs=outputs(), file=data)                   # width and height: the file's
        grey_c = b.submit(planes[:1], 0.3, [0.001], 6, bits=8, width=64, height=48)
        grey_f = b.submit(j.jpeg_header(data)["planes"][:1], 0.3, [0.001], 6, bits=8, file=data)     # component 0 of a colour file
        ta, tf, ga, gf = b.wait(a), b.wait(f), b.wait(grey_c), b.wait(grey_f)
        for i in range(2):
            assert bit_equal(tf[i].cpu().numpy(), ta[i].cpu().numpy()) and not (ta[i] == 7.0).all().item()
        assert ga.shape == (48, 64) and np.array_equal(ga, gf)
        # refused at submit
        with pytest.raises(j.J2PError, match="tile"):
            b.submit(None, *args, file=data, tile=True)
        with pytest.raises(j.J2PError, match="samples"):
            b.submit(None, *args, file=data, samples=[np.zeros((8, 8), np.uint8)] * 3)
        with pytest.raises(j.J2PError, match="neither data nor fdata"):
            b.submit(planes, *args, file=data)
        wrong = j.jpeg_header(data)["planes"]
        wrong[1].w += 8
        with pytest.raises(j.J2PError, match="the file's component") as e:
            b.submit(wrong, *args, file=data)
        assert e.value.code == -1
        progressive_like = data.replace(b"\xff\xc0", b"\xff\xc2", 1)
        with pytest.raises(j.J2PError) as e:
            b.submit(None, *args, file=progressive_like)
        assert e.value.code == j.J2P_ENOTSUP


@pytest.mark.gpu
def test_a_damaged_file_fails_its_own_job_and_not_its_neighbours(lib):
    import jpeg2png_amd as j
    case = sc.case("rgb444_48x32_q50")
    data, planes = file_of(case)
    frame = dc.parse(data)
    n = frame["scan_end"] - frame["scan_begin"]
    bad = data[:frame["scan_begin"] + n * 2 // 3] + b"\xff\xd9"                  # the headers are whole: only the data shows it
    args = (case.weight, case.pweight, 10)
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = [b.submit(None, *args, file=data), b.submit(None, *args, file=bad), b.submit(planes, *args), b.submit(None, *args, file=data),
                   b.submit(None, *args, file=bad, bits=8)]
        with pytest.raises(j.J2PError) as e:
            b.wait(tickets[1])
        assert e.value.code == j.J2P_EFORMAT
        with pytest.raises(j.J2PError) as e:
            b.wait(tickets[4])
        assert e.value.code == j.J2P_EFORMAT
        ref = b.wait(tickets[2])
        for t in (tickets[0], tickets[3]):
            assert all(bit_equal(a, r) for a, r in zip(b.wait(t), ref))
        again = b.wait(b.submit(None, *args, file=data))                        # ... and the workers that refused go on working
        assert all(bit_equal(a, r) for a, r in zip(again, ref))
