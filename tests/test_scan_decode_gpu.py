"""Reading a progressive JPEG file on the GPU (k_unstuff_* per scan, k_scans_*; j2p_entropy_decode_scans,
j2p_solver_create_from_jpeg_scans, j2p_batch_next_file_scans; the progressive= keyword of jpeg2png_amd.entropy_decode,
Solver.from_jpeg and Batch.submit): every comparison is exact, with the arrays of the plain-Python restatement in
tests/scan_decode_cases.py, which tests/test_scan_decode_cpu.py holds against libjpeg.  The files are small: PIL's of up to 83x61
pixels, the progressive coder's directed cases (the EOB-run flush at 32767, the 937-bit correction limit, refinement ZRLs, the scan
endings), and writer-made scripts (spectral selection alone, DC scans one component at a time, Al 3 refined down to 0, a script
that stops at Al 1, 128 scans), and the edge_ files of scan_decode_cases.edge_cases(): writer-made scripts with restart intervals,
1028 intervals of first scans and 257 of refinement scans, markers and fill bytes on the unstuffing kernels' edges counted from a
later scan's begin, Al 13 refined to 0, DC at the int16 limits.  The damaged files each have one fault that one kernel alone can
refuse, and the text of the refusal is the one that belongs to the restatement's reason.  At 32 bits a subsequence every boundary
is crossed: an EOBn symbol and its extra bits, a symbol that ends a band, the last symbol of an interval; 75 is a length no power
of two divides."""
import ctypes

import numpy as np
import pytest

import decode_cases as dc
import entropy_cases as ec
import scan_decode_cases as sc
from conftest import bit_equal
from test_jpeg_out_gpu import read_coefficients  # noqa: F401

J2P_EFORMAT, J2P_ENOTSUP = -6, -7
LENGTHS = (0, 32, 75, 1024)             # the default, J2P_DECODE_SUBSEQUENCE_MIN, an odd one, the default given
GROUPS = ("pil_L0", "pil_RGB0", "pil_RGB1", "pil_RGB2", "coder", "written", "edge")


def group(name):
    """the good files of a group"""
    files = sc.good_files()
    if name.startswith("pil_"):
        return sorted(n for n in files if n.startswith("pil_") and f"_{name[4:]}_" in n)
    return sorted(n for n in files if n.startswith(name + "_"))


def c_decode(lib, data, shapes, bits=0, fill=0x5A5A, address=None):
    """j2p_entropy_decode_scans into arrays pre-filled with `fill` -> (rc, arrays, stats)"""
    import jpeg2png_amd as j
    raw = np.frombuffer(data, dtype=np.uint8)
    arrays = [np.full(s, fill, dtype=np.int16) for s in shapes]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in arrays])
    stats = j._CScansStats()
    rc = lib.j2p_entropy_decode_scans(0, raw.ctypes.data if address is None else address, raw.size, ptrs, None, None, bits, ctypes.byref(stats))
    return rc, arrays, stats


def check(name, got, want):
    assert len(got) == len(want), name
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, f"{name}: component {c}: {a.shape} {b.shape}"
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)[0]
            raise AssertionError(f"{name}: component {c}: {len(np.argwhere(a != b))} values differ, the first at {tuple(at)}: {a[tuple(at)]} for {b[tuple(at)]}")


def test_the_groups_hold_every_file():
    assert sorted(n for g in GROUPS for n in group(g)) == sorted(sc.good_files())


@pytest.mark.gpu
@pytest.mark.parametrize("bits", LENGTHS)
@pytest.mark.parametrize("which", GROUPS)
def test_entropy_decode_scans_is_the_restatement(lib, which, bits):
    files = sc.good_files()
    for name in group(which):
        want = sc.expected(name)
        rc, got, stats = c_decode(lib, files[name], [a.shape for a in want], bits=bits)
        assert rc == 0, f"{name} at {bits} bits: {lib.j2p_last_error().decode()}"
        check(f"{name} at {bits} bits", got, want)
        assert stats.scans == len(sc.parse_scans(files[name])["scans"]) == stats.dc_first + stats.ac_first + stats.dc_refine + stats.ac_refine, name


@pytest.mark.gpu
def test_a_sequential_file_goes_the_old_way(lib):
    data = dc.write_case(ec.make(41, 23, 3, (2, 2), "sparse", seed=5), restart=2)
    want, _ = dc.decode(data)
    rc, got, stats = c_decode(lib, data, [a.shape for a in want])
    assert rc == 0, lib.j2p_last_error().decode()
    check("sequential", got, want)
    assert stats.scans == 1


@pytest.mark.gpu
def test_a_file_in_device_memory_gives_the_same(lib):
    import torch
    import jpeg2png_amd as j
    files = sc.good_files()
    for name in ("pil_83x61_q95_RGB2_rst_blocks", "coder_refine_zrl", "written_dc_alone_17x9"):
        data = files[name]
        # (one byte into an allocation: the scans are read in place at whatever address they have)
        buf = torch.zeros(len(data) + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        check(name, j.entropy_decode(buf[1:], progressive=True), sc.expected(name))
        check(name + ", host", j.entropy_decode(data, progressive=True), sc.expected(name))


def _longest_interval_subsequences(data, bits):
    """the subsequences of the longest restart interval of a first scan"""
    most = 0
    for s in sc.parse_scans(data)["scans"]:
        if s["ah"] == 0:
            chunks, _ = dc._intervals(data[s["begin"]:s["end"]])
            most = max(most, max(-(-len(c) * 8 // bits) for c in chunks))
    return most


@pytest.mark.gpu
def test_stats(lib):
    import jpeg2png_amd as j
    files = sc.good_files()
    for name in ("pil_83x61_q100_RGB2_plain", "pil_83x61_q95_L0_rst_rows", "coder_dense_368x368_420"):
        for bits in (32, 75, 1024):
            got, stats = j.entropy_decode(files[name], subsequence_bits=bits, stats=True, progressive=True)
            check(name, got, sc.expected(name))
            assert 1 <= stats["rounds"] <= _longest_interval_subsequences(files[name], bits), (name, bits, stats)
            assert stats["data_bytes"] == sum(s["end"] - s["begin"] for s in sc.parse_scans(files[name])["scans"])
            assert stats["decode_ms"] > 0 and 0 < stats["ac_refine_share"] < 1, stats
    # the host waits do not grow with the scans: a 3-scan and a 10-scan file of one image
    case = ec.make(16, 16, 3, (2, 2), "sparse", seed=3)
    three = sc.write_case(case, [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)])
    ten = sc.write_case(case)
    waits = []
    for data, n in ((three, 3), (ten, 10)):
        got, stats = j.entropy_decode(data, stats=True, progressive=True)
        check(f"{n} scans", got, sc.decode(data)[0])
        assert stats["scans"] == n
        waits.append(stats["host_waits"])
    assert waits[0] == waits[1] == 2, waits


DAMAGED = ("scan_cut_short", "eob_run_one_too_long", "refinement_symbol_of_two_bits", "run_past_se", "restart_out_of_sequence",
           "byte_behind_dc_refinement",
           "dc_above_int16_al0", "dc_below_int16_al0", "dc_above_int16_al1", "dc_below_int16_al1",
           "dc_refine_interval_short_next_long", "dc_refine_byte_behind_interval", "dc_refine_rst_removed", "dc_refine_rst_renumbered",
           "eob_run_crosses_restart_refine", "eob_run_crosses_restart_first", "refine_run_past_band", "refine_zrl_past_band", "first_zrl_past_band",
           "refine_byte_behind_interval", "refine_interval_cut_short", "refine_rst_removed", "refine_rst_doubled", "refine_code_in_no_table")
# what the library says of a file the restatement refuses for this reason (written from the restatement's reasons and the header's
# account of the refusals: a file with one fault has one text)
_ENDS = "the scan is truncated, or data is left over behind its last block"
WHY_TEXT = {"restart": "a restart marker is missing or out of sequence", "code": "a code that is in no Huffman table", "run": "a run past coefficient 63",
            "truncated": _ENDS, "leftover": _ENDS, "dc": "a DC value outside int16", "refine": "a refinement scan's symbol of more than one bit",
            "eobrun": "an EOB run past the last block of its restart interval"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_files_are_refused(lib, name):
    """J2P_EFORMAT with the text of the file's one fault, the pre-filled output untouched, and a good decode afterwards in the same process"""
    assert sorted(DAMAGED) == sorted(sc.damaged_cases())
    data, whys = sc.damaged_cases()[name]
    comps, _, _ = dc.geometry(sc.parse_scans(data))
    for bits in (0, 32, 75):
        rc, got, _ = c_decode(lib, data, [(gh, gw, 64) for gh, gw, _, _ in comps], bits=bits)
        assert rc == J2P_EFORMAT, f"{name} at {bits} bits: {rc} {lib.j2p_last_error().decode()}"
        assert lib.j2p_last_error().decode() in {"jpeg: " + WHY_TEXT[why] for why in whys}, f"{name} at {bits} bits: {lib.j2p_last_error().decode()}"
        assert all((a == 0x5A5A).all() for a in got), name
    ok = "pil_41x23_q75_RGB2_plain"
    want = sc.expected(ok)
    rc, got, _ = c_decode(lib, sc.good_files()[ok], [a.shape for a in want])
    assert rc == 0, lib.j2p_last_error().decode()
    check("after " + name, got, want)


# ---- solvers ----
def _baseline_of(data):
    """the baseline file that holds the coefficients of a progressive one"""
    arrays, p = sc.decode(data)
    comps = p["components"]
    sub = (comps[0][1] // comps[1][1], comps[0][2] // comps[1][2]) if len(comps) == 3 else (1, 1)
    quant = [p["quant"][c[3]] for c in comps]
    return dc.write(arrays, p["width"], p["height"], quant, sub, restart=3, tables="own")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("pil_83x61_q75_RGB2_plain", "pil_45x38_q95_RGB1_rst_blocks"))
def test_solver_from_a_progressive_file(lib, read_coefficients, tmp_path, name):  # noqa: F811
    """plane for plane after 5 iterations: the solver made from libjpeg's coefficients of the file, and Solver.from_jpeg of the
    baseline file that holds the same coefficients"""
    import jpeg2png_amd as j
    from test_jpeg_out_cli import load_coefficients
    data = sc.good_files()[name]
    path = str(tmp_path / "file.jpg")
    open(path, "wb").write(data)
    _w, _h, planes = load_coefficients(read_coefficients, path)
    args = (0.3, [0.001] * 3, 5)
    with pytest.raises(j.J2PError) as e:
        j.Solver.from_jpeg(data, *args)
    assert e.value.code == J2P_ENOTSUP
    with j.Solver(planes, *args) as ref, j.Solver.from_jpeg(data, *args, progressive=True) as s, j.Solver.from_jpeg(_baseline_of(data), *args) as base:
        assert (s.W, s.H, s.nch) == (ref.W, ref.H, 3) and s.jpeg["progressive"]
        for t in (ref, s, base):
            t.run(5)
        for c in range(3):
            assert np.array_equal(s.download_coefficients(c), np.asarray(planes[c].data).reshape(planes[c].h // 8, planes[c].w // 8, 64)), f"channel {c}"
            assert bit_equal(s.download(c), ref.download(c)), f"{name}: channel {c} against libjpeg's coefficients"
            assert bit_equal(s.download(c), base.download(c)), f"{name}: channel {c} against the baseline file"


@pytest.mark.gpu
def test_a_damaged_progressive_file_makes_no_solver(lib):
    import jpeg2png_amd as j
    bad, _ = sc.damaged_cases()["run_past_se"]
    with pytest.raises(j.J2PError) as e:
        j.Solver.from_jpeg(bad, 0.3, [0.001], 4, progressive=True)
    assert e.value.code == J2P_EFORMAT
    name = "pil_41x23_q75_L0_plain"
    with j.Solver.from_jpeg(sc.good_files()[name], 0.3, [0.001], 2, progressive=True) as s:
        assert np.array_equal(s.download_coefficients(0), sc.expected(name)[0])


# ---- batch jobs ----
@pytest.mark.gpu
def test_a_file_damaged_in_its_last_scan_fails_its_own_job_and_not_its_neighbours(lib):
    """the fault sits in the last AC refinement scan: the launches that end the decode find it, behind everything the file's other
    scans queued.  The jobs in front of it and behind it give what they give alone, bit for bit"""
    import jpeg2png_amd as j
    bad, _ = sc.damaged_cases()["eob_run_crosses_restart_refine"]
    last = sc.parse_scans(bad)["scans"][-1]
    assert last["ss"] and last["ah"] and last["intervals"] > 1
    with pytest.raises(sc.Refused):
        sc.decode(bad)
    good = [sc.good_files()[name] for name in ("edge_eob_run_ends_each_interval", "pil_41x23_q75_L0_rst_blocks")]
    args = (0.3, [0.001], 6)
    alone = []
    for data in good:
        with j.Batch(devices=(0,), slots_per_device=1) as b:
            alone.append(b.wait(b.submit(None, *args, file=data, progressive=True)))
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = [b.submit(None, *args, file=data, progressive=True) for data in (good[0], bad, good[1])]
        with pytest.raises(j.J2PError) as e:
            b.wait(tickets[1])
        assert e.value.code == J2P_EFORMAT
        for t, ref in zip((tickets[0], tickets[2]), alone):
            got = b.wait(t)
            assert len(got) == len(ref) == 1 and all(bit_equal(a, r) for a, r in zip(got, ref))
        again = b.wait(b.submit(None, *args, file=good[0], progressive=True))           # ... and the worker that refused goes on working
        assert all(bit_equal(a, r) for a, r in zip(again, alone[0]))
    assert alone[0][0].shape != alone[1][0].shape and all(np.asarray(a[0]).any() for a in alone)       # (two images, neither blank)


@pytest.mark.gpu
def test_batch_progressive_file_jobs_equal_baseline_file_jobs(lib):
    """Batch.submit(file=, progressive=True) against the same job from the baseline file of the same coefficients: joint, separate,
    grey of colour, and bytes in and bytes out (jpeg={"progressive": True}), whose decode returns what the coder was given"""
    import torch
    import jpeg2png_amd as j
    data = sc.good_files()["pil_83x61_q75_RGB2_plain"]
    base = _baseline_of(data)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    args = (0.3, [0.001] * 3, 6)
    jpeg = {"quality": 90, "subsampling": (2, 2), "progressive": True}
    grey = j.jpeg_header(base)["planes"][:1]
    want, got = {}, {}
    with j.Batch(devices=(0,), slots_per_device=3) as b:
        tickets = []
        for kind, planes, a, kw in (("joint", None, args, {}), ("separate", None, args, {"separate": True}),
                                    ("grey", grey, (0.3, [0.001], 6), {"bits": 8}), ("jpeg", None, args, {"jpeg": jpeg, "width": 83, "height": 61})):
            tickets.append((want, kind, b.submit(planes, *a, file=base, **kw)))
            tickets.append((got, (kind, "host"), b.submit(planes, *a, file=data, progressive=True, **kw)))
            tickets.append((got, (kind, "device"), b.submit(planes, *a, file=dev, progressive=True, **kw)))
        # without the keyword the same submit is refused as before, and takes nothing from the next one
        with pytest.raises(j.J2PError) as e:
            b.submit(None, *args, file=data)
        assert e.value.code == J2P_ENOTSUP
        for where, key, t in tickets:
            where[key] = b.wait(t)
    for (kind, form), have in got.items():
        ref = want[kind]
        label = f"{kind}, {form} file"
        if kind in ("joint", "separate"):
            assert len(have) == len(ref) == 3 and all(bit_equal(a, r) for a, r in zip(have, ref)), label
        elif kind == "grey":
            assert have.shape == ref.shape and np.array_equal(have, ref) and ref.any(), label
        else:
            assert len(ref) > 300 and have == ref, label
    # the file that came out goes in again: the device's decoder returns what its coder was given, as the restatement reads it
    out = got[("jpeg", "host")]
    assert sc.parse_scans(out)["progressive"] and len(sc.parse_scans(out)["scans"]) == 10
    check("the output, decoded", j.entropy_decode(out, progressive=True), sc.decode(out)[0])
