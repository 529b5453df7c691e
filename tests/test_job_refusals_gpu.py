"""Every refusal of the batch's C entry points — job_refusal_cases.RAW — at its stage, with its return code and its full message,
through _CJob and raw ctypes calls; after each refused job a good job on the same batch still succeeds."""
import ctypes

import pytest

import job_refusal_cases as rc
from conftest import bit_equal

J2P_OK = 0


@pytest.fixture(scope="module")
def kit(lib):
    import torch
    import jpeg2png_amd as j
    assert torch.cuda.is_available()
    return rc.Kit(j, torch)


@pytest.fixture(scope="module")
def batch(lib):
    """one batch on device 0 with 2 slots, as a raw handle"""
    h = ctypes.c_void_p()
    devices = (ctypes.c_int * 1)(0)
    assert lib.j2p_batch_create(ctypes.byref(h), 1, devices, 2) == J2P_OK
    yield h
    lib.j2p_batch_destroy(h)


def good_job(lib, batch, kit):
    """the planes of a job with nothing wrong"""
    for a in kit.float_planes:
        a[:] = -1.0
    ticket = ctypes.c_int(-5)
    assert lib.j2p_batch_submit(batch, kit.job(), ctypes.byref(ticket)) == J2P_OK, lib.j2p_last_error()
    assert ticket.value > 0
    assert lib.j2p_batch_wait(batch, ticket.value) == J2P_OK, lib.j2p_last_error()
    return [a.copy() for a in kit.float_planes]


@pytest.fixture(scope="module")
def good(lib, batch, kit):
    import jpeg2png_amd as j
    got = good_job(lib, batch, kit)
    with j.Solver(rc.planes(), rc.WEIGHT, rc.PWEIGHT, rc.ITERATIONS) as s:
        s.run(rc.ITERATIONS)
        for c in range(3):
            assert bit_equal(got[c], s.download(c)), f"channel {c}"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.RAW, ids=[c.name for c in rc.RAW])
def test_refused_at_its_stage_with_its_code_and_words(lib, batch, kit, good, case):
    import jpeg2png_amd as j
    if j.device_count() < case.gpus:
        pytest.skip(f"needs {case.gpus} GPUs")
    if "managed" in case.name and kit.managed() is None:
        pytest.skip("the runtime gives no managed memory")
    entry, args = case.build(kit)
    ticket = ctypes.c_int(-5)
    rcode = getattr(lib, entry)(batch, *args, ctypes.byref(ticket))
    if case.stage == "submit":
        assert (rcode, lib.j2p_last_error().decode()) == (case.rc, case.message)
        assert ticket.value == -5
    else:
        assert rcode == J2P_OK, lib.j2p_last_error()
        assert (lib.j2p_batch_wait(batch, ticket.value), lib.j2p_last_error().decode()) == (case.rc, case.message)
        # (the ticket is spent)
        assert (lib.j2p_batch_wait(batch, ticket.value), lib.j2p_last_error().decode()) == (rc.J2P_EINVAL, f"unknown ticket {ticket.value}")
    again = good_job(lib, batch, kit)
    assert all(bit_equal(a, b) for a, b in zip(again, good))


@pytest.mark.gpu
def test_wait_refuses_what_it_does_not_know(lib, batch):
    assert (lib.j2p_batch_wait(batch, 12345), lib.j2p_last_error().decode()) == (rc.J2P_EINVAL, "unknown ticket 12345")
    assert (lib.j2p_batch_wait(None, 1), lib.j2p_last_error().decode()) == (rc.J2P_EINVAL, "batch is NULL")
    ticket = ctypes.c_int(-5)
    assert (lib.j2p_batch_submit(None, None, ctypes.byref(ticket)), lib.j2p_last_error().decode()) == (rc.J2P_EINVAL, "NULL argument")


@pytest.mark.gpu
def test_degenerate_arguments_are_the_plain_forms(lib, batch, kit, good):
    """no outputs (n == 0, or outs NULL) is the job's own output; samples NULL in j2p_batch_submit_jpeg means the planes' coefficients"""
    import jpeg2png_amd as j

    def planes_of(entry, *args):
        for a in kit.float_planes:
            a[:] = -1.0
        ticket = ctypes.c_int(-5)
        assert getattr(lib, entry)(batch, *args, ctypes.byref(ticket)) == J2P_OK, lib.j2p_last_error()
        assert lib.j2p_batch_wait(batch, ticket.value) == J2P_OK, lib.j2p_last_error()
        return [a.copy() for a in kit.float_planes]

    _n, outs = kit.outputs()
    for entry, args in (("j2p_batch_submit_outputs", [kit.job(), 0, outs]), ("j2p_batch_submit_outputs", [kit.job(), 2, None]),
                        ("j2p_batch_submit_resized", [kit.job(), None]), ("j2p_batch_submit_resampled", [kit.job(), None])):
        assert all(bit_equal(a, b) for a, b in zip(planes_of(entry, *args), good)), (entry, args[1:])
    from_file = planes_of("j2p_batch_submit_file", kit.job(bare=True), *kit.file, 2, None)
    with j.Solver.from_jpeg(kit.file_bytes.tobytes(), rc.WEIGHT, rc.PWEIGHT, rc.ITERATIONS) as s:
        s.run(rc.ITERATIONS)
        assert all(bit_equal(from_file[c], s.download(c)) for c in range(3))
    spec, out, capacity, size = kit.jpeg()
    planes_of("j2p_batch_submit_jpeg", kit.job(**kit.image()), None, spec, out, capacity, size)
    with j.Solver(rc.planes(), rc.WEIGHT, rc.PWEIGHT, rc.ITERATIONS) as s:
        s.run(rc.ITERATIONS)
        want = s.to_jpeg(rc.WIDTH, rc.HEIGHT, quality=90, subsampling=(2, 2))
    got = ctypes.string_at(out, size._obj.value)
    assert got == want and got[:2] == b"\xff\xd8"
