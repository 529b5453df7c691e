"""The sixteen calls that write a JPEG file — j2p_entropy_encode, j2p_planes_to_jpeg, j2p_batch_submit_jpeg and
j2p_batch_submit_file_jpeg, each plain, _ex, _progressive and _opt — are one call with a j2p_jpeg_options record and twelve shorthands
for it (include/jpeg2png_amd.h).  What each refuses before it needs a device, a solver or a batch, it refuses with the return code and
the text it had while every family had code of its own: the texts below were taken from that library, the batch's from
tests/job_refusal_cases.py.  (What a batch job's record is refused for needs a batch, and so a device: tests/test_restart_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import job_refusal_cases as jr

J2P_EINVAL = -1
NO_SPEC = "jpeg: spec is NULL"
NO_OPTIONS = "jpeg: NULL options"
FLAG_BITS = "jpeg: unknown flag bits"
PROGRESSIVE_2 = "jpeg: progressive is 0 or 1"
BOTH_SET = "jpeg: restart_interval and restart_in_rows are both set"
JOB_NO_SPEC = next(c.message for c in jr.RAW if c.name == "JPEG without a spec")
JOB_NO_OPTIONS = "job: jpeg: options is NULL"
NULL_ARGUMENT = "NULL argument"

FAMILIES = ("j2p_entropy_encode", "j2p_planes_to_jpeg", "j2p_batch_submit_jpeg", "j2p_batch_submit_file_jpeg")
FORMS = ("", "_ex", "_progressive", "_opt")


class Parts:
    """the arguments of a call that no check before the refusal in question objects to; what they point to lives as long as this"""

    def __init__(self, j):
        self.j = j
        self.spec, self.held = j._c_jpeg(17, 9, 1, 75, None, (1, 1))
        self.coefficients = np.zeros((2, 3, 64), np.int16)
        self.ptrs = (ctypes.c_void_p * 3)(self.coefficients.ctypes.data)
        self.refs = (j._CPlaneRef * 3)()        # (no solver behind them: the refusals here come first)
        self.out = np.full(256, 0xA5, np.uint8)
        self.size, self.ticket = ctypes.c_size_t(77), ctypes.c_int(-7)
        self.job = j._CJob()
        self.file = np.frombuffer(b"\xff\xd8 no batch ever opens this", dtype=np.uint8)

    def call(self, lib, family, form, spec=True, options=(0, 0, 0, 0), flags=0):
        """family + form with these: -> (rc, the library's text).  options None: a NULL record (_opt)"""
        record = None if options is None else self.j._CJpegOptions(*options)
        spec = ctypes.byref(self.spec) if spec else None
        to = (self.out.ctypes.data, self.out.size, ctypes.byref(self.size))
        last = {"": (), "_ex": (flags,), "_progressive": (), "_opt": (None if record is None else ctypes.byref(record),)}[form]
        if family == "j2p_entropy_encode":
            args = (0, spec, self.ptrs, 1) + to + last + {"": (), "_ex": (None,), "_progressive": (None,), "_opt": (None, None, None)}[form]
        elif family == "j2p_planes_to_jpeg":
            args = (self.refs, 1, spec) + to + last
        elif family == "j2p_batch_submit_jpeg":         # (no batch: what these refuse before submit looks at it)
            args = (None, ctypes.byref(self.job), None, spec) + to + last + (ctypes.byref(self.ticket),)
        else:
            args = (None, ctypes.byref(self.job), self.file.ctypes.data, self.file.size, spec) + to + last + (ctypes.byref(self.ticket),)
        rc = getattr(lib, family + form)(*args)
        assert (self.out == 0xA5).all() and self.size.value == 77 and self.ticket.value == -7, "a refused call wrote something"
        return rc, lib.j2p_last_error().decode()


@pytest.fixture(scope="module")
def parts(lib):
    import jpeg2png_amd as j
    return Parts(j)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
def test_a_null_spec_is_refused_in_the_familys_words(lib, parts, family, form):
    want = JOB_NO_SPEC if "batch" in family else NO_SPEC
    assert parts.call(lib, family, form, spec=False) == (J2P_EINVAL, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_null_record_is_refused_after_a_null_spec(lib, parts, family):
    want = JOB_NO_OPTIONS if "batch" in family else NO_OPTIONS
    assert parts.call(lib, family, "_opt", options=None) == (J2P_EINVAL, want)
    if "batch" in family:       # (the spec first)
        assert parts.call(lib, family, "_opt", spec=False, options=None) == (J2P_EINVAL, JOB_NO_SPEC)
    else:                       # (the record first: what is wrong with it is said before the spec is looked at)
        assert parts.call(lib, family, "_opt", spec=False, options=None) == (J2P_EINVAL, NO_OPTIONS)


@pytest.mark.parametrize("family", FAMILIES[:2])
def test_what_is_wrong_with_the_record_is_said_in_its_order_and_before_the_spec(lib, parts, family):
    for spec in (True, False):
        assert parts.call(lib, family, "_ex", spec=spec, flags=2) == (J2P_EINVAL, FLAG_BITS)
        assert parts.call(lib, family, "_ex", spec=spec, flags=0x80000001) == (J2P_EINVAL, FLAG_BITS)
        for options, want in (((2, 0, 0, 0), FLAG_BITS), ((0, 2, 0, 0), PROGRESSIVE_2), ((0, 1, 1, 1), BOTH_SET), ((1, 0, 3, 2), BOTH_SET),
                              ((2, 2, 1, 1), FLAG_BITS), ((1, 2, 1, 1), PROGRESSIVE_2)):
            assert parts.call(lib, family, "_opt", spec=spec, options=options) == (J2P_EINVAL, want), options


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES[2:])
def test_a_good_record_without_a_batch_gets_as_far_as_submit(lib, parts, family, form):
    """every batch entry point hands its record on: the next refusal is submit's own"""
    assert parts.call(lib, family, form, flags=1, options=(1, 1, 0, 5)) == (J2P_EINVAL, NULL_ARGUMENT)


@pytest.mark.parametrize("family", FAMILIES[2:])
def test_the_record_of_a_batch_job_is_not_looked_at_before_there_is_a_batch(lib, parts, family):
    assert parts.call(lib, family, "_ex", flags=2) == (J2P_EINVAL, NULL_ARGUMENT)
    assert parts.call(lib, family, "_opt", options=(0, 2, 1, 1)) == (J2P_EINVAL, NULL_ARGUMENT)
