"""What Batch.submit refuses by itself, before it needs a batch or a device: every case of job_refusal_cases.PYTHON raises its
J2PError with its full text from the unbound method on a bare object."""
import pytest

import job_refusal_cases as rc


@pytest.mark.parametrize("case", rc.PYTHON, ids=[c.name for c in rc.PYTHON])
def test_submit_refuses_in_these_words_without_a_device(lib, case):
    import jpeg2png_amd as j
    planes = rc.planes()[:2] if case.planes == "two" else rc.planes()
    keywords = dict(dict(width=rc.WIDTH, height=rc.HEIGHT), **case.keywords)
    with pytest.raises(j.J2PError) as e:
        j.Batch.submit(object.__new__(j.Batch), planes, rc.WEIGHT, rc.PWEIGHT[:len(planes)], rc.ITERATIONS, **keywords)
    assert str(e.value) == case.message and e.value.code is None


def test_the_table_names_every_refusal_of_submit_once():
    """the messages are literals: none of them stands twice under one name, and every name is used once"""
    assert len({c.name for c in rc.PYTHON}) == len(rc.PYTHON)
    assert len({c.name for c in rc.RAW}) == len(rc.RAW)
    assert all(c.stage in ("submit", "wait") and c.rc < 0 and c.message for c in rc.RAW)
