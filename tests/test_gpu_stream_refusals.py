"""Every case of tests/refusal_cases.py through the C ABI of the built library, the stateful probes included: the code and the text
are the recorded ones (tests/golden/stream_refusals.json), byte for byte."""
import os

import pytest

import refusal_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_refusals.json")


@pytest.fixture(scope="module")
def golden():
    return refusal_cases.load_golden(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("name", refusal_cases.NAMES + ("unknown",))
def test_library_answers_as_recorded(gpu, golden, name):
    todo = refusal_cases.cases(name)
    assert todo
    wrong = []
    for c in todo:
        got = refusal_cases.drive(gpu, c)
        if got != golden[c.id]:
            wrong.append((c.id, got, golden[c.id]))
    assert not wrong, "%d of %d differ, e.g. %r" % (len(wrong), len(todo), wrong[:5])
