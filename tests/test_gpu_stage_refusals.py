"""Every case of tests/stage_refusals.py through the C ABI of the built library: the code and the text of the sixteen asynchronous
entry points of the roll and the zoom/crop stage are the recorded ones (tests/golden/stage_refusals.json, written by
tests/golden/make_stage_refusals.py from the commit before both stages were restated on the plane list), byte for byte."""
import json
import os

import pytest

import stage_refusals as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_refusals.json")


@pytest.fixture(scope="module")
def golden():
    rows = json.load(open(GOLDEN))
    want = {(entry, case): (rc, text) for entry, case, rc, text in rows}
    assert len(want) == len(rows)
    return want


@pytest.fixture(scope="module")
def buffers(gpu):
    return sr.buffers(gpu)


def test_the_record_holds_what_the_table_states(golden):
    asked = set()
    for stage, fam, many, c in sr.every_case():
        key = (sr.entry_name(stage, fam, many), c.name)
        asked.add(key)
        rc, text = golden[key]
        assert rc == c.rc and c.word in text, key
    assert asked == set(golden)


@pytest.mark.gpu
@pytest.mark.parametrize("stage,fam,many", sr.ENTRIES, ids=[sr.entry_name(*e) for e in sr.ENTRIES])
def test_library_answers_as_recorded(gpu, golden, buffers, stage, fam, many):
    todo = sr.cases(stage, fam, many)
    assert todo
    wrong = []
    for c in todo:
        got = sr.ask(gpu, stage, fam, many, c, *buffers)
        want = golden[(sr.entry_name(stage, fam, many), c.name)]
        if got != want:
            wrong.append((c.name, got, want))
    assert not wrong, "%d of %d differ, e.g. %r" % (len(wrong), len(todo), wrong[:5])
