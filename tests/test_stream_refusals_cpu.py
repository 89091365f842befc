"""The refusal rules of csrc/pixfmt.h, asked without a stream (tests/cpp/pixfmt_check.cpp), answer every case of tests/refusal_cases.py
as the library was recorded to answer it (tests/golden/stream_refusals.json): the same code, the same text, byte for byte."""
import os

import pixfmt_check
import refusal_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_refusals.json")


def test_the_stateful_cases_are_the_allocation_probes():
    all_cases = refusal_cases.cases()
    st = [c for c in all_cases if refusal_cases.stateful(c)]
    assert st and all(c.entry == "probe" and c.id.split("/")[1] in ("in.refused", "out.refused") for c in st)
    assert len([c for c in st if c.id.endswith("/in.refused/probe")]) == len(refusal_cases.NAMES)
    assert all(c.entry != "probe" for c in all_cases if c not in st)


def test_the_per_format_lists_of_the_gpu_test_are_the_whole_list():
    ids = [c.id for n in refusal_cases.NAMES + ("unknown",) for c in refusal_cases.cases(n)]
    assert ids == [c.id for c in refusal_cases.cases()] and len(set(ids)) == len(ids)


def test_every_case_has_a_recorded_answer():
    golden = refusal_cases.load_golden(GOLDEN)
    assert sorted(golden) == sorted(c.id for c in refusal_cases.cases())


def test_rules_answer_every_stateless_case_as_recorded():
    golden = refusal_cases.load_golden(GOLDEN)
    todo = [c for c in refusal_cases.cases() if not refusal_cases.stateful(c)]
    out = pixfmt_check.run("cases", "".join(refusal_cases.line(c) + "\n" for c in todo))
    answers = [ln.split("\t") for ln in out.split("\n") if ln]
    assert len(answers) == len(todo)
    wrong = []
    for c, (cid, rc, text) in zip(todo, answers):
        assert cid == c.id
        if (int(rc), text) != golden[c.id]:
            wrong.append((c.id, (int(rc), text), golden[c.id]))
    assert not wrong, "%d of %d differ, e.g. %r" % (len(wrong), len(todo), wrong[:5])
