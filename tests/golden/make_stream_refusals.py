"""Generates stream_refusals.json: what the stream entry points of the library answer - the code and the text - to every case of
tests/refusal_cases.py, asked through the C ABI on a GPU.  The file is the specification the rules of video-stab_amd/csrc/pixfmt.h
are held to: it is recorded from the commit BEFORE a change to those rules, never from the code under test (README.md).

    python tests/golden/make_stream_refusals.py [out.json]

Every distinct (code, text) is stored once ("answers"); "cases" maps a case id to its index."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "video-stab_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsamd import capi          # noqa: E402
import refusal_cases            # noqa: E402


def main():
    vs = capi.load()
    assert vs.lib.vs_device_count() > 0, "needs a GPU: the stream cannot be created without one"
    answers, index, cases = [], {}, {}
    for c in refusal_cases.cases():
        a = refusal_cases.drive(vs, c)
        assert c.id not in cases, c.id
        if a not in index:
            index[a] = len(answers)
            answers.append(list(a))
        cases[c.id] = index[a]
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "stream_refusals.json")
    with open(out, "w") as f:
        json.dump({"answers": answers, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d distinct answers -> %s" % (len(cases), len(answers), out))


if __name__ == "__main__":
    main()
