"""Generates stage_refusals.json: what the sixteen asynchronous entry points of the roll and the zoom/crop stage answer - the code and
the text of the object's last error - to every case of tests/stage_refusals.py, asked through the C ABI.  Creating the objects needs
a device, so this runs on a machine WITH one.  The file is the specification the host code of k_roll.hip and k_azc.hip is held to:
it is recorded from the commit BEFORE a change to them, never from the code under test.

    python tests/golden/make_stage_refusals.py [out.json]

Rows are [entry, case, rc, text]."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "video-stab_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsamd import capi          # noqa: E402
import stage_refusals           # noqa: E402


def main():
    rows = stage_refusals.recorded(capi.load())
    assert len(set((entry, case) for entry, case, _, _ in rows)) == len(rows)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "stage_refusals.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d answers -> %s" % (len(rows), out))


if __name__ == "__main__":
    main()
