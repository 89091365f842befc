"""Generates plane_job_refusals.json: what the four plane-job operators of the library answer - the code and the text of
vs_last_error - to every case of tests/plane_job_refusals.py, for sample sizes 1 and 2, asked through the C ABI on a machine WITHOUT
a device (every answer is decided on the host; an accepted call ends at VS_ERR_NO_DEVICE).  The file is the specification the
launchers of k_yuvpad.hip, k_cropzoom.hip and k_yuvfade.hip (and plane_jobs.h, which they share) are held to: it is recorded from the
commit BEFORE a change to them, never from the code under test.

    python tests/golden/make_plane_job_refusals.py [out.json]

Rows are [operator, case, rc, text]."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "video-stab_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsamd import capi          # noqa: E402
import plane_job_refusals       # noqa: E402


def main():
    rows = plane_job_refusals.recorded(capi.load().lib)
    assert len(set((op, case) for op, case, _, _ in rows)) == len(rows)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plane_job_refusals.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d answers -> %s" % (len(rows), out))


if __name__ == "__main__":
    main()
