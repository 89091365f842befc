"""The refusals of the four plane-job operators, code and text, are the recorded ones (tests/golden/plane_job_refusals.json, written
by tests/golden/make_plane_job_refusals.py from the commit before the launchers were brought to one skeleton in plane_jobs.h).  Needs
no GPU: every refusal is decided before a device call, on addresses that are never read."""
import json
import os

import plane_job_refusals as pj
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_answer_is_the_recorded_one():
    lib = capi.load().lib
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "plane_job_refusals.json")))
    want = {(op, cid): (rc, text) for op, cid, rc, text in golden}
    assert len(want) == len(golden)
    device = lib.vs_device_count() > 0
    asked = set()
    for name, cid, op, c, sb in pj.every_case():
        asked.add((name, cid))
        rc, text = want[(name, cid)]
        if rc != pj.NO_DEVICE:
            assert pj.ask(lib, op, c, sb=sb) == (rc, text), (name, cid)
        elif not device:
            # accepted: with a device the call would launch on the fake addresses; without one the text is the runtime's
            got = pj.ask(lib, op, c, sb=sb)
            assert got[0] == rc and got[1].startswith("no HIP device"), (name, cid, got)
        if sb == c.call.get("sb", 1):             # the record holds what the tables state
            assert rc == (pj.NO_DEVICE if c in op.accepted else c.rc) and c.word in text, (name, cid)
    assert asked == set(want)
