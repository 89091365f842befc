"""What the four plane-job operators - vs_op_pad_jobs, vs_op_resize_jobs, vs_op_fade_blend_jobs, vs_op_fade_update_jobs - refuse
about a launch and about a job, and, next to that, the calls of the same shape that they accept: one table per operator for the
operators' GPU tests (test_operator_refusals of test_gpu_yuv_border_pad / _cropzoom / _fade), their CPU tests (test_yuv_*_cpu.py),
tests/golden/make_plane_job_refusals.py (which records codes and texts) and tests/test_plane_job_refusals_cpu.py (which holds the
library to the record).

Every refusal is decided on the host before any device call, so the addresses of a refused call are never read: a CPU test passes
FAKE_BASE, a GPU test the address of a zeroed buffer of REGION bytes (an accepted call launches).  A case changes fields of the
operator's good job (`job`) or arguments of the call (`call`: n, sb, alpha, beta, null = no job array); `word` must appear in the text."""
import collections
import ctypes as C

from vsamd import capi

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
FAKE_BASE = 0x10000
REGION = 1 << 16

Case = collections.namedtuple("Case", "name job call rc word")
# accepted: calls that pass the checks; launch: refusals that name no job; jobs: refusals of one job ("ENTRY: job i: why")
Op = collections.namedtuple("Op", "entry struct limit weights good accepted launch jobs")


def _c(name, rc=INVALID, word="", call=None, **job):
    return Case(name, job, call or {}, rc, word)


def _launch(entry, limit, *more):
    return [_c("n-0", word=entry, call=dict(n=0)), _c("n-over", word=entry, call=dict(n=limit + 1)), _c("sb-4", word=entry, call=dict(sb=4)),
            _c("jobs-null", word=entry, call=dict(null=True))] + list(more)


def pad(base):
    S, D = base, base + 32768
    good = dict(src=S, src_stride=64, sw=20, sh=4, dst=D, dst_stride=128, bx=6, by=8, cn=1, border=0, fill=(16, 0))
    return Op("vs_op_pad_jobs", capi.VsPadJob, 96, False, good,
              [_c("good", OK), _c("copy", OK, bx=0, by=0), _c("odd-bytes", OK, src_stride=65, dst_stride=129, src=S + 1),
               _c("good-16", OK, call=dict(sb=2)), _c("fill-16", OK, call=dict(sb=2), fill=(4095, 65535))],
              _launch("vs_op_pad_jobs", 96),
              [_c("src-null", word="null", src=None), _c("dst-null", word="null", dst=None), _c("sw-0", word="sizes", sw=0), _c("bx-neg", word="sizes", bx=-1),
               _c("wide", word="32767", sw=32760, src_stride=32760, dst_stride=32800), _c("tall", word="32767", by=16382, sh=4), _c("cn-3", word="cn", cn=3),
               _c("reserved", word="reserved", reserved=1), _c("border-5", word="border", border=5), _c("border-neg", word="border", border=-1),
               _c("fill-256", word="255", fill=(256, 0)), _c("src-stride", word="stride", src_stride=19), _c("dst-stride", word="stride", dst_stride=31),
               _c("overlap-head", word="overlap", dst=S + 32), _c("overlap-tail", word="overlap", dst=S + 64 * 3 + 10),
               _c("odd-pitch-16", word="even", call=dict(sb=2), src_stride=65), _c("odd-src-16", word="even", call=dict(sb=2), src=S + 1)])


def resize(base):
    S, D = base, base + 32768
    good = dict(src=S, src_stride=64, sw=20, sh=4, dst=D, dst_stride=128, dw=64, dh=48, cn=1)
    return Op("vs_op_resize_jobs", capi.VsScaleJob, 96, False, good,
              [_c("good", OK), _c("odd-bytes", OK, src_stride=65, dst_stride=129), _c("good-16", OK, call=dict(sb=2))],
              _launch("vs_op_resize_jobs", 96),
              [_c("dw-below-sw", UNSUPPORTED, "not a general resize", dw=19), _c("dh-below-sh", UNSUPPORTED, "not a general resize", dh=3),
               _c("odd-pitch-16", word="even", call=dict(sb=2), src_stride=65), _c("src-null", word="null", src=None), _c("dst-null", word="null", dst=None),
               _c("cn-3", word="cn", cn=3), _c("reserved", word="reserved", reserved=1), _c("sw-0", word="sizes", sw=0), _c("dh-over", word="sizes", dh=32768),
               _c("src-stride", word="stride", src_stride=19), _c("dst-stride", word="stride", dst_stride=63)])


def fade_blend(base):
    S, H, D = base, base + 16384, base + 32768
    entry = "vs_op_fade_blend_jobs"
    good = dict(src=S, src_stride=64, sw=20, sh=4, hist=H, hist_stride=128, dst=D, dst_stride=128, bx=6, by=8, cn=1)
    return Op(entry, capi.VsFadeJob, 32, True, good,
              [_c("good", OK), _c("copy", OK, bx=0, by=0), _c("n-limit", OK, call=dict(n=32)), _c("odd-bytes", OK, src_stride=65, hist_stride=129, hist=H + 1),
               _c("fill-16", OK, call=dict(sb=2), fill=(4095, 65535)), _c("good-16", OK, call=dict(sb=2, alpha=0.0, beta=1.0))],
              _launch(entry, 32, _c("alpha-over", word="weights", call=dict(alpha=1.5)), _c("beta-neg", word="weights", call=dict(beta=-0.25)),
                      _c("alpha-nan", word="weights", call=dict(alpha=float("nan"))), _c("alpha-neg", word="weights", call=dict(alpha=-0.1)),
                      _c("beta-over", word="weights", call=dict(beta=1.5))),
              [_c("src-null", word="null", src=None), _c("hist-null", word="null", hist=None), _c("dst-null", word="null", dst=None), _c("sw-0", word="sizes", sw=0),
               _c("bx-neg", word="sizes", bx=-1), _c("wide", word="32767", sw=32760, src_stride=32760, hist_stride=32800, dst_stride=32800),
               _c("tall", word="32767", by=16382), _c("cn-3", word="cn", cn=3), _c("reserved", word="reserved", reserved=1),
               _c("fill1-256", word="255", fill=(0, 256)), _c("fill0-256", word="255", fill=(256, 0)), _c("src-stride", word="stride", src_stride=19),
               _c("hist-stride", word="stride", hist_stride=31), _c("dst-stride", word="stride", dst_stride=31), _c("overlap-src", word="overlap", dst=S + 32),
               _c("overlap-hist", word="overlap", dst=H + 128 * 19 + 31), _c("odd-pitch-16", word="even", call=dict(sb=2), src_stride=65),
               _c("odd-hist-16", word="even", call=dict(sb=2), hist=H + 1), _c("odd-src-16", word="even", call=dict(sb=2), src=S + 1),
               _c("odd-hist-pitch-16", word="even", call=dict(sb=2), hist_stride=129)])


def fade_update(base):
    H, D = base + 16384, base + 32768
    entry = "vs_op_fade_update_jobs"
    good = dict(hist=H, hist_stride=128, res=D, res_stride=128, w=32, h=20, cn=1)
    return Op(entry, capi.VsFadeUpdateJob, 32, False, good,
              [_c("good", OK), _c("odd-bytes", OK, res=D + 1, res_stride=129), _c("good-16", OK, call=dict(sb=2))],
              _launch(entry, 32, _c("sb-0", word=entry, call=dict(sb=0)), _c("sb-3", word=entry, call=dict(sb=3))),
              [_c("hist-null", word="null", hist=None), _c("res-null", word="null", res=None), _c("w-0", word="sizes", w=0), _c("h-over", word="sizes", h=32768),
               _c("cn-3", word="cn", cn=3), _c("cn-0", word="cn", cn=0), _c("reserved", word="reserved", reserved=1), _c("reserved-2", word="reserved", reserved=2),
               _c("hist-stride", word="stride", hist_stride=31), _c("res-stride", word="stride", res_stride=31), _c("overlap", word="overlap", res=H + 64),
               _c("odd-res-16", word="even", call=dict(sb=2), res=D + 1), _c("odd-hist-pitch-16", word="even", call=dict(sb=2), hist_stride=129)])


OPS = dict(pad=pad, resize=resize, fade_blend=fade_blend, fade_update=fade_update)


def _struct(op, fields):
    f = dict(fields)
    if "fill" in f:
        f["fill"] = (C.c_uint16 * 2)(*f["fill"])
    return op.struct(**f)


def ask(lib, op, case, lead=0, sb=None):
    """(rc, text) of the case's call, its job behind `lead` good ones; sb overrides the case's sample size."""
    call = dict(case.call)
    n = call.get("n", lead + 1)
    jobs = [op.good] * lead + [dict(op.good, **case.job)] + [op.good] * (n - lead - 1)
    arr = (op.struct * len(jobs))(*[_struct(op, j) for j in jobs])
    args = [None if call.get("null") else arr, n, sb or call.get("sb", 1)]
    if op.weights:
        args += [call.get("alpha", 0.5), call.get("beta", 0.5)]
    rc = getattr(lib, op.entry)(*args, None)
    return rc, (lib.vs_last_error() or b"").decode()


def check_refusals(lib, op):
    """Every launch case is refused with its code and names the entry point; every job case, as job 0, 1 and 2 of a launch, with its
    code, "ENTRY: job i" and its word."""
    for c in op.launch:
        rc, msg = ask(lib, op, c)
        assert rc == c.rc and op.entry in msg and c.word in msg, (c.name, rc, msg)
    for c in op.jobs:
        for lead in (0, 1, 2):
            rc, msg = ask(lib, op, c, lead)
            assert rc == c.rc and "%s: job %d" % (op.entry, lead) in msg and c.word in msg, (c.name, lead, rc, msg)


def check_accepted(lib, op, want):
    """want: OK on a device (the call launches on op's addresses), NO_DEVICE without one."""
    for c in op.accepted:
        rc, msg = ask(lib, op, c)
        assert rc == want, (c.name, rc, msg)


def every_case():
    """(operator, case id, op, case, sb) of every case at FAKE_BASE, for sample sizes 1 and 2 (a case with a sample size that is
    neither: its own, once)."""
    for name, make in OPS.items():
        op = make(FAKE_BASE)
        for c in op.accepted + op.launch + op.jobs:
            own = c.call.get("sb", 1)
            for sb in ((1, 2) if own in (1, 2) else (own,)):
                yield name, "%s/sb%d" % (c.name, sb), op, c, sb


def recorded(lib):
    """[operator, case id, rc, text] of every case, as job 0.  For a machine without a device: the accepted calls would launch on
    the fake addresses."""
    assert lib.vs_device_count() <= 0, "run this without a device"
    return [[name, cid] + list(ask(lib, op, c, sb=sb)) for name, cid, op, c, sb in every_case()]
