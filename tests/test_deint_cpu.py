"""The deinterlacer and the weave without a device.

1. The ABI surface: the three entry points, the enum and the struct are exported, declared and bound; the version stays 2.
2. tests/deintref.py: the per-pixel loop and the vectorised form give the known answer of include/vs_stab.h and equal results on
   random planes; both count the same branches, and the random inputs of the CPU and GPU tests reach all nine.
3. Properties of the statement: kept rows are C's, every result lies between sp and d, w < 7 never searches, a missing P / N is C,
   weave(first field, second field) gives the frame back.
4. Every refusal of the three calls: status and the words of its text; valid arguments give VS_ERR_NO_DEVICE here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deintref as dr
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, 1, 2
BASE = 0x10000
NEW = ("vs_op_deint_jobs", "vs_op_deint_yuv", "vs_op_interlace_yuv")


def planes(rng, h, w, cn, bits, n=3):
    dt = np.uint8 if bits == 8 else np.uint16
    return [rng.integers(0, 1 << bits, (h, w * cn)).astype(dt) for _ in range(n)]


# ---- 1. the ABI surface --------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_exported_declared_and_bound():
    vs = capi.load()
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    binding = open(os.path.join(ROOT, "video-stab_amd", "vsamd", "capi.py")).read()
    for name in NEW:
        assert hasattr(vs.lib, name), name + " is not exported by libvideo-stab.so"
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/vs_stab.h"
        assert getattr(vs.lib, name).argtypes and re.search(r"L\.%s\.argtypes" % name, binding), name
    assert vs.lib.vs_abi_version() == 2 and re.search(r"^#define VS_STAB_ABI_VERSION 2$", header, re.M)
    assert re.search(r"enum vs_deint_mode \{ VS_DEINT_LINEAR = 0, VS_DEINT_YADIF = 1 \}", header)
    assert (capi.DEINT_LINEAR, capi.DEINT_YADIF) == (dr.LINEAR, dr.YADIF) == (0, 1)
    m = re.search(r"typedef struct vs_deint_job \{(.*?)\} vs_deint_job;", header, re.S)
    assert m, "struct vs_deint_job is not declared"
    declared = re.findall(r"(\w+)\s*[;,]", m.group(1))
    assert declared == [f[0] for f in capi.VsDeintJob._fields_], declared
    assert C.sizeof(capi.VsDeintJob) == 4 * 16 + 6 * 4
    for method in ("deint_jobs", "deint_yuv", "interlace_yuv"):
        assert callable(getattr(vs, method)), method


# ---- 2. the two statements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [dr.deint_loop, dr.deint], ids=["loop", "numpy"])
def test_the_known_answer(f):
    for (keep, second, mode), rows in (((0, 0, dr.YADIF), dr.KA_YADIF_K0_S0), ((1, 1, dr.YADIF), dr.KA_YADIF_K1_S1), ((0, 0, dr.LINEAR), dr.KA_LINEAR_K0),
                                       ((0, 1, dr.LINEAR), dr.KA_LINEAR_K0)):
        o = f(dr.KA_P, dr.KA_C, dr.KA_N, 1, keep, second, mode)
        assert o.dtype == np.uint8 and o.shape == (5, 9)
        for y in range(5):
            assert o[y].tolist() == (rows[y] if y in rows else dr.KA_C[y].tolist()), (keep, second, mode, y)
    assert dr.KA_YADIF_K1_S1[0] == dr.KA_C[1].tolist()


def test_the_known_answer_reaches_every_branch():
    for f in (dr.deint_loop, dr.deint):
        counts = {}
        f(dr.KA_P, dr.KA_C, dr.KA_N, 1, 0, 0, dr.YADIF, counts)
        f(dr.KA_P, dr.KA_C, dr.KA_N, 1, 1, 1, dr.YADIF, counts)
        assert set(counts) == set(dr.BRANCHES) and all(counts[k] > 0 for k in dr.BRANCHES), counts


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_loop_and_numpy_agree_on_random_planes(bits):
    rng = np.random.default_rng(bits)
    total = {}
    for cn in (1, 2, 3, 4):
        for h in range(2, 8):
            for w in range(1, 21):
                P, Cc, N = planes(rng, h, w, cn, bits)
                for keep in (0, 1):
                    for second in (0, 1):
                        a, b = {}, {}
                        assert np.array_equal(dr.deint_loop(P, Cc, N, cn, keep, second, dr.YADIF, a), dr.deint(P, Cc, N, cn, keep, second, dr.YADIF, b)), (cn, h, w, keep, second)
                        assert a == b, (cn, h, w, keep, second, a, b)
                        for k, v in a.items():
                            total[k] = total.get(k, 0) + v
                        assert np.array_equal(dr.deint_loop(P, Cc, N, cn, keep, second, dr.LINEAR), dr.deint(P, Cc, N, cn, keep, second, dr.LINEAR))
    assert all(total[k] > 0 for k in dr.BRANCHES), total


def test_random_planes_reach_every_branch():
    """Branch coverage is a condition of the inputs: random samples of every depth at 5 x 9 and larger reach the five search picks,
    the three clamp outcomes and the widened diff (planes with w < 7 or h < 3 cannot).  The GPU tests draw their planes the same way
    - uniform bytes - and assert the same through the numpy form's counters."""
    for bits in (8, 10, 16):
        for (h, w, cn) in ((5, 9, 1), (5, 9, 3), (6, 40, 2), (33, 20, 1)):
            rng = np.random.default_rng(1000 * bits + 10 * w + cn)
            counts = {}
            for _ in range(40):
                P, Cc, N = planes(rng, h, w, cn, bits)
                for keep in (0, 1):
                    dr.deint_loop(P, Cc, N, cn, keep, keep, dr.YADIF, counts)
            assert all(counts[k] > 0 for k in dr.BRANCHES), (bits, h, w, cn, counts)
    # what cannot reach all nine
    rng = np.random.default_rng(5)
    narrow, flat = {}, {}
    for _ in range(20):
        P, Cc, N = planes(rng, 7, 6, 1, 8)
        dr.deint_loop(P, Cc, N, 1, 0, 0, dr.YADIF, narrow)
        P, Cc, N = planes(rng, 2, 20, 1, 8)
        dr.deint_loop(P, Cc, N, 1, 0, 0, dr.YADIF, flat)
        dr.deint_loop(P, Cc, N, 1, 1, 1, dr.YADIF, flat)
    assert narrow["pick_0"] > 0 and not any(narrow[k] for k in ("pick_m1", "pick_m2", "pick_p1", "pick_p2"))
    assert flat["diff_widened"] == 0


# ---- 3. properties -------------------------------------------------------------------------------------------------------------
CASES = [(8, 1, 9, 12), (8, 3, 7, 11), (16, 2, 6, 9), (10, 1, 5, 30), (8, 4, 2, 8), (16, 1, 3, 7)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "u%d-cn%d-%dx%d" % (c[0], c[1], c[3], c[2]))
def test_properties_of_the_statement(case):
    bits, cn, h, w = case
    rng = np.random.default_rng(sum(case))
    P, Cc, N = planes(rng, h, w, cn, bits)
    for mode in (dr.LINEAR, dr.YADIF):
        fields = {}
        for keep in (0, 1):
            for second in (0, 1):
                o = dr.deint(P, Cc, N, cn, keep, second, mode)
                fields[(keep, second)] = o
                assert o.dtype == Cc.dtype and np.array_equal(o[keep::2], Cc[keep::2])                    # kept rows are C's
                if mode == dr.YADIF:
                    trace = []
                    dr.deint_loop(P, Cc, N, cn, keep, second, mode, None, trace)
                    assert len(trace) == len(range(1 - keep, h, 2)) * w * cn
                    for (y, i, sp, d, out) in trace:
                        assert min(sp, d) <= out <= max(sp, d) and 0 <= out < (1 << bits), (y, i, sp, d, out)
                    # a missing P / N is C
                    assert np.array_equal(dr.deint(None, Cc, N, cn, keep, second, mode), dr.deint(Cc, Cc, N, cn, keep, second, mode))
                    assert np.array_equal(dr.deint(P, Cc, None, cn, keep, second, mode), dr.deint(P, Cc, Cc, cn, keep, second, mode))
                    assert np.array_equal(dr.deint_loop(None, Cc, None, cn, keep, second, mode), dr.deint(Cc, Cc, Cc, cn, keep, second, mode))
                else:
                    assert np.array_equal(o, dr.deint(None, Cc, None, cn, keep, 1 - second, mode))         # C only, `second` ignored
        # weave(first field, second field) of one frame gives C back
        for tff in (0, 1):
            k = 0 if tff else 1
            assert np.array_equal(dr.weave(fields[(k, 0)], fields[(1 - k, 1)], tff), Cc), (mode, tff)
    F, S = planes(rng, h, w, cn, bits, 2)
    for tff in (0, 1):
        o = dr.weave(F, S, tff)
        k = 0 if tff else 1
        assert np.array_equal(o[k::2], F[k::2]) and np.array_equal(o[1 - k::2], S[1 - k::2])


def test_a_plane_narrower_than_7_never_searches():
    rng = np.random.default_rng(6)
    for w in range(1, 7):
        for cn in (1, 2, 3):
            P, Cc, N = planes(rng, 6, w, cn, 8)
            counts, trace = {}, []
            dr.deint_loop(P, Cc, N, cn, 0, 0, dr.YADIF, counts, trace)
            assert counts["pick_0"] == 3 * w * cn and not any(counts[k] for k in ("pick_m1", "pick_m2", "pick_p1", "pick_p2"))
            for (y, i, sp, d, out) in trace:
                assert sp == (int(Cc[y - 1, i]) + int(Cc[y + 1 if y + 1 < 6 else y - 1, i])) >> 1


# ---- 4. refusals, no device ----------------------------------------------------------------------------------------------------
GOOD = dict(prev=BASE, prev_stride=400, cur=BASE + (1 << 20), cur_stride=400, next=BASE + (2 << 20), next_stride=400, dst=BASE + (3 << 20), dst_stride=400,
            w=130, h=96, cn=1, keep=0, second=0, reserved=0)


def _err(L):
    return (L.vs_last_error() or b"").decode()


def _jobs(L, jobs, n=None, sb=1, mode=1, null=False):
    arr = (capi.VsDeintJob * len(jobs))(*[capi.VsDeintJob(**j) for j in jobs])
    rc = L.vs_op_deint_jobs(None if null else arr, len(jobs) if n is None else n, sb, mode, None)
    return rc, _err(L)


def _distinct(jobs):
    """The jobs with their destinations apart (GOOD repeated would overlap itself)."""
    return [dict(j, dst=j["dst"] + (i << 16)) if j["dst"] else j for i, j in enumerate(jobs)]


def test_job_refusals_and_no_device():
    L = capi.load().lib
    name = "vs_op_deint_jobs"
    for call, word in [(dict(n=0), name), (dict(n=97), name), (dict(sb=4), name), (dict(sb=0), name), (dict(null=True), name), (dict(mode=2), "mode"),
                       (dict(mode=-1), "mode")]:
        rc, msg = _jobs(L, _distinct([GOOD] * max(1, call.get("n", 1))), **call)
        assert rc == INVALID and name in msg and word in msg, (call, rc, msg)
    far = BASE + (8 << 20)
    jobs = [(dict(cur=None), "null"), (dict(dst=None), "null"), (dict(w=0), "sizes"), (dict(h=32768), "sizes"), (dict(w=-1), "sizes"), (dict(h=1), "at least 2"),
            (dict(cn=0), "cn"), (dict(cn=5), "cn"), (dict(reserved=1), "reserved"), (dict(keep=2), "keep"), (dict(keep=-1), "keep"), (dict(second=2), "second"),
            (dict(cur_stride=129), "stride"), (dict(dst_stride=96), "stride"), (dict(prev_stride=100), "stride"), (dict(next_stride=0), "stride"),
            (dict(dst=GOOD["cur"] + 400 * 95 + 129), "overlaps cur"), (dict(dst=GOOD["prev"]), "overlaps prev"), (dict(dst=GOOD["next"] - 400 * 95), "overlaps next"),
            (dict(dst=far, prev=None, cur=far + 50), "overlaps cur")]
    for change, word in jobs:
        for lead in (0, 2):
            leads = [dict(GOOD, dst=GOOD["dst"] + ((i + 1) << 16)) for i in range(lead)]
            rc, msg = _jobs(L, leads + [dict(GOOD, **change), dict(GOOD, dst=BASE + (5 << 20))])
            assert rc == INVALID and "%s: job %d" % (name, lead) in msg and word in msg, (change, lead, rc, msg)
    # a destination against another job's source, and against another destination
    other = dict(GOOD, prev=None, next=None, cur=far, dst=far + (1 << 20))
    rc, msg = _jobs(L, [GOOD, dict(other, cur=GOOD["dst"] + 200)])
    assert rc == INVALID and name + ": job 0" in msg and "overlaps cur of job 1" in msg, (rc, msg)
    rc, msg = _jobs(L, [GOOD, dict(other, next=GOOD["dst"])])
    assert rc == INVALID and "overlaps next of job 1" in msg, (rc, msg)
    rc, msg = _jobs(L, [GOOD, dict(other, dst=GOOD["dst"] + 400 * 95)])
    assert rc == INVALID and name + ": job 1" in msg and "overlaps the destination of job 0" in msg, (rc, msg)
    for change, word in [(dict(cn=3), "cn"), (dict(cur_stride=401), "even"), (dict(cur=GOOD["cur"] + 1), "even"), (dict(dst_stride=399), "even"), (dict(prev=BASE + 1), "even"),
                         (dict(next_stride=403), "even")]:
        rc, msg = _jobs(L, [dict(GOOD, **change)], sb=2)
        assert rc == INVALID and name + ": job 0" in msg and word in msg, (change, rc, msg)
    if L.vs_device_count() <= 0:
        same = dict(GOOD, prev=GOOD["cur"], next=GOOD["cur"])                       # sources may alias each other freely
        for j, kw in [(GOOD, {}), (GOOD, dict(mode=0)), (dict(GOOD, cn=3, w=133), {}), (dict(GOOD, cn=4, w=100), {}), (dict(GOOD, cn=2, w=100), dict(sb=2)),
                      (dict(GOOD, prev=None, prev_stride=0), {}), (dict(GOOD, next=None, next_stride=1), {}), (same, {}), (dict(GOOD, h=2), {}),
                      (dict(GOOD, keep=1, second=1), {}), (dict(GOOD, w=1), {})]:
            rc, msg = _jobs(L, [j], **kw)
            assert rc == NO_DEVICE, (j, kw, rc, msg)
        assert _jobs(L, _distinct([GOOD] * 96))[0] == NO_DEVICE


def _ptrs(v, n):
    return None if v is None else (C.c_void_p * max(n, 1))(*v)


def _deint_yuv(L, fmt, n=1, w=130, h=96, in_lay=None, out_lay=None, prev=(), cur=None, nxt=(), first=None, second=(), tff=1, mode=1):
    sb = capi.PIXFMT[fmt].sample_bytes if fmt in capi.PIXFMT else 1
    lin, lout = capi.I420LayoutC(*(in_lay or (w * sb, 0, 0, 0))), capi.I420LayoutC(*(out_lay or (w * sb, 0, 0, 0)))
    m = max(n, 1)
    cur = cur or [BASE + (i << 22) for i in range(m)]
    prev = [None] + cur[:-1] if prev == () else prev
    nxt = cur[1:] + [None] if nxt == () else nxt
    first = first or [BASE + (1 << 30) + (i << 22) for i in range(m)]
    second = [BASE + (2 << 30) + (i << 22) for i in range(m)] if second == () else second
    rc = L.vs_op_deint_yuv(fmt, _ptrs(prev, n), _ptrs(cur, n), _ptrs(nxt, n), C.byref(lin), w, h, _ptrs(first, n), _ptrs(second, n), C.byref(lout), tff, mode, n, None)
    return rc, _err(L)


def _interlace_yuv(L, fmt, n=1, w=130, h=96, in_lay=None, out_lay=None, first=None, second=None, dst=None, tff=1):
    sb = capi.PIXFMT[fmt].sample_bytes if fmt in capi.PIXFMT else 1
    lin, lout = capi.I420LayoutC(*(in_lay or (w * sb, 0, 0, 0))), capi.I420LayoutC(*(out_lay or (w * sb, 0, 0, 0)))
    m = max(n, 1)
    first = first or [BASE + (i << 22) for i in range(m)]
    second = second or [BASE + (1 << 30) + (i << 22) for i in range(m)]
    dst = dst or [BASE + (2 << 30) + (i << 22) for i in range(m)]
    rc = L.vs_op_interlace_yuv(fmt, _ptrs(first, n), _ptrs(second, n), C.byref(lin), w, h, _ptrs(dst, n), C.byref(lout), tff, n, None)
    return rc, _err(L)


ALL_YUV = ("NV12", "P010", "I420", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412")


def test_surface_refusals_and_no_device():
    L = capi.load().lib
    F = capi.PIXFMT_BY_NAME
    nv12, i420, i444, p010, i010, i422 = (F[k].fmt for k in ("NV12", "I420", "I444", "P010", "I010", "I422"))
    common = [(dict(fmt=capi.FMT_BGR8), ("BGR8", "not a YUV surface format")), (dict(fmt=99), ("format 99",)), (dict(fmt=nv12, n=0), ("NV12", "n must be")),
              (dict(fmt=nv12, tff=2), ("NV12", "tff")), (dict(fmt=nv12, tff=-1), ("NV12", "tff")), (dict(fmt=nv12, w=129), ("source", "NV12", "even")),
              (dict(fmt=i420, h=95), ("I420", "even")), (dict(fmt=i422, w=97), ("I422", "even")), (dict(fmt=i444, w=0), ("I444", "size")),
              (dict(fmt=i444, w=32768, in_lay=(32768, 0, 0, 0)), ("I444", "32767")), (dict(fmt=i444, h=1), ("I444", "at least 2 rows")),
              (dict(fmt=i420, h=2), ("I420", "at least 2 rows")), (dict(fmt=nv12, h=2), ("NV12", "at least 2 rows")),
              (dict(fmt=p010, in_lay=(258, 0, 0, 0)), ("source", "P010", "pitch")), (dict(fmt=p010, out_lay=(261, 0, 0, 0)), ("destination", "P010", "even")),
              (dict(fmt=i010, in_lay=(262, 0, 0, 0)), ("source", "I010", "chroma pitch")), (dict(fmt=nv12, in_lay=(130, 0, 0, 64)), ("source", "NV12", "v_off")),
              (dict(fmt=i420, out_lay=(130, 0, 130 * 96, 130 * 96 + 8)), ("destination", "I420", "overlap"))]
    for call, f in (("vs_op_deint_yuv", _deint_yuv), ("vs_op_interlace_yuv", _interlace_yuv)):
        for kw, words in common:
            rc, msg = f(L, **kw)
            assert rc == INVALID and call in msg and all(w in msg for w in words), (call, kw, rc, msg)
    call = "vs_op_deint_yuv"
    c2 = [BASE, BASE + (1 << 22)]
    for kw, words in [(dict(fmt=nv12, n=17), ("NV12", "n must be")), (dict(fmt=nv12, mode=2), ("NV12", "mode")), (dict(fmt=nv12, mode=-1), ("NV12", "mode")),
                      (dict(fmt=nv12, first=[None]), ("destination (first)", "NV12", "null")), (dict(fmt=nv12, second=[None]), ("destination (second)", "NV12", "null")),
                      (dict(fmt=nv12, n=2, cur=c2, first=[BASE + (1 << 30), BASE + 4096]), ("NV12", "job", "overlaps")),
                      (dict(fmt=nv12, n=2, cur=c2, second=[BASE + (1 << 30), BASE + (1 << 30) + 100]), ("NV12", "job", "overlaps the destination")),
                      (dict(fmt=nv12, n=1, prev=[BASE + (1 << 30) + 64]), ("NV12", "job", "overlaps prev")),
                      (dict(fmt=p010, cur=[BASE + 1]), ("P010", "even"))]:
        rc, msg = _deint_yuv(L, **kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    call = "vs_op_interlace_yuv"
    for kw, words in [(dict(fmt=nv12, n=33), ("NV12", "n must be")), (dict(fmt=nv12, second=[None]), ("source (second)", "NV12", "null")),
                      (dict(fmt=nv12, dst=[BASE + 64]), ("NV12", "job 0", "overlaps cur")), (dict(fmt=nv12, dst=[BASE + (1 << 30)]), ("NV12", "job 0", "overlaps next")),
                      (dict(fmt=i420, n=2, dst=[BASE + (2 << 30), BASE + (2 << 30) + 130]), ("I420", "overlaps the destination"))]:
        rc, msg = _interlace_yuv(L, **kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    if L.vs_device_count() <= 0:
        for name in ALL_YUV:
            fmt = F[name].fmt
            assert _deint_yuv(L, fmt, n=16)[0] == NO_DEVICE, name
            assert _deint_yuv(L, fmt, n=3, prev=None, nxt=None, second=None, tff=0, mode=0)[0] == NO_DEVICE, name
            assert _deint_yuv(L, fmt, n=1, h=4)[0] == NO_DEVICE, name
            assert _interlace_yuv(L, fmt, n=32)[0] == NO_DEVICE, name
            assert _interlace_yuv(L, fmt, n=1, tff=0)[0] == NO_DEVICE, name
        one = [BASE]
        assert _deint_yuv(L, nv12, n=1, prev=one, cur=one, nxt=one)[0] == NO_DEVICE               # sources may alias each other
