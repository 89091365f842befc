"""Area-averaging downscale, the parts that need no GPU.

1. The axis tables: tests/arearef.py's taps are contiguous, at least one, inside the source; vs_area_axis_table equals them bit for
   bit; so does tests/cpp/area_tables_check.cpp, which compiles csrc/resize_tables.h alone.
2. The float64 anchor of the float32 statement: |out - f64| <= 0.5 + (nx + ny + 4) * 2^-24 * max_sample, no exclusions.
3. Classes: what vs_op_area_jobs_plan reports, every k d -> d integer, class 2 = resizeref's LINEAR mean, class 1 known answers with
   a tie, the identity.
4. The ABI surface, the refusals (the sibling's lists through the new names, and the upscale), VS_ERR_NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import arearef as ar
import resizeref as rr
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 4
PAIRS = [(1, 1), (5, 3), (7, 1), (64, 3), (131, 130), (300, 300), (650, 271), (1080, 720), (2160, 720), (3840, 1280), (2048, 37), (32767, 2), (32767, 32766)]


def random_pairs():
    rng = np.random.default_rng(20261021)
    out = []
    for _ in range(300):
        src = int(rng.integers(1, 4001))
        out.append((src, int(rng.integers(1, src + 1))))
    return out


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. the tables -----------------------------------------------------------------------------------------------------------
def check_table(vs, src, dst):
    first, count, wf, wm, wl = ar.axis_table(src, dst)                 # (asserts contiguity, count >= 1, the range, equal middles)
    assert count.min() >= 1 and first.min() >= 0 and (first + count - 1).max() <= src - 1
    g = vs.area_axis_table(src, dst)
    assert np.array_equal(g[0], first) and np.array_equal(g[1], count), (src, dst)
    for name, a, b in zip(("w_first", "w_mid", "w_last"), g[2:], (wf, wm, wl)):
        assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b)), (src, dst, name)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_vs_area_axis_table_equals_the_reference(pair):
    check_table(capi.load(), *pair)


def test_vs_area_axis_table_on_random_pairs():
    vs = capi.load()
    for src, dst in random_pairs():
        check_table(vs, src, dst)


def test_the_header_alone_gives_the_reference_tables():
    """tests/cpp/area_tables_check.cpp includes only csrc/resize_tables.h and is built with g++, as `make asan` builds it."""
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(ROOT, "tests", "cpp", "area_tables_check.cpp"), os.path.join(build, "area_tables_check")
    deps = [src, os.path.join(ROOT, "video-stab_amd", "csrc", "resize_tables.h")]
    assert re.findall(r'#include "([^"]+)"', open(src).read()) == ["../../video-stab_amd/csrc/resize_tables.h"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, src])
    cases = PAIRS + random_pairs()[:60]
    r = subprocess.run([exe], input="".join("%d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    for s, d in cases:
        integer, i = ar.axis_integer(s, d)
        assert next(lines).split() == [str(v) for v in (s, d, int(integer), i)]
        rows = [next(lines).split() for _ in range(d)]
        first, count, wf, wm, wl = ar.axis_table(s, d)
        assert np.array_equal(np.array([[int(r[0]), int(r[1])] for r in rows]), np.stack([first, count], 1)), (s, d)
        got = np.array([[int(x, 16) for x in r[2:]] for r in rows], np.uint32)
        assert np.array_equal(got, np.stack([bits(wf), bits(wm), bits(wl)], 1)), (s, d)
    assert next(lines, None) is None
    assert subprocess.run([exe], input="3 5\n", capture_output=True, text=True).returncode == 2          # an upscale is no table


def test_the_weights_of_an_index_may_sum_below_one():
    """The 1e-3 thresholds are OpenCV's: they drop slivers, and what is dropped is not given to the other taps.  Over the listed
    and the random pairs some index loses weight; a sliver is at most 1e-3 of a source sample and a cell at least one sample wide,
    so the float64 weights of a destination index sum to 1 - 2e-3 at the least, and never above 1 (+ rounding)."""
    lo, hi = 2.0, 0.0
    for src, dst in PAIRS[:-2] + random_pairs():
        for t in ar.axis_taps(src, dst):
            s = sum(w for _, w in t)
            lo, hi = min(lo, s), max(hi, s)
    print("weight sums: %.6f .. %.15f" % (lo, hi))
    assert 1 - 2e-3 <= lo < 1 - 1e-4 and hi <= 1.0 + 1e-12, (lo, hi)


# ---- 2. the float64 anchor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((131, 40), (130, 37), 1, 8), ((200, 64), (37, 3), 2, 8), ((97, 61), (33, 25), 1, 10), ((150, 90), (100, 37), 2, 16),
                                  ((300, 50), (300, 41), 3, 8), ((650, 100), (271, 37), 1, 12)], ids=lambda c: "%dx%d-%dx%d-cn%d-%dbit" % (c[0] + c[1] + c[2:]))
def test_the_float32_statement_against_float64(case):
    (sw, sh), (dw, dh), cn, depth = case
    top = (1 << depth) - 1
    plane = np.random.default_rng(sw + dh + depth).integers(0, top + 1, (sh, sw * cn), np.uint8 if depth == 8 else np.uint16)
    assert ar.job_class(sw, sh, dw, dh) == 0
    out = ar.resize(plane, cn, dw, dh).astype(np.float64)
    f64, nx, ny = ar.resize_f64(plane, cn, dw, dh)
    bound = 0.5 + (nx + ny + 4) * 2.0 ** -24 * top
    err = np.abs(out - f64).max()
    print("%dx%d -> %dx%d: nx %d ny %d, error %.6f of %.6f" % (sw, sh, dw, dh, nx, ny, err, bound))
    assert err <= bound


# ---- 3. classes ----------------------------------------------------------------------------------------------------------------
BASE = 0x10000


def _tuple(sw, sh, dw, dh, cn=1, sb=1):
    return (BASE, sw * cn * sb, sw, sh, BASE + (1 << 28), dw * cn * sb, dw, dh, cn)


def test_the_plan_reports_the_classes():
    vs = capi.load()
    shapes = [((66, 50), (33, 25), 2), ((99, 60), (33, 20), 1), ((96, 61), (24, 61), 1), ((7, 5), (7, 5), 1), ((1, 1), (1, 1), 1), ((600, 90), (200, 37), 0),
              ((66, 50), (33, 26), 0), ((131, 40), (130, 37), 0), ((3840, 2160), (1280, 720), 1), ((3840, 2160), (1920, 1080), 2), ((3840, 2160), (2560, 1440), 0)]
    for sb, cn in ((1, 1), (1, 3), (2, 2)):
        got = vs.area_jobs_plan([_tuple(*s, *d, cn, sb) for s, d, _ in shapes], sb)
        assert got.tolist() == [c for _, _, c in shapes], (sb, cn)
    for s, d, c in shapes:
        assert ar.job_class(*s, *d) == c


def test_every_integer_ratio_is_an_integer_axis():
    """k d -> d for k <= 16 and d < 2000: 1.0 / ((double)d / (k d)) lies within DBL_EPSILON of k, in the reference and the library."""
    for k in range(1, 17):
        d = np.arange(1, 2000, dtype=np.float64)
        scale = 1.0 / (d / (d * k))
        assert np.all(np.abs(scale - np.rint(scale)) < ar.DBL_EPSILON) and np.all(np.rint(scale) == k), k
    vs = capi.load()
    jobs = [_tuple(k * d, 3, d, 3) for k in range(1, 17) for d in (1, 3, 7, 49, 333, 1999)]
    assert np.all(vs.area_jobs_plan(jobs) >= 1)
    assert not ar.axis_integer(131, 130)[0] and not ar.axis_integer(32767, 32766)[0] and ar.axis_integer(32767, 4681) == (True, 7)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_class_2_is_the_linear_mean(cn, dtype):
    plane = np.random.default_rng(cn).integers(0, np.iinfo(dtype).max + 1, (50, 66 * cn), dtype)
    assert np.array_equal(ar.resize(plane, cn, 33, 25), rr.resize(plane, cn, 33, 25, rr.LINEAR))


def test_class_1_known_answers():
    # 3 x 1 boxes: (float)S * (1.f / 3); 1.f / 3 = 0.3333333432674408 in float32
    assert ar.resize(np.array([[1, 2, 4, 255, 255, 255, 0, 0, 1]], np.uint8), 1, 3, 1).tolist() == [[2, 255, 0]]
    # 2 x 1 boxes: exact halves go to even - 1.5 -> 2, 2.5 -> 2, 0.5 -> 0, 254.5 -> 254
    assert ar.resize(np.array([[1, 2, 2, 3, 0, 1, 254, 255]], np.uint8), 1, 4, 1).tolist() == [[2, 2, 0, 254]]
    # 4 x 2 box of 16-bit samples, cn 2: channel sums 8 * 65535 and 4 * 1 + 4 * 2 = 12 -> 65535, 1.5 -> 2
    p = np.array([[65535, 1] * 4, [65535, 2] * 4], np.uint16)
    assert ar.resize(p, 2, 1, 1).tolist() == [[65535, 2]]
    assert ar.resize(p, 2, 1, 1, 1023).tolist() == [[1023, 2]]
    assert ar.job_class(8, 1, 4, 1) == 1 and ar.job_class(4, 2, 1, 1) == 1


def test_the_same_size_is_the_identity():
    for dtype in (np.uint8, np.uint16):
        for cn in (1, 2):
            plane = np.random.default_rng(5 + cn).integers(0, np.iinfo(dtype).max + 1, (11, 37 * cn), dtype)
            assert np.array_equal(ar.resize(plane, cn, 37, 11), plane)
    t = ar.axis_table(37, 37)                                            # ... and through the tables too: one tap of weight 1
    assert np.array_equal(t[0], np.arange(37)) and np.all(t[1] == 1) and np.all(t[2] == 1)


# ---- 4. the ABI surface, refusals, no device -----------------------------------------------------------------------------------
NEW = ("vs_op_area_jobs", "vs_op_area_jobs_plan", "vs_op_area_yuv", "vs_op_area_rgb", "vs_area_axis_table")
GOOD = dict(src=BASE, src_stride=400, sw=130, sh=96, dst=BASE + (1 << 20), dst_stride=400, dw=97, dh=61, cn=1, reserved=0)


def _err(L):
    return (L.vs_last_error() or b"").decode()


def _jobs(L, jobs, n=None, sb=1, max_value=0, null=False):
    arr = (capi.VsScaleJob * len(jobs))(*[capi.VsScaleJob(**j) for j in jobs])
    rc = L.vs_op_area_jobs(None if null else arr, len(jobs) if n is None else n, sb, max_value, None)
    return rc, _err(L)


def test_the_new_entry_points_are_exported_declared_and_bound():
    vs = capi.load()
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    binding = open(os.path.join(ROOT, "video-stab_amd", "vsamd", "capi.py")).read()
    for name in NEW:
        assert hasattr(vs.lib, name), name + " is not exported by libvideo-stab.so"
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/vs_stab.h"
        assert getattr(vs.lib, name).argtypes and re.search(r"L\.%s\.argtypes" % name, binding), name
    assert vs.lib.vs_abi_version() == 2 and re.search(r"^#define VS_STAB_ABI_VERSION 2$", header, re.M)
    assert re.search(r"VS_ERR_UNSUPPORTED\s*=\s*%d\b" % UNSUPPORTED, header)


def test_job_refusals_and_no_device():
    L = capi.load().lib
    name = "vs_op_area_jobs"
    launch = [(dict(n=0), name), (dict(n=97), name), (dict(sb=4), name), (dict(sb=0), name), (dict(null=True), name), (dict(max_value=-1), "max_value"),
              (dict(max_value=256), "max_value"), (dict(sb=2, max_value=65536), "max_value")]
    for call, word in launch:
        rc, msg = _jobs(L, [GOOD] * max(1, call.get("n", 1)), **call)
        assert rc == INVALID and name in msg and word in msg, (call, rc, msg)
    jobs = [(dict(src=None), "null"), (dict(dst=None), "null"), (dict(sw=0), "sizes"), (dict(dh=32768), "sizes"), (dict(dw=-1), "sizes"), (dict(cn=0), "cn"),
            (dict(cn=5), "cn"), (dict(reserved=1), "reserved"), (dict(src_stride=129), "stride"), (dict(dst_stride=96), "stride"),
            (dict(dst=BASE + 400 * 95 + 129), "overlap"), (dict(dst=BASE), "overlap")]
    for change, word in jobs:
        for lead in (0, 2):
            rc, msg = _jobs(L, [GOOD] * lead + [dict(GOOD, **change)] + [GOOD])
            assert rc == INVALID and "%s: job %d" % (name, lead) in msg and word in msg, (change, lead, rc, msg)
    for change, word in [(dict(cn=3), "cn"), (dict(src_stride=401), "even"), (dict(src=BASE + 1), "even"), (dict(dst_stride=399), "even")]:
        rc, msg = _jobs(L, [dict(GOOD, **change)], sb=2)
        assert rc == INVALID and name + ": job 0" in msg and word in msg, (change, rc, msg)
    # the one new refusal: an upscale on either axis
    for change in (dict(dw=131), dict(dh=97), dict(sw=96, sh=60)):
        for lead in (0, 2):
            rc, msg = _jobs(L, [GOOD] * lead + [dict(GOOD, **change)] + [GOOD])
            assert rc == UNSUPPORTED and "%s: job %d" % (name, lead) in msg and "only downscales" in msg and "not built" in msg, (change, lead, rc, msg)
    if L.vs_device_count() <= 0:
        for j, kw in [(GOOD, {}), (dict(GOOD, cn=3, src_stride=390), {}), (dict(GOOD, cn=4, src_stride=520, dst_stride=388), {}),
                      (dict(GOOD, src_stride=520, dst_stride=388, cn=2), dict(sb=2, max_value=1023)), (dict(GOOD, dw=130, dh=96), {}),
                      (dict(GOOD, dw=65, dh=48), {}), (dict(GOOD, dw=26, dh=12), {})]:
            rc, msg = _jobs(L, [j], **kw)
            assert rc == NO_DEVICE, (j, kw, rc, msg)
    # the plan refuses the same and needs no device
    cls = (C.c_int32 * 1)()
    arr = (capi.VsScaleJob * 1)(capi.VsScaleJob(**dict(GOOD, cn=5)))
    assert L.vs_op_area_jobs_plan(arr, 1, 1, cls) == INVALID and "vs_op_area_jobs_plan: job 0" in _err(L)
    arr = (capi.VsScaleJob * 1)(capi.VsScaleJob(**dict(GOOD, dw=131)))
    assert L.vs_op_area_jobs_plan(arr, 1, 1, cls) == UNSUPPORTED and "vs_op_area_jobs_plan: job 0" in _err(L)
    arr = (capi.VsScaleJob * 1)(capi.VsScaleJob(**GOOD))
    assert L.vs_op_area_jobs_plan(arr, 1, 1, None) == INVALID and "null" in _err(L)
    assert L.vs_op_area_jobs_plan(arr, 1, 1, cls) == OK and cls[0] == 0


def _yuv(L, fmt, n=1, sw=130, sh=96, dw=98, dh=64, in_lay=None, out_lay=None, src=None, dst=None):
    sb = capi.PIXFMT[fmt].sample_bytes if fmt in capi.PIXFMT else 1
    lin, lout = capi.I420LayoutC(*(in_lay or (sw * sb, 0, 0, 0))), capi.I420LayoutC(*(out_lay or (dw * sb, 0, 0, 0)))
    s = (C.c_void_p * max(n, 1))(*(src or [BASE + (i << 22) for i in range(max(n, 1))]))
    d = (C.c_void_p * max(n, 1))(*(dst or [BASE + (1 << 30) + (i << 22) for i in range(max(n, 1))]))
    rc = L.vs_op_area_yuv(fmt, s, C.byref(lin), sw, sh, d, C.byref(lout), dw, dh, n, None)
    return rc, _err(L)


def test_surface_refusals_and_no_device():
    L = capi.load().lib
    call = "vs_op_area_yuv"
    for kw, words in [(dict(fmt=capi.FMT_BGR8), ("BGR8", "not a YUV surface format")), (dict(fmt=99), ("format 99",)), (dict(fmt=capi.FMT_NV12, n=0), ("NV12", "n must be")),
                      (dict(fmt=capi.FMT_NV12, n=33), ("NV12", "n must be")), (dict(fmt=capi.FMT_NV12, sw=129), ("source", "NV12", "even")),
                      (dict(fmt=capi.FMT_I420, dh=63), ("destination", "I420", "even")), (dict(fmt=capi.FMT_I422, dw=97), ("destination", "I422", "even")),
                      (dict(fmt=capi.FMT_I444, sw=0), ("source", "I444", "size")), (dict(fmt=capi.FMT_I444, sw=32768, in_lay=(32768, 0, 0, 0)), ("I444", "32767")),
                      (dict(fmt=capi.FMT_P010, in_lay=(258, 0, 0, 0)), ("source", "P010", "pitch")), (dict(fmt=capi.FMT_P010, out_lay=(197, 0, 0, 0)), ("destination", "P010", "even")),
                      (dict(fmt=capi.FMT_I010, in_lay=(262, 0, 0, 0)), ("source", "I010", "chroma pitch")),
                      (dict(fmt=capi.FMT_NV12, in_lay=(130, 0, 0, 64)), ("source", "NV12", "v_off")),
                      (dict(fmt=capi.FMT_I420, out_lay=(98, 0, 98 * 64, 98 * 64 + 8)), ("destination", "I420", "overlap")),
                      (dict(fmt=capi.FMT_NV12, n=2, src=[BASE, BASE + 4096], dst=[BASE + 8192, BASE]), ("NV12", "source surface 0 is destination surface 1"))]:
        rc, msg = _yuv(L, **kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    for kw in (dict(fmt=capi.FMT_NV12, dw=132), dict(fmt=capi.FMT_I010, dh=98), dict(fmt=capi.FMT_I444, dw=131, dh=97)):
        rc, msg = _yuv(L, **kw)
        assert rc == UNSUPPORTED and call in msg and capi.PIXFMT[kw["fmt"]].name in msg and "only downscales" in msg, (kw, rc, msg)
    call = "vs_op_area_rgb"

    def rgb(fmt=capi.FMT_BGR8, n=1, ss=400, sw=130, sh=96, ds=300, dw=97, dh=61, same=False, null=False):
        s = (C.c_void_p * max(n, 1))(*[None if null else BASE + (i << 20) for i in range(max(n, 1))])
        d = (C.c_void_p * max(n, 1))(*[BASE + (0 if same else 1 << 30) + (i << 20) for i in range(max(n, 1))])
        return L.vs_op_area_rgb(fmt, s, ss, sw, sh, d, ds, dw, dh, n, None), _err(L)
    for kw, words in [(dict(fmt=capi.FMT_NV12), ("NV12", "not an interleaved")), (dict(fmt=-1), ("format -1",)), (dict(n=0), ("BGR8", "n must be")), (dict(n=33), ("BGR8", "n must be")),
                      (dict(null=True), ("BGR8", "null")), (dict(ss=389), ("BGR8", "source", "pitch")), (dict(fmt=capi.FMT_BGRA8, ss=520, ds=387), ("BGRA8", "destination", "pitch")),
                      (dict(sw=0), ("BGR8", "sizes")), (dict(sh=40000), ("BGR8", "sizes")), (dict(same=True), ("BGR8", "is destination surface"))]:
        rc, msg = rgb(**kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    for kw in (dict(dw=131, ds=400), dict(dh=97)):
        rc, msg = rgb(**kw)
        assert rc == UNSUPPORTED and call in msg and "BGR8" in msg and "only downscales" in msg, (kw, rc, msg)
    # the table call
    i32, f32 = (C.c_int32 * 64)(), (C.c_float * 64)()
    for args, word in [((0, 0), "sizes"), ((32768, 4), "sizes"), ((4, -1), "sizes")]:
        assert L.vs_area_axis_table(*args, i32, i32, f32, f32, f32) == INVALID and "vs_area_axis_table" in _err(L) and word in _err(L), args
    assert L.vs_area_axis_table(4, 5, i32, i32, f32, f32, f32) == UNSUPPORTED and "vs_area_axis_table" in _err(L) and "not built" in _err(L)
    assert L.vs_area_axis_table(4, 4, i32, i32, f32, f32, None) == INVALID and "null" in _err(L)
    if L.vs_device_count() <= 0:
        for fmt in (capi.FMT_NV12, capi.FMT_P010, capi.FMT_I420, capi.FMT_I010, capi.FMT_I012, capi.FMT_I422, capi.FMT_I444, capi.FMT_I210, capi.FMT_I212,
                    capi.FMT_I410, capi.FMT_I412):
            assert _yuv(L, fmt, n=32)[0] == NO_DEVICE, fmt
            assert _yuv(L, fmt, n=1, dw=130, dh=96)[0] == NO_DEVICE, fmt                    # the same size is accepted
        for fmt, px in ((capi.FMT_BGR8, 3), (capi.FMT_RGB8, 3), (capi.FMT_BGRA8, 4), (capi.FMT_RGBA8, 4), (capi.FMT_GRAY8, 1)):
            assert rgb(fmt=fmt, n=32, ss=130 * px, ds=97 * px + 1)[0] == NO_DEVICE, fmt
