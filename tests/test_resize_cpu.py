"""Resize to an output size, the parts that need no GPU.

1. tests/resizeref.py LINEAR on uint8 equals the oracle's cv::resize(INTER_LINEAR) for up- and downscales, the 2 x 2 mean included.
2. ... and tests/cropzoomref.py for zoom-in shapes at both depths (so the new operator equals vs_op_resize_jobs there).
3. Lanczos known answers from the formula of include/vs_stab.h.
4. Lanczos properties: the identity, the 32-bit bound of the 8-bit sum over a dense scan of f, both clamps on checkerboards.
5. vs_resize_axis_table equals the reference's tables; so does tests/cpp/resize_tables_check.cpp, which compiles the header alone.
6. Refusals, VS_ERR_NO_DEVICE, the ABI surface.
7. The plan: which listed shape runs the staged and which the direct kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cropzoomref as cz
import resizeref as rr
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, 1, 2
LINEAR, LANCZOS4 = rr.LINEAR, rr.LANCZOS4

SHAPES = [((1, 1), (5, 3)), ((3, 2), (1, 1)), ((9, 9), (8, 8)), ((66, 50), (33, 25)), ((130, 96), (97, 61)), ((97, 61), (322, 200))]
SHAPE_IDS = ["%dx%d-%dx%d" % (s + d) for s, d in SHAPES]
PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 4), (8, 8), (64, 48), (130, 97), (97, 322), (1980, 1920), (3840, 1920), (3900, 3840), (32767, 2)]
# the shapes of the GPU tests whose kernel the plan test names
STAGED_SHAPE, DIRECT_SHAPE = ((130, 96), (97, 61)), ((322, 200), (64, 36))


def roi_plane(seed, sw, sh, cn, dtype):
    """A plane of sw x sh pixels as a VIEW into a larger random plane."""
    rng = np.random.default_rng(seed)
    parent = rng.integers(0, np.iinfo(dtype).max + 1, (sh + 5, (sw + 8) * cn), dtype=dtype)
    return parent, parent[2:2 + sh, 3 * cn:(3 + sw) * cn]


# ---- 1, 2. LINEAR ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_linear_u8_is_the_oracles_resize(oracle, shape, cn):
    (sw, sh), (dw, dh) = shape
    parent, plane = roi_plane(sw * 31 + sh + cn, sw, sh, cn, np.uint8)
    before = parent.copy()
    got = rr.resize(plane, cn, dw, dh, LINEAR)
    src = np.ascontiguousarray(plane).reshape(sh, sw) if cn == 1 else np.ascontiguousarray(plane).reshape(sh, sw, cn)
    want = np.asarray(oracle.resize(src, dw, dh)).reshape(dh, dw * cn)
    assert got.dtype == np.uint8 and got.shape == (dh, dw * cn) and np.array_equal(got, want)
    assert np.array_equal(parent, before)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("shape", [((126, 92), (130, 96)), ((20, 4), (64, 48)), ((2, 2), (64, 48)), ((1, 3), (32, 48)), ((97, 61), (322, 200)), ((7, 5), (7, 5))],
                         ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_linear_zoom_in_is_cropzoomrefs_resize(shape, cn, dtype):
    (sw, sh), (dw, dh) = shape
    _, plane = roi_plane(sw * 7 + dh + cn, sw, sh, cn, dtype)
    assert np.array_equal(rr.resize(plane, cn, dw, dh, LINEAR), cz.resize(plane, cn, dw, dh))


def test_the_mean_at_two_to_one_at_both_depths():
    for dtype in (np.uint8, np.uint16):
        _, plane = roi_plane(9, 66, 50, 2, dtype)
        p = np.ascontiguousarray(plane).reshape(50, 66, 2).astype(np.int64)
        want = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
        assert np.array_equal(rr.resize(plane, 2, 33, 25, LINEAR), want.reshape(25, 66).astype(dtype))
    # only the exact case: 66 x 50 -> 33 x 26 goes through the coefficients
    assert rr.is_mean(66, 50, 33, 25, LINEAR) and not rr.is_mean(66, 50, 33, 26, LINEAR) and not rr.is_mean(66, 50, 33, 25, LANCZOS4)


# ---- 3, 4. LANCZOS4 ----------------------------------------------------------------------------------------------------------
def test_lanczos_known_answers():
    assert rr.lanczos4_coefs(0.0) == [0, 0, 0, 2048, 0, 0, 0, 0]
    assert rr.lanczos4_coefs(0.5) == [-26, 122, -340, 1267, 1267, -340, 122, -26]
    assert rr.lanczos4_coefs(0.25) == [-31, 114, -312, 1830, 579, -188, 64, -8]


@pytest.mark.parametrize("interp", [LINEAR, LANCZOS4], ids=["linear", "lanczos4"])
def test_the_same_size_is_the_identity(interp):
    for dtype in (np.uint8, np.uint16):
        for cn in (1, 2):
            _, plane = roi_plane(5 + cn, 37, 11, cn, dtype)
            assert np.array_equal(rr.resize(plane, cn, 37, 11, interp), plane)


def test_lanczos_sums_fit_32_bits_on_8_bit_planes():
    """The bound of include/vs_stab.h over a dense scan of f: positive coefficients of an axis sum to at most 2780, negative ones to
    at most 732, all eight to 2045 .. 2051; hence |S| <= 255 * 2780^2 < 2^31 - 2^21 (and 65535 * 2780^2 < 2^39 for 16-bit planes)."""
    pos = neg = 0
    lo, hi = 1 << 30, 0
    for k in range(40000):
        c = rr.lanczos4_coefs(np.float32(k) / np.float32(40000))
        pos, neg = max(pos, sum(v for v in c if v > 0)), max(neg, -sum(v for v in c if v < 0))
        lo, hi = min(lo, sum(c)), max(hi, sum(c))
    assert pos <= 2780 and neg <= 732 and (lo, hi) == (2045, 2051), (pos, neg, lo, hi)
    assert 255 * 2780 * 2780 == 1970742000 < (1 << 31) - (1 << 21) and 65535 * 2780 * 2780 < 1 << 39


@pytest.mark.parametrize("case", [(np.uint8, 255, 0), (np.uint16, 65535, 0), (np.uint16, 1023, 1023)], ids=["255", "65535", "1023"])
def test_lanczos_checkerboards_hit_both_clamps(case):
    dtype, top, max_value = case
    board = (np.indices((24, 40)).sum(0) % 2 * top).astype(dtype)
    S = rr.lanczos_sum(board, 1, 52, 31)
    raw = (S + (1 << 21)) >> 22
    assert raw.min() < 0 and raw.max() > top                                     # both clamps are needed ...
    got = rr.resize(board, 1, 52, 31, LANCZOS4, max_value)
    assert got.min() == 0 and got.max() == top                                   # ... and hit
    assert np.array_equal(got, np.clip(raw, 0, top).astype(dtype))
    if max_value:                                                                # without the limit the type's maximum is the clamp
        assert rr.resize(board, 1, 52, 31, LANCZOS4).max() > top


# ---- 5. the tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_vs_resize_axis_table_equals_the_reference(pair):
    vs = capi.load()
    src, dst = pair
    for interp in (LINEAR, LANCZOS4):
        for axis in (0, 1):
            idx, coef = vs.resize_axis_table(src, dst, interp, axis)
            ri, rc = rr.axis_table(src, dst, interp, axis)
            assert idx.shape == ri.shape and np.array_equal(idx, ri) and np.array_equal(coef, rc), (interp, axis)
            assert idx.min() >= 0 and idx.max() <= src - 1


def test_the_header_alone_gives_the_reference_tables():
    """tests/cpp/resize_tables_check.cpp includes only csrc/resize_tables.h and is built with g++, as `make asan` builds it."""
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(ROOT, "tests", "cpp", "resize_tables_check.cpp"), os.path.join(build, "resize_tables_check")
    deps = [src, os.path.join(ROOT, "video-stab_amd", "csrc", "resize_tables.h")]
    assert re.findall(r'#include "([^"]+)"', open(src).read()) == ["../../video-stab_amd/csrc/resize_tables.h"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, src])
    cases = [(s, d, i, a) for s, d in PAIRS if max(s, d) <= 4000 for i in (LINEAR, LANCZOS4) for a in (0, 1)] + [(32767, 2, LANCZOS4, 0), (32767, 2, LINEAR, 1)]
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    for s, d, i, a in cases:
        k = rr.taps(i)
        assert next(lines).split() == [str(v) for v in (s, d, i, a, k)]
        got = np.array([next(lines).split() for _ in range(d)], np.int64)
        ri, rc = rr.axis_table(s, d, i, a)
        assert np.array_equal(got[:, :k], ri) and np.array_equal(got[:, k:], rc), (s, d, i, a)
    assert next(lines, None) is None


# ---- 6. refusals and the ABI surface -----------------------------------------------------------------------------------------
NEW = ("vs_op_resample_jobs", "vs_op_resample_jobs_plan", "vs_op_resize_yuv", "vs_op_resize_rgb", "vs_resize_axis_table")
BASE = 0x10000
GOOD = dict(src=BASE, src_stride=400, sw=130, sh=96, dst=BASE + (1 << 20), dst_stride=400, dw=97, dh=61, cn=1, reserved=0)


def _err(L):
    return (L.vs_last_error() or b"").decode()


def _jobs(L, jobs, n=None, sb=1, interp=LINEAR, max_value=0, path=0, null=False):
    arr = (capi.VsScaleJob * len(jobs))(*[capi.VsScaleJob(**j) for j in jobs])
    rc = L.vs_op_resample_jobs(None if null else arr, len(jobs) if n is None else n, sb, interp, max_value, path, None)
    return rc, _err(L)


def test_the_new_entry_points_are_exported_declared_and_bound():
    vs = capi.load()
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    binding = open(os.path.join(ROOT, "video-stab_amd", "vsamd", "capi.py")).read()
    for name in NEW:
        assert hasattr(vs.lib, name), name + " is not exported by libvideo-stab.so"
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/vs_stab.h"
        assert getattr(vs.lib, name).argtypes and re.search(r"L\.%s\.argtypes" % name, binding), name
    assert re.search(r"enum vs_interp \{ VS_INTERP_LINEAR = 0, VS_INTERP_LANCZOS4 = 1 \}", header)
    assert (capi.INTERP_LINEAR, capi.INTERP_LANCZOS4) == (0, 1)
    assert vs.lib.vs_abi_version() == 2 and re.search(r"^#define VS_STAB_ABI_VERSION 2$", header, re.M)


def test_job_refusals_and_no_device():
    L = capi.load().lib
    name = "vs_op_resample_jobs"
    launch = [(dict(n=0), name), (dict(n=97), name), (dict(sb=4), name), (dict(sb=0), name), (dict(null=True), name), (dict(interp=2), "interp"),
              (dict(interp=-1), "interp"), (dict(path=2), "path"), (dict(path=-1), "path"), (dict(max_value=-1), "max_value"),
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
    # what vs_op_resize_jobs refuses as unsupported is this operator's business: any ratio, cn 3 and 4 with 8-bit samples
    if L.vs_device_count() <= 0:
        for j, kw in [(GOOD, {}), (dict(GOOD, cn=3, src_stride=390), dict(interp=LANCZOS4)), (dict(GOOD, cn=4, src_stride=520, dst_stride=388), dict(path=1)),
                      (dict(GOOD, src_stride=520, dst_stride=388, cn=2), dict(sb=2, max_value=1023, interp=LANCZOS4)), (dict(GOOD, dw=322, dh=200, dst_stride=333), {})]:
            rc, msg = _jobs(L, [j], **kw)
            assert rc == NO_DEVICE, (j, kw, rc, msg)
    # the plan refuses the same and needs no device
    staged = (C.c_int32 * 1)()
    arr = (capi.VsScaleJob * 1)(capi.VsScaleJob(**dict(GOOD, cn=5)))
    assert L.vs_op_resample_jobs_plan(arr, 1, 1, LINEAR, staged) == INVALID and "vs_op_resample_jobs_plan: job 0" in _err(L)
    assert L.vs_op_resample_jobs_plan(arr, 1, 1, 7, staged) == INVALID and "interp" in _err(L)


def _yuv(L, fmt, n=1, sw=130, sh=96, dw=98, dh=64, interp=LINEAR, in_lay=None, out_lay=None, src=None, dst=None):
    sb = capi.PIXFMT[fmt].sample_bytes if fmt in capi.PIXFMT else 1
    lin, lout = capi.I420LayoutC(*(in_lay or (sw * sb, 0, 0, 0))), capi.I420LayoutC(*(out_lay or (dw * sb, 0, 0, 0)))
    s = (C.c_void_p * max(n, 1))(*(src or [BASE + (i << 22) for i in range(max(n, 1))]))
    d = (C.c_void_p * max(n, 1))(*(dst or [BASE + (1 << 30) + (i << 22) for i in range(max(n, 1))]))
    rc = L.vs_op_resize_yuv(fmt, s, C.byref(lin), sw, sh, d, C.byref(lout), dw, dh, n, interp, None)
    return rc, _err(L)


def test_surface_refusals_and_no_device():
    L = capi.load().lib
    call = "vs_op_resize_yuv"
    for kw, words in [(dict(fmt=capi.FMT_BGR8), ("BGR8", "not a YUV surface format")), (dict(fmt=99), ("format 99",)), (dict(fmt=capi.FMT_NV12, n=0), ("NV12", "n must be")),
                      (dict(fmt=capi.FMT_NV12, n=33), ("NV12", "n must be")), (dict(fmt=capi.FMT_NV12, sw=129), ("source", "NV12", "even")),
                      (dict(fmt=capi.FMT_I420, dh=63), ("destination", "I420", "even")), (dict(fmt=capi.FMT_I422, dw=97), ("destination", "I422", "even")),
                      (dict(fmt=capi.FMT_I444, sw=0), ("source", "I444", "size")), (dict(fmt=capi.FMT_I444, dw=32768, out_lay=(32768, 0, 0, 0)), ("I444", "32767")),
                      (dict(fmt=capi.FMT_P010, in_lay=(258, 0, 0, 0)), ("source", "P010", "pitch")), (dict(fmt=capi.FMT_P010, out_lay=(197, 0, 0, 0)), ("destination", "P010", "even")),
                      (dict(fmt=capi.FMT_I010, in_lay=(262, 0, 0, 0)), ("source", "I010", "chroma pitch")), (dict(fmt=capi.FMT_NV12, interp=2), ("NV12", "interp")),
                      (dict(fmt=capi.FMT_NV12, in_lay=(130, 0, 0, 64)), ("source", "NV12", "v_off")),
                      (dict(fmt=capi.FMT_I420, out_lay=(98, 0, 98 * 64, 98 * 64 + 8)), ("destination", "I420", "overlap")),
                      (dict(fmt=capi.FMT_NV12, n=2, src=[BASE, BASE + 4096], dst=[BASE + 8192, BASE]), ("NV12", "source surface 0 is destination surface 1"))]:
        rc, msg = _yuv(L, **kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    call = "vs_op_resize_rgb"

    def rgb(fmt=capi.FMT_BGR8, n=1, ss=400, sw=130, sh=96, ds=300, dw=97, dh=61, interp=LINEAR, same=False, null=False):
        s = (C.c_void_p * max(n, 1))(*[None if null else BASE + (i << 20) for i in range(max(n, 1))])
        d = (C.c_void_p * max(n, 1))(*[BASE + (0 if same else 1 << 30) + (i << 20) for i in range(max(n, 1))])
        return L.vs_op_resize_rgb(fmt, s, ss, sw, sh, d, ds, dw, dh, n, interp, None), _err(L)
    for kw, words in [(dict(fmt=capi.FMT_NV12), ("NV12", "not an interleaved")), (dict(fmt=-1), ("format -1",)), (dict(n=0), ("BGR8", "n must be")), (dict(n=33), ("BGR8", "n must be")),
                      (dict(null=True), ("BGR8", "null")), (dict(ss=389), ("BGR8", "source", "pitch")), (dict(fmt=capi.FMT_BGRA8, ss=520, ds=387), ("BGRA8", "destination", "pitch")),
                      (dict(sw=0), ("BGR8", "sizes")), (dict(dh=40000), ("BGR8", "sizes")), (dict(interp=5), ("BGR8", "interp")), (dict(same=True), ("BGR8", "is destination surface"))]:
        rc, msg = rgb(**kw)
        assert rc == INVALID and call in msg and all(w in msg for w in words), (kw, rc, msg)
    # the table call
    idx, coef = (C.c_int32 * 64)(), (C.c_int16 * 64)()
    for args, word in [((0, 4, 0, 0), "sizes"), ((4, 32768, 0, 0), "sizes"), ((4, 4, 2, 0), "interp"), ((4, 4, 0, 2), "axis")]:
        assert L.vs_resize_axis_table(*args, idx, coef) == INVALID and "vs_resize_axis_table" in _err(L) and word in _err(L), args
    assert L.vs_resize_axis_table(4, 4, 0, 0, None, coef) == INVALID and "null" in _err(L)
    if L.vs_device_count() <= 0:
        for fmt in (capi.FMT_NV12, capi.FMT_P010, capi.FMT_I420, capi.FMT_I010, capi.FMT_I012, capi.FMT_I422, capi.FMT_I444, capi.FMT_I210, capi.FMT_I212,
                    capi.FMT_I410, capi.FMT_I412):
            for interp in (LINEAR, LANCZOS4):
                assert _yuv(L, fmt, n=32, interp=interp)[0] == NO_DEVICE, fmt
        for fmt, px in ((capi.FMT_BGR8, 3), (capi.FMT_RGB8, 3), (capi.FMT_BGRA8, 4), (capi.FMT_RGBA8, 4), (capi.FMT_GRAY8, 1)):
            assert rgb(fmt=fmt, n=32, ss=130 * px, ds=97 * px + 1, interp=LANCZOS4)[0] == NO_DEVICE, fmt


# ---- 7. the plan -------------------------------------------------------------------------------------------------------------
def _plan(vs, shape, sb, cn, interp):
    (sw, sh), (dw, dh) = shape
    return int(vs.resample_jobs_plan([(BASE, sw * cn * sb, sw, sh, BASE + (1 << 28), dw * cn * sb, dw, dh, cn)], sb, interp)[0])


def test_the_plan_names_a_staged_and_a_direct_shape():
    """130 x 96 -> 97 x 61 runs the staged kernel, the strong downscale 322 x 200 -> 64 x 36 the direct one - for every sample size,
    channel count and interpolation of tests/test_gpu_resize.py, which therefore runs both kernels.  Every upscale is staged; so are
    the two measured 4K cases; the 2 : 1 mean rides in the staged launch."""
    vs = capi.load()
    for sb, cns in ((1, (1, 2, 3, 4)), (2, (1, 2))):
        for cn in cns:
            for interp in (LINEAR, LANCZOS4):
                assert _plan(vs, STAGED_SHAPE, sb, cn, interp) == 1, (sb, cn, interp)
                assert _plan(vs, DIRECT_SHAPE, sb, cn, interp) == 0, (sb, cn, interp)
                assert _plan(vs, ((97, 61), (322, 200)), sb, cn, interp) == 1
                assert _plan(vs, ((1, 1), (5, 3)), sb, cn, interp) == 1
    assert _plan(vs, ((3900, 2220), (3840, 2160)), 1, 1, LANCZOS4) == 1 and _plan(vs, ((3840, 2160), (1920, 1080)), 1, 1, LANCZOS4) == 1
    assert _plan(vs, ((66, 50), (33, 25)), 1, 1, LINEAR) == 1
    mixed = [(BASE, 400, 130, 96, BASE + (1 << 28), 400, 97, 61, 1), (BASE, 400, 322, 200, BASE + (1 << 28), 400, 64, 36, 1)]
    assert list(vs.resample_jobs_plan(mixed, 1, LANCZOS4)) == [1, 0]
