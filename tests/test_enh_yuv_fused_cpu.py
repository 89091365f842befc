"""vs_enh_apply_yuv_batch_dev without a GPU: the declarations, the plan (which stage lists take the fused launch), the refusals that
need no device, and the numpy / oracle statement tests/enhyuvref.py the GPU tests hold the launch to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cvtref
import enhyuvref
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_enh_apply_yuv_batch_dev", "vs_enh_last_fused", "vs_enh_yuv_plan")
INVALID_ARG, UNSUPPORTED = 1, 4
NV12 = capi.PIXFMT_BY_NAME["NV12"].fmt

TABLES = dict(brightness=1.5, contrast=1.1, gamma=1.2)
SHIPPED = dict(enable_unsharp=1, sharpness=1.0)                           # video-stab_amd/config.example.yaml
# (settings, in_place, expected)
PLANS = [
    (TABLES, 0, 1),
    (TABLES, 1, 1),                                                      # the point pass may run in place
    (dict(TABLES, enable_vibrance=1), 0, 1),
    (SHIPPED, 0, 1),
    (dict(TABLES, **SHIPPED), 0, 1),
    (dict(SHIPPED, gamma=1.2), 0, 1),                                     # gamma behind the blur
    (dict(SHIPPED, use_cuda=1, brightness=1.5, contrast=1.1, gamma=1.2), 0, 1),
    (dict(TABLES, enable_white_balance=1), 0, 0),
    (dict(TABLES, enable_clahe=1), 0, 0),
    (dict(TABLES, enable_denoise=1), 0, 0),
    (SHIPPED, 1, 0),                                                     # a tile reads its neighbours' samples
    (dict(SHIPPED, use_cuda=1, enable_vibrance=1), 0, 0),                 # vibrance behind the blur: an intermediate frame
    (dict(SHIPPED, enable_vibrance=1), 0, 0),                             # ... and in front of it: the blur takes tables only
    (dict(enable_clahe=1, clahe_tile_grid_size=17), 0, -UNSUPPORTED),
    (dict(SHIPPED, blur_sigma=0.0), 0, -INVALID_ARG),
    (dict(SHIPPED, blur_sigma=6.0), 0, -UNSUPPORTED),                     # 37 taps
]


def test_declared_exported_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(vs.lib, n) and getattr(vs.lib, n).argtypes, n
    comment = header[:header.index("#define VS_STAB_ABI_VERSION")]
    assert all(n in comment for n in NAMES)
    assert vs.lib.vs_abi_version() == 2
    assert callable(capi.Enhancer.apply_yuv_batch_dev) and callable(capi.Enhancer.last_fused) and callable(vs.enh_yuv_plan)


@pytest.mark.parametrize("k", range(len(PLANS)))
def test_plan(vs, k):
    settings, in_place, want = PLANS[k]
    p = capi.Enhancer.default_params(vs, **settings)
    for name in cvtref.YUV_FORMATS:                                      # the plan does not depend on the format
        assert vs.enh_yuv_plan(p, capi.PIXFMT_BY_NAME[name].fmt, in_place) == want, (settings, name)


def test_plan_refusals(vs):
    p = capi.Enhancer.default_params(vs, **TABLES)
    for name in ("BGR8", "RGB8", "BGRA8", "RGBA8", "GRAY8"):
        assert vs.enh_yuv_plan(p, capi.PIXFMT_BY_NAME[name].fmt) == -INVALID_ARG, name
    for bad in (-1, 16, 99):
        assert vs.enh_yuv_plan(p, bad) == -INVALID_ARG
    assert vs.enh_yuv_plan(None, NV12) == -INVALID_ARG


def test_refusals_need_no_device(vs):
    p = capi.Enhancer.default_params(vs, **TABLES)
    lay = capi.I420LayoutC(8, 0, 0, 0)
    ptrs = (C.c_void_p * 1)(0x100000)
    assert vs.lib.vs_enh_apply_yuv_batch_dev(None, C.byref(p), NV12, ptrs, C.byref(lay), ptrs, C.byref(lay), 1, 8, 4) == INVALID_ARG
    assert vs.lib.vs_enh_last_fused(None) == 0


def crop(w, h):
    return np.ascontiguousarray(synth.make_clip(synth.SEED_CONFIG1, 160, 120, 1)[0][40:40 + h, 10:10 + w])


@pytest.mark.parametrize("name", ["NV12", "P010", "I420", "YV12", "I012", "I422", "I444", "I210", "I412"])
def test_statement(oracle, name):
    w, h = 34, 6
    lay = enhyuvref.yv12_layout(w, h) if name == "YV12" else None
    size = w * h * 3 // 2 if lay else None
    surface = enhyuvref.from_bgr(name, crop(w, h), lay, size)
    if name == "YV12":                                                   # the same planes as I420, V in front
        y, u, v = enhyuvref.unpack("I420", enhyuvref.from_bgr("I420", crop(w, h)), w, h)
        assert np.array_equal(surface, np.concatenate([y.reshape(-1), v.reshape(-1), u.reshape(-1)]))
    trip = enhyuvref.round_trip(name, surface, w, h, lay, lay, size)
    neutral = enhyuvref.enhance_yuv(oracle, oracle.enh_params(), name, surface, w, h, lay, lay, size)
    assert neutral.dtype == surface.dtype and np.array_equal(neutral, trip), name
    shipped = enhyuvref.enhance_yuv(oracle, oracle.enh_params(**SHIPPED), name, surface, w, h, lay, lay, size)
    assert shipped.shape == trip.shape and not np.array_equal(shipped, trip), name
    # a result in a layout holds the fill wherever no sample lies
    if name in ("NV12", "I420"):
        pitch = w + 5
        lo = (pitch, 0, h * pitch + 7, 0) if name == "NV12" else (pitch, w // 2 + 3, h * pitch + 7, h * pitch + 7 + (h // 2) * (w // 2 + 3) + 2)
        n = capi.yuv_surface_bytes(capi.PIXFMT_BY_NAME[name].fmt, w, h, *lo) + 16
        out = enhyuvref.enhance_yuv(oracle, oracle.enh_params(**SHIPPED), name, surface, w, h, None, lo, n, 0xA5)
        assert out.size == n and np.array_equal(enhyuvref.unpack(name, out, w, h, lo)[0], enhyuvref.unpack(name, shipped, w, h)[0])
        assert (out[-16:] == 0xA5).all() and (out[:h * pitch].reshape(h, pitch)[:, w:] == 0xA5).all()
