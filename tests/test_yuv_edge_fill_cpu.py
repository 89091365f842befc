"""Edge fill on YUV streams, the parts that need no GPU.

1. tests/yuvfillref.py, the numpy statement of the fill warp: with fill 0 it is the oracle's cv::warpAffine (8-bit) and
   i010_inputs.warp_plane(BLACK) (16-bit) over the matrix classes of the warp tests and the sheared chroma matrices of 4:2:2; its sum
   obeys the exact identity S_fill = S_black(img) + F (1024 - S_black(ones)); and a constant plane equal to its fill warps to the
   constant under every matrix - what makes the surround of the picture exactly the fill colour.
2. The refusal rules (video-stab_amd/csrc/pixfmt.h through tests/cpp/yuv_pad_check.cpp): the mode adds no argument to them, so every
   recorded answer is today's, and GRAY8 and the colour formats answer as before.
3. The ABI surface: the three new entry points are exported and declared, and the operator refuses a format without chroma planes, a
   reserved field, an 8-bit sample above 255 and null arguments on the host - no device is needed to get these."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import i010_inputs as ii
import planar_inputs as pi
import ref16
import refusal_cases
import yuvfillref as yf
from p010_inputs import MATS
from test_yuv_border_pad_cpu import _pitch, _rules
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHEARED = {"422_" + k: pi.chroma_matrix(M, 1, 0) for k, M in pi.ALL_MATS.items()}
ALL = dict(pi.ALL_MATS, **SHEARED)
assert set(MATS) <= set(ALL)


# ---- 1. the numpy statement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_fill_zero_is_the_black_warp(oracle, name):
    M = ALL[name]
    rng = np.random.default_rng(len(name))
    for w, h in ((67, 41), (130, 33)):
        p8 = rng.integers(0, 256, (h, w), np.uint8)
        assert np.array_equal(yf.warp_plane(p8, M, 0), oracle.warp_affine(p8, M)), (name, w, h)
        p16 = rng.integers(0, 65536, (h, w), np.uint16)
        assert np.array_equal(yf.warp_plane(p16, M, 0), ii.warp_plane(p16, M, ii.BLACK)), (name, w, h)
        uv16 = rng.integers(0, 65536, (h, w, 2), np.uint16)
        assert np.array_equal(yf.warp_plane(uv16, M, (0, 0)), ref16.warp_affine(uv16, M)), (name, w, h)
        uv8 = rng.integers(0, 256, (h, w, 2), np.uint8)
        got = yf.warp_plane(uv8, M, (0, 0))
        for c in range(2):
            assert np.array_equal(got[..., c], oracle.warp_affine(np.ascontiguousarray(uv8[..., c]), M)), (name, w, h, c)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_the_sum_is_the_black_sum_plus_the_fill_times_the_weight_outside(dtype):
    """S_fill = S_black(img) + F * (1024 - S_black(ones)): the taps inside contribute what they do under BORDER_CONSTANT 0, the taps
    outside the fill times their weights, and the weights of a pixel sum to 1024.  Exact integers, random F and random planes."""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(top)
    for name, M in ALL.items():
        Md = np.asarray(M, np.float32).astype(np.float64)
        for w, h in ((67, 41), (9, 5)):
            img = rng.integers(0, top + 1, (h, w), dtype)
            F = int(rng.integers(1, top + 1))
            inside = ref16.warp_sum(np.ones((h, w), dtype), Md)
            assert inside.min() >= 0 and inside.max() <= 1024
            assert np.array_equal(yf.warp_sum(img, Md, F), ref16.warp_sum(img, Md) + F * (1024 - inside)), (name, w, h)
        uv = rng.integers(0, top + 1, (21, 30, 2), dtype)
        Fu, Fv = (int(v) for v in rng.integers(1, top + 1, 2))
        inside = ref16.warp_sum(np.ones((21, 30), dtype), Md)
        S = yf.warp_sum(uv, Md, (Fu, Fv))
        for c, F in enumerate((Fu, Fv)):       # the pair is not swapped and not shared
            assert np.array_equal(S[..., c], ref16.warp_sum(uv[..., c], Md) + F * (1024 - inside)), (name, c)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_a_constant_plane_equal_to_its_fill_warps_to_the_constant(dtype):
    for c in ((0, 16, 128, 235, 255) if dtype == np.uint8 else (0, 64, 512, 0x8000, 65535)):
        for name, M in ALL.items():
            got = yf.warp_plane(np.full((20, 36), c, dtype), M, c)
            assert got.dtype == dtype and np.all(got == c), (name, c)
    got = yf.warp_plane(np.full((20, 36, 2), (90, 240), np.uint8), ALL["small_rot"], (90, 240))
    assert np.all(got[..., 0] == 90) and np.all(got[..., 1] == 240)


def test_warp_surface_gives_every_plane_its_sample_and_its_matrix():
    rng = np.random.default_rng(5)
    M = pi.rotation(2.0, 9.5, -6.25)
    y, u, v = (rng.integers(0, 1024, s, np.uint16) for s in ((48, 64), (48, 32), (48, 32)))       # 4:2:2
    wy, wu, wv = yf.warp_surface([y, u, v], 1, 0, M, (64, 512, 500))
    Mc = pi.chroma_matrix(M, 1, 0)
    assert np.array_equal(yf.chroma_matrix(M, 1, 0), Mc) and np.array_equal(yf.chroma_matrix(M, 1, 1), pi.chroma_matrix(M, 1, 1))
    assert np.array_equal(wy, yf.warp_plane(y, M, 64)) and np.array_equal(wu, yf.warp_plane(u, Mc, 512)) and np.array_equal(wv, yf.warp_plane(v, Mc, 500))
    assert wy[47, 0] == 64 and wu[47, 0] == 512 and wv[47, 0] == 500            # (the corner the picture has left)
    uv = rng.integers(0, 256, (24, 32, 2), np.uint8)                            # the UV plane of a 64 x 48 NV12 surface
    wy, wuv = yf.warp_surface([y.astype(np.uint8), uv], 1, 1, M, (16, 128, 129))
    assert wuv.shape == uv.shape and tuple(wuv[23, 0]) == (128, 129) and wy[47, 0] == 16


# ---- 2. the refusal rules ----------------------------------------------------------------------------------------------------
def test_without_the_mode_every_answer_is_todays():
    """The mode is no argument of the rules (check_input, pixfmt.h): the recorded answers of the border cases
    (tests/golden/stream_refusals.json) stand, whatever the switch says - a YUV stream with a border_size and no pad mode opted in is
    refused as before."""
    golden = refusal_cases.load_golden(os.path.join(ROOT, "tests", "golden", "stream_refusals.json"))
    todo = [c for c in refusal_cases.cases() if c.entry == "push_dev" and c.border > 0 and not refusal_cases.stateful(c) and not c.data_odd and not c.out_odd
            and c.nv12 == (0, 0) and c.i420 == (0,) * 6 and c.out_pitch == c.pitch]
    assert len(todo) >= 3 * 16
    for c, (with_mode, default, _) in zip(todo, _rules([(c.fmt, c.w, c.h, c.pitch, c.border, c.crop, c.canvas, c.fade, 0, 0, 0) for c in todo])):
        assert with_mode == default == golden[c.id], c.id
    src = open(os.path.join(ROOT, "video-stab_amd", "csrc", "pixfmt.h")).read()
    assert "edge_fill" not in src and "efill" not in src          # (the rules do not know the mode)
    public = re.search(r"typedef enum vs_border \{(.*?)\}", open(os.path.join(ROOT, "include", "vs_stab.h")).read(), re.S)
    assert public and len(re.findall(r"VS_BORDER_\w+ = \d", public.group(1))) == 6 and "FILL" not in public.group(1)


def test_gray8_and_the_colour_formats_answer_as_before():
    for name in ("GRAY8", "BGR8", "BGRA8", "RGBA8", "RGB8"):
        fmt, p = getattr(capi, "FMT_" + name), _pitch(name)
        for a, d, black in _rules([(fmt, 64, 48, p, 0, 0, 0, 0, 0, 0, 0), (fmt, 64, 48, p, 8, 0, 0, 0, 0, 0, 0), (fmt, 64, 48, p, 8, 1, 0, 0, 0, 0, 0)]):
            assert a == d and black == (0, 0, 0), name
    assert _rules([(capi.FMT_GRAY8, 64, 48, 64, 8, 0, 0, 0, 0, 0, 0)])[0][0][0] == 4


# ---- 3. the ABI surface ------------------------------------------------------------------------------------------------------
NEW = ("vs_stab_set_yuv_edge_fill", "vs_batch_set_yuv_edge_fill", "vs_op_warp_affine_yuv_fill")


def test_the_new_entry_points_are_exported_and_declared():
    vs = capi.load()
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    for name in NEW:
        assert hasattr(vs.lib, name), name + " is not exported by libvideo-stab.so"
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/vs_stab.h"
    assert vs.lib.vs_abi_version() == 2
    assert vs.lib.vs_stab_set_yuv_edge_fill(None, 1, None) == 1 and vs.lib.vs_batch_set_yuv_edge_fill(None, 1, None) == 1


def test_the_operator_refuses_on_the_host():
    vs = capi.load()
    M = np.array([1, 0, 0, 0, 1, 0], np.float32)
    buf = C.create_string_buffer(16)           # never read: every call below is refused before anything touches a device

    def call(fmt, fill, src=buf, dst=buf, m=M, batch=1, w=64, h=48):
        c = C.byref(capi.VsYuvFill(*fill)) if fill is not None else None
        rc = vs.lib.vs_op_warp_affine_yuv_fill(fmt, C.cast(src, C.c_void_p) if src is not None else None, 128, 0, 0, 0,
                                               C.cast(dst, C.c_void_p) if dst is not None else None, 128, 0, 0, 0, w, h,
                                               capi._p(m, capi.f32p) if m is not None else None, batch, 0, 0, c, None)
        return rc, (vs.lib.vs_last_error() or b"").decode()
    for fmt in (capi.FMT_BGR8, capi.FMT_GRAY8, capi.FMT_RGBA8, -1, 99):
        rc, msg = call(fmt, None)
        assert rc == 1 and "vs_op_warp_affine_yuv_fill" in msg and "YUV surface format" in msg, fmt
    rc, msg = call(capi.FMT_NV12, (16, 128, 128, 1))
    assert rc == 1 and "reserved" in msg
    for name in ("NV12", "I420", "I422", "I444"):
        for bad in ((256, 0, 0, 0), (0, 300, 0, 0), (0, 0, 65535, 0)):
            rc, msg = call(getattr(capi, "FMT_" + name), bad)
            assert rc == 1 and "above 255" in msg and name in msg and "vs_op_warp_affine_yuv_fill" in msg, (name, bad)
    for kw in (dict(src=None), dict(dst=None), dict(m=None), dict(batch=0), dict(w=0), dict(h=-1)):
        rc, msg = call(capi.FMT_P010, (65535, 65535, 65535, 0), **kw)
        assert rc == 1 and "vs_op_warp_affine_yuv_fill: invalid argument" in msg, kw
