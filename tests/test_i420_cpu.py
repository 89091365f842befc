"""I420 / YV12 (planar 4:2:0) without a device: the equivalence the format rests on, the clip helpers, the public surface.

cv::warpAffine treats channels independently, so the U and the V plane of an I420 frame, each warped as a one-channel plane of
w/2 x h/2 under the matrix with the halved translation, are exactly the two channels of the NV12 chroma plane's warp.  The
GPU tests (tests/test_gpu_i420.py) therefore take the unchanged oracle's NV12 result, de-interleaved, as the expected value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the matrix classes of tests/test_gpu_pixfmt.py: identity, integer shift, sub-pixel shift, rotation, zoom, fully out of frame
MATS = {
    "identity": [1, 0, 0, 0, 1, 0],
    "int_shift": [1, 0, 7, 0, 1, -3],
    "frac_shift": [1, 0, 3.40625, 0, 1, -2.71875],
    "small_rot": [0.99995, -0.01, 3.25, 0.01, 0.99995, -7.5],
    "rot_zoom_beyond_box": [1.1 * np.cos(0.35), -1.1 * np.sin(0.35), 40.0, 1.1 * np.sin(0.35), 1.1 * np.cos(0.35), -25.0],
    "saturated": [1, 0, -40000.5, 0, 1, 35000.25],
}


def halved(M):
    """The chroma matrix: the translation halved in float, as the library and the oracle form it."""
    m = np.asarray(M, np.float32).copy()
    m[2] = m[2] * np.float32(0.5)
    m[5] = m[5] * np.float32(0.5)
    return m


@pytest.mark.parametrize("name", list(MATS))
@pytest.mark.parametrize("size", [(2, 2), (130, 34), (258, 130)], ids=lambda s: "%dx%d" % s)
def test_nv12_chroma_warp_is_the_warp_of_the_u_and_v_planes(oracle, size, name):
    w, h = size
    nv12 = np.random.default_rng(w * 13 + h).integers(0, 256, (h * 3 // 2, w), np.uint8)
    got = oracle.warp_affine_nv12(nv12, w, h, MATS[name])
    u, v = np.ascontiguousarray(nv12[h:, 0::2]), np.ascontiguousarray(nv12[h:, 1::2])
    assert np.array_equal(got[:h], oracle.warp_affine(np.ascontiguousarray(nv12[:h]), MATS[name]))
    assert np.array_equal(got[h:, 0::2], oracle.warp_affine(u, halved(MATS[name])))
    assert np.array_equal(got[h:, 1::2], oracle.warp_affine(v, halved(MATS[name])))


# ---- the clip helpers ------------------------------------------------------------------------------------------------------------
def test_packed_helpers_round_trip():
    for w, h in ((2, 2), (6, 10), (34, 18), (322, 200)):
        nv12 = np.random.default_rng(w + h).integers(0, 256, (h * 3 // 2, w), np.uint8)
        p = synth.nv12_to_i420(nv12)
        assert p.shape == nv12.shape and p.dtype == np.uint8
        assert np.array_equal(p[:h], nv12[:h])
        flat = p.reshape(-1)
        assert np.array_equal(flat[w * h:w * h + w * h // 4].reshape(h // 2, w // 2), nv12[h:, 0::2])      # U
        assert np.array_equal(flat[w * h + w * h // 4:].reshape(h // 2, w // 2), nv12[h:, 1::2])           # V
        assert np.array_equal(synth.i420_to_nv12(p, w, h), nv12)


@pytest.mark.parametrize("layout", ["padded", "odd_chroma_pitch", "yv12", "planes_apart"])
def test_padded_helpers_round_trip_and_leave_the_fill(layout):
    w, h = 34, 18
    nv12 = np.random.default_rng(5).integers(0, 255, (h * 3 // 2, w), np.uint8)     # (255 is the fill)
    kw = dict(padded=dict(pitch=48), odd_chroma_pitch=dict(pitch=48, c_pitch=19), yv12=dict(pitch=40, u_off=40 * h + 9 * 20, v_off=40 * h),
              planes_apart=dict(pitch=64, c_pitch=32, u_off=64 * 24, v_off=64 * 24 + 32 * 16, size=64 * 24 + 32 * 32))[layout]
    buf = synth.nv12_to_i420(nv12, fill=255, **kw)
    lay = {k: v for k, v in kw.items() if k != "size"}
    assert buf.ndim == 1
    assert np.array_equal(synth.i420_to_nv12(buf, w, h, **lay), nv12)
    assert np.count_nonzero(buf != 255) <= nv12.size and np.count_nonzero(buf == 255) >= buf.size - nv12.size
    pitch, c_pitch, u_off, v_off = synth.i420_layout(w, h, **lay)
    assert np.array_equal(buf[u_off:u_off + w // 2], nv12[h, 0::2]) and np.array_equal(buf[v_off:v_off + w // 2], nv12[h, 1::2])
    assert np.array_equal(buf[pitch:pitch + w], nv12[1, :]) and np.array_equal(buf[u_off + c_pitch:u_off + c_pitch + w // 2], nv12[h + 1, 0::2])


def test_layout_defaults():
    assert synth.i420_layout(64, 48) == (64, 32, 64 * 48, 64 * 48 + 24 * 32)
    assert synth.i420_layout(64, 48, pitch=80) == (80, 40, 80 * 48, 80 * 48 + 24 * 40)
    assert synth.i420_layout(64, 48, pitch=80, c_pitch=64) == (80, 64, 80 * 48, 80 * 48 + 24 * 64)


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vs_stab.h")).read()


def test_enum_value_in_the_header_and_the_binding():
    body = re.search(r"typedef enum vs_pixfmt_planar \{(.*?)\} vs_pixfmt_planar;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert {k: int(v) for k, v in re.findall(r"(VS_\w+)\s*=\s*(\d+)", body)} == {"VS_FMT_I420": 7}
    assert capi.FMT_I420 == 7
    assert re.search(r"#define VS_STAB_ABI_VERSION 2\b", _header())


@pytest.mark.parametrize("name", ["vs_stab_set_i420_layout", "vs_batch_set_i420_layout", "vs_op_warp_affine_i420"])
def test_entry_points_are_declared_and_exported(vs, name):
    assert re.search(r"\bint\s+%s\s*\(" % name, _header())
    assert hasattr(vs.lib, name)


def test_header_documents_yv12_and_ffmpeg_pitches():
    h = _header()
    assert "YV12" in h and "linesize[1]" in h


def test_shape_helpers():
    s = capi.Stabilizer.__new__(capi.Stabilizer)
    assert s._geom(np.zeros((36, 32), np.uint8), capi.FMT_I420) == (32, 24, 1)
    assert capi.fmt_dtype(capi.FMT_I420) == np.uint8 and capi.fmt_420(capi.FMT_I420) and not capi.fmt_two_planes(capi.FMT_I420)
    s.close = lambda: None


def test_null_objects_and_no_device(vs):
    assert vs.lib.vs_stab_set_i420_layout(None, 0, 0, 0, 0, 0, 0) == 1          # VS_ERR_INVALID_ARG
    assert vs.lib.vs_batch_set_i420_layout(None, 0, 0, 0, 0, 0, 0) == 1
    if vs.lib.vs_device_count() > 0:
        return                                                                 # (the GPU tests cover the calls on a device)
    M = np.asarray(MATS["identity"], np.float32)
    buf = np.zeros(64, np.uint8)
    rc = vs.lib.vs_op_warp_affine_i420(buf.ctypes.data, 4, 0, 0, 0, buf.ctypes.data, 4, 0, 0, 0, 4, 4, capi._p(M, capi.f32p), 1, 24, 24, 0, None)
    assert rc == 2                                                             # VS_ERR_NO_DEVICE
    assert b"no CPU fallback" in vs.lib.vs_last_error()
    with pytest.raises(capi.VsError):
        vs.warp_affine_i420(np.zeros((6, 4), np.uint8), 4, 4, MATS["identity"])
    h = C.c_void_p()
    p = vs.params()
    assert vs.lib.vs_stab_create(C.byref(p), 0, C.byref(h)) == 2               # no instance to push an I420 frame into
