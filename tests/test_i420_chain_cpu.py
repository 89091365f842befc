"""Roll correction and auto zoom/crop on I420 / I010 / I012 surfaces: what holds without a GPU.

1. the four entry points exist in the library, are declared in include/vs_stab.h and are bound in vsamd/capi.py;
2. without a device the objects they need cannot be created (VS_ERR_NO_DEVICE, as for the NV12 forms), and a call without an object
   is VS_ERR_INVALID_ARG.  The NV12 forms check their arguments before they touch the device, but on an object - and there is no
   object without a device: the refusals of odd geometry, odd pitches and short chroma pitches are asserted in
   tests/test_gpu_i420_chain.py;
3. the definitions the GPU tests lean on hold on the references alone: a warp treats channels independently, so the two channels of
   the NV12 / P010 chroma plane's warp are the warps of the U plane and of the V plane - for the roll stage's rotation
   (BORDER_REPLICATE) and for the zoom stage's crop-and-scale jobs (BORDER_CONSTANT), 8-bit on the oracle and 16-bit on ref16_geom."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref16_geom as geom
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vs_roll_correct_i420_dev", "vs_roll_correct_i420_dev_n", "vs_azc_apply_i420_dev", "vs_azc_apply_i420_dev_n"]
W, H = 64, 48
ANGLES = [0.0, 0.37, -1.9, 4.25]


def _header():
    with open(os.path.join(ROOT, "include", "vs_stab.h")) as f:
        return f.read()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exist_are_declared_and_bound(vs):
    hdr = _header()
    with open(capi.__file__) as f:
        binding = f.read()
    for name in NEW:
        assert hasattr(vs.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(vs.lib, name).argtypes, name
        assert re.search(r"L\.%s\.argtypes" % name, binding), name
    m = re.search(r"typedef struct vs_i420_layout \{(.*?)\} vs_i420_layout;", hdr, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split() == "size_t pitch; size_t c_pitch; size_t u_off, v_off;".split()
    assert [f[0] for f in capi.I420LayoutC._fields_] == ["pitch", "c_pitch", "u_off", "v_off"]
    assert C.sizeof(capi.I420LayoutC) == 4 * C.sizeof(C.c_size_t)
    assert vs.lib.vs_abi_version() == 2 and "#define VS_STAB_ABI_VERSION 2" in hdr
    for cls, names in ((capi.RollCorrection, ("correct_i420_dev", "correct_i420_dev_n")), (capi.AutoZoomCrop, ("apply_i420_dev", "apply_i420_dev_n"))):
        for n in names:
            assert callable(getattr(cls, n))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_calls_without_an_object_are_refused_and_no_device_means_no_object(vs):
    lay = capi.i420_layout(W)
    buf = np.zeros(W * H * 3, np.uint8)
    p, t = buf.ctypes.data, C.c_int64(-1)
    ptrs = (C.c_void_p * 1)(p)
    for fmt in (capi.FMT_I420, capi.FMT_I010, capi.FMT_I012):
        assert vs.lib.vs_roll_correct_i420_dev(None, fmt, p, W, H, C.byref(lay), p, C.byref(lay)) == 1          # VS_ERR_INVALID_ARG
        assert vs.lib.vs_roll_correct_i420_dev_n(None, fmt, ptrs, ptrs, 1, W, H, C.byref(lay), C.byref(lay)) == 1
        assert vs.lib.vs_azc_apply_i420_dev(None, fmt, p, W, H, C.byref(lay), p, C.byref(lay), C.byref(t)) == 1
        assert vs.lib.vs_azc_apply_i420_dev_n(None, fmt, ptrs, ptrs, 1, W, H, C.byref(lay), C.byref(lay), None) == 1
    # (the NV12 forms do the same)
    assert vs.lib.vs_roll_correct_nv12_dev(None, p, W, H, W, 0, p, W, 0) == 1
    assert vs.lib.vs_azc_apply_nv12_dev(None, p, W, H, W, 0, p, 640, 640 * 360, C.byref(t)) == 1
    if vs.lib.vs_device_count() > 0:
        return                                                                 # (the GPU tests cover the calls on a device)
    h = C.c_void_p()
    rp = vs.roll_params()
    assert vs.lib.vs_roll_create(C.byref(rp), 0, C.byref(h)) == 2              # VS_ERR_NO_DEVICE
    assert b"no CPU fallback" in vs.lib.vs_last_error() and not h.value
    assert vs.lib.vs_azc_create(0, C.byref(h)) == 2 and not h.value
    with pytest.raises(capi.VsError):
        vs.roll_correction()
    with pytest.raises(capi.VsError):
        vs.auto_zoom_crop()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def _nv12(seed):
    return np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), np.uint8)


def _surface16(seed):
    return np.random.default_rng(seed).integers(0, 65536, (H * 3 // 2, W), np.uint16)


@pytest.mark.parametrize("angle", ANGLES)
def test_rotation_of_the_interleaved_chroma_plane_is_the_rotation_of_u_and_of_v(oracle, angle):
    _, Mc = geom.roll_matrices(W, H, angle)
    uv8 = np.ascontiguousarray(_nv12(11)[H:].reshape(H // 2, W // 2, 2))
    both = oracle.warp_affine_d(uv8, Mc, geom.REPLICATE)              # (vso_warp_affine_d, cn 2)
    for c in range(2):
        assert np.array_equal(both[:, :, c], oracle.warp_affine_d(np.ascontiguousarray(uv8[:, :, c]), Mc, geom.REPLICATE)), c
    uv16 = _surface16(12)[H:].reshape(H // 2, W // 2, 2)
    both = geom.warp(uv16, Mc, None, geom.REPLICATE)
    for c in range(2):
        assert np.array_equal(both[:, :, c], geom.warp(uv16[:, :, c], Mc, None, geom.REPLICATE)), c


def _oracle_sized(oracle, roi, M, dsize):
    """vso_warp_affine_d warps into the source's own size: the rectangle goes into the corner of a black canvas that holds both sizes -
    the taps outside the rectangle then read the zeros BORDER_CONSTANT gives them - and the dw x dh corner of the result is the job's."""
    dw, dh = dsize
    ch, cw = roi.shape[:2]
    canvas = np.zeros((max(ch, dh) + 2, max(cw, dw) + 2) + roi.shape[2:], np.uint8)
    canvas[:ch, :cw] = roi
    return oracle.warp_affine_d(canvas, M, geom.CONSTANT)[:dh, :dw]


@pytest.mark.parametrize("rect", [(6, 4, 52, 30), (0, 0, 64, 48), (17, 9, 33, 21), (3, 5, 2, 3)], ids=lambda r: "%d_%d_%dx%d" % r)
def test_crop_and_scale_of_the_interleaved_chroma_plane_is_that_of_u_and_of_v(oracle, rect):
    info = [1, 4, rect[0], rect[1], rect[2], rect[3], 0, 1]
    _, (x, y, cw, ch, dw, dh, Mu) = geom.zoom_jobs(info)
    uv8 = _nv12(21)[H:].reshape(H // 2, W // 2, 2)
    roi = np.ascontiguousarray(uv8[y:y + ch, x:x + cw])
    both = _oracle_sized(oracle, roi, Mu, (dw, dh))
    assert np.array_equal(both, geom.warp(roi, Mu, (dw, dh), geom.CONSTANT, geom.HALF_UP))      # (the canvas form is the sized warp)
    for c in range(2):
        assert np.array_equal(both[:, :, c], _oracle_sized(oracle, np.ascontiguousarray(roi[:, :, c]), Mu, (dw, dh))), c
    uv16 = _surface16(22)[H:].reshape(H // 2, W // 2, 2)
    roi = uv16[y:y + ch, x:x + cw]
    both = geom.warp(roi, Mu, (dw, dh), geom.CONSTANT)
    for c in range(2):
        assert np.array_equal(both[:, :, c], geom.warp(roi[:, :, c], Mu, (dw, dh), geom.CONSTANT)), c


def test_planar_helpers_round_trip():
    """What the GPU tests build their surfaces with: NV12 <-> I420 and P010 <-> I010 / I012 keep every sample, padded layouts included."""
    nv = _nv12(31)
    assert np.array_equal(synth.i420_to_nv12(synth.nv12_to_i420(nv), W, H), nv)
    lay = dict(pitch=96, c_pitch=64, u_off=96 * (H + 2), v_off=96 * (H + 2) + 64 * (H // 2 + 1))
    assert np.array_equal(synth.i420_to_nv12(synth.nv12_to_i420(nv, **lay), W, H, **lay), nv)
    p = _surface16(32)
    for bits in (10, 12):
        i = synth.p010_to_i010(p, W, H, bits)
        assert i.max() < (1 << bits) and np.array_equal(synth.i010_to_p010(i, W, H, bits), p >> (16 - bits) << (16 - bits))
    for name in ("planar_planes", "planar_from_planes"):
        assert callable(getattr(synth, name))
    y, u, v = synth.planar_planes(synth.nv12_to_i420(nv), W, H)
    assert np.array_equal(y, nv[:H]) and np.array_equal(u, nv[H:, 0::2]) and np.array_equal(v, nv[H:, 1::2])
    assert np.array_equal(synth.planar_planes(synth.planar_from_planes(y, u, v, **lay), W, H, **lay)[2], v)
