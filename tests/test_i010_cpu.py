"""I010 / I012 (planar 4:2:0, 16-bit samples with the value in the low bits) without a device: the equivalence the warp's
reference rests on, inputs that can tell the rounding rules apart, the clip helpers and the public surface.

The reference of the GPU tests (tests/test_gpu_i010.py) is tests/ref16.py plane by plane.  The blend treats channels
independently, so that is the P010 reference on the interleaved surface, de-interleaved - which tests/test_p010_cpu.py pins to
the 8-bit oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import i010_inputs as ii
import ref16
from p010_inputs import MATS, NON_INTEGER
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATS))
def test_three_plane_warp_is_the_two_plane_warp_of_the_interleaved_surface(name):
    w, h = 130, 34
    for full_range in (False, True):
        frame = ii.random_frame(w + full_range, w, h, 10, full_range)
        want = ref16.warp_two_planes(ii.interleaved(frame, w, h), w, h, MATS[name])
        got = ii.interleaved(ii.warp_three_planes(frame, w, h, MATS[name]), w, h)
        assert np.array_equal(got, want), (name, full_range)


def test_replicate_reference_equals_the_constant_border_inside_the_picture():
    """Where all four taps lie inside the picture the border mode cannot matter; and a picture of one value stays that value."""
    w, h = 66, 34
    y = ii.random_frame(3, w, h)[:h]
    for name in ("identity", "frac_shift", "small_rot"):
        a, b = ii.warp_plane(y, MATS[name], ii.BLACK), ii.warp_plane(y, MATS[name], ii.REPLICATE)
        sx, sy, _, _ = ref16.coords(np.asarray(MATS[name], np.float32).astype(np.float64), w, h)
        inside = (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
        assert inside.any() and np.array_equal(a[inside], b[inside]), name
    flat = np.full((h, w), 777, np.uint16)
    assert np.all(ii.warp_plane(flat, MATS["rot_zoom_beyond_box"], ii.REPLICATE) == 777)


@pytest.mark.parametrize("name", NON_INTEGER)
def test_inputs_can_tell_half_even_from_half_up(name):
    """The 258 x 66 low-aligned frame the GPU tests warp holds rounding ties in Y and in U for every class with fractions."""
    w, h = 258, 66
    y, u, _ = ii.planes(ii.random_frame(258, w, h), w, h)
    ty = int(ref16.tie_mask(y, MATS[name]).sum())
    tu = int(ref16.tie_mask(u, ref16.chroma_matrix(MATS[name])).sum())
    print("%s: %d ties in Y, %d in U" % (name, ty, tu))
    assert ty >= 1 and tu >= 1, (name, ty, tu)


def test_analysis_byte_saturates():
    s = np.array([0, 3, 4, 1023, 1024, 4095, 4096, 65535], np.uint16)
    assert ii.analysis_byte(s, 10).tolist() == [0, 0, 1, 255, 255, 255, 255, 255]
    assert ii.analysis_byte(s, 12).tolist() == [0, 0, 0, 63, 64, 255, 255, 255]


# ---- the clip helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [10, 12])
def test_packed_helpers_round_trip(bits):
    for w, h in ((2, 2), (6, 10), (34, 18), (322, 200)):
        nv12 = np.random.default_rng(w + h).integers(0, 256, (h * 3 // 2, w), np.uint8)
        p010 = synth.nv12_to_p010(nv12, seed=w)                   # (the low six bits are zero: nothing is lost at either depth)
        f = synth.p010_to_i010(p010, w, h, bits)
        assert f.shape == p010.shape and f.dtype == np.uint16 and int(f.max()) < (1 << bits)
        y, u, v = ii.planes(f, w, h)
        assert np.array_equal(y, p010[:h] >> (16 - bits))
        assert np.array_equal(u, p010[h:, 0::2] >> (16 - bits)) and np.array_equal(v, p010[h:, 1::2] >> (16 - bits))
        assert np.array_equal(synth.i010_to_p010(f, w, h, bits), p010)
        assert np.array_equal(ii.analysis_byte(y, bits), nv12[:h])                     # the analysis sees the NV12 stream's bytes
        assert np.array_equal(ii.Layout(w, h).unpack(ii.Layout(w, h).pack(f)), f)


@pytest.mark.parametrize("layout", ["padded", "chroma_pitch_not_half", "v_first", "planes_apart"])
def test_padded_helpers_round_trip_and_leave_the_fill(layout):
    w, h = 34, 18
    p010 = synth.nv12_to_p010(np.random.default_rng(5).integers(0, 255, (h * 3 // 2, w), np.uint8), seed=1)
    kw = dict(padded=dict(pitch=96), chroma_pitch_not_half=dict(pitch=96, c_pitch=38), v_first=dict(pitch=80, u_off=80 * h + 9 * 40, v_off=80 * h),
              planes_apart=dict(pitch=128, c_pitch=64, u_off=128 * 24, v_off=128 * 24 + 64 * 16, size=128 * 24 + 64 * 32))[layout]
    buf = synth.p010_to_i010(p010, w, h, fill=0xFFFF, **kw)
    lay = {k: v for k, v in kw.items() if k != "size"}
    assert buf.ndim == 1 and buf.dtype == np.uint16
    assert np.array_equal(synth.i010_to_p010(buf, w, h, **lay), p010)
    assert np.count_nonzero(buf != 0xFFFF) <= p010.size and np.count_nonzero(buf == 0xFFFF) >= buf.size - p010.size
    pitch, c_pitch, u_off, v_off = synth.i420_layout(2 * w, h, **lay)
    assert np.array_equal(buf[u_off // 2:u_off // 2 + w // 2], p010[h, 0::2] >> 6) and np.array_equal(buf[v_off // 2:v_off // 2 + w // 2], p010[h, 1::2] >> 6)
    assert np.array_equal(buf[pitch // 2:pitch // 2 + w], p010[1] >> 6)
    # the test helper describes the same bytes
    L = ii.Layout(w, h, **kw)
    assert np.array_equal(L.unpack(np.where(buf == 0xFFFF, ii.CANARY, buf)), synth.p010_to_i010(p010, w, h))


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vs_stab.h")).read()


def test_enum_values_in_the_header_and_the_binding():
    body = re.search(r"typedef enum vs_pixfmt_planar16 \{(.*?)\} vs_pixfmt_planar16;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert {k: int(v) for k, v in re.findall(r"(VS_\w+)\s*=\s*(\d+)", body)} == {"VS_FMT_I010": 8, "VS_FMT_I012": 9}
    assert (capi.FMT_I010, capi.FMT_I012) == (8, 9)
    assert re.search(r"#define VS_STAB_ABI_VERSION 2\b", _header())


def test_operator_is_declared_and_exported(vs):
    assert re.search(r"\bint\s+vs_op_warp_affine_i010\s*\(", _header())
    assert hasattr(vs.lib, "vs_op_warp_affine_i010")
    assert vs.lib.vs_abi_version() == 2


def test_header_documents_the_sample_position_and_the_saturation():
    h = _header()
    assert "yuv420p10le" in h and "yuv420p12le" in h and "min(sample >> (bits - 8), 255)" in h


@pytest.mark.parametrize("fmt", [capi.FMT_I010, capi.FMT_I012])
def test_shape_helpers(fmt):
    s = capi.Stabilizer.__new__(capi.Stabilizer)
    assert s._geom(np.zeros((36, 32), np.uint16), fmt) == (32, 24, 2)
    assert capi.fmt_dtype(fmt) == np.uint16 and capi.fmt_420(fmt) and not capi.fmt_two_planes(fmt)
    assert capi.fmt_dtype(capi.FMT_I420) == np.uint8 and capi.fmt_dtype(capi.FMT_P010) == np.uint16 and capi.fmt_dtype(capi.FMT_BGR8) == np.uint8
    s.close = lambda: None


def test_null_arguments_and_no_device(vs):
    assert vs.lib.vs_stab_set_i420_layout(None, 0, 0, 0, 0, 0, 0) == 1             # VS_ERR_INVALID_ARG
    M = np.asarray(MATS["identity"], np.float32)
    buf = np.zeros(64, np.uint16)
    args = (8, 0, 0, 0, buf.ctypes.data, 8, 0, 0, 0, 4, 4, capi._p(M, capi.f32p), 1, 48, 48, 0, None)
    if vs.lib.vs_device_count() > 0:
        assert vs.lib.vs_op_warp_affine_i010(None, *args) == 1                 # VS_ERR_INVALID_ARG
        return                                                                 # (the GPU tests cover the calls on a device)
    assert vs.lib.vs_op_warp_affine_i010(buf.ctypes.data, *args) == 2          # VS_ERR_NO_DEVICE
    assert b"no CPU fallback" in vs.lib.vs_last_error()
    with pytest.raises(capi.VsError):
        vs.warp_affine_i010(np.zeros((6, 4), np.uint16), 4, 4, MATS["identity"])
    h = C.c_void_p()
    p = vs.params()
    assert vs.lib.vs_stab_create(C.byref(p), 0, C.byref(h)) == 2               # no instance to push an I010 frame into
