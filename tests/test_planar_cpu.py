"""Planar 4:2:2 / 4:4:4 (I422, I444, I210, I212, I410, I412) without a device: the definitions the GPU tests' references rest on,
pinned on the oracle and on tests/ref16.py alone, the clip helpers, and the public surface.

The warp treats planes independently: Y under M, U and V under Mc = S^-1 M S.  For 4:4:4 that is the three-channel warp of the
interleaved picture; for 4:2:2 Mc is a sheared matrix, for which ref16 - the 16-bit reference - is tied to the 8-bit oracle here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planar_inputs as pi
import ref16
from p010_inputs import MATS, NON_INTEGER
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [(n,) + pi.FORMATS[n] for n in pi.FORMATS]


# ---- 1. I444 is a three-channel warp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATS))
def test_i444_is_the_three_channel_warp(oracle, name):
    h, w = 34, 131
    img = np.random.default_rng(7).integers(0, 256, (h, w, 3), np.uint8)
    want = oracle.warp_affine(img, MATS[name])
    got = np.stack([oracle.warp_affine(np.ascontiguousarray(img[:, :, c]), MATS[name]) for c in range(3)], axis=2)
    assert np.array_equal(got, want)
    # ... which is what the reference of the GPU tests computes for a packed I444 frame
    frame = synth.yuv_pack(img[:, :, 0], img[:, :, 1], img[:, :, 2], 0, 0)
    y, u, v = pi.planes(pi.warp_frame(oracle, frame, "I444", w, h, MATS[name]), "I444", w, h)
    assert np.array_equal(np.stack([y, u, v], axis=2), want)


# ---- 2. ref16 holds for the sheared chroma matrix of 4:2:2 -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pi.ALL_MATS))
@pytest.mark.parametrize("size", [(65, 66), (1, 1)], ids=["65x66", "1x1"])
def test_ref16_equals_the_oracle_for_the_sheared_matrix(oracle, name, size):
    h, w = size
    Mc = pi.chroma_matrix(pi.ALL_MATS[name], 1, 0)
    plane = np.random.default_rng(h * w + 3).integers(0, 256, (h, w), np.uint8)
    assert np.array_equal(ref16.warp_affine(plane, Mc, ref16.HALF_UP), oracle.warp_affine(plane, Mc)), name


def test_chroma_matrix_is_the_conjugation_by_the_subsampling():
    for name, M in pi.ALL_MATS.items():
        m = np.asarray(M, np.float32)
        assert np.array_equal(pi.chroma_matrix(M, 1, 1), ref16.chroma_matrix(M)), name                # 4:2:0: what the suite has used so far
        assert np.array_equal(pi.chroma_matrix(M, 0, 0), m), name
        c = pi.chroma_matrix(M, 1, 0)
        # S^-1 M S in double, S = diag(2, 1): the float products are exact, so it is the same matrix
        S, Si = np.diag([2.0, 1.0, 1.0]), np.diag([0.5, 1.0, 1.0])
        full = Si @ np.vstack([m.astype(np.float64).reshape(2, 3), [0, 0, 1]]) @ S
        assert np.array_equal(c.astype(np.float64).reshape(2, 3), full[:2]), name


# ---- 3. closed form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tx,ty", [(6, 3), (-4, 5), (0, -2), (8, 0)])
def test_translation_shifts_the_422_chroma_planes_by_half_tx_and_ty(oracle, tx, ty):
    w, h = 66, 33
    for name in ("I422", "I210"):
        frame = pi.random_frame(11, name, w, h)
        out = pi.warp_frame(oracle, frame, name, w, h, [1, 0, tx, 0, 1, ty])
        for p, q, (dx, dy) in zip(pi.planes(frame, name, w, h), pi.planes(out, name, w, h), ((tx, ty), (tx // 2, ty), (tx // 2, ty))):
            want = np.zeros_like(p)
            ph, pw = p.shape
            ys, xs = slice(max(dy, 0), min(ph, ph + dy)), slice(max(dx, 0), min(pw, pw + dx))
            want[ys, xs] = p[max(-dy, 0):max(-dy, 0) + (ys.stop - ys.start), max(-dx, 0):max(-dx, 0) + (xs.stop - xs.start)]
            assert np.array_equal(q, want), (name, dx, dy)


# ---- 4. the 16-bit inputs of the GPU tests hold rounding ties --------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("I210", (258, 33)), ("I212", (130, 67)), ("I410", (258, 34)), ("I412", (131, 67))])
def test_gpu_inputs_can_tell_half_even_from_half_up(name, size):
    """The frames test_gpu_planar.py warps (random_frame(w, ...)): ties in a chroma plane under the chroma matrix, for the matrix
    classes with fractions - otherwise half-even would be untested."""
    w, h = size
    _, sx, sy, _ = pi.FORMATS[name]
    _, u, v = pi.planes(pi.random_frame(w, name, w, h), name, w, h)
    found = {}
    for m in NON_INTEGER + tuple(pi.STAGING):
        Mc = pi.chroma_matrix(pi.ALL_MATS[m], sx, sy)
        found[m] = int(ref16.tie_mask(u, Mc).sum()) + int(ref16.tie_mask(v, Mc).sum())
    print(name, found)
    assert all(found[m] >= 1 for m in NON_INTEGER), found
    # and there the two roundings do differ
    Mc = pi.chroma_matrix(MATS["small_rot"], sx, sy)
    assert not np.array_equal(ref16.warp_affine(u, Mc), ref16.warp_affine(u, Mc, ref16.HALF_UP))


# ---- the clip helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,sx,sy,bits", NEW, ids=[n[0] for n in NEW])
def test_clip_helpers(name, fmt, sx, sy, bits):
    w, h = 34, 19 if sy == 0 else 18
    full = synth.make_clip(synth.SEED_CONFIG1 + 5, w, h + (h & 1), 1)[0]
    bgr = np.ascontiguousarray(full[:h])
    f = synth.bgr_to_planar(bgr, sx, sy, bits, seed=3)
    assert f.shape == (capi.fmt_frame_rows(fmt, h), w) and f.dtype == capi.fmt_dtype(fmt) and capi.fmt_picture_rows(fmt, f.shape[0]) == h
    y, u, v = synth.yuv_unpack(f, w, h, sx, sy)
    assert u.shape == v.shape == (h >> sy, w >> sx) and int(f.max()) < (1 << bits)
    assert np.array_equal(pi.analysis_byte(y, bits), synth.bgr_to_nv12(full)[:h])          # the analysis sees the NV12 stream's luma bytes
    assert u.std() > 1 and v.std() > 1 and not np.array_equal(u, v)                       # real chroma, not constant planes
    assert capi.FMT_CHROMA_SHIFTS[fmt] == (sx, sy) and capi.FMT_PLANAR_BITS[fmt] == bits
    # layouts: padded pitches, V before U, planes apart - the canaries stay
    sb = f.dtype.itemsize
    cw, ch = (w >> sx) * sb, h >> sy
    for kw in (dict(pitch=sb * w + 12), dict(pitch=sb * w + 12, c_pitch=cw + 6), dict(pitch=96, c_pitch=80, u_off=96 * h + 80 * (ch + 2), v_off=96 * h, size=96 * h + 80 * (2 * ch + 3))):
        L = pi.Layout(name, w, h, **kw)
        buf = L.pack(f)
        assert buf.size * sb == L.size and np.count_nonzero(buf == L.canary) >= buf.size - f.size
        assert np.array_equal(L.unpack(buf), f)
        off = L.u_off // sb
        assert np.array_equal(buf[off:off + (w >> sx)], u[0])
    with pytest.raises(AssertionError):
        L = pi.Layout(name, w, h, pitch=sb * w + 12)
        bad = L.pack(f)
        bad[w + 1] ^= 1
        L.unpack(bad)


def test_the_420_case_of_the_helpers_is_the_i420_helpers():
    w, h = 34, 18
    bgr = synth.make_clip(synth.SEED_CONFIG1 + 6, w, h, 1)[0]
    assert np.array_equal(synth.bgr_to_planar(bgr, 1, 1), synth.nv12_to_i420(synth.bgr_to_nv12(bgr)))
    assert synth.yuv_layout(w, h, 1, 1, 1, 40, None, None, None) == synth.i420_layout(w, h, 40)


# ---- 5. the public surface -------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vs_stab.h")).read()


def test_enum_values_in_the_header_and_the_binding():
    body = re.search(r"typedef enum vs_pixfmt_planar4xx \{(.*?)\} vs_pixfmt_planar4xx;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert {k: int(v) for k, v in re.findall(r"(VS_\w+)\s*=\s*(\d+)", body)} == {
        "VS_FMT_I422": 10, "VS_FMT_I444": 11, "VS_FMT_I210": 12, "VS_FMT_I212": 13, "VS_FMT_I410": 14, "VS_FMT_I412": 15}
    assert (capi.FMT_I422, capi.FMT_I444, capi.FMT_I210, capi.FMT_I212, capi.FMT_I410, capi.FMT_I412) == (10, 11, 12, 13, 14, 15)
    assert re.search(r"#define VS_STAB_ABI_VERSION 2\b", _header())


def test_operator_is_declared_and_exported(vs):
    assert re.search(r"\bint\s+vs_op_warp_affine_planar\s*\(\s*int\s+fmt\s*,", _header())
    assert hasattr(vs.lib, "vs_op_warp_affine_planar")
    assert vs.lib.vs_abi_version() == 2


def test_header_states_the_definitions():
    h = _header()
    for text in ("yuv422p10le", "yuv444p", "Mc = S^-1 M S", "m3 * 2.0f", "min(sample >> (bits - 8), 255)", "half to even"):
        assert text in h, text


@pytest.mark.parametrize("name,fmt,sx,sy,bits", NEW, ids=[n[0] for n in NEW])
def test_no_device_is_reported_as_such(vs, name, fmt, sx, sy, bits):
    """Without a device every entry point that takes the format answers VS_ERR_NO_DEVICE (2) - never "bad geometry/format" (1), which
    is what an unknown format value would get.  A push itself cannot be reached here: vs_stab_push needs an instance, and
    vs_stab_create is the call that reports the missing device (for any format), so there is nothing to push into; what this test
    can see of a format without a device is the operators.  That prepare() takes the six values is shown on a device, where
    tests/test_gpu_planar.py::test_refusals pushes a frame of every format and gets VS_OK."""
    M = np.asarray(MATS["identity"], np.float32)
    sb = 1 if bits == 8 else 2
    buf = np.zeros(4096, np.uint8)
    args = (8 * sb, 0, 0, 0, buf.ctypes.data + 2048, 8 * sb, 0, 0, 0, 4, 4, capi._p(M, capi.f32p), 1, 1024, 1024, 0, None)
    if vs.lib.vs_device_count() > 0:
        assert vs.lib.vs_op_warp_affine_planar(fmt, None, *args) == 1                 # VS_ERR_INVALID_ARG: a null surface
        assert vs.lib.vs_op_warp_affine_planar(16, buf.ctypes.data, *args) == 1       # ... and a value that is no planar format
        return                                                                        # (the GPU tests cover the calls on a device)
    assert vs.lib.vs_op_warp_affine_planar(fmt, buf.ctypes.data, *args) == 2
    assert b"no CPU fallback" in vs.lib.vs_last_error()
    if bits != 8:
        assert vs.lib.vs_op_resize_gray(buf.ctypes.data, 16, 8, 8, fmt, buf.ctypes.data + 2048, 4, 4, 4, None) == 2
    with pytest.raises(capi.VsError):
        vs.warp_affine_planar(fmt, np.zeros((capi.fmt_frame_rows(fmt, 4), 4), capi.fmt_dtype(fmt)), 4, 4, MATS["identity"])
    h = C.c_void_p()
    p = vs.params()
    assert vs.lib.vs_stab_create(C.byref(p), 0, C.byref(h)) == 2                      # no instance to push a frame into: VS_ERR_NO_DEVICE
    s = capi.Stabilizer.__new__(capi.Stabilizer)
    assert s._geom(np.zeros((capi.fmt_frame_rows(fmt, 24), 32), capi.fmt_dtype(fmt)), fmt) == (32, 24, sb)
    s.close = lambda: None
