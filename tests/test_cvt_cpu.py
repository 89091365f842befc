"""The colour conversion without a GPU: the numpy statement (tests/cvtref.py) against the known answers and the properties the
exhaustive GPU test leans on, the declarations, and every refusal of vs_op_cvt_yuv_to_rgb / vs_op_cvt_rgb_to_yuv - all of them are
decided before a device is looked for, so the fake pointers below are never read."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cvtref
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_op_cvt_yuv_to_rgb", "vs_op_cvt_rgb_to_yuv", "vs_enh_apply_yuv_dev")
YUV = [capi.PIXFMT_BY_NAME[n] for n in cvtref.YUV_FORMATS]
RGB = [capi.PIXFMT_BY_NAME[n] for n in cvtref.RGB_FORMATS]
INT32 = (-(1 << 31), (1 << 31) - 1)


@pytest.fixture(scope="module")
def sweep():
    """Every (a, b, c) triple once, as flat int64 arrays (shared, read-only)."""
    planes = tuple(p.reshape(-1).astype(np.int64) for p in cvtref.all_triples())
    for p in planes:
        p.setflags(write=False)
    return planes


def test_known_answers():
    def bgr_to_yuv(b, g, r):
        return tuple(int(c) for c in cvtref.rgb_to_yuv_px(r, g, b))

    def yuv_to_bgr(y, u, v):
        r, g, b = cvtref.yuv_to_rgb_px(y, u, v)
        return int(b), int(g), int(r)
    assert bgr_to_yuv(0, 0, 255) == (82, 90, 240)
    assert bgr_to_yuv(255, 0, 0) == (41, 240, 110)
    assert bgr_to_yuv(255, 255, 255) == (235, 128, 128)
    assert yuv_to_bgr(16, 128, 128) == (0, 0, 0)
    assert yuv_to_bgr(235, 128, 128) == (255, 255, 255)


def test_yuv_to_rgb_saturates_on_both_sides_and_stays_in_int32(sweep):
    """The exhaustive GPU test cannot pass with a missing clamp: the sweep leaves 0 .. 255 on both sides, by millions of triples."""
    y, u, v = sweep
    r, g, b = cvtref.yuv_to_rgb_unclamped(y, u, v)
    for c in (r, g, b):
        assert int((c < 0).sum()) > 0 and int((c > 255).sum()) > 0
    assert 4.1e6 < int((b < 0).sum()) < 4.3e6 and 4.2e6 < int((b > 255).sum()) < 4.4e6
    # the sums before the shift, and their largest terms, in 32 bits
    yp = np.maximum(0, y - 16) * 1220542
    for t in (yp + cvtref.H + 1673527 * (v - 128), yp + cvtref.H - 852492 * (v - 128), yp + cvtref.H - 852492 * (v - 128) - 409993 * (u - 128),
              yp + cvtref.H + 2116026 * (u - 128)):
        assert INT32[0] <= int(t.min()) and int(t.max()) <= INT32[1]


def test_rgb_to_yuv_never_saturates(sweep):
    r, g, b = sweep
    y, u, v = cvtref.rgb_to_yuv_unclamped(r, g, b)
    assert (int(y.min()), int(y.max())) == (16, 235)
    assert (int(u.min()), int(u.max())) == (16, 240) and (int(v.min()), int(v.max())) == (16, 240)
    assert 460324 * 255 + 385875 * 255 + cvtref.H + (128 << 20) <= INT32[1]


def test_sample_rules_round_trip_the_byte():
    b = np.arange(256)
    for name, (kind, sb, bits, _, _) in cvtref.YUV_FORMATS.items():
        s = cvtref.byte_to_sample(name, b)
        assert s.dtype == (np.uint16 if sb == 2 else np.uint8)
        assert np.array_equal(cvtref.sample_to_byte(name, s), b), name
        if sb == 2:
            assert int(s.max()) == 255 << (8 if kind == "uv" else bits - 8)
    # live low bits do not change the byte; high bits beyond the format's range clamp to 255
    assert np.array_equal(cvtref.sample_to_byte("P010", (b << 8) | 0xC0), b)
    assert np.array_equal(cvtref.sample_to_byte("I010", (b << 2) | 3), b)
    assert np.array_equal(cvtref.sample_to_byte("I012", (b << 4) | 15), b)
    assert int(cvtref.sample_to_byte("I010", 0x0400)) == 255 and int(cvtref.sample_to_byte("I012", 0xFFFF)) == 255


def test_the_statements_format_table_is_the_librarys():
    for name, (kind, sb, bits, sx, sy) in cvtref.YUV_FORMATS.items():
        f = capi.PIXFMT_BY_NAME[name]
        assert (f.kind, f.sample_bytes, f.bits, f.sx, f.sy) == (capi.KIND_LUMA_UV if kind == "uv" else capi.KIND_THREE_PLANES, sb, bits, sx, sy)
    assert sorted(cvtref.YUV_FORMATS) == sorted(f.name for f in capi.PIXFMTS if f.kind != capi.KIND_INTERLEAVED)
    for name, (cn, _, _) in cvtref.RGB_FORMATS.items():
        assert capi.PIXFMT_BY_NAME[name].cn == cn


def test_declared_exported_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(vs.lib, n) and getattr(vs.lib, n).argtypes, n
    comment = header[:header.index("#define VS_STAB_ABI_VERSION")]
    assert all(n in comment for n in NAMES)
    assert vs.lib.vs_abi_version() == 2
    assert callable(vs.cvt_yuv_to_rgb) and callable(vs.cvt_rgb_to_yuv) and callable(capi.Enhancer.apply_yuv_dev)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
P, Q = 0x100000, 0x200000        # never read


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def call(vs, direction, f, r, w=8, h=4, lay=None, rgb_stride=None, n=1, surfaces=True, rgb=True, layout_ptr=True, sp=None, rp=None):
    """One call of either operator with fake pointers; the defaults are valid for every format."""
    lay = capi.I420LayoutC(*(lay or (f.sample_bytes * w, 0, 0, 0)))
    s = ptrs(*(sp or [P + 0x1000 * k for k in range(max(n, 1))])) if surfaces else None
    d = ptrs(*(rp or [Q + 0x1000 * k for k in range(max(n, 1))])) if rgb else None
    stride = w * r.cn if rgb_stride is None else rgb_stride
    lp = C.byref(lay) if layout_ptr else None
    if direction == 0:
        return vs.lib.vs_op_cvt_yuv_to_rgb(f.fmt, s, lp, r.fmt, d, stride, n, w, h, None)
    return vs.lib.vs_op_cvt_rgb_to_yuv(r.fmt, d, stride, f.fmt, s, lp, n, w, h, None)


def refused(vs, direction, f, r, **kw):
    rc = call(vs, direction, f, r, **kw)
    text = vs.lib.vs_last_error().decode()
    return rc == 1 and text.startswith("vs_op_cvt_yuv_to_rgb" if direction == 0 else "vs_op_cvt_rgb_to_yuv") and (f.name in text or r.name in text)


@pytest.mark.parametrize("direction", [0, 1])
def test_refusals_need_no_device(vs, direction):
    bgr = capi.PIXFMT_BY_NAME["BGR8"]
    for f in YUV:
        sb, w, h = f.sample_bytes, 8, 4
        for r in RGB:
            if vs.lib.vs_device_count() <= 0:
                assert call(vs, direction, f, r) == 2, (f.name, r.name)
                assert call(vs, direction, f, r, n=32) == 2
            assert refused(vs, direction, f, r, rgb_stride=w * r.cn - 1)
        r = bgr
        # null pointers: the lists, an entry of either, the layout
        assert refused(vs, direction, f, r, surfaces=False) and refused(vs, direction, f, r, rgb=False) and refused(vs, direction, f, r, layout_ptr=False)
        assert refused(vs, direction, f, r, n=2, sp=[P, 0]) and refused(vs, direction, f, r, n=2, rp=[Q, 0])
        assert refused(vs, direction, f, r, n=0) and refused(vs, direction, f, r, n=33) and refused(vs, direction, f, r, n=-1)
        # geometry
        assert refused(vs, direction, f, r, w=0) and refused(vs, direction, f, r, h=0)
        if f.sx:
            assert refused(vs, direction, f, r, w=7)
        if f.sy:
            assert refused(vs, direction, f, r, h=3)
        assert refused(vs, direction, f, r, lay=(sb * w - sb, 0, 0, 0))
        # 16-bit samples: pointer, pitch, chroma pitch, offsets
        if sb == 2:
            assert refused(vs, direction, f, r, sp=[P + 1])
            assert refused(vs, direction, f, r, lay=(sb * w + 1, 0, 0, 0))
            assert refused(vs, direction, f, r, lay=(sb * w + 4, 0, h * (sb * w + 4) + 1, 0))
            if f.kind == capi.KIND_THREE_PLANES:
                assert refused(vs, direction, f, r, lay=(sb * w + 4, sb * w + 1, 0, 0))
                assert refused(vs, direction, f, r, lay=(sb * w + 4, sb * w, 0, 4096 + 1))
        if f.kind == capi.KIND_THREE_PLANES:
            if f.sx:      # a defaulted half chroma pitch needs whole samples in it
                assert refused(vs, direction, f, r, lay=(sb * w + sb, 0, 0, 0))
                if vs.lib.vs_device_count() <= 0:
                    assert call(vs, direction, f, r, lay=(sb * w + sb, sb * w, 0, 0)) == 2
            crow = sb * (w >> f.sx)
            assert refused(vs, direction, f, r, lay=(sb * w, crow - sb, 0, 0))
            # planes that overlap: U inside Y, V inside U, V on U
            y_bytes, c_bytes = h * sb * w, (h >> f.sy) * crow
            assert refused(vs, direction, f, r, lay=(sb * w, 0, y_bytes - 2, 0))
            assert refused(vs, direction, f, r, lay=(sb * w, 0, y_bytes, y_bytes + c_bytes - 2))
            assert refused(vs, direction, f, r, lay=(sb * w, 0, y_bytes, y_bytes))
            assert refused(vs, direction, f, r, lay=(sb * w, 0, y_bytes + c_bytes, y_bytes - 2))
            if vs.lib.vs_device_count() <= 0:       # YV12 order and planes apart are layouts like any other
                assert call(vs, direction, f, r, lay=(sb * w, 0, y_bytes + c_bytes, y_bytes)) == 2
                assert call(vs, direction, f, r, lay=(sb * w + 8, crow + 2 * sb, y_bytes + 4 * h * sb + 64, 8192)) == 2
        else:
            assert refused(vs, direction, f, r, lay=(sb * w, 0, 0, 2 * h * sb * w))          # v_off must be 0
            assert refused(vs, direction, f, r, lay=(sb * w + 4, sb * w, 0, 0))              # c_pitch 0 or the pitch
            assert refused(vs, direction, f, r, lay=(sb * w, 0, h * sb * w - 2, 0))          # the (U, V) plane inside Y
            if vs.lib.vs_device_count() <= 0:
                assert call(vs, direction, f, r, lay=(sb * w + 4, sb * w + 4, 4096, 0)) == 2
    # a format of the wrong family on either side
    for f in RGB + [capi.PIXFMT_BY_NAME["GRAY8"]]:
        assert refused(vs, direction, f, bgr)
    for r in YUV + [capi.PIXFMT_BY_NAME["GRAY8"]]:
        assert refused(vs, direction, capi.PIXFMT_BY_NAME["NV12"], r)
    nv12 = capi.PIXFMT_BY_NAME["NV12"]
    lay = capi.I420LayoutC(8, 0, 0, 0)
    for bad in (-1, 16, 99):
        if direction == 0:
            assert vs.lib.vs_op_cvt_yuv_to_rgb(bad, ptrs(P), C.byref(lay), 0, ptrs(Q), 24, 1, 8, 4, None) == 1
            assert vs.lib.vs_op_cvt_yuv_to_rgb(nv12.fmt, ptrs(P), C.byref(lay), bad, ptrs(Q), 24, 1, 8, 4, None) == 1
        else:
            assert vs.lib.vs_op_cvt_rgb_to_yuv(0, ptrs(Q), 24, bad, ptrs(P), C.byref(lay), 1, 8, 4, None) == 1
            assert vs.lib.vs_op_cvt_rgb_to_yuv(bad, ptrs(Q), 24, nv12.fmt, ptrs(P), C.byref(lay), 1, 8, 4, None) == 1
        assert "format %d" % bad in vs.lib.vs_last_error().decode()
