"""vs_enh_apply_yuv_batch_dev on the GPU.  Two yardsticks, both independent of the fused kernels: the statement tests/enhyuvref.py
(numpy conversion, the CPU oracle's enhanceImage, numpy conversion back) and the definition on the device, vs_enh_apply_yuv_dev
surface by surface.  Every comparison is array_equal.

Sizes are the smallest at which the 64 x 32 tile kernel can still go wrong: 134 x 38 (3 x 2 tiles, ragged on both sides, halo rows
that start at an odd row), 66 x 34 (one full tile plus slivers), 34 x 6 (smaller than a tile) and the odd sizes a format allows."""
import ctypes as C

import numpy as np
import pytest

import cvtref
import enhyuvref
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

FILL = 0xA5
INVALID_ARG = 1
TABLES = dict(brightness=1.5, contrast=1.1, gamma=1.2)
SETTINGS = {
    "points": TABLES,
    "vibrance": dict(TABLES, enable_vibrance=1),
    "shipped": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0),                 # 7 taps, R = 3 (test_gpu_cvt.py)
    "narrow": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=0.4),                  # 3 taps, R = 1
    "wide": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=5.4),                    # 33 taps, R = 16
    "post": dict(TABLES, use_cuda=1, enable_unsharp=1, sharpness=1.0, blur_sigma=1.5),        # tables on both sides of an 11-tap blur
}
CLAHE_WB = dict(enable_clahe=1, clahe_tile_grid_size=2, enable_white_balance=1, wb_strength=0.7)   # test_gpu_cvt.py
FORMATS = list(cvtref.YUV_FORMATS) + ["YV12"]


def fmt_id(name):
    return capi.PIXFMT_BY_NAME["I420" if name == "YV12" else name].fmt


def fill_of(name):
    return FILL * 0x0101 if enhyuvref.fmt_of(name)[1] == 2 else FILL


def sizes(name, setting):
    _, _, _, sx, sy = enhyuvref.fmt_of(name)
    out = [(134, 38), (66, 34)] + ([] if setting == "wide" else [(34, 6)])
    if not sx:
        out.append((133, 37))
    elif not sy:
        out.append((134, 37))
    return out


@pytest.fixture(scope="module")
def picture():
    f = synth.make_clip(synth.SEED_CONFIG1, 160, 120, 1)[0]
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def enh(gpu):
    e = capi.Enhancer(gpu)
    yield e
    e.close()


def default_layout(name, w, h):
    """(layout, size) a packed surface is described with: None except for YV12, which exists through swapped offsets only."""
    if name != "YV12":
        return None, None
    return enhyuvref.yv12_layout(w, h), w * h * 3 // 2


def surfaces_of(picture, name, w, h, n, layout=None, size=None):
    """n surfaces of the format from n different crops of the picture.  16-bit samples carry live bits below the byte the conversion
    reads, and one sample in 64 of the low-bit formats lies beyond the format's range (it reads as 255)."""
    kind, sb, bits, _, _ = enhyuvref.fmt_of(name)
    out = []
    for k in range(n):
        x0, y0 = 2 + (k % 8) * 3, 30 + (k // 8) * 12
        planes = enhyuvref.unpack(name, enhyuvref.from_bgr(name, np.ascontiguousarray(picture[y0:y0 + h, x0:x0 + w])), w, h)
        if sb == 2:
            rng = np.random.default_rng(1000 + k)
            shift = cvtref.sample_shift(name)
            planes = [p | rng.integers(0, 1 << shift, p.shape, np.uint16) for p in planes]
            if kind == "3p":
                planes = [np.where(rng.integers(0, 64, p.shape) == 0, p | np.uint16(1 << bits), p).astype(np.uint16) for p in planes]
        out.append(enhyuvref.pack(name, *planes, layout, size, fill_of(name)))
    return out


def check_fused(enh, oracle, picture, name, setting, w, h, n=2):
    p = capi.Enhancer.default_params(enh.vs, **SETTINGS[setting])
    lay, size = default_layout(name, w, h)
    srcs = surfaces_of(picture, name, w, h, n, lay, size)
    assert not np.array_equal(srcs[0], srcs[1])
    single = [enh.apply_yuv_dev(p, fmt_id(name), s, w, h, layout=lay, out_size=size) for s in srcs]
    got = enh.apply_yuv_batch_dev(p, fmt_id(name), srcs, w, h, layout=lay, out_size=size)
    assert enh.last_fused() == n, (name, setting, w, h)
    assert enh.passes() == 1
    for k in range(n):
        want = enhyuvref.enhance_yuv(oracle, p, name, srcs[k], w, h, lay, lay, size, fill_of(name))
        assert not np.array_equal(want, enhyuvref.round_trip(name, srcs[k], w, h, lay, lay, size, fill_of(name)))     # the enhancer changed the picture
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (name, setting, w, h, k, "statement")
        assert np.array_equal(got[k], single[k]), (name, setting, w, h, k, "vs_enh_apply_yuv_dev")


# ---- 1. the fused launch equals both yardsticks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["points", "shipped"])
@pytest.mark.parametrize("name", FORMATS)
def test_every_format(enh, oracle, picture, name, setting):
    for w, h in sizes(name, setting)[:1] + sizes(name, setting)[3:]:
        check_fused(enh, oracle, picture, name, setting, w, h)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("name", ["NV12", "P010", "I420", "I444"])
def test_every_setting_and_size(enh, oracle, picture, name, setting):
    for w, h in sizes(name, setting):
        check_fused(enh, oracle, picture, name, setting, w, h)


# ---- 2. batch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["points", "shipped"])
@pytest.mark.parametrize("name", ["NV12", "I010", "I444"])
def test_batch_equals_single_calls(enh, picture, name, setting):
    w, h = 66, 34
    p = capi.Enhancer.default_params(enh.vs, **SETTINGS[setting])
    srcs = surfaces_of(picture, name, w, h, 32)
    single = [enh.apply_yuv_dev(p, fmt_id(name), s, w, h) for s in srcs]
    assert not np.array_equal(single[0], single[1]) and not np.array_equal(single[0], single[31])
    for n in (1, 3, 32):
        got = enh.apply_yuv_batch_dev(p, fmt_id(name), srcs[:n], w, h)
        assert enh.last_fused() == n
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, single)), (name, setting, n)


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------
def raw_call(enh, p, fmt, srcs, lin, lout, out_size, w, h, n=None, src_off=0, dst_off=0, null_src=None, null_dst=None):
    """One call on flat source buffers, each src_off bytes behind its allocation's start, into destinations of out_size bytes dst_off
    bytes behind theirs.  -> (status, text of vs_enh_last_error, [every destination allocation whole: dst_off + out_size + 16 bytes])"""
    vs = enh.vs
    d_in = [capi.DevBuf.from_array(vs, np.concatenate([np.full(src_off, FILL, np.uint8), np.ascontiguousarray(s).reshape(-1).view(np.uint8)])) for s in srcs]
    d_out = [capi.DevBuf.from_array(vs, np.full(dst_off + out_size + 16, FILL, np.uint8)) for _ in srcs]
    a = (C.c_void_p * len(srcs))(*[None if k == null_src else d.ptr + src_off for k, d in enumerate(d_in)])
    b = (C.c_void_p * len(srcs))(*[None if k == null_dst else d.ptr + dst_off for k, d in enumerate(d_out)])
    try:
        rc = enh.lib.vs_enh_apply_yuv_batch_dev(enh.h, C.byref(p), fmt, a, C.byref(capi.I420LayoutC(*lin)), b, C.byref(capi.I420LayoutC(*lout)),
                                                len(srcs) if n is None else n, w, h)
        text = (enh.lib.vs_enh_last_error(enh.h) or b"").decode()
        enh.sync()
        outs = [d.download((dst_off + out_size + 16,), np.uint8) for d in d_out]
    finally:
        for d in d_in + d_out:
            d.free()
    return rc, text, outs


def layouts(name, w, h):
    """[(label, layout, size, offset of the surface behind the allocation's start)]: bytes, resolved by hand."""
    kind, sb, bits, sx, sy = enhyuvref.fmt_of(name)
    row, crow, ch = sb * w, sb * (w >> sx), h >> sy
    if kind == "uv":
        pitch = row + 12
        out = [("packed", (row, 0, 0, 0), h * row * 3 // 2, 0),
               ("padded pitch", (pitch, 0, 0, 0), h * pitch * 3 // 2, 0),
               ("plane apart", (pitch, pitch, h * pitch + 40, 0), h * pitch + 40 + h // 2 * pitch, 0)]
        if sb == 1:
            odd = row + 13
            out.append(("odd pitch, odd address", (odd, 0, h * odd + 3, 0), h * odd + 3 + h // 2 * odd, 1))
        return out
    pitch, cp = row + 12, crow + 6
    out = [("packed", (row, 0, 0, 0), h * row + 2 * ch * crow, 0),
           ("padded pitch, chroma pitch of its own", (pitch, cp, 0, 0), h * pitch + 2 * ch * cp, 0),
           ("planes apart", (pitch, cp, h * pitch + 40, h * pitch + 40 + ch * cp + 24), h * pitch + 64 + 2 * ch * cp, 0),
           ("V before U, apart", (pitch, cp, h * pitch + 16 + ch * cp + 8, h * pitch + 16), h * pitch + 24 + 2 * ch * cp, 0)]
    if sb == 1:
        odd, ocp = row + 13, crow + 7
        out.append(("odd pitches, odd address", (odd, ocp, h * odd + 5, h * odd + 5 + ch * ocp + 2), h * odd + 7 + 2 * ch * ocp, 1))
    return out


@pytest.mark.parametrize("setting", ["points", "shipped"])
@pytest.mark.parametrize("name", ["NV12", "I420", "I210"])
def test_layouts(enh, oracle, picture, name, setting):
    w, h, n = 66, 34, 2
    p = capi.Enhancer.default_params(enh.vs, **SETTINGS[setting])
    lays = layouts(name, w, h)
    packed = surfaces_of(picture, name, w, h, n)
    want_packed = [enhyuvref.enhance_yuv(oracle, p, name, s, w, h) for s in packed]
    # every layout on the way in and on the way out, and the one behind it in the list as the output layout of a different kind
    for i, (label, lin, in_size, in_off) in enumerate(lays):
        for label_out, lout, out_size, out_off in (lays[i], lays[(i + 1) % len(lays)]):
            srcs = [enhyuvref.pack(name, *enhyuvref.unpack(name, s, w, h), lin, in_size, fill_of(name)) for s in packed]
            rc, text, outs = raw_call(enh, p, fmt_id(name), srcs, lin, lout, out_size, w, h, src_off=in_off, dst_off=out_off)
            assert rc == 0, text
            assert enh.last_fused() == n
            for k in range(n):
                surface = enhyuvref.pack(name, *enhyuvref.unpack(name, want_packed[k], w, h), lout, out_size + 16, fill_of(name))
                want = np.concatenate([np.full(out_off, FILL, np.uint8), surface.view(np.uint8)])
                assert np.array_equal(outs[k], want), (name, setting, label, label_out, k)


# ---- 4. in place -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "I010", "I422", "I444"])
def test_in_place(enh, picture, name):
    n = 3
    for w, h in sizes(name, "shipped"):
        srcs = surfaces_of(picture, name, w, h, n)
        for setting, fused in (("points", n), ("vibrance", n), ("shipped", 0)):
            p = capi.Enhancer.default_params(enh.vs, **SETTINGS[setting])
            want = enh.apply_yuv_batch_dev(p, fmt_id(name), srcs, w, h, raw=True)
            assert enh.last_fused() == n
            got = enh.apply_yuv_batch_dev(p, fmt_id(name), srcs, w, h, in_place=True, raw=True)
            assert enh.last_fused() == fused, (name, setting)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, setting, w, h)


# ---- 5. fallback -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "I420", "P010", "I422"])
def test_per_frame_statistics_take_the_three_calls(enh, picture, name):
    w, h, n = 134, 38, 3
    p = capi.Enhancer.default_params(enh.vs, **CLAHE_WB)
    assert enh.vs.enh_yuv_plan(p, fmt_id(name)) == 0
    srcs = surfaces_of(picture, name, w, h, n)
    single = [enh.apply_yuv_dev(p, fmt_id(name), s, w, h) for s in srcs]
    assert not np.array_equal(single[0], single[1])
    got = enh.apply_yuv_batch_dev(p, fmt_id(name), srcs, w, h)
    assert enh.last_fused() == 0
    assert all(np.array_equal(a, b) for a, b in zip(got, single))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "P010", "I420", "I210"])
def test_refusals_write_nothing(enh, picture, name):
    kind, sb, bits, sx, sy = enhyuvref.fmt_of(name)
    w, h = 34, 6
    p = capi.Enhancer.default_params(enh.vs, **SETTINGS["points"])
    srcs = surfaces_of(picture, name, w, h, 2)
    lay = (sb * w, 0, 0, 0)
    size = srcs[0].nbytes

    def refused(fmt=fmt_id(name), named=name, **kw):
        args = dict(lin=lay, lout=lay, out_size=size, w=w, h=h)
        args.update(kw)
        rc, text, outs = raw_call(enh, p, fmt, srcs, **args)
        return rc == INVALID_ARG and text.startswith("vs_enh_apply_yuv_batch_dev") and named in text and all((o == FILL).all() for o in outs) \
            and enh.last_fused() == 0

    assert raw_call(enh, p, fmt_id(name), srcs, lay, lay, size, w, h)[0] == 0 and enh.last_fused() == 2      # the call these are variations of
    assert refused(n=0) and refused(n=33)
    assert refused(w=w - 1)                                                                                  # an odd w (all four: sx = 1)
    assert refused(lin=(sb * w - sb, 0, 0, 0)) and refused(lout=(sb * w - sb, 0, 0, 0))                      # a pitch below a row
    if sb == 2:
        assert refused(src_off=1) and refused(dst_off=1)                                                     # an odd pointer
    assert refused(null_src=1) and refused(null_dst=0)
    assert refused(fmt=capi.PIXFMT_BY_NAME["BGR8"].fmt, named="BGR8")
    # ... and what the stage list refuses, with the code the single call gives, before anything is queued
    bad = capi.Enhancer.default_params(enh.vs, enable_clahe=1, clahe_tile_grid_size=17)
    rc, text, outs = raw_call(enh, bad, fmt_id(name), srcs, lay, lay, size, w, h)
    assert rc == 4 and text.startswith("vs_enh_apply_yuv_batch_dev") and name in text and all((o == FILL).all() for o in outs)
