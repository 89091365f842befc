"""vs_op_cvt_yuv_to_rgb_cs, vs_op_cvt_rgb_to_yuv_cs and the enhancer's YUV calls under vs_enh_set_yuv_colorimetry on the GPU, held to
the numpy statement tests/cvtref_cs.py.  Every comparison is array_equal.  Destinations are prefilled with 0xA5 and compared whole -
row padding, the gaps between planes and 16 guard bytes behind the last plane included - wherever the raw buffer is asked for.

Shapes: 70 x 6 - a lane covers 8 pixels, so one ragged lane sits beside eight whole ones; for the subsampled formats also 2 x 2 (one
block) and 518 x 4 (more than one workgroup across: 512 pixels each).  The enhancer: 70 x 6 and 134 x 10 (3 tiles of 64 across)."""
import numpy as np
import pytest

import cvtref
import cvtref_cs as cs
import enhyuvref
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

YUV = list(cvtref.YUV_FORMATS)
FILL = 0xA5
BT709_LIMITED_MEAN = (cs.BT709, cs.LIMITED, cs.MEAN)
BT2020_FULL_TOPLEFT = (cs.BT2020, cs.FULL, cs.TOPLEFT)
BT601_FULL_TOPLEFT = (cs.BT601, cs.FULL, cs.TOPLEFT)


def combo_id(c):
    return "%s-%s" % (cs.MATRIX_NAMES[c[0]], cs.RANGE_NAMES[c[1]])


def fmt(name):
    return capi.PIXFMT_BY_NAME[name]


def fill_of(name):
    return FILL * 0x0101 if cvtref.YUV_FORMATS[name][1] == 2 else FILL


def random_planes(name, w, h, seed):
    """Sample planes (Y, U, V) of the format's dtype.  8-bit: random bytes.  P010: every low bit live.  The low-bit formats: one sample
    in eight has bits above the format's range (the conversion reads it as 255)."""
    kind, sb, bits, sx, sy = cvtref.YUV_FORMATS[name]
    rng = np.random.default_rng(seed)
    out = []
    for ph, pw in ((h, w), (h >> sy, w >> sx), (h >> sy, w >> sx)):
        if sb == 1:
            out.append(rng.integers(0, 256, (ph, pw), np.uint8))
        elif kind == "uv":
            out.append(rng.integers(0, 1 << 16, (ph, pw), np.uint16))
        else:
            s = rng.integers(0, 1 << bits, (ph, pw), np.uint16)
            high = rng.integers(1, 1 << (16 - bits), (ph, pw), np.uint16) << bits
            out.append(np.where(rng.integers(0, 8, (ph, pw)) == 0, s | high, s).astype(np.uint16))
    return out


def random_frame(w, h, cn, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, cn), np.uint8)


def want_rgb(name, planes, rgb, desc):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    return cs.yuv_to_rgb(*(cvtref.sample_to_byte(name, p) for p in planes), sx, sy, rgb, desc[0], desc[1])


def want_surface(name, frame, rgb, desc, layout=None, size=None, fill=0):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    planes = cs.rgb_to_yuv(frame, sx, sy, rgb, *desc)
    return enhyuvref.pack(name, *(cvtref.byte_to_sample(name, p) for p in planes), layout, size, fill)


def up16(v):
    return (v + 15) & ~15


def layouts(name, w, h):
    """[(label, (pitch, c_pitch, u_off, v_off), size, rgb row padding)]: bytes, resolved by hand.  "aligned": every row and plane
    starts at a multiple of 16, so whole runs move as dwords; "odd": pitches and plane offsets that no run is aligned at beyond what
    the samples need (16-bit samples: even, never a multiple of 4 apart from chance), so runs go sample by sample; both with gaps."""
    kind, sb, bits, sx, sy = cvtref.YUV_FORMATS[name]
    row, crow, ch = sb * w, sb * (w >> sx), h >> sy
    if kind == "uv":
        a, o = up16(row), row + (13 if sb == 1 else 2)
        return [("aligned", (a, 0, h * a + 32, 0), h * a + 32 + ch * a, 0),
                ("odd", (o, 0, h * o + (3 if sb == 1 else 6), 0), h * o + (3 if sb == 1 else 6) + ch * o, 5)]
    a, ca = up16(row), up16(crow)
    o, co = row + (13 if sb == 1 else 2), crow + (7 if sb == 1 else 2)
    ou = h * o + (5 if sb == 1 else 6)
    return [("aligned", (a, ca, h * a + 32, h * a + 32 + ch * ca + 16), h * a + 48 + 2 * ch * ca, 0),
            ("odd", (o, co, ou, ou + ch * co + 2), ou + 2 + 2 * ch * co, 5)]


# ---- exhaustive values, per new combination ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triples():
    planes = cvtref.all_triples()
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.mark.parametrize("combo", cs.NEW_COMBINATIONS, ids=combo_id)
def test_every_yuv_triple_to_bgr8(gpu, triples, combo):
    got = gpu.cvt_yuv_to_rgb(fmt("I444").fmt, synth.yuv_pack(*triples, 0, 0), 4096, 4096, fmt("BGR8").fmt, colorimetry=combo)
    r, g, b = cs.yuv_to_rgb_px(*triples, *combo)
    assert np.array_equal(got[:, :, 0], b) and np.array_equal(got[:, :, 1], g) and np.array_equal(got[:, :, 2], r)


@pytest.mark.parametrize("combo", cs.NEW_COMBINATIONS, ids=combo_id)
def test_every_bgr_triple_to_i444(gpu, triples, combo):
    b, g, r = triples
    got = gpu.cvt_rgb_to_yuv(np.dstack([b, g, r]), fmt("I444").fmt, fmt("BGR8").fmt, colorimetry=combo)
    y, u, v = cs.rgb_to_yuv_px(r, g, b, *combo)
    gy, gu, gv = synth.yuv_unpack(got, 4096, 4096, 0, 0)
    assert np.array_equal(gy, y) and np.array_equal(gu, u) and np.array_equal(gv, v)


# ---- the default is what it was ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "P010", "I422"])
def test_default_preserved(gpu, name):
    w, h = 70, 6
    planes = random_planes(name, w, h, 61)
    surface = enhyuvref.pack(name, *planes)
    frame = random_frame(w, h, 3, 62)
    old_rgb = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, raw=True)
    old_yuv = gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, raw=True)
    # ... which is the statement of the parent, so "today's output" is pinned by more than the old entry point's word
    assert np.array_equal(old_rgb[:h * w * 3].reshape(h, w, 3), cvtref.yuv_to_rgb(*(cvtref.sample_to_byte(name, p) for p in planes),
                                                                                  *cvtref.YUV_FORMATS[name][3:], "BGR8"))
    for kw in (dict(use_cs=True), dict(colorimetry=(0, 0, 0, 0)), dict(colorimetry=capi.CvtColorimetry())):
        assert np.array_equal(gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, raw=True, **kw), old_rgb), (name, kw)
        assert np.array_equal(gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, raw=True, **kw), old_yuv), (name, kw)
    # chroma_down is ignored on the way up
    assert np.array_equal(gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, raw=True, colorimetry=(0, 0, cs.MEAN)), old_rgb)
    # ... and a descriptor does change the bytes
    assert not np.array_equal(gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, raw=True, colorimetry=(cs.BT709, 0)), old_rgb)
    assert not np.array_equal(gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, raw=True, colorimetry=(0, 0, cs.MEAN)), old_yuv)


# ---- every format under two descriptors -------------------------------------------------------------------------------------------
def shapes(name):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    return [(70, 6)] + ([(2, 2), (518, 4)] if sx else [])


@pytest.mark.parametrize("desc", [BT709_LIMITED_MEAN, BT2020_FULL_TOPLEFT], ids=["709-limited-mean", "2020-full-topleft"])
@pytest.mark.parametrize("name", YUV)
def test_formats_by_descriptor(gpu, name, desc):
    n = 3
    for k, (w, h) in enumerate(shapes(name)):
        for label, layout, size, rgb_pad in layouts(name, w, h):
            planes = [random_planes(name, w, h, 300 + 10 * k + i) for i in range(n)]
            surfaces = [enhyuvref.pack(name, *p, layout, size, fill_of(name)) for p in planes]
            for rgb in ("BGR8", "RGBA8"):
                cn = cvtref.RGB_FORMATS[rgb][0]
                stride = up16(w * cn) if label == "aligned" else w * cn + rgb_pad
                raws = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surfaces, w, h, fmt(rgb).fmt, layout=layout, rgb_stride=stride, raw=True, colorimetry=desc)
                assert len(raws) == n
                for i in range(n):
                    want = np.full(h * stride + 16, FILL, np.uint8)
                    want[:h * stride].reshape(h, stride)[:, :w * cn] = want_rgb(name, planes[i], rgb, desc).reshape(h, w * cn)
                    assert np.array_equal(raws[i], want), (name, label, rgb, w, h, i)
                frames = [random_frame(w, h, cn, 400 + 10 * k + i) for i in range(n)]
                raws = gpu.cvt_rgb_to_yuv(frames, fmt(name).fmt, fmt(rgb).fmt, layout=layout, size=size, rgb_stride=stride, raw=True, colorimetry=desc)
                assert len(raws) == n
                for i in range(n):
                    want = want_surface(name, frames[i], rgb, desc, layout, size + 16, fill_of(name)).view(np.uint8)
                    assert np.array_equal(raws[i], want), (name, label, rgb, w, h, i)


# ---- mean chroma ------------------------------------------------------------------------------------------------------------------
def extreme_frames(w, h):
    """Whole frames (B, G, R) of the extremes: red, blue, and 0 / 255 alternating along x, along y and as a checkerboard."""
    red, blue = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    red[:, :, 2], blue[:, :, 0] = 255, 255
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"red": red, "blue": blue}
    for label, m in (("alt_x", xx & 1), ("alt_y", yy & 1), ("check", (xx + yy) & 1)):
        out[label] = np.repeat((255 * m)[:, :, None], 3, 2).astype(np.uint8)
    return out


@pytest.mark.parametrize("name", ["NV12", "I420", "I422", "P010", "I012"])
def test_mean_chroma(gpu, name):
    w, h = 70, 6
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    frames = extreme_frames(w, h)
    frames.update({"random%d" % k: random_frame(w, h, 3, 500 + k) for k in range(3)})
    labels = sorted(frames)
    for combo in ((cs.BT709, cs.LIMITED), (cs.BT601, cs.FULL), (cs.BT601, cs.LIMITED)):
        desc = combo + (cs.MEAN,)
        for label_l, layout, size, rgb_pad in layouts(name, w, h):
            stride = up16(w * 3) if label_l == "aligned" else w * 3 + rgb_pad
            raws = gpu.cvt_rgb_to_yuv([frames[k] for k in labels], fmt(name).fmt, layout=layout, size=size, rgb_stride=stride, raw=True, colorimetry=desc)
            for label, raw in zip(labels, raws):
                want = want_surface(name, frames[label], "BGR8", desc, layout, size + 16, fill_of(name)).view(np.uint8)
                assert np.array_equal(raw, want), (name, combo_id(combo), label_l, label)
        # what the statement says about the extremes, seen on the device's bytes
        got = dict(zip(labels, gpu.cvt_rgb_to_yuv([frames[k] for k in labels], fmt(name).fmt, colorimetry=desc)))
        for label in ("alt_x", "check") + (("alt_y",) if sy else ()):
            _, u, v = enhyuvref.unpack(name, got[label], w, h)
            assert (cvtref.sample_to_byte(name, u) == 128).all() and (cvtref.sample_to_byte(name, v) == 128).all(), (name, label)
        for label in ("red", "blue"):
            assert np.array_equal(got[label], gpu.cvt_rgb_to_yuv(frames[label], fmt(name).fmt, colorimetry=combo + (cs.TOPLEFT,))), (name, label)


# ---- the enhancer on YUV surfaces -------------------------------------------------------------------------------------------------
TABLES = dict(brightness=1.5, contrast=1.1, gamma=1.2)
SETTINGS = {
    "points": TABLES,
    "vibrance": dict(TABLES, enable_vibrance=1),
    "shipped": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0),
}
CLAHE_WB = dict(enable_clahe=1, clahe_tile_grid_size=2, enable_white_balance=1, wb_strength=0.7)
ENH_FORMATS = ["NV12", "I420", "P010", "I422", "I444"]
ENH_DESCS = [BT709_LIMITED_MEAN, BT601_FULL_TOPLEFT]
ENH_SIZES = [(70, 6), (134, 10)]


@pytest.fixture(scope="module")
def picture():
    f = synth.make_clip(synth.SEED_CONFIG1, 160, 120, 1)[0]
    f.setflags(write=False)
    return f


@pytest.fixture()
def enh(gpu):
    e = capi.Enhancer(gpu)
    yield e
    e.close()


def surfaces_of(picture, name, w, h, n):
    """n surfaces of the format from n different crops of the picture; 16-bit samples carry live bits below the byte that is read."""
    out = []
    for k in range(n):
        x0, y0 = 2 + k * 5, 30 + k * 9
        s = enhyuvref.from_bgr(name, np.ascontiguousarray(picture[y0:y0 + h, x0:x0 + w]))
        if s.dtype == np.uint16:
            s = s | np.random.default_rng(700 + k).integers(0, 1 << cvtref.sample_shift(name), s.shape, np.uint16)
        out.append(s)
    return out


def three_calls(gpu, enh, p, name, surface, w, h, desc):
    """vs_op_cvt_yuv_to_rgb_cs -> vs_enh_apply_dev -> vs_op_cvt_rgb_to_yuv_cs, made here; rows of the BGR8 frames padded to 4 bytes."""
    pad = (w * 3 + 3) & ~3
    step1 = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, rgb_stride=pad, colorimetry=desc, use_cs=True)
    rows = np.zeros((h, pad), np.uint8)
    rows[:, :w * 3] = step1.reshape(h, w * 3)
    d_in, d_out = capi.DevBuf.from_array(gpu, rows), capi.DevBuf(gpu, h * pad)
    try:
        enh.apply_dev(p, d_in.ptr, w, h, pad, d_out.ptr, pad)
        enh.sync()
        step2 = d_out.download((h, pad), np.uint8)[:, :w * 3].reshape(h, w, 3).copy()
    finally:
        d_in.free()
        d_out.free()
    assert not np.array_equal(step2, step1)
    return gpu.cvt_rgb_to_yuv(step2, fmt(name).fmt, rgb_stride=pad, colorimetry=desc, use_cs=True)


@pytest.mark.parametrize("desc", ENH_DESCS, ids=["709-limited-mean", "601-full-topleft"])
@pytest.mark.parametrize("name", ENH_FORMATS)
def test_enhancer_on_yuv_is_the_three_calls(gpu, enh, picture, name, desc):
    for w, h in ENH_SIZES:
        surface = surfaces_of(picture, name, w, h, 1)[0]
        for setting in (SETTINGS["shipped"], CLAHE_WB):
            p = capi.Enhancer.default_params(gpu, **setting)
            enh.set_yuv_colorimetry(None)
            before = enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h)
            assert np.array_equal(before, three_calls(gpu, enh, p, name, surface, w, h, None))
            enh.set_yuv_colorimetry(desc)
            want = three_calls(gpu, enh, p, name, surface, w, h, desc)
            got = enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h)
            assert np.array_equal(got, want), (name, w, h)
            assert not np.array_equal(got, before)
            assert np.array_equal(enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h, in_place=True), want), (name, w, h, "in place")
            # a refused descriptor leaves the setting as it was; NULL restores today's output
            assert enh.lib.vs_enh_set_yuv_colorimetry(enh.h, capi._cs_ref((7, 0, 0, 0))) == 1
            assert b"matrix" in enh.lib.vs_enh_last_error(enh.h)
            assert np.array_equal(enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h), want)
            enh.set_yuv_colorimetry(None)
            assert np.array_equal(enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h), before), (name, w, h, "NULL again")


@pytest.mark.parametrize("desc", ENH_DESCS, ids=["709-limited-mean", "601-full-topleft"])
@pytest.mark.parametrize("name", ENH_FORMATS)
def test_enhancer_batch_is_fused_and_equals_single_calls(gpu, enh, picture, name, desc):
    n = 3
    for w, h in ENH_SIZES:
        srcs = surfaces_of(picture, name, w, h, n)
        for setting in ("points", "vibrance", "shipped"):
            p = capi.Enhancer.default_params(gpu, **SETTINGS[setting])
            enh.set_yuv_colorimetry(None)
            default = enh.apply_yuv_batch_dev(p, fmt(name).fmt, srcs, w, h, raw=True)
            assert enh.last_fused() == n
            enh.set_yuv_colorimetry(desc)
            single = [three_calls(gpu, enh, p, name, s, w, h, desc) for s in srcs]
            assert all(np.array_equal(enh.apply_yuv_dev(p, fmt(name).fmt, s, w, h), one) for s, one in zip(srcs, single))
            raws = enh.apply_yuv_batch_dev(p, fmt(name).fmt, srcs, w, h, raw=True)
            assert enh.last_fused() == n, (name, setting, w, h)
            for k in range(n):
                want = np.concatenate([single[k].reshape(-1).view(np.uint8), np.full(16, FILL, np.uint8)])
                assert np.array_equal(raws[k], want), (name, setting, w, h, k)
            assert not np.array_equal(raws[0], default[0])
            # in place: the point pass stays fused and equal; the unsharp pass takes the three calls, and is equal
            inplace = enh.apply_yuv_batch_dev(p, fmt(name).fmt, srcs, w, h, in_place=True, raw=True)
            assert enh.last_fused() == (0 if setting == "shipped" else n), (name, setting)
            assert all(np.array_equal(a, b) for a, b in zip(inplace, raws)), (name, setting, w, h, "in place")
            # NULL again: today's output
            enh.set_yuv_colorimetry(None)
            again = enh.apply_yuv_batch_dev(p, fmt(name).fmt, srcs, w, h, raw=True)
            assert enh.last_fused() == n and all(np.array_equal(a, b) for a, b in zip(again, default)), (name, setting, w, h, "NULL again")
