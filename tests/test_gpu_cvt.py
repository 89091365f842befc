"""vs_op_cvt_yuv_to_rgb, vs_op_cvt_rgb_to_yuv and vs_enh_apply_yuv_dev on the GPU, held to the numpy statement tests/cvtref.py.
Every comparison is array_equal.  Destinations are prefilled with 0xA5 and compared whole - row padding, the gap between planes
and 16 guard bytes behind the last plane included - wherever the raw buffer is asked for."""
import numpy as np
import pytest

import cvtref
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

YUV = list(cvtref.YUV_FORMATS)
RGB = list(cvtref.RGB_FORMATS)
FILL = 0xA5


def fmt(name):
    return capi.PIXFMT_BY_NAME[name]


# ---- surfaces of every format from byte or sample planes, in any layout -----------------------------------------------------------
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


def pack(name, y, u, v, layout=None, size=None, fill=0):
    """The surface of three sample planes: packed (rows, w), or a flat buffer of `size` bytes in `layout` (bytes, 0 = default)."""
    kind, sb, bits, sx, sy = cvtref.YUV_FORMATS[name]
    if kind == "3p":
        if not layout:
            return synth.yuv_pack(y, u, v, sx, sy)
        pitch, c_pitch, u_off, v_off = (x or None for x in layout)
        return synth.yuv_pack(y, u, v, sx, sy, pitch, c_pitch, u_off, v_off, size, fill)
    h, w = y.shape
    uv = np.empty((h // 2, w), y.dtype)
    uv[:, 0::2], uv[:, 1::2] = u, v
    if not layout:
        return np.vstack([y, uv])
    pitch, uv_off = layout[0], layout[2] or h * layout[0]
    buf = np.full(size // sb, fill, y.dtype)
    buf[:h * pitch // sb].reshape(h, pitch // sb)[:, :w] = y
    buf[uv_off // sb:(uv_off + h // 2 * pitch) // sb].reshape(h // 2, pitch // sb)[:, :w] = uv
    return buf


def byte_planes(name, planes):
    return [cvtref.sample_to_byte(name, p) for p in planes]


def want_rgb(name, planes, rgb):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    return cvtref.yuv_to_rgb(*byte_planes(name, planes), sx, sy, rgb)


def want_surface(name, frame, rgb, layout=None, size=None, fill=0):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    return pack(name, *(cvtref.byte_to_sample(name, p) for p in cvtref.rgb_to_yuv(frame, sx, sy, rgb)), layout, size, fill)


def random_frame(w, h, cn, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, cn), np.uint8)


def fill_of(name):
    return FILL * 0x0101 if cvtref.YUV_FORMATS[name][1] == 2 else FILL


# ---- exhaustive values ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triples():
    planes = cvtref.all_triples()
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.fixture(scope="module")
def triples_rgb(triples):
    r, g, b = cvtref.yuv_to_rgb_px(*triples)
    out = tuple(c.astype(np.uint8) for c in (r, g, b))
    for c in out:
        c.setflags(write=False)
    return out


def test_every_yuv_triple_to_bgr8(gpu, triples, triples_rgb):
    got = gpu.cvt_yuv_to_rgb(fmt("I444").fmt, synth.yuv_pack(*triples, 0, 0), 4096, 4096, fmt("BGR8").fmt)
    r, g, b = triples_rgb
    assert np.array_equal(got[:, :, 0], b) and np.array_equal(got[:, :, 1], g) and np.array_equal(got[:, :, 2], r)


def test_every_yuv_triple_to_bgra8(gpu, triples, triples_rgb):
    got = gpu.cvt_yuv_to_rgb(fmt("I444").fmt, synth.yuv_pack(*triples, 0, 0), 4096, 4096, fmt("BGRA8").fmt)
    r, g, b = triples_rgb
    assert np.array_equal(got[:, :, 0], b) and np.array_equal(got[:, :, 1], g) and np.array_equal(got[:, :, 2], r)
    assert (got[:, :, 3] == 255).all()


def test_every_bgr_triple_to_i444(gpu, triples):
    b, g, r = triples
    got = gpu.cvt_rgb_to_yuv(np.dstack([b, g, r]), fmt("I444").fmt, fmt("BGR8").fmt)
    y, u, v = cvtref.rgb_to_yuv_px(r, g, b)
    gy, gu, gv = synth.yuv_unpack(got, 4096, 4096, 0, 0)
    assert np.array_equal(gy, y) and np.array_equal(gu, u) and np.array_equal(gv, v)


# ---- small shapes: one partial wave, ragged runs of every length a format allows, more than one block down (18 rows > 4 chroma
# rows) and - a lane covers 8 pixels, a block 512 - across (522 = a block, one whole run and a ragged one) -------------------------
def shapes(name):
    _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
    ws = [2, 6, 10, 34, 130, 258] + ([1, 5, 33] if sx == 0 else [])
    hs = [2, 6, 18] + ([1, 7] if sy == 0 else [])
    return [(w, h) for w in ws for h in hs] + [(522, 6)]


@pytest.mark.parametrize("name", YUV)
def test_small_shapes_yuv_to_rgb(gpu, name):
    for k, (w, h) in enumerate(shapes(name)):
        planes = random_planes(name, w, h, 100 + k)
        surface = pack(name, *planes)
        for rgb in RGB:
            cn = cvtref.RGB_FORMATS[rgb][0]
            raw = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, fmt(rgb).fmt, raw=True)
            assert np.array_equal(raw[:h * w * cn].reshape(h, w, cn), want_rgb(name, planes, rgb)), (name, rgb, w, h)
            assert (raw[h * w * cn:] == FILL).all(), (name, rgb, w, h)


@pytest.mark.parametrize("name", YUV)
def test_small_shapes_rgb_to_yuv(gpu, name):
    for k, (w, h) in enumerate(shapes(name)):
        for rgb in RGB:
            frame = random_frame(w, h, cvtref.RGB_FORMATS[rgb][0], 200 + k)
            raw = gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, fmt(rgb).fmt, raw=True)
            want = want_surface(name, frame, rgb)
            assert np.array_equal(raw[:want.nbytes].view(want.dtype).reshape(want.shape), want), (name, rgb, w, h)
            assert (raw[want.nbytes:] == FILL).all(), (name, rgb, w, h)


# ---- random content of the 16-bit formats -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in YUV if cvtref.YUV_FORMATS[n][1] == 2])
def test_sixteen_bit_content(gpu, name):
    kind, sb, bits, sx, sy = cvtref.YUV_FORMATS[name]
    w, h = 130, 18
    planes = random_planes(name, w, h, 7)
    if kind == "uv":
        assert all((p & 0xFF).any() and (p & 0x3F).any() for p in planes)                   # live low bits, below the ten as well
    else:
        assert all((p >> bits).any() for p in planes)                                        # samples beyond the format's range
        assert all((cvtref.sample_to_byte(name, p) == 255).sum() > (p >> bits != 0).sum() // 2 for p in planes)
    got = gpu.cvt_yuv_to_rgb(fmt(name).fmt, pack(name, *planes), w, h, fmt("BGR8").fmt)
    assert np.array_equal(got, want_rgb(name, planes, "BGR8"))
    # ... and what is written holds the byte in the format's place, nothing in the bits below
    frame = random_frame(w, h, 3, 8)
    got = gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, fmt("BGR8").fmt)
    assert np.array_equal(got, want_surface(name, frame, "BGR8"))
    assert not (got & ((1 << cvtref.sample_shift(name)) - 1)).any()


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def layouts(name, w, h):
    """[(label, (pitch, c_pitch, u_off, v_off), size)]: bytes, resolved by hand."""
    kind, sb, bits, sx, sy = cvtref.YUV_FORMATS[name]
    row, crow, ch = sb * w, sb * (w >> sx), h >> sy
    if kind == "uv":
        pitch = row + 12
        return [("packed", None, None),
                ("padded pitch", (pitch, 0, 0, 0), h * pitch + h // 2 * pitch),
                ("explicit c_pitch, plane apart", (pitch, pitch, h * pitch + 40, 0), h * pitch + 40 + h // 2 * pitch)]
    pitch, cp = row + 12, crow + 6
    return [("packed", None, None),
            ("padded pitch, explicit c_pitch", (pitch, cp, 0, 0), h * pitch + 2 * ch * cp),
            ("planes apart", (pitch, cp, h * pitch + 40, h * pitch + 40 + ch * cp + 24), h * pitch + 64 + 2 * ch * cp),
            ("V before U", (row, 0, h * row + ch * crow, h * row), h * row + 2 * ch * crow),
            ("V before U, apart", (pitch, cp, h * pitch + 16 + ch * cp + 8, h * pitch + 16), h * pitch + 24 + 2 * ch * cp)]


@pytest.mark.parametrize("name", YUV)
def test_layouts(gpu, name):
    w, h = 34, 6
    planes = random_planes(name, w, h, 31)
    for label, layout, size in layouts(name, w, h):
        surface = pack(name, *planes, layout, size, fill_of(name))
        for rgb in ("BGR8", "RGBA8"):
            cn = cvtref.RGB_FORMATS[rgb][0]
            for stride in (w * cn, w * cn + 5):
                raw = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, fmt(rgb).fmt, layout=layout, rgb_stride=stride, raw=True)
                want = np.full(h * stride + 16, FILL, np.uint8)
                want[:h * stride].reshape(h, stride)[:, :w * cn] = want_rgb(name, planes, rgb).reshape(h, w * cn)
                assert np.array_equal(raw, want), (name, label, rgb, stride)
                frame = random_frame(w, h, cn, 32)
                raw = gpu.cvt_rgb_to_yuv(frame, fmt(name).fmt, fmt(rgb).fmt, layout=layout, size=size, rgb_stride=stride, raw=True)
                if layout:
                    want = want_surface(name, frame, rgb, layout, size + 16, fill_of(name)).view(np.uint8)
                else:
                    want = np.concatenate([want_surface(name, frame, rgb).reshape(-1).view(np.uint8), np.full(16, FILL, np.uint8)])
                assert np.array_equal(raw, want), (name, label, rgb, stride)


# ---- batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "I010", "I444"])
def test_batch_equals_single_calls(gpu, name):
    w, h = 34, 6
    surfaces = [pack(name, *random_planes(name, w, h, 400 + k)) for k in range(32)]
    frames = [random_frame(w, h, 3, 500 + k) for k in range(32)]
    single_rgb = [gpu.cvt_yuv_to_rgb(fmt(name).fmt, s, w, h) for s in surfaces]
    single_yuv = [gpu.cvt_rgb_to_yuv(f, fmt(name).fmt) for f in frames]
    assert not np.array_equal(single_rgb[0], single_rgb[1]) and not np.array_equal(single_yuv[0], single_yuv[31])
    for n in (1, 3, 32):
        got = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surfaces[:n], w, h)
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, single_rgb)), (name, n)
        got = gpu.cvt_rgb_to_yuv(frames[:n], fmt(name).fmt)
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, single_yuv)), (name, n)


# ---- the enhancer on YUV surfaces -------------------------------------------------------------------------------------------------
ENH_SETTINGS = {
    "shipped": dict(brightness=1.5, contrast=1.1, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0, gamma=1.2),
    "clahe_wb": dict(enable_clahe=1, clahe_tile_grid_size=2, enable_white_balance=1, wb_strength=0.7),
}


@pytest.fixture(scope="module")
def enh(gpu):
    e = capi.Enhancer(gpu)
    yield e
    e.close()


@pytest.mark.parametrize("setting", sorted(ENH_SETTINGS))
@pytest.mark.parametrize("name", ["NV12", "I420", "P010", "I422"])
def test_enhancer_on_yuv_is_the_three_calls(gpu, enh, name, setting):
    p = capi.Enhancer.default_params(gpu, **ENH_SETTINGS[setting])
    for w, h in ((130, 18), (34, 6)):
        _, _, _, sx, sy = cvtref.YUV_FORMATS[name]
        # a picture, not noise: the stages have something to work on
        bgr = np.ascontiguousarray(synth.make_clip(synth.SEED_CONFIG1, 160, 120, 1)[0][40:40 + h, 10:10 + w])
        surface = want_surface(name, bgr, "BGR8")
        pad = (w * 3 + 3) & ~3
        step1 = gpu.cvt_yuv_to_rgb(fmt(name).fmt, surface, w, h, rgb_stride=pad)
        step2 = enh.apply(step1, p)
        want = gpu.cvt_rgb_to_yuv(step2, fmt(name).fmt, rgb_stride=pad)
        assert not np.array_equal(step2, step1)
        got = enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h)
        assert np.array_equal(got, want), (name, setting, w, h)
        assert np.array_equal(enh.apply_yuv_dev(p, fmt(name).fmt, surface, w, h, in_place=True), want), (name, setting, w, h, "in place")
