"""vs_op_cvt_yuv_to_yuv on the GPU, held to the numpy statement tests/yuvref.py.  Every comparison is array_equal.  Destinations are
prefilled with 0xA5 and compared whole: row padding, the gaps between planes and 16 guard bytes behind the last sample included."""
import ctypes as C

import numpy as np
import pytest

import yuvref
from test_gpu_cvt import pack, random_planes
from vsamd import capi

pytestmark = pytest.mark.gpu

NAMES = list(yuvref.FORMATS)
FILL = 0xA5
T, R, TL, MEAN = yuvref.TRUNCATE, yuvref.ROUND, yuvref.TOPLEFT, yuvref.MEAN


def fmt(name):
    return capi.PIXFMT_BY_NAME[name].fmt


def fill_of(name):
    return FILL * 0x0101 if yuvref.FORMATS[name][2] == np.uint16 else FILL


def surface(gpu, name, planes, w, h, layout=None):
    """The surface of three sample planes: the packed frame, or the flat buffer of `layout` with 0xA5 wherever no sample lies."""
    if not layout:
        return pack(name, *planes)
    lay, size = gpu.yuv_surface_layout(fmt(name), w, h, layout)
    return pack(name, *planes, lay, size + 16, fill_of(name))


def whole(gpu, name, planes, w, h, layout=None):
    """Every byte of a destination that was prefilled with 0xA5: the surface and 16 guard bytes."""
    if layout:
        return surface(gpu, name, planes, w, h, layout).view(np.uint8)
    return np.concatenate([pack(name, *planes).reshape(-1).view(np.uint8), np.full(16, FILL, np.uint8)])


def check(gpu, src, dst, planes, w, h, desc=None, lin=None, lout=None, tag=None):
    got = gpu.cvt_yuv_to_yuv(fmt(src), surface(gpu, src, planes, w, h, lin), w, h, fmt(dst), lin, lout, desc, raw=True)
    want = yuvref.convert(src, planes, dst, *(desc or (T, TL)))
    assert np.array_equal(got, whole(gpu, dst, want, w, h, lout)), (src, dst, w, h, desc, tag)


# ---- every pair of formats, every descriptor --------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", NAMES)
def test_every_pair_and_descriptor(gpu, src):
    w, h = 24, 8
    planes = random_planes(src, w, h, 50 + NAMES.index(src))
    if yuvref.FORMATS[src][1]:
        assert all((p >> yuvref.FORMATS[src][0]).any() for p in planes)          # samples beyond the format's range
    for dst in NAMES:
        for desc in yuvref.DESCRIPTORS:
            check(gpu, src, dst, planes, w, h, desc)
        check(gpu, src, dst, planes, w, h, None)                                 # a null descriptor: truncate, top-left


# ---- shapes: a single chroma sample, a ragged 8-pixel run, the 512-pixel block edge, more than one block down with a partial
# last one (a block covers four groups of rows) ------------------------------------------------------------------------------------
CASES = [("I420", "NV12", (T, TL)), ("NV12", "I444", (T, TL)), ("I444", "NV12", (T, MEAN)), ("I210", "P010", (R, MEAN)), ("P010", "I012", (T, TL)),
         ("I412", "I420", (R, MEAN)), ("I422", "I422", (T, TL))]
SHAPES = [(2, 2), (18, 6), (520, 10), (1032, 18)]


@pytest.mark.parametrize("src,dst,desc", CASES)
def test_shapes(gpu, src, dst, desc):
    for k, (w, h) in enumerate(SHAPES):
        check(gpu, src, dst, random_planes(src, w, h, 300 + k), w, h, desc)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def layouts(name, w, h):
    """[(label, (pitch, c_pitch, u_off, v_off))]: bytes, 0 = the default of a field."""
    _, _, dt, sx, sy = yuvref.FORMATS[name]
    sb = np.dtype(dt).itemsize
    row, crow, ch = sb * w, sb * (w >> sx), h >> sy
    if name in ("NV12", "P010"):
        pitch = row + 2
        return [("pitch + 2", (pitch, 0, 0, 0)), ("plane apart", (pitch, pitch, h * pitch + 40, 0))]
    pitch, cp = row + 2, crow + 2
    return [("pitch + 2, chroma pitch + 2", (pitch, cp, 0, 0)),
            ("YV12 offsets", (row, 0, h * row + ch * crow, h * row)),
            ("planes apart", (pitch, cp, h * pitch + 40, h * pitch + 40 + ch * cp + 24)),
            ("V before U, apart", (pitch, cp, h * pitch + 16 + ch * cp + 8, h * pitch + 16))]


@pytest.mark.parametrize("src,dst,desc", [("I420", "NV12", (T, TL)), ("NV12", "I420", (T, TL)), ("I210", "P010", (R, MEAN)), ("P010", "I012", (T, TL)),
                                          ("I444", "I422", (T, MEAN)), ("I422", "I422", (T, TL))])
def test_layouts_on_either_side(gpu, src, dst, desc):
    w, h = 34, 6
    planes = random_planes(src, w, h, 31)
    for label, lin in layouts(src, w, h):
        check(gpu, src, dst, planes, w, h, desc, lin=lin, tag=("source", label))
    for label, lout in layouts(dst, w, h):
        check(gpu, src, dst, planes, w, h, desc, lout=lout, tag=("destination", label))
    check(gpu, src, dst, planes, w, h, desc, lin=layouts(src, w, h)[-1][1], lout=layouts(dst, w, h)[-1][1], tag="both")


def test_yv12_is_i420_with_the_offsets_swapped(gpu):
    w, h = 34, 6
    y, u, v = random_planes("I420", w, h, 32)
    yv12 = (w, 0, h * w + (h // 2) * (w // 2), h * w)
    got = gpu.cvt_yuv_to_yuv(fmt("I420"), pack("I420", y, u, v), w, h, fmt("I420"), None, yv12)
    assert np.array_equal(got.reshape(-1), pack("I420", y, v, u).reshape(-1))


def convert_at(gpu, src, dst, buf_in, w, h, lin, lout, off_in, off_out, desc=None):
    """One call on a source that lies off_in bytes into its allocation and a destination off_out bytes into its own -> the whole
    destination allocation (prefilled with 0xA5; 16 guard bytes behind the last sample)."""
    _, size = gpu.yuv_surface_layout(fmt(dst), w, h, lout)
    raw_in = np.concatenate([np.full(off_in, FILL, np.uint8), np.ascontiguousarray(buf_in).reshape(-1).view(np.uint8)])
    d_in = capi.DevBuf.from_array(gpu, raw_in)
    d_out = capi.DevBuf.from_array(gpu, np.full(off_out + size + 16, FILL, np.uint8))
    try:
        ps, pd = (C.c_void_p * 1)(d_in.ptr + off_in), (C.c_void_p * 1)(d_out.ptr + off_out)
        d = C.byref(capi.VsYuvCvtDesc(*desc)) if desc else None
        gpu.check(gpu.lib.vs_op_cvt_yuv_to_yuv(fmt(src), ps, C.byref(capi.I420LayoutC(*lin)), fmt(dst), pd, C.byref(capi.I420LayoutC(*lout)), 1, w, h, d, None))
        gpu.sync()
        return d_out.download((off_out + size + 16,), np.uint8)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("src,dst,desc,off,pad", [("I420", "NV12", (T, TL), 1, 1), ("NV12", "I444", (T, TL), 1, 1), ("I444", "I420", (T, MEAN), 3, 1),
                                                  ("I210", "P010", (R, MEAN), 2, 0), ("P010", "I012", (T, TL), 2, 0), ("I010", "I420", (R, TL), 2, 0)])
def test_unaligned_surfaces_go_sample_by_sample(gpu, src, dst, desc, off, pad):
    """8-bit surfaces at an odd pointer and an odd pitch, 16-bit ones at pointer + 2: no run of theirs is aligned to its size."""
    w, h = 40, 6
    planes = random_planes(src, w, h, 77)

    def lay(name):
        _, _, dt, sx, sy = yuvref.FORMATS[name]
        sb = np.dtype(dt).itemsize
        if sb == 2:
            return (sb * w, 0, 0, 0)
        pitch = w + pad          # odd
        return (pitch, pitch, 0, 0) if name == "NV12" else (pitch, (w >> sx) + pad, 0, 0)
    lin, lout = lay(src), lay(dst)
    dst_off = off if yuvref.FORMATS[dst][2] == yuvref.FORMATS[src][2] else (2 if yuvref.FORMATS[dst][2] == np.uint16 else 1)
    got = convert_at(gpu, src, dst, surface(gpu, src, planes, w, h, lin), w, h, lin, lout, off, dst_off, desc)
    want = yuvref.convert(src, planes, dst, *desc)
    assert np.array_equal(got, np.concatenate([np.full(dst_off, FILL, np.uint8), whole(gpu, dst, want, w, h, lout)])), (src, dst)


# ---- batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,desc", [("I420", "NV12", (T, TL)), ("I210", "P010", (R, MEAN))])
def test_batches_of_distinct_surfaces(gpu, src, dst, desc):
    w, h = 24, 8
    planes = [random_planes(src, w, h, 400 + k) for k in range(32)]
    want = [whole(gpu, dst, yuvref.convert(src, p, dst, *desc), w, h) for p in planes]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[2], want[31])
    for n in (3, 32):
        got = gpu.cvt_yuv_to_yuv(fmt(src), [pack(src, *p) for p in planes[:n]], w, h, fmt(dst), desc=desc, raw=True)
        assert len(got) == n
        for k in range(n):
            assert np.array_equal(got[k], want[k]), (src, dst, n, k)


# ---- every 16-bit word through every pair of depths -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words():
    w = np.arange(1 << 16, dtype=np.uint16).reshape(256, 256)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("src", ["I444", "I410", "I412", "P010"])
def test_every_word_through_every_depth(gpu, words, src):
    _, _, dt, sx, sy = yuvref.FORMATS[src]
    y = words if dt == np.uint16 else (words & 255).astype(np.uint8)
    planes = [y, np.ascontiguousarray(y[::-1][:256 >> sy, :256 >> sx]), np.ascontiguousarray(y[:, ::-1][:256 >> sy, :256 >> sx])]
    for dst in ("I444", "I410", "I412", "P010"):
        for rule in (T, R):
            got = gpu.cvt_yuv_to_yuv(fmt(src), pack(src, *planes), 256, 256, fmt(dst), desc=(rule, TL))
            want = yuvref.convert(src, planes, dst, rule, TL)
            assert np.array_equal(got, pack(dst, *want)), (src, dst, rule)


# ---- composition with the colour conversion, round trips --------------------------------------------------------------------------
@pytest.mark.parametrize("deep,eight", [("I210", "I422"), ("P010", "NV12")])
def test_colour_conversion_reads_the_truncated_surface_alike(gpu, deep, eight):
    w, h = 130, 18
    s = pack(deep, *random_planes(deep, w, h, 61))
    s8 = gpu.cvt_yuv_to_yuv(fmt(deep), s, w, h, fmt(eight))
    assert s8.dtype == np.uint8
    assert np.array_equal(gpu.cvt_yuv_to_rgb(fmt(deep), s, w, h), gpu.cvt_yuv_to_rgb(fmt(eight), s8, w, h))


def test_round_trips(gpu):
    w, h = 130, 18
    s = pack("I420", *random_planes("I420", w, h, 62))
    nv12 = gpu.cvt_yuv_to_yuv(fmt("I420"), s, w, h, fmt("NV12"))
    assert np.array_equal(gpu.cvt_yuv_to_yuv(fmt("NV12"), nv12, w, h, fmt("I420")), s)
    s = pack("I010", *(p & 1023 for p in random_planes("I010", w, h, 63)))
    p010 = gpu.cvt_yuv_to_yuv(fmt("I010"), s, w, h, fmt("P010"))
    assert p010.dtype == np.uint16 and not (p010 & 63).any() and (p010 >> 6).max() > 255
    for desc in (None, (R, MEAN)):
        assert np.array_equal(gpu.cvt_yuv_to_yuv(fmt("P010"), p010, w, h, fmt("I010"), desc=desc), s)
