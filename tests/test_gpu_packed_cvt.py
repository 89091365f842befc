"""vs_op_cvt_packed_to_yuv and vs_op_cvt_yuv_to_packed on the GPU, held to the numpy statement tests/packedref.py.  Every comparison is
array_equal.  Destinations are prefilled with 0xA5 and compared whole: row padding, the gaps between planes and 16 guard bytes
behind the last byte included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packedref
import yuvref
from test_gpu_cvt import pack, random_planes
from test_gpu_yuv_cvt import FILL, fmt, layouts, surface, whole
from vsamd import capi

pytestmark = pytest.mark.gpu

PACKED = list(packedref.FORMATS)
SURFACES = list(yuvref.FORMATS)
T, R, TL, MEAN = yuvref.TRUNCATE, yuvref.ROUND, yuvref.TOPLEFT, yuvref.MEAN
DESCS = yuvref.DESCRIPTORS + [None]          # None: a null descriptor - truncate, top-left

# the kernel's constants (csrc/k_yuvpacked.hip): the pixels of a lane's run and the lanes along a row, for the 8-bit orders and Y210
# and for v210; a wave of 64 lanes and a block of YP_THREADS cover YP_BX * YP_PX (YP_BX_V210 * YP_PX_V210) pixels across, a block
# YP_THREADS / YP_BX (/ YP_BX_V210) groups of rows down
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-stab_amd", "csrc", "k_yuvpacked.hip")).read()
K = {k: int(re.search(r"constexpr int %s = (\d+);" % k, _SRC).group(1)) for k in ("YP_PX", "YP_PX_V210", "YP_BX", "YP_BX_V210", "YP_THREADS")}


def lane_px(name):
    return K["YP_PX_V210"] if name == "v210" else K["YP_PX"]


def span_px(name):
    """Pixels across of one wave's lanes along a row, which is the block's width."""
    return lane_px(name) * (K["YP_BX_V210"] if name == "v210" else K["YP_BX"])


def block_rows(name, surf):
    return (K["YP_THREADS"] // (K["YP_BX_V210"] if name == "v210" else K["YP_BX"])) << yuvref.FORMATS[surf][4]


def test_the_kernels_constants_are_the_ones_the_shapes_below_assume():
    assert (lane_px("UYVY"), lane_px("v210"), span_px("YUY2"), span_px("Y210"), span_px("v210")) == (8, 24, 512, 512, 768)
    assert (block_rows("UYVY", "NV12"), block_rows("UYVY", "I422"), block_rows("v210", "P010"), block_rows("v210", "I444")) == (8, 4, 16, 8)


# ---- the packed side as bytes -------------------------------------------------------------------------------------------------
def packed_source(name, w, h, seed, pitch=0):
    """(planes, buffer): random sample planes and the frame that holds them, rows `pitch` apart with 0xA5 between them.  v210: bits
    30 - 31 of every word and the fields of pixels >= w in the last group carry noise, which the operator must not look at."""
    wide = 6 * ((w + 5) // 6) if name == "v210" else w
    planes = packedref.random_planes(name, wide, h, seed)
    rows = packedref.pack(name, planes)
    if name == "v210":
        words = rows.view("<u4")
        rows = (words | np.random.default_rng(seed).integers(0, 4, words.shape, dtype=np.uint32) << 30).astype("<u4").view(np.uint8)
        planes = [np.ascontiguousarray(p[:, :pw]) for p, pw in zip(planes, (w, w // 2, w // 2))]
    return planes, packed_frame(name, rows, w, h, pitch)


def packed_frame(name, rows, w, h, pitch=0, guard=0):
    """The bytes of a packed frame from its first to the last byte of its last row (+ guard), 0xA5 wherever no row lies."""
    row, pitch = packedref.row_bytes(name, w), pitch or packedref.default_pitch(name, w)
    assert rows.shape == (h, row)
    buf = np.full((h - 1) * pitch + row + guard, FILL, np.uint8)
    for y in range(h):
        buf[y * pitch:y * pitch + row] = rows[y]
    return buf


def check_to_yuv(gpu, name, dst, w, h, desc, seed, pitch=0, lout=None, tag=None):
    planes, buf = packed_source(name, w, h, seed, pitch)
    got = gpu.cvt_packed_to_yuv(packedref.ENUM[name], buf, w, h, fmt(dst), pitch, lout, desc, raw=True)
    want = packedref.packed_to_yuv(name, planes, dst, *(desc or (T, TL)))
    assert np.array_equal(got, whole(gpu, dst, want, w, h, lout)), (name, dst, w, h, desc, pitch, tag)


def check_to_packed(gpu, src, name, w, h, desc, seed, pitch=0, lin=None, tag=None):
    planes = random_planes(src, w, h, seed)
    got = gpu.cvt_yuv_to_packed(fmt(src), surface(gpu, src, planes, w, h, lin), w, h, packedref.ENUM[name], lin, pitch, desc, raw=True)
    want = packedref.pack(name, packedref.yuv_to_packed(src, planes, name, *(desc or (T, TL))))
    assert np.array_equal(got, packed_frame(name, want, w, h, pitch, 16)), (src, name, w, h, desc, pitch, tag)


def check(gpu, to_packed, name, surf, *a, **kw):
    (check_to_packed if to_packed else check_to_yuv)(gpu, *((surf, name) if to_packed else (name, surf)), *a, **kw)


# ---- every pairing, both directions, every descriptor ---------------------------------------------------------------------------
@pytest.mark.parametrize("to_packed", [False, True])
@pytest.mark.parametrize("name", PACKED)
def test_every_pairing_and_descriptor(gpu, name, to_packed):
    for k, surf in enumerate(SURFACES):
        if to_packed and yuvref.FORMATS[surf][1]:          # samples beyond a low-bit format's range
            assert all((p >> yuvref.FORMATS[surf][0]).any() for p in random_planes(surf, 24, 8, 50 + k))
        for w, h in ((24, 8), (26, 8)):
            for desc in DESCS:
                check(gpu, to_packed, name, surf, w, h, desc, 50 + k)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def shapes(name, surf):
    """The smallest shapes at which each path can go wrong: one macropixel; a v210 group that is partial and one that is exactly
    full; the 128-byte steps of the v210 pitch; two pixels either side of one lane's run, of one wave's span (which is one block's
    width); odd heights where the surface takes them; more than one block down with a partial last one."""
    sy = yuvref.FORMATS[surf][4]
    lane, span, rows = lane_px(name), span_px(name), block_rows(name, surf)
    out = [(w, 2) for w in (2, 4, 6, 8, 46, 48, 50, lane - 2, lane, lane + 2, span - 2, span, span + 2)]
    if not sy:
        out += [(2, 1), (lane + 2, 3), (50, 1)]
    out.append((lane + 2, 2 * rows + (2 if sy else 1)))
    return out


@pytest.mark.parametrize("to_packed", [False, True])
@pytest.mark.parametrize("surf", ["NV12", "I422", "I444", "P010"])
@pytest.mark.parametrize("name", PACKED)
def test_shapes(gpu, name, surf, to_packed):
    for k, (w, h) in enumerate(shapes(name, surf)):
        check(gpu, to_packed, name, surf, w, h, (R, MEAN), 300 + k)


# ---- layout: pitches, base pointers, explicit surface layouts -------------------------------------------------------------------
@pytest.mark.parametrize("to_packed", [False, True])
@pytest.mark.parametrize("name", PACKED)
def test_a_packed_pitch_of_four_bytes_more_than_a_row(gpu, name, to_packed):
    for surf, desc in (("NV12", (T, MEAN)), ("I210", (R, TL))):
        for w, h in ((40, 6), (50, 4)):
            check(gpu, to_packed, name, surf, w, h, desc, 70, pitch=packedref.row_bytes(name, w) + 4)


def convert_at(gpu, to_packed, name, surf, src_bytes, w, h, pitch, off_in, off_out, out_bytes, desc):
    """One call on a source that lies off_in bytes into its allocation and a destination off_out bytes into its own -> the whole
    destination allocation (prefilled with 0xA5; out_bytes + 16 guard bytes behind off_out)."""
    d_in = capi.DevBuf.from_array(gpu, np.concatenate([np.full(off_in, FILL, np.uint8), np.ascontiguousarray(src_bytes).reshape(-1).view(np.uint8)]))
    d_out = capi.DevBuf.from_array(gpu, np.full(off_out + out_bytes + 16, FILL, np.uint8))
    try:
        ps, pd = (C.c_void_p * 1)(d_in.ptr + off_in), (C.c_void_p * 1)(d_out.ptr + off_out)
        lay = C.byref(capi.I420LayoutC(np.dtype(yuvref.FORMATS[surf][2]).itemsize * w, 0, 0, 0))
        d = C.byref(capi.VsYuvCvtDesc(*desc))
        if to_packed:
            gpu.check(gpu.lib.vs_op_cvt_yuv_to_packed(fmt(surf), ps, lay, packedref.ENUM[name], pd, pitch, 1, w, h, d, None))
        else:
            gpu.check(gpu.lib.vs_op_cvt_packed_to_yuv(packedref.ENUM[name], ps, pitch, fmt(surf), pd, lay, 1, w, h, d, None))
        gpu.sync()
        return d_out.download((off_out + out_bytes + 16,), np.uint8)
    finally:
        d_in.free()
        d_out.free()


OFFSETS = {"YUY2": (1, 2, 3), "UYVY": (1, 2, 3), "YVYU": (1, 2, 3), "Y210": (2,), "v210": (4, 8, 12)}


@pytest.mark.parametrize("to_packed", [False, True])
@pytest.mark.parametrize("name", PACKED)
def test_packed_frames_at_unaligned_pointers(gpu, name, to_packed):
    """No 16-byte run of such a frame is aligned to its size: it moves by the unit the format guarantees."""
    w, h, desc = 50, 4, (R, MEAN)
    for surf in ("NV12", "I210"):
        for off in OFFSETS[name]:
            if to_packed:
                planes = random_planes(surf, w, h, 77)
                size = gpu.packed_layout(packedref.ENUM[name], w, h)[2]
                got = convert_at(gpu, True, name, surf, pack(surf, *planes), w, h, 0, 0, off, size, desc)
                want = packed_frame(name, packedref.pack(name, packedref.yuv_to_packed(surf, planes, name, *desc)), w, h, 0, 16)
            else:
                planes, buf = packed_source(name, w, h, 78)
                _, size = gpu.yuv_surface_layout(fmt(surf), w, h)
                got = convert_at(gpu, False, name, surf, buf, w, h, 0, off, 0, size, desc)
                want = whole(gpu, surf, packedref.packed_to_yuv(name, planes, surf, *desc), w, h)
                off = 0
            assert np.array_equal(got, np.concatenate([np.full(off, FILL, np.uint8), want])), (name, surf, off)


@pytest.mark.parametrize("to_packed", [False, True])
@pytest.mark.parametrize("name,surf,desc", [("UYVY", "NV12", (T, MEAN)), ("YUY2", "I422", (T, TL)), ("v210", "P010", (R, MEAN)), ("v210", "I210", (T, TL)),
                                            ("Y210", "I444", (R, MEAN)), ("YVYU", "I012", (T, TL))])
def test_explicit_layouts_on_the_surface_side(gpu, name, surf, desc, to_packed):
    w, h = 34, 6
    for label, lay in layouts(surf, w, h):
        check(gpu, to_packed, name, surf, w, h, desc, 31, **{"lin" if to_packed else "lout": lay}, tag=label)


# ---- batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,surf,desc", [("UYVY", "NV12", (T, MEAN)), ("v210", "P010", (R, TL))])
def test_batches_of_distinct_surfaces(gpu, name, surf, desc):
    w, h = 26, 8
    sources = [packed_source(name, w, h, 400 + k) for k in range(32)]
    want = [whole(gpu, surf, packedref.packed_to_yuv(name, p, surf, *desc), w, h) for p, _ in sources]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[2], want[31])
    planes = [random_planes(surf, w, h, 500 + k) for k in range(32)]
    back = [packed_frame(name, packedref.pack(name, packedref.yuv_to_packed(surf, p, name, *desc)), w, h, 0, 16) for p in planes]
    assert not np.array_equal(back[0], back[1]) and not np.array_equal(back[2], back[31])
    for n in (1, 32):
        got = gpu.cvt_packed_to_yuv(packedref.ENUM[name], [b for _, b in sources[:n]], w, h, fmt(surf), desc=desc, raw=True)
        assert len(got) == n and all(np.array_equal(got[k], want[k]) for k in range(n)), (name, surf, n)
        got = gpu.cvt_yuv_to_packed(fmt(surf), [pack(surf, *p) for p in planes[:n]], w, h, packedref.ENUM[name], desc=desc, raw=True)
        assert len(got) == n and all(np.array_equal(got[k], back[k]) for k in range(n)), (surf, name, n)


# ---- v210 as a destination ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surf", ["I210", "I010", "I412", "P010", "NV12"])
def test_v210_padding_fields_and_top_bits_are_zero_and_the_pitch_padding_is_untouched(gpu, surf):
    h = 4
    for w in (2, 4, 8, 26, 50):
        planes = random_planes(surf, w, h, 90 + w)
        row, pitch, size = gpu.packed_layout(capi.PACKED_V210, w, h)
        got = gpu.cvt_yuv_to_packed(fmt(surf), pack(surf, *planes), w, h, capi.PACKED_V210, raw=True)
        assert got.shape == (size + 16,) and pitch % 128 == 0 and row == 16 * ((w + 5) // 6)
        for y in range(h):
            words = got[y * pitch:y * pitch + row].view("<u4")
            assert not (words >> 30).any()
            fields = np.stack([words & 1023, (words >> 10) & 1023, (words >> 20) & 1023], axis=1).reshape(-1, 4, 3)[-1]       # the last group
            # its fields in pixel order: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
            luma = [fields[0][1], fields[1][0], fields[1][2], fields[2][1], fields[3][0], fields[3][2]]
            chroma = [fields[0][0], fields[0][2], fields[1][1], fields[2][0], fields[2][2], fields[3][1]]
            used = w - 6 * ((w - 1) // 6)
            assert not any(luma[used:]) and not any(chroma[used:]), (surf, w, y)
            end = (y + 1) * pitch if y < h - 1 else size + 16
            assert (got[y * pitch + row:end] == FILL).all(), (surf, w, y)
        # a 10-bit low-bit source keeps its word under d = 0 elsewhere; a v210 field takes min(value, 1023)
        rows = np.stack([got[y * pitch:y * pitch + row] for y in range(h)])
        want = packedref.yuv_to_packed(surf, planes, "v210")
        assert all(np.array_equal(g, p) and int(g.max()) <= 1023 for g, p in zip(packedref.unpack("v210", rows, w), want)), (surf, w)


# ---- the identities against the existing operator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,twin,dst", [("UYVY", "I422", "NV12"), ("YUY2", "I422", "I420"), ("YVYU", "I422", "I444"), ("v210", "I210", "P010"),
                                           ("v210", "I210", "NV12"), ("v210", "I210", "I412")])
def test_packed_sources_convert_as_their_deinterleaved_planes(gpu, name, twin, dst):
    for w, h in ((26, 8), (span_px(name) + 2, 4)):
        planes, buf = packed_source(name, w, h, 600)
        for desc in DESCS:
            got = gpu.cvt_packed_to_yuv(packedref.ENUM[name], buf, w, h, fmt(dst), desc=desc, raw=True)
            want = gpu.cvt_yuv_to_yuv(fmt(twin), pack(twin, *planes), w, h, fmt(dst), desc=desc, raw=True)
            assert np.array_equal(got, want), (name, dst, w, h, desc)


def test_round_trips(gpu):
    w, h = 130, 6
    for name, surf in (("UYVY", "I422"), ("YUY2", "I422"), ("YVYU", "I422"), ("Y210", "I212"), ("v210", "I210")):
        planes, buf = packed_source(name, w, h, 62)
        s = gpu.cvt_packed_to_yuv(packedref.ENUM[name], buf, w, h, fmt(surf))
        assert np.array_equal(s, pack(surf, *(p if name != "Y210" else p >> 4 for p in planes)))
        rows = gpu.cvt_yuv_to_packed(fmt(surf), s, w, h, packedref.ENUM[name])
        back = packedref.unpack(name, rows, w)
        assert all(np.array_equal(b, p if name != "Y210" else p >> 4 << 4) for b, p in zip(back, planes)), name
