"""The packed 4:2:2 capture formats without a GPU: the declarations, every refusal of vs_op_cvt_packed_to_yuv and
vs_op_cvt_yuv_to_packed - all decided before a device is looked for, so the fake pointers below are never read -, vs_packed_layout,
which needs no device at all, and the numpy statement (tests/packedref.py) against things it shares no code with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import packedref
import yuvref
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_op_cvt_packed_to_yuv", "vs_op_cvt_yuv_to_packed", "vs_packed_layout")
PACKED = list(packedref.FORMATS)
YUV = [capi.PIXFMT_BY_NAME[n] for n in yuvref.FORMATS]
T, R, TL, MEAN = yuvref.TRUNCATE, yuvref.ROUND, yuvref.TOPLEFT, yuvref.MEAN


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_declared_exported_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(vs.lib, n) and getattr(vs.lib, n).argtypes, n
    comment = header[:header.index("#define VS_STAB_ABI_VERSION")]
    assert all(n in comment for n in NAMES) and "vs_packed_fmt" in comment
    assert vs.lib.vs_abi_version() == 2
    assert callable(vs.cvt_packed_to_yuv) and callable(vs.cvt_yuv_to_packed) and callable(vs.packed_layout)
    assert (capi.PACKED_YUY2, capi.PACKED_UYVY, capi.PACKED_YVYU, capi.PACKED_Y210, capi.PACKED_V210) == (0, 1, 2, 3, 4)
    assert capi.PACKED_BY_NAME == packedref.ENUM
    prog = ('#include "vs_stab.h"\n'
            'static_assert(VS_PACKED_YUY2 == 0 && VS_PACKED_UYVY == 1 && VS_PACKED_YVYU == 2 && VS_PACKED_Y210 == 3 && VS_PACKED_V210 == 4, "enum");\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=prog, text=True, check=True)


def test_the_packed_formats_are_no_pixel_formats():
    assert not set(PACKED) & {f.name for f in capi.PIXFMTS} and len(capi.PIXFMTS) == 16


# ---- the statement against things it shares no code with ------------------------------------------------------------------------
def test_v210_known_answer():
    y = np.arange(0x040, 0x046, dtype=np.uint16)[None]
    cb, cr = np.array([[0x200, 0x201, 0x202]], np.uint16), np.array([[0x300, 0x301, 0x302]], np.uint16)
    rows = packedref.pack("v210", (y, cb, cr))
    assert rows.dtype == np.uint8 and rows.shape == (1, 16)
    assert rows.view("<u4").tolist() == [[0x30010200, 0x04280441, 0x20210F01, 0x045C0844]]
    got = packedref.unpack("v210", rows, 6)
    assert all(np.array_equal(g, p) and g.dtype == np.uint16 for g, p in zip(got, (y, cb, cr)))


def loop_pack(name, y, u, v):
    """The header's memory layouts, pixel by pixel, on lists of int -> the bytes of every row."""
    rows = []
    for r in range(len(y)):
        w = len(y[r])
        if name == "v210":
            words = [0] * (4 * ((w + 5) // 6))
            for x in range(w):                          # luma of pixel x: group x // 6, place x % 6
                word, shift = [(0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20)][x % 6]
                words[4 * (x // 6) + word] |= y[r][x] << shift
            for c in range(w // 2):                     # chroma pair c: group c // 3, place c % 3
                (uw, us), (vw, vs_) = [((0, 0), (0, 20)), ((1, 10), (2, 0)), ((2, 20), (3, 10))][c % 3]
                words[4 * (c // 3) + uw] |= u[r][c] << us
                words[4 * (c // 3) + vw] |= v[r][c] << vs_
            rows.append([(wd >> (8 * b)) & 255 for wd in words for b in range(4)])
            continue
        row = []
        for c in range(w // 2):
            macro = {"YUY2": (y[r][2 * c], u[r][c], y[r][2 * c + 1], v[r][c]), "UYVY": (u[r][c], y[r][2 * c], v[r][c], y[r][2 * c + 1]),
                     "YVYU": (y[r][2 * c], v[r][c], y[r][2 * c + 1], u[r][c]), "Y210": (y[r][2 * c], u[r][c], y[r][2 * c + 1], v[r][c])}[name]
            for s in macro:
                row += [s & 255, s >> 8] if name == "Y210" else [s]
        rows.append(row)
    return rows


@pytest.mark.parametrize("name", PACKED)
def test_statement_is_the_loop(name):
    w, h = 10, 3
    planes = packedref.random_planes(name, w, h, 7)
    rows = packedref.pack(name, planes)
    assert rows.shape == (h, packedref.row_bytes(name, w)) and rows.tolist() == loop_pack(name, *(p.tolist() for p in planes))
    for g, p in zip(packedref.unpack(name, rows, w), planes):
        assert g.dtype == p.dtype and np.array_equal(g, p)


@pytest.mark.parametrize("name", PACKED)
def test_unpack_of_pack_is_the_identity(name):
    for w in (2, 4, 6, 8, 46, 48, 50):
        planes = packedref.random_planes(name, w, 2, 100 + w)
        rows = packedref.pack(name, planes)
        assert rows.shape == (2, packedref.row_bytes(name, w))
        assert all(np.array_equal(g, p) for g, p in zip(packedref.unpack(name, rows, w), planes)), (name, w)
        wide = np.concatenate([rows, np.full((2, 5), 0xA5, np.uint8)], axis=1)          # a pitch beyond the row is not looked at
        assert all(np.array_equal(g, p) for g, p in zip(packedref.unpack(name, wide, w), planes)), (name, w)


def test_v210_words_with_zero_padding_come_back_and_the_top_bits_are_ignored():
    rng = np.random.default_rng(5)
    for w in (6, 12, 48):
        words = rng.integers(0, 1 << 30, (3, 4 * (w // 6)), dtype=np.uint32).astype("<u4")
        rows = words.view(np.uint8)
        planes = packedref.unpack("v210", rows, w)
        assert np.array_equal(packedref.pack("v210", planes), rows)
        noisy = (words | rng.integers(0, 4, words.shape, dtype=np.uint32) << 30).astype("<u4")
        assert (noisy >> 30).any()
        assert all(np.array_equal(g, p) for g, p in zip(packedref.unpack("v210", noisy.view(np.uint8), w), planes))
    # a partial last group: the fields of pixels >= w are ignored on the way in and 0 on the way out
    words = rng.integers(0, 1 << 32, (2, 8), dtype=np.uint32).astype("<u4")
    planes = packedref.unpack("v210", words.view(np.uint8), 8)
    back = packedref.pack("v210", planes).view("<u4")
    assert np.array_equal(back[:, :4], words[:, :4] & 0x3FFFFFFF)
    # pixels 6, 7: Cb2 Y6 Cr2 in word 4, Y7 in the low field of word 5; the rest of the group is 0
    assert np.array_equal(back[:, 4], words[:, 4] & 0x3FFFFFFF) and np.array_equal(back[:, 5], words[:, 5] & 1023) and not back[:, 6:].any()


def deinterleaved(name, w, h, seed):
    """Planes of a packed format, its rows, and the surface format that holds the same samples as planes."""
    planes = packedref.random_planes(name, w, h, seed)
    return planes, packedref.pack(name, planes), {8: "I422", 10: "I210"}.get(packedref.FORMATS[name][0])


@pytest.mark.parametrize("name", ["YUY2", "UYVY", "YVYU", "v210"])
def test_packed_sources_are_i422_and_i210(name):
    w, h = 12, 4
    planes, rows, twin = deinterleaved(name, w, h, 11)
    for dst in yuvref.FORMATS:
        for dd, cd in yuvref.DESCRIPTORS:
            got = packedref.packed_to_yuv(name, packedref.unpack(name, rows, w), dst, dd, cd)
            want = yuvref.convert(twin, planes, dst, dd, cd)
            assert all(np.array_equal(g, p) and g.dtype == p.dtype for g, p in zip(got, want)), (name, dst, dd, cd)


def test_packed_destinations_are_i422_and_i210_but_for_the_ten_bits_of_a_field():
    w, h = 12, 4
    from test_yuv_cvt_cpu import random_planes
    for k, src in enumerate(yuvref.FORMATS):
        planes = random_planes(src, w, h, 20 + k)
        for dd, cd in yuvref.DESCRIPTORS:
            want8, want10 = yuvref.convert(src, planes, "I422", dd, cd), yuvref.convert(src, planes, "I210", dd, cd)
            for name in ("YUY2", "UYVY", "YVYU"):
                assert all(np.array_equal(g, p) for g, p in zip(packedref.yuv_to_packed(src, planes, name, dd, cd), want8)), (src, name)
            got = packedref.yuv_to_packed(src, planes, "v210", dd, cd)
            if yuvref.FORMATS[src][0] == 10:       # d = 0 copies the word, out-of-range high bits and all: the field clamps them, in step 1
                assert any((p > 1023).any() for p in want10) and all(g.max() <= 1023 for g in got)
                want10 = yuvref.convert(src, [np.minimum(p, 1023) for p in planes], "I210", dd, cd)
            assert all(np.array_equal(g, p) for g, p in zip(got, want10)), src
    # Y210 is a 16-bit 4:2:2 format, the whole word: from P010 only the siting moves
    planes = random_planes("P010", w, h, 40)
    y, u, v = packedref.yuv_to_packed("P010", planes, "Y210")
    assert np.array_equal(y, planes[0]) and np.array_equal(u[0::2], planes[1]) and np.array_equal(u[1::2], planes[1]) and np.array_equal(v[1::2], planes[2])
    back = packedref.packed_to_yuv("Y210", (y, u, v), "P010", R, MEAN)
    assert all(np.array_equal(g, p) for g, p in zip(back, planes))
    assert int(packedref.packed_to_yuv("Y210", [np.full((2, 2), 0xABCD, np.uint16), np.full((2, 1), 0xFFFF, np.uint16), np.zeros((2, 1), np.uint16)],
                                       "I010", R, TL)[1][0, 0]) == 1023


# ---- refusals -------------------------------------------------------------------------------------------------------------------
P, Q = 0x100000, 0x200000        # never read
TO_YUV, TO_PACKED = "vs_op_cvt_packed_to_yuv", "vs_op_cvt_yuv_to_packed"


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


class _Fmt:
    """A surface format number that is none, for call()."""
    sample_bytes = 1

    def __init__(self, fmt):
        self.fmt, self.name = fmt, "format %d" % fmt


def call(vs, to_packed, packed, f, w=8, h=4, pitch=0, lay=None, n=1, pp=None, sp=None, packed_list=True, surface_list=True, lay_ptr=True, desc=None):
    """One call with fake pointers; the defaults are valid for every pairing.  packed: a name or a number; pp, sp: the packed and
    the surface pointers.  -> (status, text)"""
    lay = capi.I420LayoutC(*(lay or (f.sample_bytes * w, 0, 0, 0)))
    a = ptrs(*(pp or [P + 0x1000 * k for k in range(max(n, 1))])) if packed_list else None
    b = ptrs(*(sp or [Q + 0x1000 * k for k in range(max(n, 1))])) if surface_list else None
    if desc is not None:
        desc = C.byref(capi.VsYuvCvtDesc(desc[0], desc[1], (C.c_int32 * 2)(*desc[2:])))
    pf = packedref.ENUM.get(packed, packed)
    lp = C.byref(lay) if lay_ptr else None
    if to_packed:
        rc = vs.lib.vs_op_cvt_yuv_to_packed(f.fmt, b, lp, pf, a, pitch, n, w, h, desc, None)
    else:
        rc = vs.lib.vs_op_cvt_packed_to_yuv(pf, a, pitch, f.fmt, b, lp, n, w, h, desc, None)
    return rc, vs.lib.vs_last_error().decode()


def valid(vs, to_packed, packed, f, **kw):
    """Valid arguments: without a device the call says so (with one, the fake pointers must not be launched on)."""
    if vs.lib.vs_device_count() > 0:
        return True
    return call(vs, to_packed, packed, f, **kw)[0] == 2


def refused(vs, to_packed, packed, f, packed_side, **kw):
    """Refused with a text that names the call, the side and that side's format.  packed_side: True, False, or None for both."""
    rc, text = call(vs, to_packed, packed, f, **kw)
    sides = {True: "destination" if to_packed else "source", False: "source" if to_packed else "destination"}
    pname = packed if isinstance(packed, str) else "packed format %d" % packed
    want = {True: [sides[True], pname], False: [sides[False], f.name], None: ["source", "destination", pname, f.name]}[packed_side]
    return rc == 1 and text.startswith((TO_PACKED if to_packed else TO_YUV) + ":") and all(t in text for t in want) and \
        (packed_side is None or sides[not packed_side] not in text)


@pytest.mark.parametrize("to_packed", [False, True])
def test_valid_calls_need_a_device(vs, to_packed):
    for name in PACKED:
        for f in YUV:
            assert valid(vs, to_packed, name, f), (name, f.name)
            assert valid(vs, to_packed, name, f, n=32) and valid(vs, to_packed, name, f, desc=(1, 1, 0, 0)) and valid(vs, to_packed, name, f, desc=(0, 0, 0, 0))
        i422 = capi.PIXFMT_BY_NAME["I422"]
        # any even w (v210: no multiple of 6), any h for a 4:2:2 surface; a pitch beyond the row; the alignment the format asks for
        a = packedref.ALIGN[name]
        assert valid(vs, to_packed, name, i422, w=2, h=1, lay=(2, 1, 0, 0)) and valid(vs, to_packed, name, i422, w=50, h=3, lay=(50, 25, 0, 0))
        assert valid(vs, to_packed, name, i422, pitch=packedref.row_bytes(name, 8) + a, pp=[P + a])
        assert valid(vs, to_packed, name, i422, pitch=packedref.row_bytes(name, 8))
        assert valid(vs, to_packed, name, i422, n=2, pp=[P, P + 4096], sp=[Q, Q + 4096])


@pytest.mark.parametrize("to_packed", [False, True])
def test_refusals_of_the_packed_side_need_no_device(vs, to_packed):
    i444 = capi.PIXFMT_BY_NAME["I444"]
    for name in PACKED:
        def no(**kw):
            return refused(vs, to_packed, name, i444, True, **kw)
        row, a = packedref.row_bytes(name, 8), packedref.ALIGN[name]
        assert no(packed_list=False) and no(pp=[P, 0], n=2) and no(pp=[0])
        # the count and the size belong to neither side: the source, checked first, is named
        for kw, why in (({"n": 0}, "n must be 1 .. 32"), ({"n": 33}, "n must be 1 .. 32"), ({"n": -1}, "n must be 1 .. 32"), ({"w": 0}, "size out of range"),
                        ({"h": 0}, "size out of range"), ({"w": 65538, "lay": (65538, 0, 0, 0)}, "size out of range"), ({"h": 65537}, "size out of range")):
            rc, text = call(vs, to_packed, name, i444, **kw)
            assert rc == 1 and text.startswith((TO_PACKED if to_packed else TO_YUV) + ": source") and why in text, (kw, text)
        assert no(w=7) and no(w=9, lay=(10, 0, 0, 0))
        assert no(pitch=row - a) and no(pitch=1)
        if a > 1:
            assert no(pp=[P + 1]) and no(pitch=row + 1) and no(pp=[P + a // 2]) and no(pitch=row + a // 2) and no(n=2, pp=[P, P + 4096 + 1])
            assert "multiples of 4" in vs.lib.vs_last_error().decode() if name == "v210" else "even" in vs.lib.vs_last_error().decode()
        else:
            assert valid(vs, to_packed, name, i444, pp=[P + 1], pitch=row + 1)
    # v210: a row is whole groups of 16 bytes, and the default pitch is the format's own
    assert refused(vs, to_packed, "v210", i444, True, w=8, pitch=16) and valid(vs, to_packed, "v210", i444, w=8, pitch=32)
    assert refused(vs, to_packed, "v210", i444, True, w=50, lay=(50, 0, 0, 0), pitch=128) and valid(vs, to_packed, "v210", i444, w=50, lay=(50, 0, 0, 0), pitch=144)
    for bad in (-1, 5, 99):
        assert refused(vs, to_packed, bad, i444, True)


@pytest.mark.parametrize("to_packed", [False, True])
def test_refusals_of_the_surface_side_are_those_of_the_surface_conversion(vs, to_packed):
    for name in ("UYVY", "v210"):
        for f in YUV:
            def no(**kw):
                return refused(vs, to_packed, name, f, False, **kw)
            sb, w, h = f.sample_bytes, 8, 4
            assert no(surface_list=False) and no(lay_ptr=False) and no(sp=[Q, 0], n=2)
            assert no(lay=(sb * w - sb, 0, 0, 0))
            if f.sy:
                assert no(h=3)
            if sb == 2:
                assert no(sp=[Q + 1]) and no(lay=(sb * w + 1, 0, 0, 0))
            if f.kind == capi.KIND_THREE_PLANES:
                y_bytes = h * sb * w
                assert no(lay=(sb * w, sb * (w >> f.sx) - sb, 0, 0)) and no(lay=(sb * w, 0, y_bytes - 2, 0)) and no(lay=(sb * w, 0, y_bytes, y_bytes))
            else:
                assert no(lay=(sb * w, 0, 0, 2 * h * sb * w)) and no(lay=(sb * w + 4, sb * w, 0, 0))
        i420 = capi.PIXFMT_BY_NAME["I420"]
        for f in [x for x in capi.PIXFMTS if x.kind == capi.KIND_INTERLEAVED]:
            assert refused(vs, to_packed, name, f, False)
        for bad in (-1, 16, 99):
            rc, text = call(vs, to_packed, name, _Fmt(bad))
            assert rc == 1 and "format %d" % bad in text and ("source" if to_packed else "destination") in text and text.startswith(TO_PACKED if to_packed else TO_YUV)
        assert valid(vs, to_packed, name, i420)


@pytest.mark.parametrize("to_packed", [False, True])
def test_equal_pointers_and_descriptors_are_refused(vs, to_packed):
    for name, f in (("YUY2", capi.PIXFMT_BY_NAME["NV12"]), ("Y210", capi.PIXFMT_BY_NAME["P010"]), ("v210", capi.PIXFMT_BY_NAME["I422"])):
        assert refused(vs, to_packed, name, f, None, pp=[P], sp=[P])
        assert refused(vs, to_packed, name, f, None, n=3, pp=[P, P + 0x1000, P + 0x2000], sp=[Q, Q + 0x1000, P + 0x1000])
        assert valid(vs, to_packed, name, f, n=2, pp=[P, P + 0x1000], sp=[Q, Q + 0x1000])
        for desc, field in (((2, 0, 0, 0), "depth_down"), ((-1, 0, 0, 0), "depth_down"), ((0, 2, 0, 0), "chroma_down"), ((0, -1, 0, 0), "chroma_down"),
                            ((0, 0, 1, 0), "reserved"), ((0, 0, 0, 1), "reserved"), ((1, 1, 0, -1), "reserved")):
            assert refused(vs, to_packed, name, f, None, desc=desc), desc
            assert field in vs.lib.vs_last_error().decode()


# ---- vs_packed_layout -------------------------------------------------------------------------------------------------------------
WIDTHS = (2, 6, 8, 46, 48, 50)


def test_packed_layout(vs):
    h = 5
    v210 = dict(zip(WIDTHS, ((16, 128), (16, 128), (32, 128), (128, 128), (128, 128), (144, 256))))
    for w in WIDTHS:
        for name, (row, pitch) in (("YUY2", (2 * w, 2 * w)), ("UYVY", (2 * w, 2 * w)), ("YVYU", (2 * w, 2 * w)), ("Y210", (4 * w, 4 * w)), ("v210", v210[w])):
            assert (row, pitch) == (packedref.row_bytes(name, w), packedref.default_pitch(name, w))
            assert vs.packed_layout(packedref.ENUM[name], w, h) == (row, pitch, (h - 1) * pitch + row), (name, w)
            assert vs.packed_layout(packedref.ENUM[name], w, 1) == (row, pitch, row)
            p = row + 8
            assert vs.packed_layout(packedref.ENUM[name], w, h, p) == (row, p, (h - 1) * p + row)
            assert vs.packed_layout(packedref.ENUM[name], w, h, row) == (row, row, h * row)
    # each result may be left out
    assert vs.lib.vs_packed_layout(4, 8, 4, 0, None, None, None) == 0
    n = C.c_size_t()
    assert vs.lib.vs_packed_layout(4, 50, 2, 0, None, None, C.byref(n)) == 0 and n.value == 256 + 144


def test_packed_layout_refuses_what_the_operators_refuse(vs):
    def no(fmt, w, h, pitch=0):
        rc = vs.lib.vs_packed_layout(packedref.ENUM.get(fmt, fmt), w, h, pitch, None, None, None)
        text = vs.lib.vs_last_error().decode()
        return rc == 1 and text.startswith("vs_packed_layout:") and (fmt if isinstance(fmt, str) else "packed format %d" % fmt) in text
    for name in PACKED:
        row, a = packedref.row_bytes(name, 8), packedref.ALIGN[name]
        assert no(name, 0, 4) and no(name, 8, 0) and no(name, 7, 4) and no(name, 65538, 4) and no(name, 8, 65537) and no(name, 8, 4, row - a)
        if a > 1:
            assert no(name, 8, 4, row + 1) and no(name, 8, 4, row + a // 2)
    for bad in (-1, 5, 99):
        assert no(bad, 8, 4)
