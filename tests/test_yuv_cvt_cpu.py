"""The conversion between YUV surface formats without a GPU: the numpy statement (tests/yuvref.py) against things it shares nothing
with, the declarations, every refusal of vs_op_cvt_yuv_to_yuv - all decided before a device is looked for, so the fake pointers
below are never read - and vs_yuv_surface_layout, which needs no device at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cvtref
import yuvref
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_op_cvt_yuv_to_yuv", "vs_yuv_surface_layout")
YUV = [capi.PIXFMT_BY_NAME[n] for n in yuvref.FORMATS]
WORDS = np.arange(1 << 16, dtype=np.int64)
WORDS.setflags(write=False)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_declared_exported_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(vs.lib, n) and getattr(vs.lib, n).argtypes, n
    comment = header[:header.index("#define VS_STAB_ABI_VERSION")]
    assert all(n in comment for n in NAMES) and "vs_yuv_cvt_desc" in comment
    assert vs.lib.vs_abi_version() == 2
    assert callable(vs.cvt_yuv_to_yuv) and callable(vs.yuv_surface_layout)
    assert C.sizeof(capi.VsYuvCvtDesc) == 16
    assert (capi.YUV_DEPTH_TRUNCATE, capi.YUV_DEPTH_ROUND) == (0, 1)
    # ... and the C struct itself, with its enum
    prog = ('#include "vs_stab.h"\n'
            'static_assert(sizeof(vs_yuv_cvt_desc) == 16, "size");\n'
            'static_assert(VS_YUV_DEPTH_TRUNCATE == 0 && VS_YUV_DEPTH_ROUND == 1, "enum");\n'
            'static_assert(sizeof(((vs_yuv_cvt_desc*)0)->reserved) == 8, "reserved");\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=prog, text=True, check=True)


def test_the_statements_format_table_is_the_librarys():
    assert sorted(yuvref.FORMATS) == sorted(f.name for f in capi.PIXFMTS if f.kind != capi.KIND_INTERLEAVED) and len(yuvref.FORMATS) == 11
    for name, (b, low, dt, sx, sy) in yuvref.FORMATS.items():
        f = capi.PIXFMT_BY_NAME[name]
        assert (f.sx, f.sy, f.sample_bytes) == (sx, sy, np.dtype(dt).itemsize), name
        assert low == (f.kind == capi.KIND_THREE_PLANES and f.sample_bytes == 2), name
        assert b == (16 if f.kind == capi.KIND_LUMA_UV and f.sample_bytes == 2 else f.bits), name


# ---- the statement against a loop over Python ints --------------------------------------------------------------------------------
def loop_convert(src, planes, dst, depth_down, chroma_down):
    """The header's two steps, sample by sample, on lists of lists of int."""
    b_in, low, _, sxi, syi = yuvref.FORMATS[src]
    b_out, _, _, sxo, syo = yuvref.FORMATS[dst]
    d = b_in - b_out

    def step1(s):
        if d == 0:
            return s
        v = min(s, 2 ** b_in - 1) if low else s
        if d < 0:
            return v * 2 ** -d
        if depth_down == 0:
            return v // 2 ** d
        return min((v + 2 ** (d - 1)) // 2 ** d, 2 ** b_out - 1)

    y, u, v = ([[step1(int(s)) for s in row] for row in p] for p in planes)
    h, w = len(y), len(y[0])

    def step2(c):
        out = []
        for cy in range(h >> syo):
            row = []
            for cx in range(w >> sxo):
                if sxo >= sxi and syo >= syi:
                    bx, by = 2 ** (sxo - sxi), 2 ** (syo - syi)
                    if chroma_down == 0 or bx * by == 1:
                        row.append(c[cy * by][cx * bx])
                    else:
                        total = sum(c[cy * by + j][cx * bx + i] for j in range(by) for i in range(bx))
                        row.append((total + bx * by // 2) // (bx * by))
                else:
                    row.append(c[cy // 2 ** (syi - syo)][cx // 2 ** (sxi - sxo)])
            out.append(row)
        return out
    return y, step2(u), step2(v)


def random_planes(name, w, h, seed):
    """Sample planes of the format's dtype; one sample in eight of a low-bit format has bits above its range."""
    b, low, dt, sx, sy = yuvref.FORMATS[name]
    rng = np.random.default_rng(seed)
    out = []
    for ph, pw in ((h, w), (h >> sy, w >> sx), (h >> sy, w >> sx)):
        s = rng.integers(0, 1 << b, (ph, pw)).astype(dt)
        if low:
            high = (rng.integers(1, 1 << (16 - b), (ph, pw)) << b).astype(dt)
            s = np.where(rng.integers(0, 8, (ph, pw)) == 0, s | high, s).astype(dt)
        out.append(s)
    return out


def test_statement_is_the_loop_for_every_pair_and_descriptor():
    pairs = 0
    for k, src in enumerate(yuvref.FORMATS):
        planes = random_planes(src, 8, 4, 900 + k)
        for dst in yuvref.FORMATS:
            for dd, cd in yuvref.DESCRIPTORS:
                got = yuvref.convert(src, planes, dst, dd, cd)
                want = loop_convert(src, planes, dst, dd, cd)
                for g, wnt in zip(got, want):
                    assert g.dtype == yuvref.FORMATS[dst][2] and g.tolist() == wnt, (src, dst, dd, cd)
            pairs += 1
    assert pairs == 121


# ---- ... against the byte view of the colour conversion ---------------------------------------------------------------------------
def sibling(name):
    _, _, _, sx, sy = yuvref.FORMATS[name]
    if name == "P010":
        return "NV12"
    return {(1, 1): "I420", (1, 0): "I422", (0, 0): "I444"}[(sx, sy)]


def word_planes(values, sx, sy, dt):
    y = np.asarray(values).reshape(256, -1).astype(dt)
    return [y, y[:y.shape[0] >> sy, :y.shape[1] >> sx].copy(), y[y.shape[0] - (y.shape[0] >> sy):, y.shape[1] - (y.shape[1] >> sx):].copy()]


@pytest.mark.parametrize("name", [n for n in yuvref.FORMATS if yuvref.FORMATS[n][2] == np.uint16])
def test_truncation_is_the_byte_the_colour_conversion_reads(name):
    _, _, _, sx, sy = yuvref.FORMATS[name]
    eight = sibling(name)
    planes = word_planes(WORDS, sx, sy, np.uint16)
    for g, p in zip(yuvref.convert(name, planes, eight, yuvref.TRUNCATE, yuvref.TOPLEFT), planes):
        assert g.dtype == np.uint8 and np.array_equal(g, cvtref.sample_to_byte(name, p))
    planes = word_planes(np.arange(256).repeat(256), sx, sy, np.uint8)
    for dd, cd in yuvref.DESCRIPTORS:       # going up takes no rule
        for g, p in zip(yuvref.convert(eight, planes, name, dd, cd), planes):
            assert g.dtype == np.uint16 and np.array_equal(g, cvtref.byte_to_sample(name, p))


def test_up_then_down_is_the_identity():
    low = {8: False, 10: True, 12: True, 16: False}
    pairs = [(lo, hi) for lo in low for hi in low if lo < hi]
    assert len(pairs) == 6
    for lo, hi in pairs:
        v = np.arange(1 << lo, dtype=np.int64)
        up = yuvref.depth(v, lo, low[lo], hi)
        assert int(up.max()) == ((1 << lo) - 1) << (hi - lo)
        for rule in (yuvref.TRUNCATE, yuvref.ROUND):
            assert np.array_equal(yuvref.depth(up, hi, low[hi], lo, rule), v), (lo, hi, rule)


def test_round_saturates_and_rounds_half_up():
    assert int(yuvref.depth(1023, 10, True, 8, yuvref.ROUND)) == 255 and int(yuvref.depth(1021, 10, True, 8, yuvref.ROUND)) == 255
    assert int(yuvref.depth(65535, 16, False, 10, yuvref.ROUND)) == 1023
    assert int(yuvref.depth(4095, 12, True, 10, yuvref.ROUND)) == 1023 and int(yuvref.depth(65535, 16, False, 8, yuvref.ROUND)) == 255
    assert [int(yuvref.depth(s, 10, True, 8, yuvref.ROUND)) for s in (0, 1, 2, 3, 5, 6)] == [0, 0, 1, 1, 1, 2]
    assert [int(yuvref.depth(s, 10, True, 8, yuvref.TRUNCATE)) for s in (0, 1, 2, 3, 5, 6, 1023)] == [0, 0, 0, 0, 1, 1, 255]
    # a low-bit source clamps before anything else; an equal depth copies the word as it is
    assert int(yuvref.depth(0x0400, 10, True, 8)) == 255 and int(yuvref.depth(0xFFFF, 12, True, 16)) == 4095 << 4
    assert int(yuvref.depth(0xFFFF, 10, True, 10)) == 0xFFFF
    assert int(yuvref.depth(0xABCD, 16, False, 8)) == 0xAB and int(yuvref.depth(0xABCD, 16, False, 12)) == 0xABC


def test_mean_of_blocks():
    # sums congruent to 0, 1, 2, 3 modulo 4, and a block of the largest words
    c = np.array([[4, 4, 4, 4, 4, 4, 4, 4, 65535, 65535],
                  [4, 4, 4, 5, 4, 6, 4, 7, 65535, 65535]], np.int64)
    assert yuvref.siting(c, 0, 0, 1, 1, yuvref.MEAN).tolist() == [[4, 4, 5, 5, 65535]]
    assert yuvref.siting(c, 0, 0, 1, 1, yuvref.TOPLEFT).tolist() == [[4, 4, 4, 4, 65535]]
    # one axis: halves round up
    assert yuvref.siting(c, 0, 0, 1, 0, yuvref.MEAN).tolist() == [[4, 4, 4, 4, 65535], [4, 5, 5, 6, 65535]]
    assert yuvref.siting(c, 1, 0, 1, 1, yuvref.MEAN).tolist() == [[4, 4, 4, 5, 4, 5, 4, 6, 65535, 65535]]
    # up: nearest
    assert yuvref.siting(c[:, :2] + np.array([[0, 1], [2, 3]]), 1, 1, 0, 0).tolist() == [[4, 4, 5, 5], [4, 4, 5, 5], [6, 6, 7, 7], [6, 6, 7, 7]]
    assert yuvref.siting(c, 1, 0, 1, 0, yuvref.MEAN) is c


# ---- refusals -------------------------------------------------------------------------------------------------------------------
P, Q = 0x100000, 0x200000        # never read
CALL = "vs_op_cvt_yuv_to_yuv"


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def call(vs, fs, fd, w=8, h=4, lin=None, lout=None, n=1, sp=None, dp=None, src=True, dst=True, lin_ptr=True, lout_ptr=True, desc=None):
    """One call with fake pointers; the defaults are valid for every pair of formats."""
    lin = capi.I420LayoutC(*(lin or (fs.sample_bytes * w, 0, 0, 0)))
    lout = capi.I420LayoutC(*(lout or (fd.sample_bytes * w, 0, 0, 0)))
    s = ptrs(*(sp or [P + 0x1000 * k for k in range(max(n, 1))])) if src else None
    d = ptrs(*(dp or [Q + 0x1000 * k for k in range(max(n, 1))])) if dst else None
    if desc is not None and not isinstance(desc, capi.VsYuvCvtDesc):
        desc = capi.VsYuvCvtDesc(desc[0], desc[1], (C.c_int32 * 2)(*desc[2:]))
    return vs.lib.vs_op_cvt_yuv_to_yuv(fs.fmt, s, C.byref(lin) if lin_ptr else None, fd.fmt, d, C.byref(lout) if lout_ptr else None, n, w, h,
                                       C.byref(desc) if desc is not None else None, None)


def valid(vs, fs, fd, **kw):
    """Valid arguments: without a device the call says so (with one, the fake pointers must not be launched on)."""
    if vs.lib.vs_device_count() > 0:
        return True
    return call(vs, fs, fd, **kw) == 2


def refused(vs, fs, fd, side, **kw):
    """Refused with a text that names the call, the side and that side's format.  side: 0 source, 1 destination, None both."""
    rc = call(vs, fs, fd, **kw)
    text = vs.lib.vs_last_error().decode()
    want = {0: ["source", fs.name], 1: ["destination", fd.name], None: ["source", fs.name, "destination", fd.name]}[side]
    return rc == 1 and text.startswith(CALL + ":") and all(t in text for t in want) and (side is None or ["destination", "source"][side] not in text)


def test_valid_calls_need_a_device(vs):
    for fs in YUV:
        for fd in YUV:
            assert valid(vs, fs, fd), (fs.name, fd.name)
            assert valid(vs, fs, fd, n=32)
            assert valid(vs, fs, fd, desc=(0, 0, 0, 0)) and valid(vs, fs, fd, desc=(1, 1, 0, 0))


@pytest.mark.parametrize("side", [0, 1])
def test_refusals_of_a_side_need_no_device(vs, side):
    for f in YUV:
        other = capi.PIXFMT_BY_NAME["I410" if f.name == "I444" else "I444"]      # takes any size, and is not f
        fs, fd = (f, other) if side == 0 else (other, f)
        key = ("lin", "sp", "src", "lin_ptr") if side == 0 else ("lout", "dp", "dst", "lout_ptr")

        def no(lay=None, p=None, **kw):
            if lay is not None:
                kw[key[0]] = lay
            if p is not None:
                kw[key[1]] = p
            return refused(vs, fs, fd, side, **kw)

        def yes(lay):
            return valid(vs, fs, fd, **{key[0]: lay})
        sb, w, h = f.sample_bytes, 8, 4
        base = P if side == 0 else Q
        # null pointers: the list, an entry, the layout; the count
        assert no(**{key[2]: False}) and no(**{key[3]: False}) and no(p=[base, 0], n=2)
        assert refused(vs, fs, fd, 0, n=0) and refused(vs, fs, fd, 0, n=33) and refused(vs, fs, fd, 0, n=-1)
        # geometry
        assert refused(vs, fs, fd, 0, w=0) and refused(vs, fs, fd, 0, h=0) and refused(vs, fs, fd, 0, w=65537, lin=(4 * 65537, 0, 0, 0))
        if f.sx:
            assert no(w=7, **{key[0]: (sb * 8, 0, 0, 0)})
        if f.sy:
            assert no(h=3)
        assert no(lay=(sb * w - sb, 0, 0, 0))
        # 16-bit samples: pointer, pitch, chroma pitch, offsets
        if sb == 2:
            assert no(p=[base + 1])
            assert no(lay=(sb * w + 1, 0, 0, 0))
            assert no(lay=(sb * w + 4, 0, h * (sb * w + 4) + 1, 0))
            if f.kind == capi.KIND_THREE_PLANES:
                assert no(lay=(sb * w + 4, sb * w + 1, 0, 0))
                assert no(lay=(sb * w + 4, sb * w, 0, 4096 + 1))
        if f.kind == capi.KIND_THREE_PLANES:
            if f.sx:      # a defaulted half chroma pitch needs whole samples in it
                assert no(lay=(sb * w + sb, 0, 0, 0))
                assert yes((sb * w + sb, sb * w, 0, 0))
            crow = sb * (w >> f.sx)
            assert no(lay=(sb * w, crow - sb, 0, 0))
            # planes that overlap: U inside Y, V inside U, V on U
            y_bytes, c_bytes = h * sb * w, (h >> f.sy) * crow
            assert no(lay=(sb * w, 0, y_bytes - 2, 0))
            assert no(lay=(sb * w, 0, y_bytes, y_bytes + c_bytes - 2))
            assert no(lay=(sb * w, 0, y_bytes, y_bytes))
            assert no(lay=(sb * w, 0, y_bytes + c_bytes, y_bytes - 2))
            # YV12 order and planes apart are layouts like any other
            assert yes((sb * w, 0, y_bytes + c_bytes, y_bytes))
            assert yes((sb * w + 8, crow + 2 * sb, y_bytes + 4 * h * sb + 64, 8192))
        else:
            assert no(lay=(sb * w, 0, 0, 2 * h * sb * w))          # v_off must be 0
            assert no(lay=(sb * w + 4, sb * w, 0, 0))              # c_pitch 0 or the pitch
            assert no(lay=(sb * w, 0, h * sb * w - 2, 0))          # the (U, V) plane inside Y
            assert yes((sb * w + 4, sb * w + 4, 4096, 0))
    # a format of the wrong family
    i420 = capi.PIXFMT_BY_NAME["I420"]
    for f in [x for x in capi.PIXFMTS if x.kind == capi.KIND_INTERLEAVED]:
        assert refused(vs, *((f, i420) if side == 0 else (i420, f)), side)
    lay = capi.I420LayoutC(8, 0, 0, 0)
    for bad in (-1, 16, 99):
        fmts = (bad, i420.fmt) if side == 0 else (i420.fmt, bad)
        assert vs.lib.vs_op_cvt_yuv_to_yuv(fmts[0], ptrs(P), C.byref(lay), fmts[1], ptrs(Q), C.byref(lay), 1, 8, 4, None, None) == 1
        text = vs.lib.vs_last_error().decode()
        assert "format %d" % bad in text and ("source", "destination")[side] in text and text.startswith(CALL)


def test_size_must_suit_the_coarser_side(vs):
    f = capi.PIXFMT_BY_NAME
    # w a multiple of 1 << max(sx_in, sx_out), h of 1 << max(sy_in, sy_out): the side that needs it is named
    assert refused(vs, f["I444"], f["I420"], 1, w=7) and refused(vs, f["I420"], f["I410"], 0, w=7, lin=(8, 0, 0, 0))
    assert refused(vs, f["I444"], f["I422"], 1, w=7) and refused(vs, f["I210"], f["I444"], 0, w=7, lin=(16, 0, 0, 0))
    assert refused(vs, f["I422"], f["NV12"], 1, h=3) and refused(vs, f["P010"], f["I422"], 0, h=3)
    assert refused(vs, f["I444"], f["I010"], 1, h=3) and refused(vs, f["I012"], f["I212"], 0, h=5)
    assert valid(vs, f["I444"], f["I412"], w=7, h=3) and valid(vs, f["I422"], f["I210"], w=6, h=3, lin=(8, 4, 0, 0))


def test_equal_pointers_and_descriptors_are_refused(vs):
    for fs, fd in ((capi.PIXFMT_BY_NAME[a], capi.PIXFMT_BY_NAME[b]) for a, b in (("I420", "NV12"), ("I210", "P010"), ("I422", "I422"), ("P010", "I444"))):
        assert refused(vs, fs, fd, None, sp=[P], dp=[P])
        assert refused(vs, fs, fd, None, n=3, sp=[P, P + 0x1000, P + 0x2000], dp=[Q, Q + 0x1000, P + 0x1000])
        assert refused(vs, fs, fd, None, n=2, sp=[P, Q], dp=[Q, Q + 0x1000])
        assert valid(vs, fs, fd, n=2, sp=[P, P], dp=[Q, Q + 0x1000])         # a source may be read twice
        for desc, field in (((2, 0, 0, 0), "depth_down"), ((-1, 0, 0, 0), "depth_down"), ((0, 2, 0, 0), "chroma_down"), ((0, -1, 0, 0), "chroma_down"),
                            ((0, 0, 1, 0), "reserved"), ((0, 0, 0, 1), "reserved"), ((1, 1, 0, -1), "reserved")):
            assert refused(vs, fs, fd, None, desc=desc), desc
            assert field in vs.lib.vs_last_error().decode()


# ---- vs_yuv_surface_layout --------------------------------------------------------------------------------------------------------
def test_surface_layout_defaults_and_sizes(vs):
    for f in YUV:
        sb = f.sample_bytes
        for w, h in ((24, 8), (2, 2), (3840, 2160)):
            packed = capi.fmt_frame_rows(f.fmt, h) * w * sb
            for lay in (None, (sb * w,), (sb * w, 0, 0, 0)):
                got, nbytes = vs.yuv_surface_layout(f.fmt, w, h, lay)
                if f.kind == capi.KIND_THREE_PLANES:
                    assert got == synth.yuv_layout(w, h, f.sx, f.sy, sb), (f.name, w, h)
                else:
                    assert got == (sb * w, sb * w, h * sb * w, 0), (f.name, w, h)
                assert nbytes == packed, (f.name, w, h)
            # a resolved layout says the same when handed back
            assert vs.yuv_surface_layout(f.fmt, w, h, got) == (got, nbytes)
        # padded rows: the bytes end with the last sample, not with its row's padding
        w, h = 24, 8
        pitch = sb * w + 8
        got, nbytes = vs.yuv_surface_layout(f.fmt, w, h, (pitch,))
        if f.kind == capi.KIND_THREE_PLANES:
            want = synth.yuv_layout(w, h, f.sx, f.sy, sb, pitch)
            assert got == want
            assert nbytes == want[3] + ((h >> f.sy) - 1) * want[1] + sb * (w >> f.sx)
        else:
            assert got == (pitch, pitch, h * pitch, 0) and nbytes == h * pitch + (h // 2 - 1) * pitch + sb * w
        # either result may be left out
        assert vs.lib.vs_yuv_surface_layout(f.fmt, w, h, None, None, None) == 0
        n = C.c_size_t()
        assert vs.lib.vs_yuv_surface_layout(f.fmt, w, h, None, None, C.byref(n)) == 0 and n.value == capi.fmt_frame_rows(f.fmt, h) * w * sb


def test_surface_layout_explicit_offsets(vs):
    w, h = 24, 8
    for name in ("I420", "I010", "I422", "I212", "I444"):
        f = capi.PIXFMT_BY_NAME[name]
        sb = f.sample_bytes
        pitch, cp, y_bytes, c_bytes = synth.yuv_layout(w, h, f.sx, f.sy, sb)[:2] + (h * sb * w, (h >> f.sy) * sb * (w >> f.sx))
        # YV12 order: V behind the luma rows, U behind V
        got, nbytes = vs.yuv_surface_layout(f.fmt, w, h, (pitch, 0, y_bytes + c_bytes, y_bytes))
        assert got == synth.yuv_layout(w, h, f.sx, f.sy, sb, None, None, y_bytes + c_bytes, y_bytes) == (pitch, cp, y_bytes + c_bytes, y_bytes)
        assert nbytes == y_bytes + 2 * c_bytes
        # planes apart, a chroma pitch of its own
        lay = (pitch + 8, cp + 2 * sb, y_bytes + 8 * h + 64, 8192)
        got, nbytes = vs.yuv_surface_layout(f.fmt, w, h, lay)
        assert got == lay == synth.yuv_layout(w, h, f.sx, f.sy, sb, *lay)
        assert nbytes == 8192 + ((h >> f.sy) - 1) * lay[1] + sb * (w >> f.sx)
    nv12 = capi.PIXFMT_BY_NAME["NV12"]
    assert vs.yuv_surface_layout(nv12.fmt, w, h, (w + 4, w + 4, 4096, 0)) == ((w + 4, w + 4, 4096, 0), 4096 + (h // 2 - 1) * (w + 4) + w)


def test_surface_layout_refuses_what_the_conversion_refuses(vs):
    def no(f, w, h, lay):
        rc = vs.lib.vs_yuv_surface_layout(f.fmt if hasattr(f, "fmt") else f, w, h, C.byref(capi.I420LayoutC(*lay)) if lay else None, None, None)
        text = vs.lib.vs_last_error().decode()
        return rc == 1 and text.startswith("vs_yuv_surface_layout:") and (f.name if hasattr(f, "name") else "format %d" % f) in text
    for f in YUV:
        sb, w, h = f.sample_bytes, 8, 4
        assert no(f, 0, 4, None) and no(f, 8, 0, None) and no(f, 65537, 4, None) and no(f, 8, 4, (sb * w - sb,))
        if f.sx:
            assert no(f, 7, 4, None)
        if f.sy:
            assert no(f, 8, 3, None)
        if sb == 2:
            assert no(f, w, h, (sb * w + 1,)) and no(f, w, h, (sb * w + 4, 0, h * (sb * w + 4) + 1, 0))
        if f.kind == capi.KIND_THREE_PLANES:
            y_bytes = h * sb * w
            if f.sx:
                assert no(f, w, h, (sb * w + sb,))
            assert no(f, w, h, (sb * w, sb * (w >> f.sx) - sb)) and no(f, w, h, (sb * w, 0, y_bytes - 2, 0)) and no(f, w, h, (sb * w, 0, y_bytes, y_bytes))
        else:
            assert no(f, w, h, (sb * w, 0, 0, 2 * h * sb * w)) and no(f, w, h, (sb * w + 4, sb * w, 0, 0)) and no(f, w, h, (sb * w, 0, h * sb * w - 2, 0))
    for f in [x for x in capi.PIXFMTS if x.kind == capi.KIND_INTERLEAVED]:
        assert no(f, 8, 4, None)
    for bad in (-1, 16, 99):
        assert no(bad, 8, 4, None)
