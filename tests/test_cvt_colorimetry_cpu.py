"""The colour space of the conversions without a GPU: the declarations; the integers of vs_cvt_coefficients against OpenCV's (the
default) and against the rule of include/vs_stab.h recomputed here with fractions.Fraction (the other five combinations); every
refusal of a descriptor - decided before a device is looked for, so the fake pointers below are never read -; the guess for
untagged video; and the numpy statement tests/cvtref_cs.py against the float64 textbook formulas, the grey axis, tests/cvtref.py
and the properties of mean chroma."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cvtref
import cvtref_cs as cs
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_op_cvt_yuv_to_rgb_cs", "vs_op_cvt_rgb_to_yuv_cs", "vs_enh_set_yuv_colorimetry", "vs_cvt_coefficients")
COMBOS = cs.COMBINATIONS
NEW = cs.NEW_COMBINATIONS


def combo_id(c):
    return "%s-%s" % (cs.MATRIX_NAMES[c[0]], cs.RANGE_NAMES[c[1]])


@pytest.fixture(scope="module")
def sweep():
    """Every (a, b, c) triple once, as flat uint8 arrays (shared, read-only)."""
    planes = tuple(p.reshape(-1) for p in cvtref.all_triples())
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.fixture(scope="module", autouse=True)
def statement_is_the_librarys(vs):
    """Everything below speaks about ONE set of integers: those of tests/cvtref_cs.py are the library's, for all six combinations."""
    for combo in COMBOS:
        assert vs.cvt_coefficients(combo).tolist()[:15] == list(cs.coefficients(*combo)), combo_id(combo)


# ---- declarations -----------------------------------------------------------------------------------------------------------------
def test_declared_exported_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(vs.lib, n) and getattr(vs.lib, n).argtypes, n
    assert re.search(r"\bvoid\s+vs_cvt_colorimetry_guess\s*\(", code)
    assert vs.lib.vs_cvt_colorimetry_guess.argtypes
    comment = header[:header.index("#define VS_STAB_ABI_VERSION")]
    assert all(n in comment for n in NAMES + ("vs_cvt_colorimetry_guess",))
    assert vs.lib.vs_abi_version() == 2
    # the struct and the enums as the header states them
    m = re.search(r"typedef\s+struct\s+vs_cvt_colorimetry\s*\{\s*int32_t\s+matrix\s*,\s*range\s*,\s*chroma_down\s*,\s*reserved\s*;\s*\}", code)
    assert m
    assert C.sizeof(capi.CvtColorimetry) == 16 and [f[0] for f in capi.CvtColorimetry._fields_] == ["matrix", "range", "chroma_down", "reserved"]
    for name, value in (("VS_CVT_MATRIX_BT601", 0), ("VS_CVT_MATRIX_BT709", 1), ("VS_CVT_MATRIX_BT2020", 2), ("VS_CVT_RANGE_LIMITED", 0),
                        ("VS_CVT_RANGE_FULL", 1), ("VS_CVT_CHROMA_TOPLEFT", 0), ("VS_CVT_CHROMA_MEAN", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), code), name
    assert (capi.CVT_MATRIX_BT601, capi.CVT_MATRIX_BT709, capi.CVT_MATRIX_BT2020) == (cs.BT601, cs.BT709, cs.BT2020)
    assert (capi.CVT_RANGE_LIMITED, capi.CVT_RANGE_FULL, capi.CVT_CHROMA_TOPLEFT, capi.CVT_CHROMA_MEAN) == (cs.LIMITED, cs.FULL, cs.TOPLEFT, cs.MEAN)
    # the Python side: the keyword of the two operators, the object's setting, the two host functions
    import inspect
    assert inspect.signature(vs.cvt_yuv_to_rgb).parameters["colorimetry"].default is None
    assert inspect.signature(vs.cvt_rgb_to_yuv).parameters["colorimetry"].default is None
    assert callable(capi.Enhancer.set_yuv_colorimetry) and callable(vs.cvt_coefficients) and callable(vs.cvt_colorimetry_guess)


# ---- the integers -----------------------------------------------------------------------------------------------------------------
def test_default_coefficients_are_opencvs(vs):
    # the fifteen constants of tests/cvtref.py, read off its formulas
    want = [16, 1220542, 1673527, 852492, 409993, 2116026, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448, 0]
    src = open(os.path.join(ROOT, "tests", "cvtref.py")).read()
    for v in want[1:15]:
        assert re.search(r"(?<!\d)%d(?!\d)" % abs(v), src), v
    assert vs.cvt_coefficients().tolist() == want
    assert vs.cvt_coefficients((0, 0, 0, 0)).tolist() == want
    assert vs.cvt_coefficients((cs.BT601, cs.LIMITED, cs.MEAN)).tolist() == want       # the chroma rule is no coefficient
    # ... and they are what cvtref computes with: one probe per coefficient
    k = want
    y, u, v = cvtref.rgb_to_yuv_unclamped(np.array([1, 0, 0]), np.array([0, 1, 0]), np.array([0, 0, 1]))
    base = cvtref.H + (16 << 20), cvtref.H + (128 << 20)
    assert [(base[0] + c) >> 20 for c in k[6:9]] == y.tolist()
    assert [(base[1] + c) >> 20 for c in k[9:12]] == u.tolist() and [(base[1] + c) >> 20 for c in k[12:15]] == v.tolist()
    r, g, b = cvtref.yuv_to_rgb_unclamped(np.array([17, 16, 16]), np.array([128, 129, 128]), np.array([128, 128, 129]))
    assert r.tolist() == [(k[1] + cvtref.H) >> 20, cvtref.H >> 20, (cvtref.H + k[2]) >> 20]
    assert g.tolist() == [(k[1] + cvtref.H) >> 20, (cvtref.H - k[4]) >> 20, (cvtref.H - k[3]) >> 20]
    assert b.tolist() == [(k[1] + cvtref.H) >> 20, (cvtref.H + k[5]) >> 20, cvtref.H >> 20]


def rule(matrix, rng):
    """The rule of the header, recomputed here: Kr, Kb -> fifteen integers."""
    kr, kb = {0: (Fraction(299, 1000), Fraction(114, 1000)), 1: (Fraction(2126, 10000), Fraction(722, 10000)),
              2: (Fraction(2627, 10000), Fraction(593, 10000))}[matrix]
    kg = 1 - kr - kb
    ys, sc, y_off = (Fraction(219, 255), Fraction(224, 255), 16) if rng == 0 else (Fraction(1), Fraction(1), 0)
    vals = [1 / ys, 2 * (1 - kr) / sc, 2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) * kb / kg / sc, 2 * (1 - kb) / sc,
            kr * ys, kg * ys, kb * ys,
            -kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, sc / 2,
            sc / 2, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]

    def rnd(q):        # half away from zero
        q = q * (1 << 20)
        n = (2 * abs(q.numerator) + q.denominator) // (2 * q.denominator)
        return n if q >= 0 else -n
    return [y_off] + [rnd(x) for x in vals]


# the table of the issue this feature was built from, for cross-checking the recomputation (the rule wins)
TABLE = {
    (0, 1): [0, 1048576, 1470104, 748826, 360853, 1858077, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262],
    (1, 0): [16, 1220945, 1879825, 558796, 223607, 2215014, 191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230],
    (1, 1): [0, 1048576, 1651297, 490864, 196424, 1945738, 222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074],
    (2, 0): [16, 1220945, 1760217, 682019, 196426, 2245811, 236572, 610567, 53402, -128614, -331937, 460551, 460551, -423510, -37041],
    (2, 1): [0, 1048576, 1546230, 599107, 172546, 1972791, 275461, 710935, 62181, -146413, -377875, 524288, 524288, -482120, -42168],
}


@pytest.mark.parametrize("combo", NEW, ids=combo_id)
def test_coefficients_follow_the_rule(vs, combo):
    want = rule(*combo)
    assert want == TABLE[combo]
    for chroma in (cs.TOPLEFT, cs.MEAN):
        got = vs.cvt_coefficients(combo + (chroma,)).tolist()
        assert got[:15] == want and got[15] == 0
    assert list(cs.coefficients(*combo)) == want
    assert sum(want[9:12]) == 0 and sum(want[12:15]) == 0
    if combo[1] == cs.FULL:
        assert abs(sum(want[6:9]) - (1 << 20)) <= 1


def test_chroma_rows_sum_to_zero_for_the_default_too(vs):
    k = vs.cvt_coefficients().tolist()
    assert abs(sum(k[9:12])) <= 1 and abs(sum(k[12:15])) <= 1        # OpenCV's own rounding: U sums to 1, V to 1


def test_every_product_fits_32_bits(vs):
    """The kernels multiply in 32-bit integers: a coefficient times a byte, a byte minus 128 or a sum of four bytes never leaves them."""
    for combo in COMBOS:
        k = vs.cvt_coefficients(combo).tolist()
        assert max(abs(v) for v in k[1:6]) * 255 < 1 << 31
        assert max(abs(v) for v in k[6:15]) * 1020 < 1 << 31


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
P, Q = 0x100000, 0x200000        # never read
BAD = [("matrix", (3, 0, 0, 0)), ("matrix", (-1, 0, 0, 0)), ("range", (0, 2, 0, 0)), ("range", (0, -1, 0, 0)),
       ("chroma_down", (0, 0, 2, 0)), ("chroma_down", (1, 1, -1, 0)), ("reserved", (1, 1, 1, 1)), ("reserved", (0, 0, 0, -5))]
GOOD = [None] + [(m, r, c, 0) for m in cs.MATRICES for r in cs.RANGES for c in (cs.TOPLEFT, cs.MEAN)]


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def op_call(vs, direction, f, desc, n=1, w=8, h=4):
    lay = capi.I420LayoutC(f.sample_bytes * w, 0, 0, 0)
    s, d = ptrs(*[P + 0x1000 * k for k in range(n)]), ptrs(*[Q + 0x1000 * k for k in range(n)])
    ref = capi._cs_ref(desc)
    if direction == 0:
        return vs.lib.vs_op_cvt_yuv_to_rgb_cs(f.fmt, s, C.byref(lay), capi.FMT_BGR8, d, w * 3, n, w, h, ref, None)
    return vs.lib.vs_op_cvt_rgb_to_yuv_cs(capi.FMT_BGR8, d, w * 3, f.fmt, s, C.byref(lay), n, w, h, ref, None)


@pytest.mark.parametrize("direction", [0, 1])
def test_operator_refusals_need_no_device(vs, direction):
    call = "vs_op_cvt_yuv_to_rgb" if direction == 0 else "vs_op_cvt_rgb_to_yuv"
    for name in ("NV12", "P010", "I422", "I444"):
        f = capi.PIXFMT_BY_NAME[name]
        for field, desc in BAD:
            assert op_call(vs, direction, f, desc) == 1, (name, desc)
            text = vs.lib.vs_last_error().decode()
            assert text.startswith(call) and field in text, text
            assert op_call(vs, direction, f, desc, n=32) == 1
        if vs.lib.vs_device_count() <= 0:
            for desc in GOOD:
                assert op_call(vs, direction, f, desc) == 2, (name, desc)
                assert op_call(vs, direction, f, desc, n=32) == 2
    # what the operators refuse without a descriptor, they refuse with one
    f = capi.PIXFMT_BY_NAME["NV12"]
    assert op_call(vs, direction, f, (1, 0, 1, 0), w=7) == 1 and op_call(vs, direction, f, (1, 0, 1, 0), n=33) == 1
    assert op_call(vs, direction, f, None, h=3) == 1


def test_coefficients_refusals(vs):
    out = (C.c_int32 * 16)(*([77] * 16))
    for field, desc in BAD:
        assert vs.lib.vs_cvt_coefficients(capi._cs_ref(desc), out) == 1
        text = vs.lib.vs_last_error().decode()
        assert text.startswith("vs_cvt_coefficients") and field in text
        assert list(out) == [77] * 16                                   # a refused call writes nothing
    assert vs.lib.vs_cvt_coefficients(None, None) == 1
    for desc in GOOD:
        assert vs.lib.vs_cvt_coefficients(capi._cs_ref(desc), out) == 0


def test_enhancer_setting_refusals_need_no_device(vs):
    """Without a device there is no object: the descriptor is judged first, so the refusal and its text are reachable with none."""
    for field, desc in BAD:
        assert vs.lib.vs_enh_set_yuv_colorimetry(None, capi._cs_ref(desc)) == 1
        text = vs.lib.vs_last_error().decode()
        assert text.startswith("vs_enh_set_yuv_colorimetry") and field in text
    for desc in GOOD:
        assert vs.lib.vs_enh_set_yuv_colorimetry(None, capi._cs_ref(desc)) == 1      # a good descriptor, no object
        text = vs.lib.vs_last_error().decode()
        assert text.startswith("vs_enh_set_yuv_colorimetry") and not any(f in text for f in ("matrix", "range", "chroma_down", "reserved"))


def test_the_plan_does_not_depend_on_a_descriptor(vs):
    """vs_enh_yuv_plan takes no descriptor and answers what it answered: the fused launch for the same stage lists."""
    assert "vs_cvt_colorimetry" not in " ".join(str(t) for t in vs.lib.vs_enh_yuv_plan.argtypes)
    tables = capi.Enhancer.default_params(vs, brightness=1.5, contrast=1.1, gamma=1.2)
    unsharp = capi.Enhancer.default_params(vs, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0)
    clahe = capi.Enhancer.default_params(vs, enable_clahe=1, clahe_tile_grid_size=2)
    for name in ("NV12", "I420", "P010", "I422", "I444"):
        f = capi.PIXFMT_BY_NAME[name].fmt
        assert vs.enh_yuv_plan(tables, f) == 1 and vs.enh_yuv_plan(tables, f, in_place=True) == 1
        assert vs.enh_yuv_plan(unsharp, f) == 1 and vs.enh_yuv_plan(unsharp, f, in_place=True) == 0
        assert vs.enh_yuv_plan(clahe, f) == 0


def test_guess(vs):
    def fields(c):
        return (c.matrix, c.range, c.chroma_down, c.reserved)
    assert fields(vs.cvt_colorimetry_guess(720, 576)) == (cs.BT601, cs.LIMITED, cs.TOPLEFT, 0)
    assert fields(vs.cvt_colorimetry_guess(1280, 720)) == (cs.BT709, cs.LIMITED, cs.TOPLEFT, 0)
    assert fields(vs.cvt_colorimetry_guess(3840, 2160)) == (cs.BT709, cs.LIMITED, cs.TOPLEFT, 0)
    assert fields(vs.cvt_colorimetry_guess(720, 480)) == (cs.BT601, cs.LIMITED, cs.TOPLEFT, 0)
    assert fields(vs.cvt_colorimetry_guess(1024, 577)) == (cs.BT709, cs.LIMITED, cs.TOPLEFT, 0)
    vs.lib.vs_cvt_colorimetry_guess(1920, 1080, None)                   # a null pointer is ignored


# ---- the statement against the standard -------------------------------------------------------------------------------------------
# per channel over all 2^24 triples: never more than 1 apart from clip(floor(x + 0.5)) of the float64 formula, and apart in at most
# 16 777 triples (1 in 1000).  (Recorded when this was written: the worst channel is B of BT.601 full, YUV -> RGB, 8 704 triples.)
MAX_APART = 16777


@pytest.mark.parametrize("combo", NEW, ids=combo_id)
def test_yuv_to_rgb_against_the_textbook(sweep, combo):
    y, u, v = sweep
    got = cs.yuv_to_rgb_px(y, u, v, *combo)
    want = cs.textbook_yuv_to_rgb(y, u, v, *combo)
    for name, a, b in zip("RGB", got, want):
        d = np.abs(a - b)
        print(combo_id(combo), "YUV->RGB", name, "max", int(d.max()), "apart", int((d != 0).sum()))
        assert int(d.max()) <= 1, name
        assert int((d != 0).sum()) <= MAX_APART, name


@pytest.mark.parametrize("combo", NEW, ids=combo_id)
def test_rgb_to_yuv_against_the_textbook(sweep, combo):
    r, g, b = sweep
    got = cs.rgb_to_yuv_px(r, g, b, *combo)
    want = cs.textbook_rgb_to_yuv(r, g, b, *combo)
    for name, a, w in zip("YUV", got, want):
        d = np.abs(a - w)
        print(combo_id(combo), "RGB->YUV", name, "max", int(d.max()), "apart", int((d != 0).sum()))
        assert int(d.max()) <= 1, name
        assert int((d != 0).sum()) <= MAX_APART, name


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_grey_axis(combo):
    grey = np.arange(256)
    y, u, v = cs.rgb_to_yuv_px(grey, grey, grey, *combo)
    assert (u == 128).all() and (v == 128).all()
    assert (int(y.min()), int(y.max())) == ((16, 235) if combo[1] == cs.LIMITED else (0, 255))
    assert (np.diff(y) >= 0).all()
    r, g, b = cs.yuv_to_rgb_px(y, u, v, *combo)
    if combo[1] == cs.FULL:
        assert np.array_equal(y, grey)
        assert np.array_equal(r, grey) and np.array_equal(g, grey) and np.array_equal(b, grey)
    else:
        assert np.array_equal(r, g) and np.array_equal(g, b) and int(np.abs(r - grey).max()) <= 1
        assert (int(r[0]), int(r[255])) == (0, 255)


def test_default_descriptor_is_cvtref(sweep):
    a, b, c = sweep
    for got, want in zip(cs.yuv_to_rgb_px(a, b, c), cvtref.yuv_to_rgb_px(a, b, c)):
        assert np.array_equal(got, want)
    for got, want in zip(cs.rgb_to_yuv_px(a, b, c), cvtref.rgb_to_yuv_px(a, b, c)):
        assert np.array_equal(got, want)
    frame = np.random.default_rng(5).integers(0, 256, (6, 10, 3), np.uint8)
    for sx, sy in ((1, 1), (1, 0), (0, 0)):
        for got, want in zip(cs.rgb_to_yuv(frame, sx, sy), cvtref.rgb_to_yuv(frame, sx, sy)):
            assert np.array_equal(got, want)
        planes = cvtref.rgb_to_yuv(frame, sx, sy)
        assert np.array_equal(cs.yuv_to_rgb(*planes, sx, sy, "RGBA8"), cvtref.yuv_to_rgb(*planes, sx, sy, "RGBA8"))


# ---- mean chroma in the statement -------------------------------------------------------------------------------------------------
def extreme_frames(w, h):
    """Whole frames of the extremes (B, G, R): red, blue, and 0 / 255 alternating along x, along y, and as a checkerboard."""
    red, blue = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    red[:, :, 2], blue[:, :, 0] = 255, 255
    yy, xx = np.mgrid[0:h, 0:w]
    alt_x = np.repeat((255 * (xx & 1))[:, :, None], 3, 2).astype(np.uint8)
    alt_y = np.repeat((255 * (yy & 1))[:, :, None], 3, 2).astype(np.uint8)
    check = np.repeat((255 * ((xx + yy) & 1))[:, :, None], 3, 2).astype(np.uint8)
    return {"red": red, "blue": blue, "alt_x": alt_x, "alt_y": alt_y, "check": check}


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_mean_chroma_in_the_statement(combo):
    rng = np.random.default_rng(11)
    # four (two) equal pixels per block: the top-left result
    small = rng.integers(0, 256, (3, 5, 3), np.uint8)
    for sx, sy in ((1, 1), (1, 0)):
        frame = np.repeat(np.repeat(small, 1 << sy, 0), 1 << sx, 1)
        a = cs.rgb_to_yuv(frame, sx, sy, "BGR8", *combo, cs.MEAN)
        b = cs.rgb_to_yuv(frame, sx, sy, "BGR8", *combo, cs.TOPLEFT)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # 4:4:4: the top-left rule; luma never depends on the chroma rule
    frame = rng.integers(0, 256, (6, 10, 3), np.uint8)
    assert all(np.array_equal(p, q) for p, q in zip(cs.rgb_to_yuv(frame, 0, 0, "BGR8", *combo, cs.MEAN), cs.rgb_to_yuv(frame, 0, 0, "BGR8", *combo)))
    assert np.array_equal(cs.rgb_to_yuv(frame, 1, 1, "BGR8", *combo, cs.MEAN)[0], cs.rgb_to_yuv(frame, 1, 1, "BGR8", *combo)[0])
    assert not np.array_equal(cs.rgb_to_yuv(frame, 1, 1, "BGR8", *combo, cs.MEAN)[1], cs.rgb_to_yuv(frame, 1, 1, "BGR8", *combo)[1])
    # the extremes: in-range U and V, every sum inside 32 bits
    k = cs.coefficients(*combo)
    lo, hi = (16, 240) if combo[1] == cs.LIMITED else (0, 255)
    largest = 0
    for label, f in extreme_frames(4, 4).items():
        for sx, sy in ((1, 1), (1, 0)):
            s = sx + sy
            h, w = f.shape[:2]
            sums = [f[:, :, c].astype(np.int64).reshape(h >> sy, 1 << sy, w >> sx, 1 << sx).sum(axis=(1, 3)) for c in (2, 1, 0)]
            for row in (k[9:12], k[12:15]):
                t = row[0] * sums[0] + row[1] * sums[1] + row[2] * sums[2] + (cs.H << s) + (128 << (20 + s))
                assert 0 <= int(t.min()) and int(t.max()) <= 1 << 30, (label, sx, sy)
                largest = max(largest, int(t.max()))
                # before the clamp: 16 .. 240 in limited range; in full range pure red and pure blue reach 256, which sat makes 255
                assert lo <= int((t >> (20 + s)).min()) and int((t >> (20 + s)).max()) <= (240 if combo[1] == cs.LIMITED else 256), (label, sx, sy)
            y, u, v = cs.rgb_to_yuv(f, sx, sy, "BGR8", *combo, cs.MEAN)
            if label in ("red", "blue"):
                one = cs.rgb_to_yuv_px(*(int(f[0, 0, c]) for c in (2, 1, 0)), *combo)
                assert (u == one[1]).all() and (v == one[2]).all()
                assert lo <= int(one[1]) <= hi and lo <= int(one[2]) <= hi
            elif label != "alt_y" or sy:
                assert (u == 128).all() and (v == 128).all(), (label, sx, sy)     # a block that is half black, half white is grey
    # the largest intermediate of all: exactly 2^30 in full range (s = 2, four blue pixels into U, four red ones into V)
    assert largest == (1 << 30 if combo[1] == cs.FULL else (k[11] * 1020 + (cs.H << 2) + (128 << 22)))
