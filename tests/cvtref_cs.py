"""What vs_op_cvt_yuv_to_rgb_cs and vs_op_cvt_rgb_to_yuv_cs compute for a colorimetry descriptor, stated in numpy (int64) from the
text of include/vs_stab.h alone.  Shares nothing with the library: the constants of the five rule-derived combinations are computed
here from the standards' Kr, Kb in exact rational arithmetic (fractions.Fraction); those of (BT.601, limited) are OpenCV's, written
out, as the header writes them out.

Planes are (rows, cols) arrays of bytes, as in tests/cvtref.py; the 16-bit formats enter and leave through its sample_to_byte /
byte_to_sample."""
from fractions import Fraction

import numpy as np

H = 1 << 19
BT601, BT709, BT2020 = 0, 1, 2
LIMITED, FULL = 0, 1
TOPLEFT, MEAN = 0, 1
MATRICES = (BT601, BT709, BT2020)
RANGES = (LIMITED, FULL)
COMBINATIONS = [(m, r) for m in MATRICES for r in RANGES]
NEW_COMBINATIONS = [c for c in COMBINATIONS if c != (BT601, LIMITED)]
MATRIX_NAMES = {BT601: "BT.601", BT709: "BT.709", BT2020: "BT.2020"}
RANGE_NAMES = {LIMITED: "limited", FULL: "full"}

KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)),
         BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
         BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}

NAMES = ("y_off", "CY", "RV", "GV", "GU", "BU", "YR", "YG", "YB", "UR", "UG", "UB", "VR", "VG", "VB")
OPENCV_BT601_LIMITED = (16, 1220542, 1673527, 852492, 409993, 2116026, 269484, 528482, 102760, -155188, -305135, 460324,
                        460324, -385875, -74448)


def round_half_away(q):
    """A Fraction to the nearest integer, halves away from zero."""
    n = (abs(q) * 2 + 1) // 2
    return int(n if q >= 0 else -n)


def rule_fractions(matrix, rng):
    """The fifteen values of the rule before scaling by 2^20 and rounding (y_off as it is)."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs = (Fraction(219, 255), Fraction(224, 255)) if rng == LIMITED else (Fraction(1), Fraction(1))
    return (16 if rng == LIMITED else 0,
            1 / ys, 2 * (1 - kr) / cs, 2 * (1 - kr) * kr / kg / cs, 2 * (1 - kb) * kb / kg / cs, 2 * (1 - kb) / cs,
            kr * ys, kg * ys, kb * ys,
            -kr / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, cs / 2,
            cs / 2, -kg / (2 * (1 - kr)) * cs, -kb / (2 * (1 - kr)) * cs)


def rule_coefficients(matrix, rng):
    f = rule_fractions(matrix, rng)
    return (f[0],) + tuple(round_half_away(x * (1 << 20)) for x in f[1:])


def coefficients(matrix=BT601, rng=LIMITED):
    """The fifteen integers in the order of NAMES."""
    if (matrix, rng) == (BT601, LIMITED):
        return OPENCV_BT601_LIMITED
    return rule_coefficients(matrix, rng)


def _sat(v):
    return np.clip(v, 0, 255)


def yuv_to_rgb_px(y, u, v, matrix=BT601, rng=LIMITED):
    """(R, G, B), int64 in 0 .. 255, for arrays of bytes of one shape."""
    y_off, CY, RV, GV, GU, BU = coefficients(matrix, rng)[:6]
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    yp = np.maximum(0, y - y_off) * CY
    u = u - 128
    v = v - 128
    return _sat((yp + H + RV * v) >> 20), _sat((yp + H - GV * v - GU * u) >> 20), _sat((yp + H + BU * u) >> 20)


def luma_px(r, g, b, matrix=BT601, rng=LIMITED):
    c = coefficients(matrix, rng)
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    return _sat((c[6] * r + c[7] * g + c[8] * b + H + (c[0] << 20)) >> 20)


def chroma_sums(sr, sg, sb, s, matrix=BT601, rng=LIMITED):
    """(U, V) of the sums of R, G, B over the 1 << s pixels of a chroma block (s = 0: of one pixel)."""
    c = coefficients(matrix, rng)
    sr, sg, sb = (np.asarray(a, np.int64) for a in (sr, sg, sb))
    bias = (H << s) + (128 << (20 + s))
    return (_sat((c[9] * sr + c[10] * sg + c[11] * sb + bias) >> (20 + s)),
            _sat((c[12] * sr + c[13] * sg + c[14] * sb + bias) >> (20 + s)))


def rgb_to_yuv_px(r, g, b, matrix=BT601, rng=LIMITED):
    return (luma_px(r, g, b, matrix, rng),) + chroma_sums(r, g, b, 0, matrix, rng)


def yuv_to_rgb(y, u, v, sx, sy, rgb="BGR8", matrix=BT601, rng=LIMITED):
    """Byte planes Y (h, w), U and V (h >> sy, w >> sx) -> (h, w, cn) uint8: pixel (x, y) takes the chroma sample (x >> sx, y >> sy)."""
    from cvtref import RGB_FORMATS
    h, w = np.shape(y)
    yi, xi = np.arange(h)[:, None] >> sy, np.arange(w)[None, :] >> sx
    r, g, b = yuv_to_rgb_px(y, np.asarray(u)[yi, xi], np.asarray(v)[yi, xi], matrix, rng)
    cn, ri, bi = RGB_FORMATS[rgb]
    out = np.full((h, w, cn), 255, np.uint8)
    out[:, :, ri], out[:, :, 1], out[:, :, bi] = r, g, b
    return out


def rgb_to_yuv(frame, sx, sy, rgb="BGR8", matrix=BT601, rng=LIMITED, chroma_down=TOPLEFT):
    """(h, w, cn) uint8 -> byte planes (Y, U, V): Y of every pixel; U and V of the top-left pixel of each (1 << sx) x (1 << sy)
    block, or (MEAN) of the sums over the block."""
    from cvtref import RGB_FORMATS
    frame = np.asarray(frame)
    cn, ri, bi = RGB_FORMATS[rgb]
    assert frame.shape[2] == cn
    h, w = frame.shape[:2]
    assert w % (1 << sx) == 0 and h % (1 << sy) == 0
    r, g, b = (frame[:, :, k].astype(np.int64) for k in (ri, 1, bi))
    y = luma_px(r, g, b, matrix, rng)
    if chroma_down == MEAN:
        def block_sum(p):
            return p.reshape(h >> sy, 1 << sy, w >> sx, 1 << sx).sum(axis=(1, 3))
        u, v = chroma_sums(block_sum(r), block_sum(g), block_sum(b), sx + sy, matrix, rng)
    else:
        u, v = chroma_sums(r[::1 << sy, ::1 << sx], g[::1 << sy, ::1 << sx], b[::1 << sy, ::1 << sx], 0, matrix, rng)
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


# ---- the float64 textbook formulas the integers are held to (tests/test_cvt_colorimetry_cpu.py) ---------------------------------------
def textbook_yuv_to_rgb(y, u, v, matrix, rng):
    """clip(floor(x + 0.5)) of the standard's float64 formula; luma below the range's black is black, as in the integer form."""
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1.0 - kr - kb
    y_off, ys, cs = (16.0, 219.0 / 255.0, 224.0 / 255.0) if rng == LIMITED else (0.0, 1.0, 1.0)
    yl = np.maximum(0.0, np.asarray(y, np.float64) - y_off) / ys
    pb = (np.asarray(u, np.float64) - 128.0) / cs
    pr = (np.asarray(v, np.float64) - 128.0) / cs
    r = yl + 2.0 * (1.0 - kr) * pr
    b = yl + 2.0 * (1.0 - kb) * pb
    g = yl - 2.0 * (1.0 - kr) * kr / kg * pr - 2.0 * (1.0 - kb) * kb / kg * pb
    return tuple(np.clip(np.floor(c + 0.5), 0, 255).astype(np.int64) for c in (r, g, b))


def textbook_rgb_to_yuv(r, g, b, matrix, rng):
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1.0 - kr - kb
    y_off, ys, cs = (16.0, 219.0 / 255.0, 224.0 / 255.0) if rng == LIMITED else (0.0, 1.0, 1.0)
    r, g, b = (np.asarray(a, np.float64) for a in (r, g, b))
    yl = kr * r + kg * g + kb * b
    y = y_off + ys * yl
    u = 128.0 + cs * (b - yl) / (2.0 * (1.0 - kb))
    v = 128.0 + cs * (r - yl) / (2.0 * (1.0 - kr))
    return tuple(np.clip(np.floor(c + 0.5), 0, 255).astype(np.int64) for c in (y, u, v))
