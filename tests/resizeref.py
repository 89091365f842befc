"""Resize to an output size, stated in numpy and `math` (include/vs_stab.h: vs_op_resample_jobs, vs_op_resize_yuv, vs_op_resize_rgb,
vs_resize_axis_table).  None of the library's code.

Coordinates, both interpolations: scale = 1.0 / ((double)dst / src), f = (float)((d + 0.5) * scale - 0.5), s = floor(f),
f = f - (float)s in float32.

LINEAR is cv::resize(INTER_LINEAR) as oracle/vso_resize_linear_u8 restates it and tests/cropzoomref.py states it for zoom-in: columns
under HResizeLinear's edge rule, rows with both tap rows clamped, the exact 2 : 1 case (sw == 2 dw and sh == 2 dh) the 2 x 2 mean
at both depths; 8-bit vertical pass (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 16-bit one rounding half to
even at bit 22.

LANCZOS4 is cv::resize(INTER_LANCZOS4) for CV_8U: neither s nor f clamped, eight taps at clamp(s - 3 + k, 0, src - 1) on both axes,
weights from the double sin / cos of `math`, coefficients saturate_cast<short>(w * 2048.f) and not renormalised,
out = clamp((S + 2^21) >> 22, 0, max_value) with S the exact integer sum over the 64 taps (16-bit: the same with S in 64 bits, a
definition of this library).

max_value: every result is clamped to 0 .. max_value (0 = the sample type's maximum)."""
import math

import numpy as np

LINEAR, LANCZOS4 = 0, 1
COEF = 2048
FLT_EPSILON = float(np.finfo(np.float32).eps)
_R = 0.70710678118654752440084436210485
_PI = 3.1415926535897932384626433832795
_CS = ((1.0, 0.0), (-_R, -_R), (0.0, 1.0), (_R, -_R), (-1.0, 0.0), (_R, _R), (0.0, -1.0), (-_R, _R))


def taps(interp):
    return 8 if interp == LANCZOS4 else 2


def coords(src, dst):
    """-> s (int64, not clamped), f (float32) per destination index."""
    scale = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    d = np.arange(dst, dtype=np.float64)
    v = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(v).astype(np.int64)
    return s, (v - s.astype(np.float32)).astype(np.float32)


def _sat_short(v):
    """saturate_cast<short> of float32 values: round half to even, saturate."""
    return np.clip(np.rint(v).astype(np.int64), -32768, 32767)


def lanczos4_coefs(f):
    """The eight 11-bit coefficients of one float32 f, as a list of ints."""
    f = np.float32(f)
    if float(f) < FLT_EPSILON:
        w = [np.float32(0)] * 8
        w[3] = np.float32(1)
    else:
        y0 = -(float(f) + 3.0) * _PI * 0.25
        s0, c0 = math.sin(y0), math.cos(y0)
        w, total = [], np.float32(0)
        for i in range(8):
            y = -(float(f) + 3.0 - float(i)) * _PI * 0.25
            wi = np.float32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
            w.append(wi)
            total = np.float32(total + wi)
        inv = np.float32(np.float32(1) / total)
        w = [np.float32(x * inv) for x in w]
    return [int(_sat_short(np.float32(x * np.float32(COEF)))) for x in w]


def axis_table(src, dst, interp, axis):
    """-> idx (dst, K) int64, already clamped into the source, and coef (dst, K) int64.  axis 0 = columns, 1 = rows."""
    s, f = coords(src, dst)
    if interp == LANCZOS4:
        idx = np.clip(s[:, None] - 3 + np.arange(8)[None, :], 0, src - 1)
        memo, coef = {}, np.empty((dst, 8), np.int64)
        for d in range(dst):
            key = float(f[d])
            if key not in memo:
                memo[key] = lanczos4_coefs(f[d])
            coef[d] = memo[key]
        return idx, coef
    assert interp == LINEAR
    if axis == 0:
        f = np.where(s < 0, np.float32(0), f).astype(np.float32)
        s = np.maximum(s, 0)
        edge = s + 1 >= src
        f = np.where(s >= src - 1, np.float32(0), f).astype(np.float32)
        s = np.minimum(s, src - 1)
    c0 = _sat_short((np.float32(1) - f) * np.float32(COEF))
    c1 = _sat_short(f * np.float32(COEF))
    if axis == 0:
        return (np.stack([s, np.where(edge, s, s + 1)], 1), np.stack([np.where(edge, COEF, c0), np.where(edge, 0, c1)], 1))
    return np.stack([np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)], 1), np.stack([c0, c1], 1)


def type_max(dtype):
    return int(np.iinfo(dtype).max)


def is_mean(sw, sh, dw, dh, interp):
    return interp == LINEAR and sw == 2 * dw and sh == 2 * dh


def resize(plane, cn, dw, dh, interp, max_value=0):
    """plane: uint8 or uint16 (sh, sw * cn), possibly a view into a larger array -> the same dtype, (dh, dw * cn)."""
    dtype = plane.dtype
    assert dtype in (np.uint8, np.uint16)
    top = max_value or type_max(dtype)
    sh, row = plane.shape
    assert row % cn == 0
    sw = row // cn
    p = plane.reshape(sh, sw, cn).astype(np.int64)
    if is_mean(sw, sh, dw, dh, interp):
        v = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
        return np.minimum(v, top).astype(dtype).reshape(dh, dw * cn)
    xi, xc = axis_table(sw, dw, interp, 0)
    yi, yc = axis_table(sh, dh, interp, 1)
    K = taps(interp)
    H = sum(p[:, xi[:, k], :] * xc[None, :, k, None] for k in range(K))             # (sh, dw, cn), exact integers
    if interp == LANCZOS4:
        S = sum(H[yi[:, k]] * yc[:, k, None, None] for k in range(K))
        v = np.clip((S + (1 << 21)) >> 22, 0, top)
    elif dtype == np.uint8:
        b0, b1 = yc[:, 0, None, None], yc[:, 1, None, None]
        v = ((((b0 * (H[yi[:, 0]] >> 4)) >> 16) + ((b1 * (H[yi[:, 1]] >> 4)) >> 16) + 2) >> 2) & 255
        v = np.minimum(v, top)
    else:
        S = H[yi[:, 0]] * yc[:, 0, None, None] + H[yi[:, 1]] * yc[:, 1, None, None]
        v = np.minimum(np.minimum(65535, (S + (1 << 21) - 1 + ((S >> 22) & 1)) >> 22), top)
    return v.astype(dtype).reshape(dh, dw * cn)


def lanczos_sum(plane, cn, dw, dh):
    """The exact integer S of every destination sample under LANCZOS4, (dh, dw * cn) int64."""
    sh, row = plane.shape
    sw = row // cn
    p = plane.reshape(sh, sw, cn).astype(np.int64)
    xi, xc = axis_table(sw, dw, LANCZOS4, 0)
    yi, yc = axis_table(sh, dh, LANCZOS4, 1)
    H = sum(p[:, xi[:, k], :] * xc[None, :, k, None] for k in range(8))
    return sum(H[yi[:, k]] * yc[:, k, None, None] for k in range(8)).reshape(dh, dw * cn)


def lanczos_max_value(bits, low_bit):
    """What vs_op_resize_yuv passes with LANCZOS4: (1 << bits) - 1 for the low-bit formats (I010 ... I412), else the type's maximum."""
    return (1 << bits) - 1 if low_bit else 0
