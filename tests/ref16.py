"""The reference of the 16-bit warp (P010 planes), in numpy integers.

cv::warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) computes the fixed-point source coordinates the same way for every depth:
the forward matrix is inverted in double, adelta / bdelta per column and X0 / Y0 per row are rounded once each at
AB_BITS = 10, and a pixel's taps and 1/32-px fractions follow from (X0 + adelta) >> 5 - exactly as oracle/vso_imgproc.cpp
states it for 8-bit planes (rint, + 16, >> 5, short saturation).  The blend is the exact integer

    S = sum v_i n_i,   n = ((32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy fx),   sum n_i = 1024,

taps outside the picture 0 each by itself, rounded once:

    half to even  (S + 511 + ((S >> 10) & 1)) >> 10     the 16-bit definition: what remapBilinear<Cast<float, ushort>> and
                                                        saturate_cast<ushort> give wherever the float sum is exact
    half up       (S + 512) >> 10                       the 8-bit path: (S * 32 + 2^14) >> 15 of the fixed-point table

With half-up rounding on 8-bit planes this file equals the oracle byte for byte (tests/test_p010_cpu.py), which is what lets
the unchanged 8-bit oracle vouch for the coordinates of the 16-bit warp.
"""
import numpy as np

HALF_EVEN, HALF_UP = "half_even", "half_up"


def invert(M):
    """cv::warpAffine's inversion of the forward 2x3 matrix, in double (the operation order of the oracle's warp_prepare)."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _rint_sat(v):
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def coords(M, dw, dh):
    """(sx, sy, fx, fy) of every destination pixel: int64 arrays of shape (dh, dw)."""
    m = invert(M)
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = _rint_sat(m[0] * x * 1024)
    bdelta = _rint_sat(m[3] * x * 1024)
    X0 = _rint_sat((m[1] * y + m[2]) * 1024) + 16
    Y0 = _rint_sat((m[4] * y + m[5]) * 1024) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    return sx, sy, X & 31, Y & 31


def warp_sum(img, M):
    """S of every sample: int64, the shape of img ((h, w) or (h, w, cn))."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    src = img.reshape(h, w, -1).astype(np.int64)
    sx, sy, fx, fy = coords(M, w, h)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok[..., None], v, 0)

    n = [(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx]
    S = (tap(sx, sy) * n[0][..., None] + tap(sx + 1, sy) * n[1][..., None] + tap(sx, sy + 1) * n[2][..., None] +
         tap(sx + 1, sy + 1) * n[3][..., None])
    return S.reshape(img.shape)


def round_sum(S, rounding=HALF_EVEN):
    if rounding == HALF_UP:
        return (S + 512) >> 10
    assert rounding == HALF_EVEN
    return (S + 511 + ((S >> 10) & 1)) >> 10


def warp_affine(img, M, rounding=HALF_EVEN):
    """img: (h, w) or (h, w, cn), uint8 or uint16; M: the forward 2x3 matrix as float32 values.  Same shape and dtype out."""
    img = np.asarray(img)
    M = np.asarray(M, np.float32).astype(np.float64)
    return round_sum(warp_sum(img, M), rounding).astype(img.dtype)


def chroma_matrix(M):
    """The chroma plane's matrix: the translation halved in float."""
    m = np.asarray(M, np.float32).reshape(6).copy()
    m[2] = m[2] * np.float32(0.5)
    m[5] = m[5] * np.float32(0.5)
    return m


def warp_two_planes(surf, w, h, M, rounding=HALF_EVEN):
    """An NV12 (uint8) or P010 (uint16) surface of shape (h * 3 / 2, w): the luma plane by M, the interleaved chroma plane
    (h / 2, w / 2, 2) by the matrix with the halved translation."""
    surf = np.asarray(surf)
    out = np.empty_like(surf)
    out[:h] = warp_affine(surf[:h], M, rounding)
    uv = surf[h:].reshape(h // 2, w // 2, 2)
    out[h:] = warp_affine(uv, chroma_matrix(M), rounding).reshape(h // 2, w)
    return out


def tie_mask(img, M):
    """True where S mod 1024 == 512 and S >> 10 is even: the samples on which half-even and half-up give different values."""
    S = warp_sum(img, np.asarray(M, np.float32).astype(np.float64))
    return ((S & 1023) == 512) & (((S >> 10) & 1) == 0)
