"""The reference of roll correction and auto zoom/crop on P010 surfaces, in numpy integers, on top of tests/ref16.py.

warp(): cv::warpAffine on a plane of 16-bit (or 8-bit) samples with a DOUBLE forward matrix, a destination size of its own and a
constant, replicate or reflect border.  Coordinates are ref16.coords (the 8-bit path: AB_BITS 10, 1/32 px); a tap outside the source is 0
(constant), the nearest edge sample (replicate) or the sample of the even extension (reflect: reflect_index, each axis by
itself - the virtual canvas's compensation warp, tests/compref.py), each tap by itself; the blend is ref16's S with its HALF_EVEN / HALF_UP switch.

On top of it the two stages as include/vs_stab.h defines them for P010 (vs_pixfmt16):
    rotate_surface      the roll stage's rotation for a given smoothed angle (the matrix of oracle/vso_roll.cpp: centre, angle;
                        the chroma plane with the translation halved), BORDER_REPLICATE
    crop_scale_surface  the zoom stage's crop-and-scale for a given info8 (rectangle as found for luma, halved for chroma; each
                        plane to its share of 640 x 360 by the reference's CV_32F scale matrix), BORDER_CONSTANT 0; the unchanged
                        surface when info8 says "not cropped"
    roll_p010, azc_p010 the same with angle and rectangle taken from the ORACLE's NV12 objects run on the high-byte surface - that
                        is the definition of the analysis plane, so no line search and no contour code is restated here.
With HALF_UP on surfaces whose samples are all <= 255 the first two equal the oracle's NV12 functions byte for byte
(tests/test_p010_geom_cpu.py), which pins coordinates, replicate handling, rectangle halving and the scale matrix."""
import math

import numpy as np

import ref16
from ref16 import HALF_EVEN, HALF_UP

CONSTANT, REFLECT, REPLICATE = 0, 1, 3          # VS_BORDER_BLACK, VS_BORDER_REFLECT, VS_BORDER_REPLICATE


def reflect_index(p, n):
    """cv::borderInterpolate(BORDER_REFLECT) by its definition: the even extension  ... c b a | a b c | c b a ...  has period 2n."""
    q = np.mod(np.asarray(p, np.int64), 2 * n)
    return np.where(q >= n, 2 * n - 1 - q, q)


def warp_sum(img, M, dsize=None, border=CONSTANT):
    """S of every destination sample: int64 of shape (dh, dw[, cn]).  img: (sh, sw) or (sh, sw, cn); M: forward 2x3, double."""
    img = np.asarray(img)
    sh, sw = img.shape[:2]
    dw, dh = dsize if dsize else (sw, sh)
    src = img.reshape(sh, sw, -1).astype(np.int64)
    sx, sy, fx, fy = ref16.coords(np.asarray(M, np.float64), dw, dh)

    def tap(xx, yy):
        if border == REFLECT:
            return src[reflect_index(yy, sh), reflect_index(xx, sw)]
        v = src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
        if border == REPLICATE:
            return v
        assert border == CONSTANT
        ok = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        return np.where(ok[..., None], v, 0)

    n = [(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx]
    S = (tap(sx, sy) * n[0][..., None] + tap(sx + 1, sy) * n[1][..., None] + tap(sx, sy + 1) * n[2][..., None] +
         tap(sx + 1, sy + 1) * n[3][..., None])
    return S.reshape((dh, dw) + img.shape[2:])


def warp(img, M, dsize=None, border=CONSTANT, rounding=HALF_EVEN):
    img = np.asarray(img)
    return ref16.round_sum(warp_sum(img, M, dsize, border), rounding).astype(img.dtype)


def tie_mask(img, M, dsize=None, border=CONSTANT):
    """ref16.tie_mask for this warp: True where half-even and half-up give different values."""
    S = warp_sum(img, M, dsize, border)
    return ((S & 1023) == 512) & (((S >> 10) & 1) == 0)


# ---- roll ------------------------------------------------------------------------------------------------------------------------
def roll_matrices(w, h, angle_deg):
    """cv::getRotationMatrix2D((w / 2.0f, h / 2.0f), angle, 1.0) in double, and the chroma plane's: the translation halved."""
    cx, cy = float(np.float32(w / 2.0)), float(np.float32(h / 2.0))
    a = angle_deg * 3.1415926535897932384626433832795 / 180
    al, be = math.cos(a), math.sin(a)
    M = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    return M, [M[0], M[1], M[2] * 0.5, M[3], M[4], M[5] * 0.5]


def planes(surf, w, h):
    """(luma (h, w), chroma (h / 2, w / 2, 2)) of a packed NV12 / P010 surface (h * 3 / 2, w)."""
    surf = np.asarray(surf)
    return surf[:h], surf[h:].reshape(h // 2, w // 2, 2)


def rotate_surface(surf, w, h, angle_deg, rounding=HALF_EVEN):
    y, uv = planes(surf, w, h)
    M, Mc = roll_matrices(w, h, angle_deg)
    out = np.empty_like(np.asarray(surf))
    out[:h] = warp(y, M, None, REPLICATE, rounding)
    out[h:] = warp(uv, Mc, None, REPLICATE, rounding).reshape(h // 2, w)
    return out


def high_bytes(surf):
    return np.ascontiguousarray((np.asarray(surf) >> 8).astype(np.uint8))


def roll_p010(surf, w, h, oracle_roll, rounding=HALF_EVEN):
    """One frame through the roll stage.  oracle_roll: the oracle's roll object (it carries the smoothed angle from frame to frame); it
    is advanced by its NV12 call on the high-byte surface, and its smoothed angle after that call rotates the 16-bit planes."""
    oracle_roll.correct_nv12(high_bytes(surf), w, h)
    return rotate_surface(surf, w, h, oracle_roll.state()[0], rounding)


# ---- zoom ------------------------------------------------------------------------------------------------------------------------
def zoom_jobs(info):
    """[(x, y, w, h, dw, dh, M)] for luma and chroma from info8: M = [sx 0 0; 0 sy 0] held as CV_32F, used as double."""
    cx, cy, cw, ch = (int(v) for v in info[2:6])
    ux, uy, uw, uh = cx // 2, cy // 2, max(1, cw // 2), max(1, ch // 2)
    My = [float(np.float32(640.0 / cw)), 0.0, 0.0, 0.0, float(np.float32(360.0 / ch)), 0.0]
    Mu = [float(np.float32(320.0 / uw)), 0.0, 0.0, 0.0, float(np.float32(180.0 / uh)), 0.0]
    return [(cx, cy, cw, ch, 640, 360, My), (ux, uy, uw, uh, 320, 180, Mu)]


def crop_scale_surface(surf, w, h, info, rounding=HALF_EVEN):
    """The (360 * 3 / 2, 640) result, or the unchanged surface when info8[7] == 0."""
    surf = np.asarray(surf)
    if not info[7]:
        return surf.copy()
    y, uv = planes(surf, w, h)
    (x0, y0, cw, ch, dw, dh, My), (x1, y1, uw, uh, dw2, dh2, Mu) = zoom_jobs(info)
    out = np.empty((540, 640), surf.dtype)
    out[:360] = warp(y[y0:y0 + ch, x0:x0 + cw], My, (dw, dh), CONSTANT, rounding)
    out[360:] = warp(uv[y1:y1 + uh, x1:x1 + uw], Mu, (dw2, dh2), CONSTANT, rounding).reshape(180, 640)
    return out


def azc_p010(surf, w, h, oracle, rounding=HALF_EVEN):
    """(result, info8): info8 from the oracle's NV12 auto zoom/crop on the high-byte surface."""
    _, info = oracle.auto_zoom_crop_nv12(high_bytes(surf), w, h)
    return crop_scale_surface(surf, w, h, info, rounding), info
