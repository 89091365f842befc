"""The fade border on YUV surfaces, stated in numpy: the blend of one padded plane with its history (cv::addWeighted on 8- or 16-bit
samples), the update of the history, and the step of a whole surface around the warp (include/vs_stab.h, vs_stab_set_yuv_fade (a) -
(e); vs_op_fade_blend_jobs, vs_op_fade_update_jobs).  On top of yuvpadref (the pad) and compref (fade_alpha).  Nothing is imported
from the oracle or the library."""
import numpy as np

import compref
import yuvpadref as yp

F = np.float32


def blend_plane(plane, hist, bx, by, fill, alpha, beta):
    """plane: (h, w) or (h, w, cn) samples, uint8 or uint16; hist: the padded size.  -> addWeighted(hist, alpha, padded, beta) where
    padded is the plane with a border of `fill`: t = fl32(padded * beta); v = fl32(hist * alpha + t) (one rounding: a fused
    multiply-add); rint (half to even); saturate.
    Each float32 rounding is taken from an exact float64 value while each weight is 0 or in [2^-12, 1]: such a weight is a multiple
    of 2^-36, so hist * alpha (16 x 24 bits) and t are multiples of 2^-36 below 2^16, and their sum, below 2^17, fits 53 bits."""
    plane = np.asarray(plane)
    padded = yp.pad_plane(plane, bx, by, yp.BLACK, fill)
    hist = np.asarray(hist)
    assert hist.dtype == plane.dtype and hist.shape == padded.shape and plane.dtype in (np.uint8, np.uint16)
    al, be = float(F(alpha)), float(F(beta))
    assert all(w == 0.0 or 2.0 ** -12 <= w <= 1.0 for w in (al, be))
    t = (padded.astype(np.float64) * be).astype(np.float32)
    v = (hist.astype(np.float64) * al + t.astype(np.float64)).astype(np.float32)
    return np.clip(np.rint(v.astype(np.float64)), 0, np.iinfo(plane.dtype).max).astype(plane.dtype)


def update_plane(hist, result):
    """history <- (T)((1.0f - 0.1f) * history + 0.1f * result): two float32 products, one float32 sum, truncation"""
    hist, result = np.asarray(hist), np.asarray(result)
    assert hist.dtype == result.dtype and hist.shape == result.shape and hist.dtype in (np.uint8, np.uint16)
    rate = F(0.1)
    keep = F(1.0) - rate
    v = keep * hist.astype(np.float32) + rate * result.astype(np.float32)
    assert v.dtype == np.float32
    return np.trunc(v).astype(hist.dtype)


def plane_borders(nplanes, sx, sy, b):
    assert b % (1 << sx) == 0 and b % (1 << sy) == 0
    return [(b, b)] + [(b >> sx, b >> sy)] * (nplanes - 1)


def plane_fills(nplanes, fill):
    y, u, v = fill
    return [y, (u, v)] if nplanes == 2 else [y, u, v]


def stream_step(hist, count, planes, sx, sy, b, fill, alpha, duration):
    """The stream's logic in front of the warp.  planes: [Y, U, V], or [Y, UV] with UV of (h >> sy, w >> sx, 2); hist: the list of
    padded history planes, or None.  The first padded frame is the history (count 0), also when the padded size changes.
    -> (blended padded planes, history planes, count after the frame, alpha used).  Behind the warp:
    history <- [update_plane(h, r) for h, r in zip(history, result planes)]."""
    borders, fills = plane_borders(len(planes), sx, sy, b), plane_fills(len(planes), fill)
    padded = yp.pad_surface(planes, sx, sy, b, yp.BLACK, fill)
    if hist is None or [h.shape for h in hist] != [p.shape for p in padded]:
        hist, count = [p.copy() for p in padded], 0
    a, count = compref.fade_alpha(alpha, count, duration)
    beta = F(1.0) - a
    blended = [blend_plane(p, h, bx, by, fl, a, beta) for p, h, (bx, by), fl in zip(planes, hist, borders, fills)]
    return blended, hist, count, a
