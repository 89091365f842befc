"""Border pad on YUV surfaces, stated in numpy: the pad of one plane - cv::copyMakeBorder as compref.copy_make_border states it, with
a fill sample per channel where the reference writes 0 - and the pad of a whole surface with the chroma shifts of its format
(include/vs_stab.h, vs_stab_set_yuv_border_pad (a); vs_op_pad_jobs).  Nothing is imported from the oracle or the library."""
import numpy as np

import compref

BLACK, REFLECT, REFLECT_101, REPLICATE, WRAP = compref.BLACK, compref.REFLECT, compref.REFLECT_101, compref.REPLICATE, compref.WRAP
MODES = (BLACK, REFLECT, REFLECT_101, REPLICATE, WRAP)


def video_black(bits, high_bits=False):
    """(y, u, v) of limited-range black as the samples lie in memory: 16 and 128 at the format's depth; P010 (high_bits) keeps its ten
    bits at the top of the word."""
    sh = 8 if high_bits else bits - 8
    return 16 << sh, 128 << sh, 128 << sh


def pad_plane(plane, bx, by, mode, fill=0):
    """plane: (h, w) or (h, w, cn) samples -> (h + 2 by, w + 2 bx[, cn]).  fill: one sample, or one per channel (BLACK only)."""
    plane = np.asarray(plane)
    h, w = plane.shape[:2]
    if bx == by:
        out = compref.copy_make_border(plane, bx, mode)
    else:
        iy = compref.border_index(np.arange(-by, h + by), h, mode)
        ix = compref.border_index(np.arange(-bx, w + bx), w, mode)
        out = plane[np.clip(iy, 0, h - 1)][:, np.clip(ix, 0, w - 1)].copy()
        out[iy < 0] = 0
        out[:, ix < 0] = 0
    if mode == BLACK:
        inside = np.zeros(out.shape[:2], bool)
        inside[by:by + h, bx:bx + w] = True
        out[~inside] = np.asarray(fill, plane.dtype)
    return out


def pad_surface(planes, sx, sy, b, mode, fill):
    """planes: [Y, U, V] of (h, w) samples, or [Y, UV] with UV of (h >> sy, w >> sx, 2); fill = (y, u, v).  Y gets b on every side,
    the chroma planes (b >> sx) columns and (b >> sy) rows; b must be a multiple of 2^sx and 2^sy."""
    assert b % (1 << sx) == 0 and b % (1 << sy) == 0
    y, u, v = fill
    out = [pad_plane(planes[0], b, b, mode, y)]
    if len(planes) == 2:
        return out + [pad_plane(planes[1], b >> sx, b >> sy, mode, (u, v))]
    return out + [pad_plane(planes[1], b >> sx, b >> sy, mode, u), pad_plane(planes[2], b >> sx, b >> sy, mode, v)]
