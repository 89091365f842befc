"""Inputs and the reference shared by tests/test_azc_size_cpu.py and tests/test_gpu_azc_size.py: auto zoom/crop at a chosen output size.

The reference of a crop-and-scale job is ref16_geom.warp(roi, M, (dw, dh), CONSTANT, rounding) with the reference's CV_32F scale matrix
(scale_matrix) - HALF_UP for 8-bit samples, HALF_EVEN for 16-bit ones; the CPU test pins it to the oracle's warp.

STAGING: the staged kernel works on output tiles of T_w x T_h = 128 x 16 samples and a staging area of 160 x 24 source samples.  A job
is staged when the source box of a full tile fits: with the inverse factors ix = 1 / (float)(dw / sw), iy = 1 / (float)(dh / sh),
    floor(127 ix + 2 / 1024) + 3 + 6 <= 160      that is  127 ix < 152  (ix < 1.1968)
    floor( 15 iy + 2 / 1024) + 3     <=  24      that is   15 iy <  22  (iy < 1.4667)
Every zoom-in is staged, and so are mild downscales.  OP_DESTS are one tile (128 x 16), a ragged second tile column and second tile
row (T_w + 2 = 130, T_h + 3 = 19: two samples in tile column 1, three rows in tile row 1) and two full tile columns plus two samples
(258: tile column 2 holds two).  Per destination the crops of op_crops(): 1 x 1 and 3 x 2 (every tap of the right and lower half reads
the border), a prime-sized crop (53 x 11), the exact 2 x zoom across (dw / 2; down too where dh is even), the identity, and three
downscales: one just inside the limit both ways, one just outside across (127 ix >= 152), one just outside down (15 iy >= 22):
    dw 128: sw 153 -> 127 ix = 151.8 staged, 154 -> 152.8 direct        dh 16: sh 23 -> 15 iy = 21.6 staged, 24 -> 22.5 direct
    dw 130: sw 155 -> 151.4 staged,          156 -> 152.4 direct        dh 19: sh 27 -> 21.3 staged,         28 -> 22.1 direct
    dw 258: sw 308 -> 151.6 staged,          310 -> 152.6 direct
3 x 8 = 24 jobs: the most one call takes, of mixed geometry and of both classes (OP_STAGED says which)."""
import numpy as np

import ref16_geom as geom

TILE = (128, 16)
# the crop -> output pairs on which the reference is pinned to the oracle (the issue's list)
PAIRS = [((52, 30), (64, 48)), ((97, 55), (130, 66)), ((33, 21), (258, 34)), ((200, 120), (130, 66)), ((3, 2), (130, 66)),
         ((240, 136), (258, 146)), ((129, 65), (258, 130))]

OP_DESTS = [(128, 16), (130, 19), (258, 16)]
_LIMIT_W = {128: (153, 154), 130: (155, 156), 258: (308, 310)}      # (widest staged, narrowest direct) crop width per dw
_LIMIT_H = {16: (23, 24), 19: (27, 28)}


def op_crops(dsize):
    dw, dh = dsize
    (w_in, w_out), (h_in, h_out) = _LIMIT_W[dw], _LIMIT_H[dh]
    return [(1, 1), (3, 2), (53, 11), (dw // 2, dh // 2 if dh % 2 == 0 else dh), (dw, dh), (w_in, h_in), (w_out, dh), (dw, h_out)]


OP_CASES = [(crop, d) for d in OP_DESTS for crop in op_crops(d)]          # 24 (crop, destination) pairs
OP_STAGED = [1, 1, 1, 1, 1, 1, 0, 0] * 3


def scale_matrix(ssize, dsize):
    """[(float)((double)dw / sw), 0, 0; 0, (float)((double)dh / sh), 0] as doubles: AutoZoomCrop.cpp:261-262 with dw, dh for 640, 360."""
    (sw, sh), (dw, dh) = ssize, dsize
    return [float(np.float32(dw / sw)), 0.0, 0.0, 0.0, float(np.float32(dh / sh)), 0.0]


def rounding_of(dtype):
    return geom.HALF_UP if np.dtype(dtype) == np.uint8 else geom.HALF_EVEN


def reference(roi, dsize):
    """The job's result: roi (sh, sw[, cn]) uint8 or uint16 -> (dh, dw[, cn])."""
    roi = np.asarray(roi)
    return geom.warp(roi, scale_matrix((roi.shape[1], roi.shape[0]), dsize), dsize, geom.CONSTANT, rounding_of(roi.dtype))


def random_plane(ssize, cn, dtype, seed):
    """Samples over the whole range of the type (16-bit: all sixteen bits), none of them 0."""
    sw, sh = ssize
    shape = (sh, sw) if cn == 1 else (sh, sw, cn)
    return np.random.default_rng(seed).integers(1, np.iinfo(dtype).max + 1, shape, dtype)


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
STAGE_SIZES = [(800, 450), (804, 452)]
OUT_SIZES = [(0, 0), (1280, 720), (322, 182), (640, 360)]


def resolved(out_size, w, h):
    return (w, h) if out_size == (0, 0) else out_size


def stage_planes(planes, info, out_size):
    """(Y, U, V) of the result for a surface's three planes (h x w, h/2 x w/2 twice), its info8 and the resolved output size: the
    rectangle for Y, halved for U and V, each through reference(); the planes themselves where info8 says "not cropped"."""
    if not info[7]:
        return tuple(np.array(p) for p in planes)
    ow, oh = out_size
    cx, cy, cw, ch = (int(v) for v in info[2:6])
    ux, uy, uw, uh = cx // 2, cy // 2, max(1, cw // 2), max(1, ch // 2)
    y, u, v = planes
    return (reference(y[cy:cy + ch, cx:cx + cw], (ow, oh)), reference(u[uy:uy + uh, ux:ux + uw], (ow // 2, oh // 2)),
            reference(v[uy:uy + uh, ux:ux + uw], (ow // 2, oh // 2)))


_caches = {}


def cache(name):
    """A dictionary per name, for references that several tests of a session share (callers must not write into what they get)."""
    return _caches.setdefault(name, {})
