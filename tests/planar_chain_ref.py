"""The reference of roll correction and auto zoom/crop on three-plane surfaces of any subsampling (I420 ... I412), in numpy integers,
on top of tests/ref16_geom.py: include/vs_stab.h's definitions with the chroma shifts (sx, sy) made explicit.

A surface is three planes (Y (h, w), U and V ((h >> sy), (w >> sx))), uint8 or uint16 with the value in the low bits; `fmt` is a
format NAME of planar_inputs ("I422", "I210", ...).

    rotate_planar       Y under the double matrix M of cv::getRotationMatrix2D((w / 2.0f, h / 2.0f), angle, 1), U and V under
                        Mc = S^-1 M S, S = diag(2^sx, 2^sy) - exact products by powers of two -, BORDER_REPLICATE
    crop_scale_planar   the rectangle of info8 on Y, (x >> sx, y >> sy, max(1, cw >> sx), max(1, ch >> sy)) on U and V; Y scaled to
                        ow x oh, U and V to (ow >> sx) x (oh >> sy) by the CV_32F scale matrix, BORDER_CONSTANT 0; the unchanged planes
                        when info8 says "not cropped"
    roll_planar, azc_planar   the same with angle and info8 from the ORACLE's NV12 objects run on the analysis plane of Y (Y itself, or
                        min(sample >> (bits - 8), 255)) with a flat chroma plane behind it - angle, line counts, mask and contours do
                        not look at chroma -, as ref16_geom.roll_p010 / azc_p010 do: no line search or contour code is restated.
The blend is ref16's S, rounded HALF_UP for 8-bit planes (cv::warpAffine's 8-bit arithmetic) and HALF_EVEN for 16-bit planes (P010's
blend).  tests/test_planar_chain_cpu.py pins the 8-bit half to the oracle's cv::warpAffine per plane and the (1, 1) case to
ref16_geom.rotate_surface / crop_scale_surface."""
import numpy as np

import planar_inputs as pin
import ref16_geom as geom
from ref16 import HALF_EVEN, HALF_UP

ALL = dict(pin.FORMATS, **pin.OLD)        # name -> (format value, sx, sy, bits)


def shifts(fmt):
    return ALL[fmt][1], ALL[fmt][2]


def bits(fmt):
    return ALL[fmt][3]


def rounding(fmt):
    return HALF_UP if bits(fmt) == 8 else HALF_EVEN


def plane_shapes(fmt, w, h):
    sx, sy = shifts(fmt)
    return (h, w), (h >> sy, w >> sx), (h >> sy, w >> sx)


def chroma_matrix(M, sx, sy):
    """S^-1 M S in double: [[m0, m1 2^(sy - sx), m2 / 2^sx], [m3 2^(sx - sy), m4, m5 / 2^sy]]."""
    return [M[0], M[1] * 2.0 ** (sy - sx), M[2] / 2.0 ** sx, M[3] * 2.0 ** (sx - sy), M[4], M[5] / 2.0 ** sy]


def roll_matrices(fmt, w, h, angle):
    M, _ = geom.roll_matrices(w, h, angle)
    return M, chroma_matrix(M, *shifts(fmt))


def rotate_planar(planes, fmt, angle):
    h, w = planes[0].shape
    M, Mc = roll_matrices(fmt, w, h, angle)
    r = rounding(fmt)
    return [geom.warp(planes[0], M, None, geom.REPLICATE, r), geom.warp(planes[1], Mc, None, geom.REPLICATE, r),
            geom.warp(planes[2], Mc, None, geom.REPLICATE, r)]


def zoom_jobs(info, sx, sy, ow, oh):
    """[(x, y, w, h, dw, dh, M)] for Y and for a chroma plane: M = [fx 0 0; 0 fy 0] held as CV_32F, used as double."""
    cx, cy, cw, ch = (int(v) for v in info[2:6])
    ux, uy, uw, uh = cx >> sx, cy >> sy, max(1, cw >> sx), max(1, ch >> sy)
    My = [float(np.float32(float(ow) / cw)), 0.0, 0.0, 0.0, float(np.float32(float(oh) / ch)), 0.0]
    Mu = [float(np.float32(float(ow >> sx) / uw)), 0.0, 0.0, 0.0, float(np.float32(float(oh >> sy) / uh)), 0.0]
    return [(cx, cy, cw, ch, ow, oh, My), (ux, uy, uw, uh, ow >> sx, oh >> sy, Mu)]


def crop_scale_planar(planes, fmt, info8, ow, oh):
    """[Y (oh, ow), U, V ((oh >> sy), (ow >> sx))], or copies of the unchanged planes when info8[7] == 0."""
    if not info8[7]:
        return [np.array(p) for p in planes]
    (x0, y0, cw, ch, dw, dh, My), (x1, y1, uw, uh, dw2, dh2, Mu) = zoom_jobs(info8, *shifts(fmt), ow, oh)
    r = rounding(fmt)
    return [geom.warp(planes[0][y0:y0 + ch, x0:x0 + cw], My, (dw, dh), geom.CONSTANT, r),
            geom.warp(planes[1][y1:y1 + uh, x1:x1 + uw], Mu, (dw2, dh2), geom.CONSTANT, r),
            geom.warp(planes[2][y1:y1 + uh, x1:x1 + uw], Mu, (dw2, dh2), geom.CONSTANT, r)]


def analysis_nv12(planes, fmt):
    """The NV12 surface the oracle's objects are run on: the analysis plane of Y with a flat chroma plane behind it."""
    y8 = pin.analysis_byte(planes[0], bits(fmt))
    h, w = y8.shape
    return np.ascontiguousarray(np.concatenate([y8, np.full((h // 2, w), 128, np.uint8)]))


def roll_planar(planes, fmt, oracle_roll):
    """One surface through the roll stage.  oracle_roll: the oracle's roll object (it carries the smoothed angle from frame to frame);
    its NV12 call on the analysis surface advances it, its smoothed angle after that call rotates the planes."""
    h, w = planes[0].shape
    oracle_roll.correct_nv12(analysis_nv12(planes, fmt), w, h)
    return rotate_planar(planes, fmt, oracle_roll.state()[0])


def azc_planar(planes, fmt, oracle, ow=640, oh=360):
    """(planes of the result, info8); (ow, oh) = (0, 0): the surface's own size."""
    h, w = planes[0].shape
    _, info = oracle.auto_zoom_crop_nv12(analysis_nv12(planes, fmt), w, h)
    return crop_scale_planar(planes, fmt, info, ow or w, oh or h), info
