"""Crop-and-zoom on YUV surfaces, stated in numpy (include/vs_stab.h, vs_stab_set_yuv_crop_zoom and vs_op_resize_jobs).

With border_size = b every plane of a warped surface is cropped - (b, b, w - 2b, h - 2b) for Y, the same rectangle shifted right by
the plane's chroma shifts for U, V or the interleaved UV plane - and the crop is resized back to the plane's size:

* 8-bit planes: cv::resize(INTER_LINEAR) as oracle/vso_resize_linear_u8 restates it - source coordinate
  (float)((d + 0.5) * scale - 0.5) with scale = 1 / ((double)dst / src), 11-bit coefficients rounded and saturated to int16, the edge
  rule of HResizeLinear (from the first column whose right tap would leave the crop on: the sample times 2048), the vertical pass
  (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.  tests/test_yuv_cropzoom_cpu.py holds resize_u8 to the oracle.
* 16-bit planes: the same coordinates, the same four coefficients a0, a1, b0, b1 and the same edge rule; the blend is the exact
  integer S = sum of v_ij * a_i * b_j over the four taps with ONE rounding, half to even, at bit 22:
  min(65535, (S + 2^21 - 1 + ((S >> 22) & 1)) >> 22).  A definition of this library: OpenCV's CV_16U resize blends with float
  coefficients.

The taps clamp to the crop, never to the plane around it.  Plain integer numpy, no GPU, none of the library's code."""
import numpy as np

COEF = 2048                      # INTER_RESIZE_COEF_SCALE


def _round_half_even_f32(v):
    """cvRound of float32 values (np.rint rounds half to even, as lrintf does)."""
    return np.rint(v).astype(np.int64)


def axis_coefs(src, dst, edge_rule):
    """Per destination index of one axis: (tap 0's index, tap 1's index, coefficient of tap 0, of tap 1), int64.

    edge_rule True (columns): from the first column whose tap 1 would leave the source on, the sample itself times 2048.
    edge_rule False (rows): both tap rows are clamped into the source and the coefficients stay as computed."""
    scale = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if edge_rule:
        f = np.where(s < 0, np.float32(0), f).astype(np.float32)
        s = np.maximum(s, 0)
        edge = s + 1 >= src
        f = np.where(s >= src - 1, np.float32(0), f).astype(np.float32)
        s = np.minimum(s, src - 1)
    c0 = np.clip(_round_half_even_f32((np.float32(1) - f) * np.float32(COEF)), -32768, 32767)
    c1 = np.clip(_round_half_even_f32(f * np.float32(COEF)), -32768, 32767)
    if edge_rule:
        c0 = np.where(edge, COEF, c0)
        c1 = np.where(edge, 0, c1)
        return s, np.where(edge, s, s + 1), c0, c1
    return np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1), c0, c1


def _h_sums(plane, cn, dw, dh):
    """plane: (sh, sw * cn) samples.  -> h0, h1 (dh, dw, cn) int64 horizontal sums of the two tap rows, and b0, b1 (dh,)."""
    sh, row = plane.shape
    assert row % cn == 0
    sw = row // cn
    p = plane.reshape(sh, sw, cn).astype(np.int64)
    x0, x1, a0, a1 = axis_coefs(sw, dw, True)
    y0, y1, b0, b1 = axis_coefs(sh, dh, False)
    h = p[:, x0, :] * a0[None, :, None] + p[:, x1, :] * a1[None, :, None]          # (sh, dw, cn)
    return h[y0], h[y1], b0, b1


def resize_u8(plane, cn, dw, dh):
    """plane: uint8 (sh, sw * cn), possibly a view into a larger array -> uint8 (dh, dw * cn)."""
    assert plane.dtype == np.uint8
    h0, h1, b0, b1 = _h_sums(plane, cn, dw, dh)
    v = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return (v & 255).astype(np.uint8).reshape(dh, dw * cn)


def blend_sum_u16(plane, cn, dw, dh):
    """The exact integer S of every destination sample, (dh, dw * cn) int64 (at most 65535 * 2049 * 2049 < 2^39)."""
    h0, h1, b0, b1 = _h_sums(plane, cn, dw, dh)
    return (h0 * b0[:, None, None] + h1 * b1[:, None, None]).reshape(dh, dw * cn)


def resize_u16(plane, cn, dw, dh):
    """plane: uint16 (sh, sw * cn) -> uint16 (dh, dw * cn)."""
    assert plane.dtype == np.uint16
    S = blend_sum_u16(plane, cn, dw, dh)
    return np.minimum(65535, (S + (1 << 21) - 1 + ((S >> 22) & 1)) >> 22).astype(np.uint16)


def resize(plane, cn, dw, dh):
    return resize_u8(plane, cn, dw, dh) if plane.dtype == np.uint8 else resize_u16(plane, cn, dw, dh)


def plane_crop(b, sx, sy, pw, ph):
    """The crop of a plane of pw x ph samples whose chroma shifts are sx, sy (0, 0 for Y): x, y, cw, ch."""
    return b >> sx, b >> sy, pw - 2 * (b >> sx), ph - 2 * (b >> sy)


def crop_zoom_plane(plane, cn, b, sx=0, sy=0):
    """plane: (ph, pw * cn) -> the same shape: crop b luma pixels in from every side, zoom back."""
    ph, row = plane.shape
    pw = row // cn
    x, y, cw, ch = plane_crop(b, sx, sy, pw, ph)
    return resize(plane[y:y + ch, x * cn:(x + cw) * cn], cn, pw, ph)


def crop_zoom_surface(fmt, planes, b):
    """planes: the planes of one warped surface as 2-D arrays - (Y, UV) with UV of (h / 2, w) samples for the luma + interleaved
    chroma formats, (Y, U, V) for the three-plane formats.  fmt: (kind, sx, sy) with kind "uv" or "planar".  -> the planes of the
    result.  w - 2b <= 0 or h - 2b <= 0: the surface as it is (only warped)."""
    kind, sx, sy = fmt
    h, w = planes[0].shape
    if w - 2 * b <= 0 or h - 2 * b <= 0:
        return [p.copy() for p in planes]
    assert b % (1 << sx) == 0 and b % (1 << sy) == 0, "b must be a multiple of the chroma subsampling"
    out = [crop_zoom_plane(planes[0], 1, b)]
    if kind == "uv":
        out.append(crop_zoom_plane(planes[1], 2, b, sx, sy))
    else:
        out += [crop_zoom_plane(p, 1, b, sx, sy) for p in planes[1:]]
    return out
