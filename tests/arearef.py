"""Area-averaging downscale, stated in numpy and `math` (include/vs_stab.h: vs_op_area_jobs, vs_op_area_yuv, vs_op_area_rgb,
vs_area_axis_table).  None of the library's code.

cv::resize(INTER_AREA) for dst <= src on both axes.  Per axis scale = 1.0 / ((double)dst / src) and i = rint(scale); the axis is
integer when |scale - i| < DBL_EPSILON.  A job has a class:

2  both axes integer with i = 2: (s00 + s01 + s10 + s11 + 2) >> 2 at both depths and every cn.
1  both axes integer otherwise: S = the exact integer sum of the ix * iy samples, out = rint_half_even((float)S * (1.f / (ix * iy))).
0  every other job, both axes through computeResizeAreaTab's taps (axis_taps below): float32 sums, every product and every sum
   rounded on its own - per tap row, ascending: buf = 0, buf += (float)S[sx] * alpha over the column taps, ascending; first tap
   row: sum = beta * buf, later ones: sum += beta * buf; out = rint_half_even(sum).

Every result is clamped to 0 .. max_value (0 = the sample type's maximum)."""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
F32 = np.float32


def scale_of(src, dst):
    return 1.0 / (float(dst) / float(src))


def axis_integer(src, dst):
    """-> (is the axis integer, i)."""
    scale = scale_of(src, dst)
    i = int(np.rint(scale))
    return abs(scale - i) < DBL_EPSILON, i


def job_class(sw, sh, dw, dh):
    (x, ix), (y, iy) = axis_integer(sw, dw), axis_integer(sh, dh)
    if not (x and y):
        return 0
    return 2 if ix == 2 and iy == 2 else 1


def axis_taps(src, dst):
    """computeResizeAreaTab: per destination index the list of (source index, weight as a Python float = double), in tap order.
    The float32 weight of a tap is np.float32(weight)."""
    assert 1 <= dst <= src
    scale = scale_of(src, dst)
    out = []
    for d in range(dst):
        f1 = d * scale
        f2 = f1 + scale
        cw = min(scale, src - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, src - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, (s1 - f1) / cw))
        for sx in range(s1, s2):
            taps.append((sx, 1.0 / cw))
        if f2 - s2 > 1e-3:
            taps.append((s2, min(min(f2 - s2, 1.0), cw) / cw))
        out.append(taps)
    return out


def axis_table(src, dst):
    """-> first, count (int64) and w_first, w_mid, w_last (float32), dst entries each: vs_area_axis_table's output.  Asserts what
    the compact form rests on: contiguous taps, at least one, indices inside the source, all middle weights equal."""
    scale = scale_of(src, dst)
    taps = axis_taps(src, dst)
    first, count = np.empty(dst, np.int64), np.empty(dst, np.int64)
    wf, wm, wl = np.empty(dst, F32), np.empty(dst, F32), np.empty(dst, F32)
    for d, t in enumerate(taps):
        idx = [s for s, _ in t]
        assert len(t) >= 1 and idx == list(range(idx[0], idx[0] + len(t))) and idx[0] >= 0 and idx[-1] <= src - 1, (src, dst, d, t)
        mid = F32(1.0 / min(scale, src - d * scale))
        assert all(F32(w) == mid for _, w in t[1:-1]), (src, dst, d)
        first[d], count[d] = idx[0], len(t)
        wf[d], wm[d], wl[d] = F32(t[0][1]), mid, F32(t[-1][1])
    return first, count, wf, wm, wl


def _planes(plane, cn):
    sh, row = plane.shape
    assert plane.dtype in (np.uint8, np.uint16) and row % cn == 0
    return sh, row // cn


def resize(plane, cn, dw, dh, max_value=0):
    """plane: uint8 or uint16 (sh, sw * cn), possibly a view into a larger array -> the same dtype, (dh, dw * cn)."""
    dtype = plane.dtype
    sh, sw = _planes(plane, cn)
    assert dw <= sw and dh <= sh
    top = max_value or int(np.iinfo(dtype).max)
    cls = job_class(sw, sh, dw, dh)
    if cls:
        ix, iy = sw // dw, sh // dh
        assert ix * dw == sw and iy * dh == sh
        S = plane.reshape(dh, iy, dw, ix, cn).astype(np.int64).sum(axis=(1, 3))
        if cls == 2:
            v = (S + 2) >> 2
        else:
            inv = F32(1) / F32(ix * iy)
            v = np.rint(S.astype(F32) * inv).astype(np.int64)
        return np.clip(v, 0, top).astype(dtype).reshape(dh, dw * cn)
    p = plane.reshape(sh, sw, cn).astype(F32)
    xt, yt = axis_taps(sw, dw), axis_taps(sh, dh)
    # buf of every source row: (sh, dw, cn), products and sums in float32, taps ascending
    buf = np.zeros((sh, dw, cn), F32)
    nx = max(len(t) for t in xt)
    for k in range(nx):
        cols = [d for d in range(dw) if len(xt[d]) > k]
        sx = np.array([xt[d][k][0] for d in cols])
        a = np.array([xt[d][k][1] for d in cols]).astype(F32)
        buf[:, cols, :] = buf[:, cols, :] + p[:, sx, :] * a[None, :, None]
    out = np.empty((dh, dw, cn), F32)
    for d, t in enumerate(yt):
        s = F32(t[0][1]) * buf[t[0][0]]
        for sy, b in t[1:]:
            s = s + F32(b) * buf[sy]
        out[d] = s
    assert buf.dtype == F32 and out.dtype == F32
    return np.clip(np.rint(out).astype(np.int64), 0, top).astype(dtype).reshape(dh, dw * cn)


def resize_f64(plane, cn, dw, dh):
    """The general arithmetic with the double weights in float64, not rounded: (dh, dw * cn) float64, and the job's largest tap
    counts (nx, ny)."""
    sh, sw = _planes(plane, cn)
    p = plane.reshape(sh, sw, cn).astype(np.float64)
    xt, yt = axis_taps(sw, dw), axis_taps(sh, dh)
    buf = np.zeros((sh, dw, cn))
    for d, t in enumerate(xt):
        for sx, a in t:
            buf[:, d, :] += p[:, sx, :] * a
    out = np.zeros((dh, dw, cn))
    for d, t in enumerate(yt):
        for sy, b in t:
            out[d] += buf[sy] * b
    return out.reshape(dh, dw * cn), max(len(t) for t in xt), max(len(t) for t in yt)
