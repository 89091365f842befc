"""Statements of the compositing stages, written from their definitions in numpy / scipy: the border pad, the fade blend and
its history, cv::resize's 8-bit linear upscale, and the virtual canvas (the reference's Stabilizer.cpp:914-990, 1069-1106,
2066-2443, with the OpenCV 4.11 primitives as docs/opencv_semantics.md lists them).  Nothing is imported from the oracle or the
library; the oracle (tests/test_compref_oracle.py) and the kernels (tests/test_gpu_compref.py) are both held to this file, and
every statement is exact: comparisons are array_equal.

    copy_make_border   cv::copyMakeBorder through border_index = cv::borderInterpolate by its definition
    fade_blend         cv::addWeighted on 8-bit data: fma(a, alpha, fl(b * beta)) in float32, rint, saturate; fade_real: the real a alpha + b beta
    fade_update        (uchar)((1 - 0.1f) * h + 0.1f * s): two float32 products, one float32 sum, truncation
    resize_linear_u8   cv::resize(INTER_LINEAR) on 8-bit data, upscaling (the only direction the canvas uses)
    warp_reflect       cv::warpAffine(INTER_LINEAR, BORDER_REFLECT): ref16_geom's warp with its REFLECT tap mode, half-up rounding
    canvas             one call of applyVirtualCanvasStabilization on a CanvasState
    fade_stream_step   the stream's host logic around the fade kernels

float32 arithmetic is numpy's float32 scalars and arrays: one IEEE operation per numpy operation, never contracted.
"""
import math

import numpy as np
from scipy import ndimage

import ref16
import ref16_geom

F = np.float32
BLACK, REFLECT, REFLECT_101, REPLICATE, WRAP = 0, 1, 2, 3, 4         # enum vs_border


# ---- border pad --------------------------------------------------------------------------------------------------------------------
def border_index(p, n, mode):
    """Source index of coordinate p (int array) on an axis of n samples; -1 where the constant border applies."""
    p = np.asarray(p, np.int64)
    if mode == BLACK:
        return np.where((p >= 0) & (p < n), p, -1)
    if mode == REPLICATE:
        return np.clip(p, 0, n - 1)
    if mode == WRAP:
        return np.mod(p, n)
    if mode == REFLECT:                         # ... c b a | a b c | c b a ...: even extension, period 2n
        return ref16_geom.reflect_index(p, n)
    assert mode == REFLECT_101                  # ... c b | a b c | b a ...: period 2n - 2; a single sample is repeated
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q >= n, 2 * n - 2 - q, q)


def border_passes(p, n, mode):
    """How many times the loop of cv::borderInterpolate (reflect, reflect-101) has to fold coordinate p, or for wrap how many
    periods p lies outside: 0 inside the axis."""
    p = np.asarray(p, np.int64)
    if mode == WRAP:
        return np.abs(np.floor_divide(p, n))
    if mode not in (REFLECT, REFLECT_101) or n == 1:
        return np.zeros_like(p)
    d = 1 if mode == REFLECT_101 else 0
    count = np.zeros_like(p)
    q = p.copy()
    while True:
        out = (q < 0) | (q >= n)
        if not out.any():
            return count
        q = np.where(q < 0, -q - 1 + d, np.where(q >= n, 2 * n - 1 - q - d, q))
        count += out


def copy_make_border(img, b, mode):
    img = np.asarray(img)
    h, w = img.shape[:2]
    iy = border_index(np.arange(-b, h + b), h, mode)
    ix = border_index(np.arange(-b, w + b), w, mode)
    out = img[np.clip(iy, 0, h - 1)][:, np.clip(ix, 0, w - 1)].copy()
    out[iy < 0] = 0
    out[:, ix < 0] = 0
    return out


NP_PAD = {BLACK: "constant", REFLECT: "symmetric", REFLECT_101: "reflect", REPLICATE: "edge", WRAP: "wrap"}


# ---- fade --------------------------------------------------------------------------------------------------------------------------
def fade_real(a, b, alpha, beta):
    """The real value a alpha + b beta for the float32 weights alpha and beta.  In float64 both products are exact (8 x 24 bits) and
    so is their sum while the weights are 0 or in [2^-20, 1]: it is below 2^9 and a multiple of 2^-44."""
    al, be = float(F(alpha)), float(F(beta))
    assert all(w == 0.0 or 2.0 ** -20 <= w <= 1.0 for w in (al, be))
    return np.asarray(a, np.float64) * al + np.asarray(b, np.float64) * be


def fade_blend(a, b, alpha, beta):
    """cv::addWeighted(a, alpha, b, beta, 0) on uint8: t = fl32(b * beta); v = fl32(a * alpha + t) (one rounding: a fused
    multiply-add); rint (half to even); saturate.  Each float32 rounding is taken from an exact float64 value."""
    al, be = float(F(alpha)), float(F(beta))
    assert all(w == 0.0 or 2.0 ** -20 <= w <= 1.0 for w in (al, be))
    t = (np.asarray(b, np.float64) * be).astype(np.float32)
    v = (np.asarray(a, np.float64) * al + t.astype(np.float64)).astype(np.float32)      # exact in float64, then rounded once
    return np.clip(np.rint(v.astype(np.float64)), 0, 255).astype(np.uint8)


def fade_update(h, s):
    """history <- (uchar)((1.0f - 0.1f) * h + 0.1f * s)"""
    rate = F(0.1)
    keep = F(1.0) - rate
    v = keep * np.asarray(h, np.uint8).astype(np.float32) + rate * np.asarray(s, np.uint8).astype(np.float32)
    assert v.dtype == np.float32
    return np.trunc(v).astype(np.uint8)


def fade_alpha(alpha, count, duration):
    """(alpha of this frame, count after it): alpha * (count / duration) in float32 while count < duration (Stabilizer.cpp:953-961)"""
    a = F(alpha)
    if count < duration:
        return a * (F(count) / F(duration)), count + 1
    return a, count


def fade_stream_step(hist, count, frame, b, alpha, duration):
    """The host logic of a fade stream before the warp: pad black; the first padded frame is the history; blend with the history.
    -> (blended padded frame, history to update, count, alpha used).  After the warp: history <- fade_update(history, output)."""
    padded = copy_make_border(frame, b, BLACK)
    if hist is None or hist.shape != padded.shape:
        hist, count = padded.copy(), 0
    a, count = fade_alpha(alpha, count, duration)
    return fade_blend(hist, padded, a, F(1.0) - a), hist, count, a


# ---- cv::resize, INTER_LINEAR, 8-bit, upscaling ------------------------------------------------------------------------------------
def _sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int64)


def _resize_axis(d, s):
    """(first tap, fraction) of every sample of a destination axis of d from a source axis of s, before any clamp: the source
    coordinate (x + 0.5) * scale - 0.5 in double, taken to float, floored; the fraction a float32 difference"""
    scale = 1.0 / (float(d) / float(s))                              # cv::resize: scale = 1 / inv_scale, in double
    f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    return i, f


def resize_linear_u8(img, dw, dh):
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    assert dw >= sw and dh >= sh, "upscaling only: downscales take other paths of cv::resize"
    src = img.reshape(sh, sw, -1).astype(np.int64)
    # columns: the tap pair (sx, sx + 1) with 11-bit weights; from the first column whose pair would leave the row, one tap times 2048
    sx, fx = _resize_axis(dw, sw)
    fx = np.where(sx < 0, F(0), fx)
    sx = np.maximum(sx, 0)
    single = sx + 1 >= sw
    fx = np.where(sx >= sw - 1, F(0), fx)
    sx = np.minimum(sx, sw - 1)
    assert np.all(np.diff(sx) >= 0)                                  # (so "from the first such column on" is "every such column")
    a0 = _sat16(np.rint((F(1) - fx) * F(2048)))
    a1 = _sat16(np.rint(fx * F(2048)))
    x1 = np.minimum(sx + 1, sw - 1)
    rows = np.where(single[None, :, None], src[:, sx] * 2048, src[:, sx] * a0[None, :, None] + src[:, x1] * a1[None, :, None])
    # rows: the fraction is not clamped, the row indices are
    sy, fy = _resize_axis(dh, sh)
    b0 = _sat16(np.rint((F(1) - fy) * F(2048)))
    b1 = _sat16(np.rint(fy * F(2048)))
    S0 = rows[np.clip(sy, 0, sh - 1)]
    S1 = rows[np.clip(sy + 1, 0, sh - 1)]
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape((dh, dw) + img.shape[2:])


# ---- the reflect warp --------------------------------------------------------------------------------------------------------------
def warp_reflect(img, M):
    """cv::warpAffine(img, M (double, forward), img.size(), INTER_LINEAR, BORDER_REFLECT) on uint8"""
    return ref16_geom.warp(np.asarray(img, np.uint8), M, None, ref16_geom.REFLECT, ref16.HALF_UP)


def reflect_tap_passes(shape, M, x0, y0, x1, y1):
    """Folds needed by the taps of the destination pixels [y0, y1) x [x0, x1): (n taps, n that fold, n that fold more than once).
    A tap = one of the four (column, row) pairs; its folds = the larger of its two axes'."""
    sh, sw = shape[:2]
    sx, sy, _, _ = ref16.coords(np.asarray(M, np.float64), sw, sh)
    sx, sy = sx[y0:y1, x0:x1], sy[y0:y1, x0:x1]
    n = once = twice = 0
    for dx in (0, 1):
        for dy in (0, 1):
            p = np.maximum(border_passes(sx + dx, sw, REFLECT), border_passes(sy + dy, sh, REFLECT))
            n += p.size
            once += int((p >= 1).sum())
            twice += int((p >= 2).sum())
    return n, once, twice


def _midpoint_margin(d):
    """Distance of the double d from the nearest rounding boundary of float32, in float32 ulps of d"""
    if d == 0.0:
        return 1.0
    m, e = math.frexp(abs(d))                                        # |d| = m 2^e, m in [0.5, 1)
    ulp = 2.0 ** (max(e, -125) - 24)
    q = abs(d) / ulp                                                 # the boundaries are at k + 0.5
    return abs(q - math.floor(q) - 0.5)


def cos_sin32(x):
    """(cosf(x), sinf(x)) of the float32 x as any faithful float32 libm gives them: the float64 values rounded to float32.
    The sincosf kernels of glibc that video-stab_amd/csrc/vs_libm.h restates (sysdeps/ieee754/flt-32/s_sincosf.c, the ARM
    optimized-routines code) document a worst-case error of 0.5607 ulp (quoted from that source's comment, not re-derived here); such a function can return another float than the
    correctly rounded one only where the true value lies within 0.0607 ulp of a rounding boundary.  Every angle that reaches this
    function must keep its cosine and sine 1/8 ulp away from one (math.cos / math.sin in double are far more accurate than that),
    and tests/test_compref_oracle.py also asks the host's own cosf / sinf for the same angles."""
    x = float(F(x))
    c, s = math.cos(x), math.sin(x)
    assert _midpoint_margin(c) >= 0.125 and _midpoint_margin(s) >= 0.125, "angle %r: too close to a float32 rounding boundary" % x
    ANGLES_USED.add(x)
    return F(c), F(s)


ANGLES_USED = set()


# ---- the virtual canvas ------------------------------------------------------------------------------------------------------------
def _inter(a, b):
    """cv::Rect_::operator&: (x, y, w, h), the empty rectangle as (0, 0, 0, 0)"""
    x, y = max(a[0], b[0]), max(a[1], b[1])
    w, h = min(a[0] + a[2], b[0] + b[2]) - x, min(a[1] + a[3], b[1] + b[3]) - y
    return (0, 0, 0, 0) if w <= 0 or h <= 0 else (x, y, w, h)


EIGHT = np.ones((3, 3), bool)
FOUR = ndimage.generate_binary_structure(2, 1)


def external_regions(mask):
    """Bounding boxes (x, y, w, h) of the 8-connected components of `mask` that no other component encloses (those that touch the
    picture's border or the background connected to it), in the order of cv::findContours(RETR_EXTERNAL)'s vector: a component is
    found at its first pixel in raster order and every finished contour goes to the head of the list, so the last found comes
    first."""
    mask = np.asarray(mask, bool)
    lab, n = ndimage.label(mask, structure=EIGHT)
    if n == 0:
        return []
    bl, _ = ndimage.label(np.pad(~mask, 1, constant_values=True), structure=FOUR)
    outside = bl == bl[0, 0]                                         # padded: the frame around the picture is outside
    near = ndimage.binary_dilation(outside, structure=FOUR)[1:-1, 1:-1]
    ext = np.unique(lab[near & mask])
    first = {}
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    labs, pos = np.unique(flat[idx], return_index=True)              # first occurrence of each label in raster order
    for l, q in zip(labs, idx[pos]):
        first[int(l)] = int(q)
    boxes = []
    sl = ndimage.find_objects(lab)
    for l in sorted((int(v) for v in ext), key=lambda v: -first[v]):
        ys, xs = sl[l - 1]
        boxes.append((xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start))
    return boxes


def empty_mask(bgr):
    """gray <= 1 with cv::cvtColor's 8-bit BGR2GRAY: (3735 B + 19235 G + 9798 R + 2^14) >> 15"""
    v = np.asarray(bgr, np.uint8).astype(np.int64)
    return ((v[..., 0] * 3735 + v[..., 1] * 19235 + v[..., 2] * 9798 + (1 << 14)) >> 15) <= 1


class CanvasState:
    """What survives between two calls: the temporal buffer, the scale, the canvas geometry.  stats counts the branches taken."""

    def __init__(self):
        self.frames, self.ts = [], []
        self.have_canvas = False
        self.cols = self.rows = 0
        self.scale, self.scale_init = F(0), False
        self.cw = self.ch = 0
        self.cx = self.cy = F(0)
        self.stats = dict(calls=0, fills=0, stretch=0, no_stretch=0, stretch_two_sides=0, ringed=0, mask=0, mask_3_regions=0, older_chosen=0,
                          newest_refused=0, none_available=0, no_fit=0, clamped=set(), reinit=0, other_size=0, taps=0, taps_fold=0,
                          taps_fold_twice=0, regions_small=0)
        self.fill_log = []          # per call: [(region, buffer index)] in blend order


def optimal_scale(p, transforms):
    """calculateOptimalCanvasSize (:2281-2314), float32 throughout"""
    tr = np.asarray(transforms, np.float32).reshape(-1, 3)
    n = len(tr)
    if n == 0:
        return F(p.canvas_scale_factor)
    mx = F(0)
    for i in range(n - min(30, n), n):
        a, b = tr[i, 0], tr[i, 1]
        mx = max(mx, np.sqrt(a * a + b * b))
    factor = max(F(1), mx / F(50))
    s = F(p.canvas_scale_factor) + (factor - F(1)) * F(0.5)
    return max(F(p.min_canvas_scale), min(F(p.max_canvas_scale), s))


def _fill(frame, region, rel, st):
    """extractTemporalRegion (:2316-2347): the buffered frame motion-compensated, cut to the moved region, stretched if clipped"""
    c, s = cos_sin32(-rel[2])
    M = np.array([c, -s, -rel[0], s, c, -rel[1]], np.float32).astype(np.float64)
    if rel[2] == 0:
        assert c == 1 and s == 0 and M[1] == 0 and M[3] == 0             # the identity rotation, exactly
    comp = warp_reflect(frame, M)
    fh, fw = frame.shape[:2]
    moved = (region[0] + int(rel[0]), region[1] + int(rel[1]), region[2], region[3])
    x, y, w, h = _inter(moved, (0, 0, fw, fh))
    assert w > 0 and h > 0 and x >= 0 and y >= 0 and x + w <= fw and y + h <= fh
    n, once, twice = reflect_tap_passes(frame.shape, M, x, y, x + w, y + h)
    st["taps"] += n; st["taps_fold"] += once; st["taps_fold_twice"] += twice
    cut = comp[y:y + h, x:x + w]
    if (w, h) == (region[2], region[3]):
        st["no_stretch"] += 1
        return cut
    st["stretch"] += 1
    st["stretch_two_sides"] += int(w != region[2] and h != region[3])
    return resize_linear_u8(cut, region[2], region[3])


def blend_region(canvas, fill, region, weight, edge_blend_radius):
    """seamlessBlend (:2349-2403) in place: alpha = weight, times (distance to the region's edge / radius) inside the edge band"""
    x0, y0, w, h = region
    radius = min(int(edge_blend_radius), min(w, h) // 4)
    ys, xs = np.mgrid[0:h, 0:w]
    dist = np.minimum(np.minimum(xs, ys), np.minimum(w - xs - 1, h - ys - 1)).astype(np.float32)
    alpha = np.full((h, w), F(1.0) * F(weight), np.float32)
    if radius > 0:
        alpha = np.where(dist < F(radius), alpha * (dist / F(radius)), alpha).astype(np.float32)
    t = canvas[y0:y0 + h, x0:x0 + w].astype(np.float32)
    v = (F(1.0) - alpha)[..., None] * t + alpha[..., None] * fill.astype(np.float32)
    assert v.dtype == np.float32 and v.min() >= 0 and v.max() < 256
    canvas[y0:y0 + h, x0:x0 + w] = np.trunc(v).astype(np.uint8)


def canvas(state, p, frame, t, transforms=None, fill_order=None):
    """One call.  p: any object with vs_params_c's canvas fields; frame (h, w, 3) uint8; t = (dx, dy, da); transforms (n, 3) = the
    past transforms (read when the scale is chosen).  -> (output (h, w, 3), info8 int32).  fill_order: a permutation applied to the
    list of fills before they are blended (to show that their order matters); None = the list's order."""
    st = state
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    t = np.asarray(t, np.float32).reshape(3)
    tr = np.zeros((0, 3), np.float32) if transforms is None else np.asarray(transforms, np.float32).reshape(-1, 3)
    S = st.stats
    S["calls"] += 1
    if not st.scale_init:
        st.scale, st.scale_init = F(p.canvas_scale_factor), True
    # updateTemporalFrameBuffer (:2151-2167): the frame joins the buffer before it is looked at
    st.frames.append(frame.copy()); st.ts.append(t.copy())
    while len(st.frames) > int(p.temporal_buffer_size):
        st.frames.pop(0); st.ts.pop(0)
    # (:2066-2149)
    if not st.have_canvas or st.cols != int(F(w) * st.scale) or st.rows != int(F(h) * st.scale):
        S["reinit"] += 1
        st.scale = optimal_scale(p, tr) if p.adaptive_canvas_size and len(tr) else F(p.canvas_scale_factor)
        st.cw, st.ch = int(F(w) * st.scale), int(F(h) * st.scale)
        assert 1 <= st.cw <= 65535 and 1 <= st.ch <= 32767
        st.cx, st.cy = F(st.cw) / F(2), F(st.ch) / F(2)
    cw, ch = st.cw, st.ch
    # createVirtualCanvas (:2169-2212)
    cv = np.zeros((ch, cw, 3), np.uint8)
    frame_rect = (int(st.cx - F(w) / F(2)), int(st.cy - F(h) / F(2)), w, h)
    valid = _inter(frame_rect, (0, 0, cw, ch))
    if valid[2] > 0 and valid[3] > 0:
        sx, sy = valid[0] - frame_rect[0], valid[1] - frame_rect[1]
        if sx >= 0 and sy >= 0 and sx + valid[2] <= w and sy + valid[3] <= h:
            cv[valid[1]:valid[1] + valid[3], valid[0]:valid[0] + valid[2]] = frame[sy:sy + valid[3], sx:sx + valid[2]]
    st.have_canvas, st.cols, st.rows = True, cw, ch
    # blendTemporalRegions (:2214-2279)
    n_regions = n_fills = 0
    last_best = -1
    nbuf = len(st.frames)
    log = []
    if nbuf >= 2:
        ringed = valid[2] == w and valid[3] == h and valid[0] > 0 and valid[1] > 0 and valid[0] + w < cw and valid[1] + h < ch
        boxes = external_regions(empty_mask(cv))
        if ringed:
            assert boxes == [(0, 0, cw, ch)]          # the black ring encloses everything else
            S["ringed"] += 1
        else:
            S["mask"] += 1
        regions = [b for b in boxes if b[2] * b[3] > 100]
        S["regions_small"] += len(boxes) - len(regions)
        S["mask_3_regions"] += int(not ringed and len(regions) >= 3)
        n_regions = len(regions)
        fills = []
        for region in regions:
            best, best_w, best_rel = -1, F(0), None
            avail = []
            for i in range(nbuf - 1):
                rel = t - st.ts[i]                                     # float32
                fh, fw = st.frames[i].shape[:2]
                moved = (region[0] + int(rel[0]), region[1] + int(rel[1]), region[2], region[3])
                it = _inter(moved, (0, 0, fw, fh))
                coverage = F(it[2] * it[3]) / F(region[2] * region[3])
                avail.append(bool(coverage > F(0.5)))
                if not avail[-1]:
                    continue
                wgt = F(i + 1) / F(nbuf)
                wgt = wgt * F(p.canvas_blend_weight)
                if wgt > best_w:
                    best, best_w, best_rel = i, wgt, rel
            S["none_available"] += int(not any(avail))
            if best >= 0 and best_w > 0:
                newest = nbuf - 2
                S["newest_refused"] += int(not avail[newest])
                S["older_chosen"] += int(best < newest)
                S["other_size"] += int(st.frames[best].shape[:2] != (h, w))
                fills.append((region, best, best_w, best_rel))
                n_fills += 1
                last_best = best
        order = range(len(fills)) if fill_order is None else fill_order(len(fills))
        for k in order:
            region, best, best_w, best_rel = fills[k]
            blend_region(cv, _fill(st.frames[best], region, best_rel, S), region, best_w, p.edge_blend_radius)
            log.append((region, best))
        S["fills"] += n_fills
    st.fill_log.append(log)
    # the window (:2115-2149)
    ox, oy = st.cx - F(w) / F(2) - t[0], st.cy - F(h) / F(2) - t[1]
    ex_x, ex_y, ex_w, ex_h = max(0, int(ox)), max(0, int(oy)), w, h
    if int(ox) < 0: S["clamped"].add("left")
    if int(oy) < 0: S["clamped"].add("top")
    if ex_x > cw - ex_w: S["clamped"].add("right")
    if ex_y > ch - ex_h: S["clamped"].add("bottom")
    ex_x, ex_y = min(ex_x, cw - ex_w), min(ex_y, ch - ex_h)
    ex_w, ex_h = min(ex_w, cw - ex_x), min(ex_h, ch - ex_y)
    info = np.array([cw, ch, int(np.array([st.scale], np.float32).view(np.int32)[0]), n_regions, n_fills, last_best, ex_x, ex_y], np.int32)
    if ex_w > 0 and ex_h > 0 and ex_x >= 0 and ex_y >= 0 and ex_x + ex_w <= cw and ex_y + ex_h <= ch:
        assert (ex_w, ex_h) == (w, h)                  # so the reference's LANCZOS4 resize of the window never runs
        return cv[ex_y:ex_y + h, ex_x:ex_x + w].copy(), info
    S["no_fit"] += 1
    return frame.copy(), info                          # :2148 the frame as it came
