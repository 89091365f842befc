"""Tolerances that hold a fixed-point result (oracle or HIP kernel) against the float64 statements of ref64.py.

Each bound is derived from the fixed-point format of the operation; the comment at each constant says how.  The
same checks run on the CPU oracle (test_ref64_oracle.py) and on the kernels (test_gpu_ref64.py), so neither is
judged by the other.
"""
import numpy as np

import ref64

# ---- warpAffine (WarpAffineInvoker + remapBilinear, 8U) -------------------------------------------------------------
# The source coordinate is formed in AB_BITS = 10 fixed point from two rounded terms (adelta[x] and the row term),
# each within 2^-11 px, so within 2^-10 px together; it is then rounded to INTER_BITS = 5 (1/32 px) with +16, an error
# of at most 1/64 px.  The 15-bit bilinear weights of a 1/32 grid point are exact products, so the sum before the
# final rounding is the bilinear value at a coordinate at most 1/64 + 2^-10 px away per axis.  The bilinear value
# moves by at most Lx (Ly) per pixel along x (y) within the cells that coordinate error can reach; the final
# (t + 2^14) >> 15 adds at most 0.5.  (The saturated (0, 0) table entry 32767 + 1 only arises at integer coordinates,
# where it cannot change the rounded byte.)
WARP_COORD_ERR = 1.0 / 64 + 2.0 ** -10
WARP_ROUND = 0.5
TINY = 1e-6
# Mean signed error over the interior of a linear ramp, pooled over rotations that spread the sample fractions over
# the grid.  The coordinate rounding (round half up on the 1/1024 grid) leaves about +0.002 on a slope-8 ramp.  The
# final (t + 2^14) >> 15 is round half up too, and on a ramp of integer taps the bilinear value at 1/32 px steps lands
# on an exact .5 far more often than once in 1024: those ties add +0.020 to +0.024 per rotation, inherent to OpenCV's
# format.  Together about +0.03, plus sampling noise (std of the mean <= 0.005 over >= 5000 samples); the bound is
# 0.06, under half of the signature of truncating the 1/32 coordinate instead of rounding it (every sample moves by
# 1/64 px: -0.125 on a slope-8 ramp).
WARP_RAMP_BIAS = 0.06


def warp_bound(Lx, Ly):
    return WARP_ROUND + WARP_COORD_ERR * (Lx + Ly) + TINY


def check_warp(dev, img, M, border="constant", dsize=None, what=""):
    """Per-pixel bound of a warped uint8 image; returns the largest |error| / bound."""
    val, Lx, Ly = ref64.warp_affine(img, M, border, dsize)
    return check_warp_planes(dev, val, Lx, Ly, what)


def check_warp_planes(dev, val, Lx, Ly, what=""):
    err = np.abs(np.asarray(dev, np.float64) - val)
    b = warp_bound(Lx, Ly)
    bad = err > b
    assert not bad.any(), "%s: %d samples outside the warp bound, first at %s: dev %s ref %.4f bound %.4f" % (
        what, bad.sum(), np.argwhere(bad)[0], np.asarray(dev)[bad][0], val[bad][0], b[bad][0])
    return float((err / b).max()) if err.size else 0.0


def warp_interior_errors(dev, img, M):
    """Signed errors (dev - ref) of a warped image at the samples whose four taps lie inside the source."""
    val, _, _ = ref64.warp_affine(img, M)
    h, w = np.asarray(img).shape[:2]
    Mi = ref64.invert_affine(M)
    ys, xs = np.mgrid[0:val.shape[0], 0:val.shape[1]].astype(np.float64)
    sx = Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2]
    sy = Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]
    inside = (sx >= 1) & (sx <= w - 2) & (sy >= 1) & (sy <= h - 2)
    return (np.asarray(dev, np.float64) - val)[inside]


def check_warp_nv12(dev, surf, w, h, M, what=""):
    (vy, lxy, lyy), (vc, lxc, lyc) = ref64.warp_affine_nv12(surf, w, h, M)
    r1 = check_warp_planes(dev[:h], vy, lxy, lyy, what + " Y")
    r2 = check_warp_planes(dev[h:h + h // 2].reshape(h // 2, w // 2, 2), vc, lxc, lyc, what + " UV")
    return max(r1, r2)


# ---- resize INTER_LINEAR 8U + BGR2GRAY ------------------------------------------------------------------------------
# Per channel (HResizeLinear + VResizeLinear, INTER_RESIZE_COEF_BITS = 11):
#  * the source coordinate is computed in float (error <= 2^-13 px below 4096) and the weights are rounded to
#    1/2048 (error <= 2^-12): at most 2^-12 + 2^-13 px per axis, times the largest tap difference L;
#  * the vertical pass truncates three times: S >> 4 (< 15/16 of 1/128 of a level, weighted by b0 + b1 = 2048:
#    < 2^-7 after >> 16 / 4), then each of the two (b * (S >> 4)) >> 16 (< 1/4 of a level each), then
#    (F + 2) >> 2 rounds half up: dev - ref lies in (-(1 + 2^-7), 0.5] before the coordinate term.
RESIZE_COORD_ERR = 2 * (2.0 ** -12 + 2.0 ** -13)          # both axes, times L
RESIZE_LO = 1.0 + 2.0 ** -7
RESIZE_HI = 0.5
# cvtColor's 15-bit weights (3735, 19235, 9798) / 32768 differ from 0.114 / 0.587 / 0.299 by 3.4e-5 in sum, times
# 255 levels; the gray step rounds half up once more ((... + 2^14) >> 15).
GRAY_COEF_ERR = 255 * (abs(3735 / 32768 - 0.114) + abs(19235 / 32768 - 0.587) + abs(9798 / 32768 - 0.299))
GRAY_ROUND = 0.5


def check_resize_channels(dev, img, dw, dh, what=""):
    """Signed per-sample bound of a resized uint8 image (any channel count); returns (worst low, worst high) errors."""
    val, L = ref64.resize_linear(img, dw, dh)
    e = np.asarray(dev, np.float64) - val
    lo, hi = -(RESIZE_LO + RESIZE_COORD_ERR * L) - TINY, RESIZE_HI + RESIZE_COORD_ERR * L + TINY
    bad = (e < lo) | (e > hi)
    assert not bad.any(), "%s: %d samples outside the resize bound, first at %s: err %.4f" % (
        what, bad.sum(), np.argwhere(bad)[0], e[bad][0])
    return float(e.min()), float(e.max())


def check_resize_gray(dev, bgr, dw, dh, what=""):
    """Analysis gray image of a BGR frame: ref64 resize of every channel, then the float64 luma.  Returns the share
    of samples that differ from the rounded float64 luma by one level or more (near-ties of the two roundings)."""
    val, L = ref64.resize_linear(bgr, dw, dh)
    ref = ref64.bgr2gray(val)
    Lg = L.max(axis=-1)
    e = np.asarray(dev, np.float64) - ref
    lo = -(RESIZE_LO + RESIZE_COORD_ERR * Lg + GRAY_COEF_ERR + GRAY_ROUND) - TINY
    hi = RESIZE_HI + RESIZE_COORD_ERR * Lg + GRAY_COEF_ERR + GRAY_ROUND + TINY
    bad = (e < lo) | (e > hi)
    assert not bad.any(), "%s: %d gray samples outside the bound, first at %s: err %.4f" % (
        what, bad.sum(), np.argwhere(bad)[0], e[bad][0])
    return float((np.abs(np.asarray(dev, np.float64) - ref64.round_half_up(ref)) >= 1).mean())


def exact_mean2x2(plane, step):
    """The exact 2x and 4x INTER_LINEAR value: the mean of the 2x2 source block at the sample's centre (offset 0 for
    2x, 1 for 4x), rounded half up."""
    p = np.asarray(plane, np.int64)
    o = (step - 2) // 2
    h, w = p.shape[0] // step, p.shape[1] // step
    s = lambda dy, dx: p[o + dy::step, o + dx::step][:h, :w]
    return (s(0, 0) + s(0, 1) + s(1, 0) + s(1, 1) + 2) // 4


# ---- min-eigenvalue map ---------------------------------------------------------------------------------------------
# Float32 formation (oracle/vso_gftt.cpp, cornerEigenValsVecs' scalar order):
#  * relative terms: f1 = (float)(1/(4*bs*255)) and the roundings of dx, of each product and of each box sum are
#    relative errors of a few 2^-24 of terms bounded by A + C; the final (a+c) - sqrt((a-c)^2 + b^2) adds a few more.
#    2^-20 (16 ulps) covers them.
#  * the cancellation in dy: dy = t(y+1) - t(y-1) with t = c*f0 + (a+b)*f1 <= 1/3 rounded three times, so every dy
#    carries an absolute error below 1.5 * 2^-24 whatever its size.  Summed over the 3x3 box it moves C by at most
#    2 * 1.5 * 2^-24 * sum|dy| <= 9 * 2^-24 * sqrt(C) and B by 4.5 * 2^-24 * sqrt(A) if all nine errors align;
#    they are independent roundings, so the bound takes sqrt(9) = 3 of the nine: 2^-23 * sqrt(A + C).
#    (The oracle's worst is 0.6 * 2^-23 * sqrt(A + C) over the CPU test images.)
EIG_REL = 2.0 ** -20
EIG_SQRT = 2.0 ** -23
EIG_ABS = 1e-12


def min_eigen_tol(tr):
    return EIG_REL * tr + EIG_SQRT * np.sqrt(tr) + EIG_ABS


def check_min_eigen(dev, g, block_size=3, what=""):
    lam, tr = ref64.min_eigen(g, block_size)
    err = np.abs(np.asarray(dev, np.float64) - lam)
    b = min_eigen_tol(tr)
    bad = err > b
    assert not bad.any(), "%s: %d eigenvalues outside the bound, first at %s: dev %.9g ref %.9g" % (
        what, bad.sum(), np.argwhere(bad)[0], np.asarray(dev)[bad][0], lam[bad][0])
    return float((err / b).max())


# ---- goodFeaturesToTrack, as properties of the float64 map ----------------------------------------------------------
def _max8(a):
    """Largest of the 8 neighbours of every pixel; neighbours outside the map are ignored (-inf), as in the 3x3 dilation."""
    h, w = a.shape
    P = np.pad(a, 1, constant_values=-np.inf)
    return np.max([P[j:j + h, i:i + w] for j in range(3) for i in range(3) if (j, i) != (1, 1)], axis=0)


def check_gftt(pts, g, max_corners, quality, min_distance, block_size=3, what=""):
    """Corners against the ref64 map, with the min-eigen tolerance t on every comparison of lambda (the kernel's value of a
    pixel lies within lam +- t):
    * at most max_corners, on whole pixels, never on the outermost row or column (goodFeaturesToTrack's scan);
    * each is above quality * max and a 3x3 local maximum; the order is non-increasing; pairs are min_distance apart;
    * completeness: every pixel that is surely a selectable local maximum (lam - t above the threshold's upper end and
      above lam + t of all 8 neighbours) and surely stronger than the last kept corner (when the list is full) is kept,
      or lies within min_distance of a kept corner that may be at least as strong - the only reason the greedy
      min-distance pass drops a candidate."""
    lam, tr = ref64.min_eigen(g, block_size)
    tol = min_eigen_tol(tr)
    h, w = lam.shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    assert max_corners <= 0 or len(pts) <= max_corners, what
    thr_lo = quality * (lam.max() - tol.max())
    thr_hi = quality * (lam.max() + tol.max())
    if len(pts):
        assert np.all(pts == np.round(pts)), what
        xi, yi = pts[:, 0].astype(int), pts[:, 1].astype(int)
        assert xi.min() >= 1 and yi.min() >= 1 and xi.max() <= w - 2 and yi.max() <= h - 2, "%s: a corner on the border" % what
        v, t = lam[yi, xi], tol[yi, xi]
        assert np.all(v + t > thr_lo), "%s: a corner below quality * max" % what
        assert np.all(v[1:] <= v[:-1] + t[1:] + t[:-1]), "%s: corners out of order" % what
        assert np.all(v + t >= _max8(lam - tol)[yi, xi]), "%s: a corner that is not a local maximum" % what
        if min_distance >= 1 and len(pts) > 1:
            d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
            np.fill_diagonal(d2, np.inf)
            assert d2.min() >= min_distance ** 2, "%s: two corners %.3f px apart" % (what, np.sqrt(d2.min()))
    surely = (lam - tol >= _max8(lam + tol)) & (lam - tol > thr_hi)
    surely[[0, -1], :] = False
    surely[:, [0, -1]] = False
    if max_corners > 0 and len(pts) == max_corners:
        surely &= lam - tol > v[-1] + t[-1]          # visited before the list filled up
    kept = set(zip(yi.tolist(), xi.tolist())) if len(pts) else set()
    for y, x in np.argwhere(surely):
        if (y, x) in kept:
            continue
        if len(pts) and min_distance >= 1:
            near = (pts[:, 0] - x) ** 2 + (pts[:, 1] - y) ** 2 < min_distance ** 2
            if np.any(v[near] + t[near] >= lam[y, x] - tol[y, x]):
                continue
        raise AssertionError("%s: local maximum (%d, %d) = %.6g is missing with no stronger kept corner near it" % (
            what, x, y, lam[y, x]))
    return int(surely.sum())


# ---- estimateAffinePartial2D ----------------------------------------------------------------------------------------
SIM_REL = 1e-9        # the refinement is the closed-form least squares in double: it must agree to double accuracy


def check_similarity_model(model, src, dst, inliers, what=""):
    """The model equals the float64 least-squares similarity on the reported inlier set."""
    inl = np.asarray(inliers).astype(bool)
    ref = ref64.similarity_lsq(np.asarray(src, np.float64)[inl], np.asarray(dst, np.float64)[inl])
    assert ref is not None, what
    model = np.asarray(model, np.float64).reshape(6)
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(model - ref).max()
    assert err <= SIM_REL * scale, "%s: model %s, float64 least squares %s" % (what, model, ref)


def similarity_case(n, outlier_share, seed, extent=1000.0, sigma=0.3):
    """n correspondences under a random similarity: inliers with N(0, sigma) noise, outliers at least 20 px off."""
    rng = np.random.default_rng(seed)
    ang, s = rng.uniform(-0.05, 0.05), rng.uniform(0.97, 1.03)
    M = np.array([s * np.cos(ang), -s * np.sin(ang), rng.uniform(-8, 8),
                  s * np.sin(ang), s * np.cos(ang), rng.uniform(-8, 8)])
    src = rng.uniform(0, extent, (n, 2))
    dst = ref64.apply_affine(M, src) + rng.normal(0, sigma, (n, 2))
    n_out = int(round(n * outlier_share))
    out = rng.permutation(n)[:n_out]
    off = rng.uniform(20, 80, n_out) * np.exp(1j * rng.uniform(0, 2 * np.pi, n_out))
    dst[out, 0] += off.real
    dst[out, 1] += off.imag
    truth = np.ones(n, np.uint8)
    truth[out] = 0
    return src.astype(np.float32), dst.astype(np.float32), truth, M
