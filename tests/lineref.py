"""Plain numpy / scipy statements of the roll stage's line search and of the zoom stage's content mask.

Independent of the CPU oracle (oracle/vso_roll.cpp, oracle/vso_azc.cpp) and of the HIP library: written from OpenCV's
documented definitions of cv::Sobel, cv::Canny (L1 gradient, aperture 3), cv::HoughLines (standard transform) and
cv::morphologyEx(MORPH_CLOSE) - docs/opencv_semantics.md - with every loop of those functions stated as array
arithmetic, and the hysteresis as what it computes: the connected components of the candidate set that hold a strong
pixel.  All results are exact (integers, or floats formed by the same float32 / float64 operations), so the tests
compare with array_equal: the oracle in tests/test_lineref_oracle.py, the kernels in tests/test_gpu_lineref.py.
"""
import math
from types import SimpleNamespace

import numpy as np
from scipy import ndimage

import ref64_checks

PI = 3.1415926535897932384626433832795
TG22 = 13573                     # tan(22.5 deg) * 2^15, rounded
HOUGH_CAP = 8192                 # peaks the library keeps (include/vs_stab.h, vs_op_hough_lines)


# ---- Sobel, Canny -------------------------------------------------------------------------------------------------
def sobel(g):
    """(dx, dy), int64: dx = [-1 0 1] x [1 2 1]^T, dy its transpose, on the picture with a replicated border."""
    P = np.pad(np.asarray(g).astype(np.int64), 1, mode="edge")
    h, w = P.shape[0] - 2, P.shape[1] - 2
    s = lambda j, i: P[j:j + h, i:i + w]
    dx = (s(0, 2) + 2 * s(1, 2) + s(2, 2)) - (s(0, 0) + 2 * s(1, 0) + s(2, 0))
    dy = (s(2, 0) + 2 * s(2, 1) + s(2, 2)) - (s(0, 0) + 2 * s(0, 1) + s(0, 2))
    return dx, dy


def canny_candidates(g, low, high):
    """(candidates, strong): the local maxima above `low` and, of those, the ones above `high` (bool maps)."""
    if low > high:
        low, high = high, low
    low, high = math.floor(low), math.floor(high)
    dx, dy = sobel(g)
    h, w = dx.shape
    mag = np.abs(dx) + np.abs(dy)
    M = np.pad(mag, 1)                                   # a frame of zeros: nothing outside the picture competes
    at = lambda j, i: M[1 + j:1 + j + h, 1 + i:1 + i + w]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    horizontal = ay < ax * TG22
    vertical = ay > ax * (TG22 + (1 << 16))
    same_sign = (dx < 0) == (dy < 0)                     # zero counts as non-negative
    is_max = np.where(horizontal, (mag > at(0, -1)) & (mag >= at(0, 1)),
             np.where(vertical, (mag > at(-1, 0)) & (mag >= at(1, 0)),
             np.where(same_sign, (mag > at(-1, -1)) & (mag > at(1, 1)),
                                 (mag > at(-1, 1)) & (mag > at(1, -1)))))
    cand = is_max & (mag > low)
    return cand, cand & (mag > high)


def canny(g, low, high):
    """cv::Canny(g, low, high, 3, L2gradient=false) as uint8 0 / 255."""
    cand, strong = canny_candidates(g, low, high)
    lab, n = ndimage.label(cand, structure=np.ones((3, 3), int))
    keep = np.zeros(n + 1, bool)
    keep[lab[strong]] = True
    keep[0] = False
    return np.where(keep[lab], 255, 0).astype(np.uint8)


# ---- HoughLines ---------------------------------------------------------------------------------------------------
def hough_geometry(w, h, rho, theta):
    """(numangle, numrho) as cv::HoughLines forms them for min_theta 0, max_theta pi."""
    theta = float(np.float32(theta))
    numangle = math.floor(PI / theta) + 1
    if numangle > 1 and abs(PI - (numangle - 1) * theta) < theta / 2:
        numangle -= 1
    # (max_rho - min_rho + 1) / rho is a float32 division of an int by the float rho, rounded to nearest even
    numrho = int(np.rint(np.float32(2 * (w + h) + 1) / np.float32(rho)))
    return numangle, numrho


def hough_accumulator(edges, rho, theta):
    """The (numangle + 2, numrho + 2) int64 vote array with its frame of zeros."""
    edges = np.asarray(edges)
    h, w = edges.shape
    rho32, theta32 = np.float32(rho), np.float32(theta)
    numangle, numrho = hough_geometry(w, h, rho32, theta32)
    irho = float(np.float32(1) / rho32)
    ang = np.empty(numangle, np.float32)
    a = np.float32(0)
    for n in range(numangle):                            # float32 accumulation, as the table is built
        ang[n] = a
        a = np.float32(a + theta32)
    tab_sin = (np.sin(ang.astype(np.float64)) * irho).astype(np.float32)
    tab_cos = (np.cos(ang.astype(np.float64)) * irho).astype(np.float32)
    ys, xs = np.nonzero(edges)
    accum = np.zeros((numangle + 2, numrho + 2), np.int64)
    if len(xs):
        px = xs.astype(np.float32)[:, None] * tab_cos[None, :]          # each product rounded to float32 by itself
        py = ys.astype(np.float32)[:, None] * tab_sin[None, :]
        r = np.rint((px + py).astype(np.float32)).astype(np.int64) + (numrho - 1) // 2
        n = np.broadcast_to(np.arange(numangle)[None, :], r.shape)
        np.add.at(accum, (n + 1, r + 1), 1)
    return accum


def hough_lines(edges, rho, theta, threshold, cap=None):
    """cv::HoughLines(edges, rho, theta, threshold): (n, 2) float32 rows (rho, theta), votes descending, ties by ascending
    accumulator index; cap: keep the first `cap` lines of that order."""
    accum = hough_accumulator(edges, rho, theta)
    numangle, numrho = accum.shape[0] - 2, accum.shape[1] - 2
    c = accum[1:-1, 1:-1]
    peak = ((c > threshold) & (c > accum[1:-1, :-2]) & (c >= accum[1:-1, 2:]) &
            (c > accum[:-2, 1:-1]) & (c >= accum[2:, 1:-1]))
    n, r = np.nonzero(peak)
    index = (n + 1) * (numrho + 2) + r + 1
    order = np.lexsort((index, -c[n, r]))
    n, r = n[order], r[order]
    if cap is not None:
        n, r = n[:cap], r[:cap]
    lines = np.empty((len(n), 2), np.float32)
    half = np.float32((numrho - 1) * 0.5)
    lines[:, 0] = (r.astype(np.float32) - half) * np.float32(rho)
    lines[:, 1] = n.astype(np.float32) * np.float32(theta)
    return lines


# ---- the roll stage's angle statistics and recurrence ---------------------------------------------------------------
def roll_params(**kw):
    """The defaults of RollCorrection.h; fields as in vs_roll_params_c."""
    p = SimpleNamespace(scale_factor=0.25, canny_threshold_low=50.0, canny_threshold_high=150.0, hough_rho=np.float32(1.0),
                        hough_theta=np.float32(PI / float(np.float32(180.0))), hough_threshold=100, angle_filter_min=-10.0,
                        angle_filter_max=10.0, angle_smoothing_alpha=0.1, angle_decay=0.995, max_angle_change_deg=0.5)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def roll_step(state, analysis_gray, params, cap=HOUGH_CAP):
    """One frame of the roll stage on its analysis image.  state: the smoothed angle before the frame (degrees); returns
    (smoothed, detected, n_lines, n_used), the tuple the objects' state() gives."""
    p = params
    edges = canny(analysis_gray, p.canny_threshold_low, p.canny_threshold_high)
    lines = hough_lines(edges, p.hough_rho, p.hough_theta, p.hough_threshold, cap=cap)
    total, count = 0.0, 0
    for th in lines[:, 1]:
        deg = float(th) * 180.0 / PI - 90.0
        if p.angle_filter_min <= deg <= p.angle_filter_max:
            total += deg
            count += 1
    if count == 0:
        return state * p.angle_decay, 0.0, len(lines), 0
    detected = total / count
    new = p.angle_smoothing_alpha * detected + (1.0 - p.angle_smoothing_alpha) * state
    diff = new - state
    if p.max_angle_change_deg > 0.0 and abs(diff) > p.max_angle_change_deg:
        new = state + (p.max_angle_change_deg if diff > 0 else -p.max_angle_change_deg)
    return new, detected, len(lines), count


def roll_run(images, params, cap=HOUGH_CAP):
    """The states after each analysis image of a sequence, starting from angle 0."""
    out, s = [], 0.0
    for g in images:
        st = roll_step(s, g, params, cap)
        out.append(st)
        s = st[0]
    return out


# ---- analysis image of a frame --------------------------------------------------------------------------------------
def bgr2gray(img):
    p = np.asarray(img).astype(np.int64)
    return ((3735 * p[..., 0] + 19235 * p[..., 1] + 9798 * p[..., 2] + (1 << 14)) >> 15).astype(np.uint8)


def analysis_image(frame, scale_factor):
    """The picture the line search runs on.  frame: a gray / luma plane (h, w) or a BGR frame (h, w, 3), uint8; scale_factor 1, or
    0.5 / 0.25 on sides divisible by 2 / 4, where INTER_LINEAR is exactly the mean of the 2 x 2 block at the sample's centre."""
    frame = np.asarray(frame)
    if scale_factor == 1.0:
        return bgr2gray(frame) if frame.ndim == 3 else frame.copy()
    step = {0.5: 2, 0.25: 4}[scale_factor]
    assert frame.shape[0] % step == 0 and frame.shape[1] % step == 0
    if frame.ndim == 2:
        return ref64_checks.exact_mean2x2(frame, step).astype(np.uint8)
    return bgr2gray(np.stack([ref64_checks.exact_mean2x2(frame[..., c], step) for c in range(3)], axis=-1))


# ---- content mask of auto zoom/crop ---------------------------------------------------------------------------------
ELLIPSE5 = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], bool)


def content_mask(img):
    """gray > 1, closed with the 5 x 5 ellipse; pixels outside the picture take part in neither half."""
    img = np.asarray(img)
    g = bgr2gray(img) if img.ndim == 3 else img
    d = ndimage.binary_dilation(g > 1, structure=ELLIPSE5, border_value=0)
    e = ndimage.binary_erosion(d, structure=ELLIPSE5, border_value=1)
    return np.where(e, 255, 0).astype(np.uint8)
