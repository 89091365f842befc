"""The corner selection of cv::goodFeaturesToTrack as a numpy statement: from a float32 min-eigenvalue map to the list of
corners.  It is written from OpenCV's definition (imgproc/src/featureselect.cpp), not from the oracle's loops
(oracle/vso_gftt.cpp) and not from the kernels (k_gftt.hip: nms_row, select_corners); tests/test_gfttref_oracle.py holds it
against the oracle, tests/test_gpu_gftt_ties.py holds the kernels against it.

The definition:

  * threshold(eig, eig, maxVal * qualityLevel, 0, THRESH_TOZERO): maxVal is a double, the product is taken in double and
    rounded to the map's float; a value stays when it is strictly larger, everything else becomes 0.
  * dilate(eig, tmp, 3 x 3); a candidate is a pixel of the interior (the one-pixel frame is not visited) with
    val != 0 && val == tmp: equality, so every pixel of a plateau is a candidate.  The dilation ignores what lies outside
    the map, and because no value is negative after the threshold that is the same as a border of zeros.
  * std::sort(greaterThanPtr): value descending; among equal values the higher address, i.e. the larger y * w + x, first.
  * minDistance >= 1: walk the list, reject a candidate when dx*dx + dy*dy < minDistance * minDistance to any point accepted
    before it, stop at maxCorners accepted.  dx and dy are integers below 2^16: the float sum of squares is exact.
  * minDistance < 1: the head of the list, maxCorners long.

The distance test here is brute force over ALL accepted points.  OpenCV looks only into the 3 x 3 grid cells around the
candidate's cell, with cells of cell = cvRound(minDistance) pixels.  That finds the same conflicts: cvRound rounds to
nearest, so cell >= minDistance - 0.5.  Two points closer than minDistance have an integer |dx| < minDistance; the largest
integer below minDistance is at most the nearest integer to minDistance, so |dx| <= cell, and likewise |dy| <= cell.  Two
coordinates that differ by at most one cell size lie in the same cell or in neighbouring ones.  Every accepted point that
can reject a candidate is therefore among the nine cells searched, and the points of all other cells pass the distance test.
"""
import numpy as np


def threshold(eig, quality):
    """float32(float64(max) * quality), as cv::threshold receives it"""
    return np.float32(np.float64(eig.max()) * np.float64(quality))


def candidates(eig, quality):
    """Flat indices y * w + x of the candidates in sort order (value descending, index descending), and their values."""
    eig = np.asarray(eig)
    assert eig.dtype == np.float32 and eig.ndim == 2
    h, w = eig.shape
    if h < 3 or w < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    t = np.where(eig > threshold(eig, quality), eig, np.float32(0))
    assert (t >= 0).all()              # what makes a zero border equal to an ignored one
    p = np.pad(t, 1)
    dil = t
    for j in range(3):
        for i in range(3):
            dil = np.maximum(dil, p[j:j + h, i:i + w])
    is_cand = (t != 0) & (t == dil)
    is_cand[0, :] = is_cand[-1, :] = False
    is_cand[:, 0] = is_cand[:, -1] = False
    idx = np.flatnonzero(is_cand).astype(np.int64)
    val = t.reshape(-1)[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))        # the last key is the first: value descending, then index descending
    return idx[order], val[order]


def select(eig, max_corners, quality, min_distance):
    """(points (n, 2) float32 as x, y; number of candidates)"""
    h, w = np.asarray(eig).shape
    idx, _ = candidates(eig, quality)
    xs, ys = idx % w, idx // w
    if not min_distance >= 1:
        keep = np.arange(len(idx))[:max_corners if max_corners > 0 else None]
    else:
        md2 = float(min_distance) * float(min_distance)
        ax, ay = np.zeros(len(idx), np.int64), np.zeros(len(idx), np.int64)
        keep, n = [], 0
        for k in range(len(idx)):
            dx, dy = ax[:n] - xs[k], ay[:n] - ys[k]
            if n and ((dx * dx + dy * dy) < md2).any():
                continue
            ax[n], ay[n] = xs[k], ys[k]
            n += 1
            keep.append(k)
            if max_corners > 0 and n == max_corners:
                break
        keep = np.asarray(keep, np.int64)
    pts = np.stack([xs[keep], ys[keep]], axis=1).astype(np.float32).reshape(-1, 2)
    return pts, len(idx)
