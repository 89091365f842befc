"""Plain float64 statements of the analysis and warp operations, in numpy.

Independent of both the CPU oracle (oracle/) and the HIP library: each
function states one operation as math on continuous coordinates, with no
fixed point.  Border rules are np.pad modes: "reflect" is OpenCV's
REFLECT_101, "symmetric" is REFLECT, "edge" is REPLICATE, "constant" is a
zero border (docs/opencv_semantics.md).  The tests compare the oracle and the
kernels with these values under tolerances derived from the fixed-point
formats (tests/test_ref64_oracle.py, tests/test_gpu_ref64.py).
"""
import numpy as np

GRAY_W = (0.114, 0.587, 0.299)          # BGR -> gray, the ITU-R 601 luma weights
BORDERS = {"constant": "constant", "replicate": "edge", "reflect": "symmetric", "reflect101": "reflect"}


def invert_affine(M):
    """Inverse of a forward 2x3 matrix (given in float32 or float64), computed in float64."""
    M = np.asarray(M, np.float64).reshape(2, 3)
    A = np.linalg.inv(M[:, :2])
    return np.concatenate([A, -A @ M[:, 2:]], 1)


def _planes(img):
    img = np.asarray(img)
    return (img[..., None] if img.ndim == 2 else img).astype(np.float64)


def _window_max(D, ys, xs):
    """out[y, x] = max of D[y + j, x + i] over j in range(*ys), i in range(*xs) (zero outside D)."""
    h, w = D.shape[:2]
    Z = np.pad(D, ((2, 3), (2, 3), (0, 0)))
    out = np.zeros((h + 1, w + 1) + D.shape[2:], D.dtype)
    for j in range(*ys):
        for i in range(*xs):
            np.maximum(out, Z[2 + j:2 + j + h + 1, 2 + i:2 + i + w + 1], out=out)
    return out


def warp_affine(img, M, border="constant", dsize=None):
    """cv::warpAffine(INTER_LINEAR): dst(x, y) = bilinear src at Minv (x, y, 1), Minv the float64 inverse of the
    forward matrix M.  Returns (value, Lx, Ly): the float64 value of every destination sample, and the largest
    absolute difference between horizontally (Lx) and vertically (Ly) adjacent taps of the 3x3 source cells around
    the sample's cell (taps x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2), border taps included: a coordinate error below one
    pixel keeps the sample inside those cells."""
    src = _planes(img)
    h, w, cn = src.shape
    dw, dh = dsize if dsize else (w, h)
    Mi = invert_affine(M)
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    sx = Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2]
    sy = Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    # pad far enough that every tap of the 3x3 neighbourhood (x0 - 1 .. x0 + 2) is a padded index
    px = int(max(2, -x0.min() + 2, x0.max() + 3 - w)) if x0.size else 2
    py = int(max(2, -y0.min() + 2, y0.max() + 3 - h)) if y0.size else 2
    P = np.pad(src, ((py, py), (px, px), (0, 0)), mode=BORDERS[border])
    xi, yi = x0.astype(np.int64) + px, y0.astype(np.int64) + py

    def tap(dy, dx):
        return P[yi + dy, xi + dx]

    v00, v01, v10, v11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    fx, fy = fx[..., None], fy[..., None]
    val = (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)
    Lx = _window_max(np.abs(np.diff(P, axis=1)), (-1, 3), (-1, 2))[yi, xi]
    Ly = _window_max(np.abs(np.diff(P, axis=0)), (-1, 2), (-1, 3))[yi, xi]
    squeeze = (lambda a: a[..., 0]) if np.asarray(img).ndim == 2 else (lambda a: a)
    return squeeze(val), squeeze(Lx), squeeze(Ly)


def warp_affine_nv12(surf, w, h, M):
    """NV12 surface ((h * 3 / 2, w) bytes): Y warped with M, the interleaved (w/2 x h/2) UV plane with the same
    rotation and the translation halved.  Returns [(value, Lx, Ly) of Y, (value, Lx, Ly) of UV (h/2, w/2, 2)]."""
    surf = np.asarray(surf)
    M = np.asarray(M, np.float32).reshape(6)
    Mc = np.array([M[0], M[1], M[2] * np.float32(0.5), M[3], M[4], M[5] * np.float32(0.5)], np.float32)
    uv = surf[h:h + h // 2].reshape(h // 2, w // 2, 2)
    return [warp_affine(surf[:h], M), warp_affine(uv, Mc)]


def resize_coords(sn, dn):
    """INTER_LINEAR source coordinates of dn destination samples over sn source samples: (i0, i1, frac), the
    coordinate (d + 0.5) * sn / dn - 0.5 clamped to [0, sn - 1]."""
    c = (np.arange(dn, dtype=np.float64) + 0.5) * sn / dn - 0.5
    c = np.clip(c, 0, sn - 1)
    i0 = np.floor(c).astype(np.int64)
    i1 = np.minimum(i0 + 1, sn - 1)
    return i0, i1, c - i0


def resize_linear(img, dw, dh):
    """cv::resize(INTER_LINEAR) in float64, per channel; returns (value, L): L the largest difference between the
    taps a sample blends (horizontally or vertically)."""
    src = _planes(img)
    h, w, _ = src.shape
    x0, x1, fx = resize_coords(w, dw)
    y0, y1, fy = resize_coords(h, dh)
    fx, fy = fx[None, :, None], fy[:, None, None]
    a, b = src[y0][:, x0], src[y0][:, x1]
    c, d = src[y1][:, x0], src[y1][:, x1]
    val = (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)
    L = np.maximum.reduce([np.abs(b - a), np.abs(d - c), np.abs(c - a), np.abs(d - b)])
    if np.asarray(img).ndim == 2:
        return val[..., 0], L[..., 0]
    return val, L


def bgr2gray(bgr):
    """Luma of float64 BGR samples (..., 3)."""
    bgr = np.asarray(bgr, np.float64)
    return bgr[..., 0] * GRAY_W[0] + bgr[..., 1] * GRAY_W[1] + bgr[..., 2] * GRAY_W[2]


def round_half_up(v):
    return np.floor(np.asarray(v, np.float64) + 0.5)


def pyr_down(g):
    """cv::pyrDown: [1 4 6 4 1] x [1 4 6 4 1] / 256 with REFLECT_101, sampled at even coordinates; output
    ((w + 1) / 2, (h + 1) / 2).  Exact rational value (float64 holds it exactly)."""
    g = np.asarray(g, np.float64)
    h, w = g.shape
    k = np.array([1, 4, 6, 4, 1], np.float64)
    P = np.pad(g, 2, mode="reflect")
    rows = sum(k[i] * P[i:i + h] for i in range(5))                 # vertical pass, rows 0..h-1
    full = sum(k[i] * rows[:, i:i + w] for i in range(5))
    return full[0::2, 0::2] / 256.0


def scharr(g):
    """Scharr derivatives (dx, dy), [3 10 3] smoothing x [-1 0 1] difference, REFLECT_101: exact integers."""
    g = np.asarray(g, np.float64)
    h, w = g.shape
    P = np.pad(g, 1, mode="reflect")
    s = lambda dy, dx: P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    dx = 3 * (s(-1, 1) - s(-1, -1)) + 10 * (s(0, 1) - s(0, -1)) + 3 * (s(1, 1) - s(1, -1))
    dy = 3 * (s(1, -1) - s(-1, -1)) + 10 * (s(1, 0) - s(-1, 0)) + 3 * (s(1, 1) - s(-1, 1))
    return dx, dy


def structure_tensor(g, block_size=3):
    """cornerMinEigenVal's structure tensor: Sobel 3x3 on the image (REFLECT_101) scaled by 1 / (4 * blockSize * 255),
    products box-summed (unnormalised) over blockSize x blockSize with REFLECT_101.  Returns (A, B, C) = sums of
    dx^2, dx*dy, dy^2."""
    g = np.asarray(g, np.float64)
    h, w = g.shape
    P = np.pad(g, 1, mode="reflect")
    s = lambda dy, dx: P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    scale = 1.0 / (4 * block_size * 255.0)
    dx = ((s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))) * scale
    dy = ((s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))) * scale
    a = block_size // 2
    out = []
    for p in (dx * dx, dx * dy, dy * dy):
        Q = np.pad(p, ((a, block_size - 1 - a), (a, block_size - 1 - a)), mode="reflect")
        out.append(sum(Q[j:j + h, i:i + w] for j in range(block_size) for i in range(block_size)))
    return tuple(out)


def min_eigen(g, block_size=3):
    """Smaller eigenvalue of the structure tensor [[A, B], [B, C]] per pixel; returns (lambda_min, A + C)."""
    A, B, C = structure_tensor(g, block_size)
    T = np.stack([np.stack([A, B], -1), np.stack([B, C], -1)], -2)
    return np.linalg.eigvalsh(T)[..., 0], A + C


def similarity_lsq(src, dst):
    """Float64 least-squares similarity dst ~ [[a, -b], [b, a]] src + t; returns the 2x3 model as 6 values, or None
    when the points coincide (no scale is defined)."""
    p = np.asarray(src, np.float64).reshape(-1, 2)
    q = np.asarray(dst, np.float64).reshape(-1, 2)
    pc, qc = p - p.mean(0), q - q.mean(0)
    den = (pc ** 2).sum()
    if not den > 0:
        return None
    a = (pc[:, 0] * qc[:, 0] + pc[:, 1] * qc[:, 1]).sum() / den
    b = (pc[:, 0] * qc[:, 1] - pc[:, 1] * qc[:, 0]).sum() / den
    t = q.mean(0) - np.array([a * p[:, 0].mean() - b * p[:, 1].mean(), b * p[:, 0].mean() + a * p[:, 1].mean()])
    return np.array([a, -b, t[0], b, a, t[1]])


def apply_affine(M, pts):
    M = np.asarray(M, np.float64).reshape(2, 3)
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    return pts @ M[:, :2].T + M[:, 2]


def scene(w, h, Minv=None, seed=0, n_blobs=None):
    """A smooth textured scene rendered analytically in float64: Gaussian blobs of radius 3-8 px on a gentle
    gradient, sampled at Minv (x, y, 1) (the inverse of the motion applied to the scene; None: identity), rounded to
    uint8.  The same seed gives the same scene, so two renders differ exactly by the motion."""
    rng = np.random.default_rng(seed)
    n = n_blobs or max(8, w * h // 300)
    cx, cy = rng.uniform(-10, w + 10, n), rng.uniform(-10, h + 10, n)
    r = rng.uniform(3, 8, n)
    amp = rng.uniform(-90, 90, n)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    if Minv is not None:
        Mi = np.asarray(Minv, np.float64).reshape(2, 3)
        xs, ys = Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2], Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]
    v = 128 + 20 * np.sin(xs / 37.0) + 15 * np.cos(ys / 29.0)
    for i in range(n):
        d2 = (xs - cx[i]) ** 2 + (ys - cy[i]) ** 2
        near = d2 < (4 * r[i]) ** 2
        v[near] += amp[i] * np.exp(-d2[near] / (2 * r[i] ** 2))
    return np.clip(round_half_up(v), 0, 255).astype(np.uint8)


def bilinear(img, xs, ys):
    """Bilinear samples of a float64 image at continuous (xs, ys); every tap must lie inside the image."""
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = xs - x0, ys - y0
    h, w = img.shape
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < w and y0.max() + 1 < h, "window leaves the image"
    return ((1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) +
            fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1]))


def lk_track(prev, nxt, pt, win, iters, guess=None):
    """Single-level Lucas-Kanade (calcOpticalFlowPyrLK at maxLevel 0) in float64: the template window of prev around
    pt and its Scharr gradient (Scharr / 32, the derivative per pixel) are sampled bilinearly, then `iters`
    Gauss-Newton steps q <- q - G^-1 sum((J(q + d) - I(p + d)) grad I(p + d)) move the guess (default: pt).  Returns
    the position after each step."""
    I, J = np.asarray(prev, np.float64), np.asarray(nxt, np.float64)
    gx, gy = scharr(prev)
    hw = (win - 1) * 0.5
    oy, ox = np.mgrid[0:win, 0:win].astype(np.float64)
    px, py = pt[0] - hw + ox, pt[1] - hw + oy
    Iw, Gx, Gy = bilinear(I, px, py), bilinear(gx / 32, px, py), bilinear(gy / 32, px, py)
    G = np.array([[(Gx * Gx).sum(), (Gx * Gy).sum()], [(Gx * Gy).sum(), (Gy * Gy).sum()]])
    q = np.array(pt if guess is None else guess, np.float64)
    out = []
    for _ in range(iters):
        diff = bilinear(J, q[0] - hw + ox, q[1] - hw + oy) - Iw
        q = q - np.linalg.solve(G, [(diff * Gx).sum(), (diff * Gy).sum()])
        out.append(q.copy())
    return out
