"""Inputs shared by tests/test_ref64_oracle.py and tests/test_gpu_ref64.py: images, matrices, LK scenes and the LK
ground-truth check (every quantity against tests/ref64.py)."""
import numpy as np

import ref64


def ramp(h, w, cn=1, sx=3.0, sy=2.0, base=20.0):
    """Linear ramp, slope sx (sy) levels per pixel along x (y), channels offset by 17 levels; clipped to 0..255."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.stack([base + 17 * c + sx * x + sy * y for c in range(cn)], -1)
    v = np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return v[..., 0] if cn == 1 else v


def smooth(h, w, cn=1, seed=0):
    """A mix of sinusoids, a few levels per pixel."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for c in range(cn):
        a = r.uniform(0.02, 0.2, 4)
        ch.append(128 + 50 * np.sin(a[0] * x + a[1] * y + c) + 40 * np.cos(a[2] * x - a[3] * y))
    v = np.clip(np.floor(np.stack(ch, -1) + 0.5), 0, 255).astype(np.uint8)
    return v[..., 0] if cn == 1 else v


def noise(h, w, cn=1, seed=0):
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


def const(h, w, cn=1, v=173):
    return np.full((h, w) if cn == 1 else (h, w, cn), v, np.uint8)


IMAGES = {"ramp": ramp, "smooth": smooth, "noise": noise, "const": const}
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (7, 13), (31, 17), (97, 131)]


def rot(deg, w, h, s=1.0, tx=0.0, ty=0.0):
    """Forward similarity about the image centre, then a shift, as float32 (the stabilizer's matrix type)."""
    t = np.deg2rad(deg)
    c, sn = s * np.cos(t), s * np.sin(t)
    cx, cy = w / 2.0, h / 2.0
    return np.array([c, -sn, cx - c * cx + sn * cy + tx, sn, c, cy - sn * cx - c * cy + ty], np.float32)


def matrices(w, h):
    return {
        "identity": np.array([1, 0, 0, 0, 1, 0], np.float32),
        "subpixel": np.array([1, 0, 0.37, 0, 1, -0.61], np.float32),
        "rot+0.7": rot(0.7, w, h, tx=0.3),
        "rot-1.3": rot(-1.3, w, h, ty=-0.2),
        "rot30": rot(30, w, h),
        "rot90": rot(90, w, h),
        "rot180": rot(180, w, h),
        "scale0.5": rot(0, w, h, 0.5),
        "scale2": rot(0, w, h, 2.0),
        "shear": np.array([1, 0.21, -3.3, 0.07, 1, 1.7], np.float32),
        "mirror": np.array([-1, 0, w - 1, 0, 1, 0], np.float32),
        "leaves": np.array([1, 0, 0.75 * w + 0.25, 0, 1, -0.8 * h - 0.5], np.float32),
    }


RAMP_MOTIONS = [(17.0, 1.0), (-31.0, 1.0), (7.0, 1.05), (3.0, 1.0), (-11.0, 0.97), (45.0, 1.0), (61.0, 1.0),
                (-77.0, 1.02)]



# Ground truth: a scene rendered analytically in float64 (ref64.scene), moved by a known forward matrix, rounded once.
# A translation-only window tracker is biased under rotation by about (angle x the offset of the window's gradient
# energy from its centre), so the rotations stay small.  Well-conditioned points: the smaller eigenvalue of the
# window's gradient tensor, per pixel, is at least LK_COND levels^2/px^2.
LK_COND = 10.0
LK_MEDIAN, LK_MAX = 0.02, 0.1     # px; the oracle measures about 0.01 and 0.045 at win 15


def lk_points(w, h, n, margin, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1).astype(np.float32)


def lk_conditioned(g, pts, win):
    gx, gy = ref64.scharr(g)
    hw = (win - 1) * 0.5
    oy, ox = np.mgrid[0:win, 0:win].astype(np.float64)
    out = []
    for p in pts:
        X, Y = ox + p[0] - hw, oy + p[1] - hw
        Gx, Gy = ref64.bilinear(gx / 32, X, Y), ref64.bilinear(gy / 32, X, Y)
        G = np.array([[(Gx * Gx).sum(), (Gx * Gy).sum()], [(Gx * Gy).sum(), (Gy * Gy).sum()]]) / win ** 2
        out.append(np.linalg.eigvalsh(G)[0] >= LK_COND)
    return np.array(out)


LK_MOTIONS = {"shift": np.array([1, 0, 0.83, 0, 1, -0.57]),
              "rotation": np.array([np.cos(0.003), -np.sin(0.003), 0.61, np.sin(0.003), np.cos(0.003), -0.44])}


def lk_scene(w, h, motion):
    M = LK_MOTIONS[motion]
    return ref64.scene(w, h, seed=3, n_blobs=w * h // 70), ref64.scene(w, h, ref64.invert_affine(M), seed=3,
                                                                      n_blobs=w * h // 70), M


def check_lk_truth(out, st, pts, M, good, what=""):
    if not good.any():
        return
    assert np.all(st[good] == 1), what
    e = np.linalg.norm(out - ref64.apply_affine(M, pts), axis=1)[good]
    assert np.median(e) <= LK_MEDIAN and e.max() <= LK_MAX, "%s: median %.4f max %.4f" % (what, np.median(e), e.max())
