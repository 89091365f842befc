"""The CPU oracle against the float64 statements of tests/ref64.py (no GPU).

The GPU parity tests hold the kernels to the oracle bit for bit; these hold the oracle itself to the plain math of
each operation, under the fixed-point tolerances of tests/ref64_checks.py, so that a misreading shared by the
oracle and a kernel (a half-pixel offset, a border rule, truncation for rounding, a scale, a stop rule) fails here.
"""
import numpy as np
import pytest

import ref64
import ref64_checks as rc
from ref64_inputs import (IMAGES, LK_MOTIONS, RAMP_MOTIONS, SHAPES, check_lk_truth, const, lk_conditioned, lk_points,
                          lk_scene, matrices, noise, ramp, rot, smooth)

# ---- warpAffine -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cn", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_warp_affine_within_bound(oracle, kind, cn):
    worst = 0.0
    for (h, w) in SHAPES:
        img = IMAGES[kind](h, w, cn)
        for name, M in matrices(w, h).items():
            worst = max(worst, rc.check_warp(oracle.warp_affine(img, M), img, M, what="%s %dx%d cn%d %s" % (
                kind, w, h, cn, name)))
    # the derivation is not loose: smooth content reaches most of the bound
    if kind in ("smooth", "noise"):
        assert worst > 0.5


def test_warp_affine_exact_cases(oracle):
    img = smooth(31, 17, 3)
    # (rot90 about (w/2, h/2) of a non-square image lands on half pixels: not exact)
    for name in ("identity", "rot180", "mirror"):
        M = matrices(17, 31)[name]
        val, _, _ = ref64.warp_affine(img, M)
        assert np.array_equal(oracle.warp_affine(img, M), ref64.round_half_up(val)), name


@pytest.mark.parametrize("border,code", [("replicate", 3), ("reflect", 1), ("constant", 0)])
def test_warp_affine_other_borders_within_bound(oracle, border, code):
    for (h, w) in [(1, 1), (2, 7), (31, 17), (97, 131)]:
        for cn in (1, 3):
            img = smooth(h, w, cn, seed=2)
            for name, M in matrices(w, h).items():
                M64 = M.astype(np.float64)
                rc.check_warp(oracle.warp_affine_d(img, M64, code), img, M64, border,
                              what="%s %dx%d cn%d %s" % (border, w, h, cn, name))


@pytest.mark.parametrize("slopes", [(7.7, 0.53), (0.53, 7.7), (2.1, 1.7)])
def test_warp_affine_ramp_is_unbiased(oracle, slopes):
    # Ramps of slope up to 7.7 levels / px, sized so every value stays inside 0..255, under rotations that spread the
    # sample fractions over the 1/32 grid.  (A pure translation does not: every sample then shares one fraction, and
    # its rounding error is the same constant everywhere.)
    sx, sy = slopes
    h, w = (40, 28) if sx > 4 else (28, 40) if sy > 4 else (60, 60)
    img = ramp(h, w, 1, sx=sx, sy=sy, base=10)
    errs = np.concatenate([rc.warp_interior_errors(oracle.warp_affine(img, M), img, M)
                           for M in (rot(d, w, h, s, 0.3, -0.2) for d, s in RAMP_MOTIONS)])
    assert errs.size >= 5000
    assert abs(errs.mean()) <= rc.WARP_RAMP_BIAS, errs.mean()


def test_warp_affine_nv12_within_bound(oracle):
    w, h = 64, 36
    y = smooth(h, w, 1, seed=5)
    uv = smooth(h // 2, w // 2, 2, seed=6)
    surf = np.concatenate([y, uv.reshape(h // 2, w)])
    for name, M in matrices(w, h).items():
        rc.check_warp_nv12(oracle.warp_affine_nv12(surf, w, h, M), surf, w, h, M, what=name)


def test_warp_affine_1080p(oracle):
    img = smooth(1080, 1920, 3, seed=7)
    M = rot(-0.4, 1920, 1080, 1.003, 2.31, -1.77)
    assert rc.check_warp(oracle.warp_affine(img, M, threads=4), img, M, what="1080p") > 0.5


# ---- resize + gray --------------------------------------------------------------------------------------------------

RESIZES = [((320, 240), (960, 540)), ((1280, 720), (960, 540)), ((131, 97), (60, 44)), ((97, 131), (131, 97)),
           ((7, 5), (3, 2)), ((1, 1), (5, 3)), ((9, 1), (4, 1)), ((1, 9), (1, 4)), ((640, 360), (480, 270))]


@pytest.mark.parametrize("kind", ["smooth", "noise", "ramp"])
def test_resize_linear_within_bound(oracle, kind):
    lo, hi = 0.0, 0.0
    for (sw, sh), (dw, dh) in RESIZES:
        img = IMAGES[kind](sh, sw, 3)
        a, b = rc.check_resize_channels(oracle.resize(img, dw, dh), img, dw, dh, what="%s %dx%d->%dx%d" % (
            kind, sw, sh, dw, dh))
        lo, hi = min(lo, a), max(hi, b)
    if kind != "ramp":
        # observed on the oracle: about -0.74 and +0.5; the bound (-1.0078, +0.5) is within 2x of it
        assert lo < -0.5 and hi > 0.3, (lo, hi)


def test_resize_gray_within_bound(oracle):
    for (sw, sh), (dw, dh) in RESIZES:
        img = smooth(sh, sw, 3, seed=3)
        share = rc.check_resize_gray(oracle.analysis_gray(img, dw, dh), img, dw, dh, what="%dx%d" % (sw, sh))
        # a one-level difference from the rounded float64 luma needs the truncating vertical pass or a near-tie
        assert share <= 0.35, share


@pytest.mark.parametrize("step", [2, 4])
def test_resize_exact_ratios(oracle, step):
    for (h, w) in [(4, 4), (8, 12), (36, 64), (1080, 1920) if step == 2 else (2160, 3840)]:
        g = noise(h, w, 1, seed=step)
        exp = rc.exact_mean2x2(g, step)
        assert np.array_equal(oracle.resize(g, w // step, h // step), exp), (h, w)
        val, _ = ref64.resize_linear(g, w // step, h // step)
        assert np.array_equal(exp, ref64.round_half_up(val))
    if step == 2:
        # BGR at 2x: the same mean per channel
        img = noise(36, 64, 3, seed=9)
        exp = np.stack([rc.exact_mean2x2(img[..., c], 2) for c in range(3)], -1)
        assert np.array_equal(oracle.resize(img, 32, 18), exp)


# ---- pyrDown, Scharr ------------------------------------------------------------------------------------------------

PYR_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 1), (2, 7), (5, 3), (3, 3), (17, 31), (97, 131), (1080, 1920)]


@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_pyr_down_exact(oracle, kind):
    for (h, w) in PYR_SHAPES:
        g = IMAGES[kind](h, w, 1)
        assert np.array_equal(oracle.pyr_down(g), ref64.round_half_up(ref64.pyr_down(g))), (kind, h, w)


@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_scharr_exact(oracle, kind):
    for (h, w) in PYR_SHAPES:
        g = IMAGES[kind](h, w, 1)
        d = oracle.scharr(g)
        dx, dy = ref64.scharr(g)
        assert np.array_equal(d[..., 0], dx) and np.array_equal(d[..., 1], dy), (kind, h, w)


# ---- min-eigenvalue map, GFTT ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_min_eigen_within_bound(oracle, kind):
    for (h, w) in [(1, 1), (2, 2), (3, 3), (1, 9), (9, 1), (7, 13), (97, 131)]:
        g = IMAGES[kind](h, w, 1)
        rc.check_min_eigen(oracle.min_eigen(g), g, what="%s %dx%d" % (kind, w, h))
    g = ref64.scene(320, 240, seed=1)
    rc.check_min_eigen(oracle.min_eigen(g), g, what="scene")


def test_min_eigen_1080p(oracle):
    g = ref64.scene(960, 540, seed=2)
    rc.check_min_eigen(oracle.min_eigen(g), g, what="960x540")


@pytest.mark.parametrize("max_corners,quality,min_distance", [(200, 0.01, 10.0), (1, 0.01, 10.0), (5000, 0.01, 0.0),
                                                              (5000, 0.05, 1.0), (50, 0.1, 40.0), (300, 0.3, 3.0)])
def test_gftt_properties(oracle, max_corners, quality, min_distance):
    g = ref64.scene(160, 120, seed=4)
    pts, _ = oracle.gftt(g, max_corners, quality, min_distance)
    assert len(pts) > 0
    rc.check_gftt(pts, g, max_corners, quality, min_distance, what="scene")


def test_gftt_check_rejects_incomplete_lists(oracle):
    # the completeness property has teeth: dropping corners from the oracle's own list must fail it
    g = ref64.scene(160, 120, seed=4)
    for args in [(200, 0.01, 10.0), (5000, 0.01, 0.0), (50, 0.1, 40.0)]:
        pts, _ = oracle.gftt(g, *args)
        assert rc.check_gftt(pts, g, *args) > 0
        for sub in (pts[:3], pts[::7], pts[:-1], np.delete(pts, len(pts) // 2, 0)):
            with pytest.raises(AssertionError, match="missing"):
                rc.check_gftt(sub, g, *args)


def test_gftt_flat_and_border(oracle):
    pts, _ = oracle.gftt(const(40, 50), 100, 0.01, 5.0)
    rc.check_gftt(pts, const(40, 50), 100, 0.01, 5.0, what="flat")
    g = const(40, 50, v=30)
    g[0:3, 0:3] = 220          # corners hugging the border
    g[-4:, -2:] = 200
    pts, _ = oracle.gftt(g, 100, 0.01, 3.0)
    assert len(pts) >= 2
    rc.check_gftt(pts, g, 100, 0.01, 3.0, what="border")


# ---- pyramidal LK ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("motion", sorted(LK_MOTIONS))
def test_pyr_lk_against_ground_truth(oracle, motion):
    w, h = 192, 144
    a, b, M = lk_scene(w, h, motion)
    pts = lk_points(w, h, 120, 24)
    for win in (15, 21, 31):
        good = lk_conditioned(a, pts, win)
        assert good.sum() > 40
        for max_level in (0, 3):
            out, st, _ = oracle.pyr_lk(a, b, pts, win=win, max_level=max_level)
            check_lk_truth(out, st, pts, M, good, "%s win %d level %d" % (motion, win, max_level))


def test_pyr_lk_status_rules(oracle):
    w, h = 96, 72
    a, b, _ = lk_scene(w, h, "shift")
    flat = np.full((h, w), 90, np.uint8)
    pts = np.array([[48, 36], [-40, 30], [w + 30, 10], [30, h + 40]], np.float32)
    _, st, _ = oracle.pyr_lk(a, b, pts, win=15, max_level=2)
    assert list(st[1:]) == [0, 0, 0]
    _, st, _ = oracle.pyr_lk(flat, flat, pts[:1], win=15, max_level=2)     # min-eigen below 1e-4: lost
    assert st[0] == 0


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_pyr_lk_iterations_match_float64(oracle, iters):
    # maxLevel 0, eps 0: exactly `iters` Gauss-Newton steps.  The fixed point (intensities in 1/32, 14-bit window
    # weights, Scharr rounded to an integer) moves a step by well under 0.01 px on this scene.
    w, h = 160, 120
    a, b, _ = lk_scene(w, h, "shift")
    pts = lk_points(w, h, 40, 20, seed=2)
    good = lk_conditioned(a, pts, 15)
    out, st, _ = oracle.pyr_lk(a, b, pts, win=15, max_level=0, iters=iters, eps=0.0)
    ref = np.array([ref64.lk_track(a, b, p.astype(np.float64), 15, iters)[-1] for p in pts])
    e = np.linalg.norm(out - ref, axis=1)[good]
    assert e.max() <= 0.01, e.max()


# ---- estimateAffinePartial2D ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,outliers,extent", [(200, 0.0, 960), (200, 0.3, 960), (300, 0.7, 1920), (150, 0.5, 3840),
                                               (64, 0.2, 640)])
def test_ransac_recovers_inliers_and_least_squares(oracle, n, outliers, extent):
    src, dst, truth, _ = rc.similarity_case(n, outliers, seed=n + int(outliers * 10), extent=extent)
    ok, model, inl, _ = oracle.estimate_affine_partial2d(src, dst)
    assert ok
    assert np.array_equal(inl, truth)
    rc.check_similarity_model(model, src, dst, inl)


def test_ransac_small_and_degenerate(oracle):
    src = np.array([[10, 20], [200, 150]], np.float32)
    dst = ref64.apply_affine([0.98, -0.05, 3, 0.05, 0.98, -2], src).astype(np.float32)
    ok, model, inl, _ = oracle.estimate_affine_partial2d(src, dst)
    assert ok and list(inl) == [1, 1]
    rc.check_similarity_model(model, src, dst, inl, "2 points")
    src3 = np.array([[10, 20], [200, 150], [90, 300]], np.float32)
    dst3 = ref64.apply_affine([1.01, -0.02, -4, 0.02, 1.01, 1.5], src3).astype(np.float32)
    ok, model, inl, _ = oracle.estimate_affine_partial2d(src3, dst3)
    assert ok and list(inl) == [1, 1, 1]
    rc.check_similarity_model(model, src3, dst3, inl, "3 points")
    # collinear points still define a similarity
    line = np.stack([np.arange(10) * 30.0, np.arange(10) * 7.0 + 5], 1).astype(np.float32)
    dl = ref64.apply_affine([0.99, -0.03, 2, 0.03, 0.99, -1], line).astype(np.float32)
    ok, model, inl, _ = oracle.estimate_affine_partial2d(line, dl)
    assert ok and inl.all()
    rc.check_similarity_model(model, line, dl, inl, "collinear")
    # all points coincide: no model
    same = np.tile(np.float32([[40, 50]]), (6, 1))
    ok, model, inl, _ = oracle.estimate_affine_partial2d(same, same + 1)
    assert not ok and not inl.any()
