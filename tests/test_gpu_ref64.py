"""The HIP kernels against the float64 statements of tests/ref64.py, with no oracle in between.

Same tolerances as tests/test_ref64_oracle.py (tests/ref64_checks.py): the operator entry points (vs_op_*) at every
launch form, then the batch analysis kernels that bench.py times, reached through the pipeline at the bench's shapes.
"""
import numpy as np
import pytest

import ref64
import ref64_checks as rc
from ref64_inputs import (IMAGES, LK_MOTIONS, RAMP_MOTIONS, SHAPES, check_lk_truth, lk_conditioned, lk_points, lk_scene,
                          matrices, noise, ramp, rot, smooth)
from vsamd import capi

pytestmark = pytest.mark.gpu

# ---- warp -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("frames", [1, 4, 17, 33])
@pytest.mark.parametrize("cn", [1, 2, 3])
def test_warp_affine_launches_within_bound(gpu, frames, cn):
    for (h, w) in [(1, 1), (7, 13), (97, 131), (67, 250)]:
        imgs = np.stack([smooth(h, w, cn, seed=i) for i in range(frames)])
        mats = list(matrices(w, h).values())
        Ms = np.stack([mats[i % len(mats)] for i in range(frames)])
        out = gpu.warp_affine(imgs, Ms, batch=True)
        for i in range(frames):
            rc.check_warp(out[i], imgs[i], Ms[i], what="%dx%d cn%d frame %d of %d" % (w, h, cn, i, frames))


@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_warp_affine_single_images_within_bound(gpu, kind):
    for (h, w) in SHAPES:
        img = IMAGES[kind](h, w, 3)
        for name, M in matrices(w, h).items():
            rc.check_warp(gpu.warp_affine(img, M), img, M, what="%s %dx%d %s" % (kind, w, h, name))


@pytest.mark.parametrize("slopes", [(7.7, 0.53), (0.53, 7.7), (2.1, 1.7)])
def test_warp_affine_ramp_is_unbiased(gpu, slopes):
    sx, sy = slopes
    h, w = (40, 28) if sx > 4 else (28, 40) if sy > 4 else (60, 60)
    img = ramp(h, w, 1, sx=sx, sy=sy, base=10)
    Ms = np.stack([rot(d, w, h, s, 0.3, -0.2) for d, s in RAMP_MOTIONS])
    out = gpu.warp_affine(np.stack([img] * len(Ms)), Ms, batch=True)
    errs = np.concatenate([rc.warp_interior_errors(out[i], img, Ms[i]) for i in range(len(Ms))])
    assert abs(errs.mean()) <= rc.WARP_RAMP_BIAS, errs.mean()


@pytest.mark.parametrize("surfaces", [1, 4, 33])
def test_warp_affine_nv12_launches_within_bound(gpu, surfaces):
    for (w, h) in [(64, 36), (130, 74)]:
        surfs = np.stack([np.concatenate([smooth(h, w, 1, seed=i), smooth(h // 2, w // 2, 2, seed=50 + i).reshape(h // 2, w)])
                          for i in range(surfaces)])
        mats = list(matrices(w, h).values())
        Ms = np.stack([mats[(i + 1) % len(mats)] for i in range(surfaces)])
        out = gpu.warp_affine_nv12(surfs, w, h, Ms)
        for i in range(surfaces):
            rc.check_warp_nv12(out[i], surfs[i], w, h, Ms[i], what="%dx%d surface %d of %d" % (w, h, i, surfaces))


@pytest.mark.parametrize("border,code", [("constant", capi.BORDER_BLACK), ("replicate", capi.BORDER_REPLICATE)])
def test_warp_affine_ex_borders_within_bound(gpu, border, code):
    # (vs_op_warp_affine_ex takes VS_BORDER_BLACK and VS_BORDER_REPLICATE only; other borders are refused)
    with pytest.raises(capi.VsError):
        gpu.warp_affine_ex(smooth(8, 8, 1), np.eye(2, 3), capi.BORDER_REFLECT)
    for (h, w) in [(1, 1), (2, 7), (31, 17), (97, 131)]:
        for cn in (1, 3):
            img = smooth(h, w, cn, seed=2)
            for name, M in matrices(w, h).items():
                M64 = M.astype(np.float64)
                rc.check_warp(gpu.warp_affine_ex(img, M64, code), img, M64, border,
                              what="%s %dx%d cn%d %s" % (border, w, h, cn, name))


# ---- resize_gray, pyr_down, scharr, pyr_level -----------------------------------------------------------------------


@pytest.mark.parametrize("src,dst", [((320, 240), (960, 540)), ((1280, 720), (960, 540)), ((131, 97), (60, 44)),
                                     ((1920, 1080), (960, 540)), ((7, 5), (3, 2))])
def test_resize_gray_bgr_within_bound(gpu, src, dst):
    (sw, sh), (dw, dh) = src, dst
    img = smooth(sh, sw, 3, seed=3)
    share = rc.check_resize_gray(gpu.resize_gray(img, dw, dh), img, dw, dh, what="%dx%d" % src)
    assert share <= 0.35, share
    if (sw, sh) == (2 * dw, 2 * dh):
        g = np.stack([rc.exact_mean2x2(img[..., c], 2) for c in range(3)], -1)
        w15 = np.array([3735, 19235, 9798])
        assert np.array_equal(gpu.resize_gray(img, dw, dh), ((g * w15).sum(-1) + (1 << 14)) >> 15)


@pytest.mark.parametrize("fmt", [capi.FMT_GRAY8, capi.FMT_NV12])
def test_resize_gray_luma(gpu, fmt):
    for (sw, sh), (dw, dh) in [((320, 240), (960, 540)), ((131, 97), (60, 44)), ((640, 360), (160, 90)),
                               ((3840, 2160), (960, 540)), ((1128, 640), (282, 160)), ((64, 36), (32, 18))]:
        if fmt == capi.FMT_NV12 and (sw % 2 or sh % 2):
            continue            # an NV12 surface has even sides
        y = noise(sh, sw, 1, seed=sw)
        img = y if fmt == capi.FMT_GRAY8 else np.concatenate([y, noise(sh // 2, sw, 1, seed=1)])
        got = gpu.resize_gray(img, dw, dh, fmt)
        rc.check_resize_channels(got, y, dw, dh, what="%dx%d->%dx%d" % (sw, sh, dw, dh))
        for step in (2, 4):
            if (sw, sh) == (step * dw, step * dh):
                assert np.array_equal(got, rc.exact_mean2x2(y, step)), (sw, sh, step)


def test_resize_gray_pitched_input(gpu):
    for (sw, sh), (dw, dh), fmt in [((1128, 640), (282, 160), capi.FMT_GRAY8), ((640, 360), (320, 180), capi.FMT_BGR8),
                                    ((131, 97), (60, 44), capi.FMT_BGR8)]:
        cn = 3 if fmt == capi.FMT_BGR8 else 1
        pitch = sw * cn + 37
        buf = noise(sh, pitch, 1, seed=7)
        img = buf[:, :sw * cn].reshape(sh, sw, cn) if cn == 3 else buf[:, :sw]
        d_in = capi.DevBuf.from_array(gpu, buf)
        d_out = capi.DevBuf(gpu, dw * dh)
        gpu.check(gpu.lib.vs_op_resize_gray(d_in.ptr, pitch, sw, sh, fmt, d_out.ptr, dw, dw, dh, None))
        gpu.sync()
        got = d_out.download((dh, dw), np.uint8)
        if cn == 3:
            rc.check_resize_gray(got, img, dw, dh, what="pitched %dx%d" % (sw, sh))
        else:
            assert np.array_equal(got, rc.exact_mean2x2(img, 4))


PYR_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 1), (2, 7), (5, 3), (3, 3), (17, 31), (97, 131), (541, 961)]


@pytest.mark.parametrize("kind", sorted(IMAGES))
def test_pyr_down_scharr_pyr_level_exact(gpu, kind):
    for (h, w) in PYR_SHAPES:
        g = IMAGES[kind](h, w, 1)
        down = ref64.round_half_up(ref64.pyr_down(g))
        dx, dy = ref64.scharr(g)
        assert np.array_equal(gpu.pyr_down(g), down), (kind, h, w)
        s = gpu.scharr(g)
        assert np.array_equal(s[..., 0], dx) and np.array_equal(s[..., 1], dy), (kind, h, w)
        der, nxt = gpu.pyr_level(g)
        assert np.array_equal(der[..., 0], dx) and np.array_equal(der[..., 1], dy), (kind, h, w)
        assert np.array_equal(nxt, down), (kind, h, w)


# ---- min-eigen map, GFTT --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", sorted(IMAGES) + ["scene"])
def test_min_eigen_map_within_bound(gpu, kind):
    for (h, w) in [(3, 3), (7, 13), (97, 131), (540, 960)]:
        g = ref64.scene(w, h, seed=1) if kind == "scene" else IMAGES[kind](h, w, 1)
        _, eig = gpu.gftt(g, 100, 0.01, 10.0, want_eig=True)
        rc.check_min_eigen(eig, g, what="%s %dx%d" % (kind, w, h))


@pytest.mark.parametrize("max_corners,quality,min_distance", [(200, 0.01, 10.0), (1, 0.01, 10.0), (2000, 0.01, 0.0),
                                                              (2000, 0.05, 1.0), (50, 0.1, 40.0), (300, 0.3, 3.0)])
def test_gftt_properties(gpu, max_corners, quality, min_distance):
    g = ref64.scene(160, 120, seed=4)
    pts = gpu.gftt(g, max_corners, quality, min_distance)
    assert len(pts) > 0
    rc.check_gftt(pts, g, max_corners, quality, min_distance, what="scene")


def test_gftt_flat_and_border(gpu):
    flat = np.full((40, 50), 173, np.uint8)
    rc.check_gftt(gpu.gftt(flat, 100, 0.01, 5.0), flat, 100, 0.01, 5.0, what="flat")
    g = np.full((40, 50), 30, np.uint8)
    g[0:3, 0:3] = 220
    g[-4:, -2:] = 200
    pts = gpu.gftt(g, 100, 0.01, 3.0)
    assert len(pts) >= 2
    rc.check_gftt(pts, g, 100, 0.01, 3.0, what="border")


# ---- LK -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("motion", sorted(LK_MOTIONS))
def test_pyr_lk_against_ground_truth(gpu, motion):
    w, h = 192, 144
    a, b, M = lk_scene(w, h, motion)
    for n in (1, 100, 2000):
        pts = lk_points(w, h, n, 24, seed=n)
        for win in (15, 21, 31):
            good = lk_conditioned(a, pts, win) if n <= 100 else None
            for max_level in (0, 2, 4):
                out, st, _ = gpu.pyr_lk(a, b, pts, win=win, max_level=max_level)
                if good is not None:
                    check_lk_truth(out, st, pts, M, good, "%s n %d win %d level %d" % (motion, n, win, max_level))
                else:
                    e = np.linalg.norm(out - ref64.apply_affine(M, pts), axis=1)[st == 1]
                    assert st.mean() > 0.9 and np.median(e) <= 0.02, (n, win, max_level)


def test_pyr_lk_status_rules(gpu):
    w, h = 96, 72
    a, b, _ = lk_scene(w, h, "shift")
    pts = np.array([[48, 36], [-40, 30], [w + 30, 10], [30, h + 40], [2, 3], [w - 2, h - 1]], np.float32)
    out, st, _ = gpu.pyr_lk(a, b, pts, win=21, max_level=2)
    assert list(st[1:4]) == [0, 0, 0]
    for i in (4, 5):            # windows that hang over the border still track when they converge
        if st[i]:
            assert np.linalg.norm(out[i] - ref64.apply_affine(LK_MOTIONS["shift"], pts[i:i + 1])[0]) < 0.5
    flat = np.full((h, w), 90, np.uint8)
    _, st, _ = gpu.pyr_lk(flat, flat, pts[:1], win=15, max_level=2)
    assert st[0] == 0


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_pyr_lk_iterations_match_float64(gpu, iters):
    w, h = 160, 120
    a, b, _ = lk_scene(w, h, "shift")
    pts = lk_points(w, h, 40, 20, seed=2)
    good = lk_conditioned(a, pts, 15)
    out, _, _ = gpu.pyr_lk(a, b, pts, win=15, max_level=0, iters=iters, eps=0.0)
    ref = np.array([ref64.lk_track(a, b, p.astype(np.float64), 15, iters)[-1] for p in pts])
    assert np.linalg.norm(out - ref, axis=1)[good].max() <= 0.01


# ---- RANSAC ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,outliers,extent", [(200, 0.0, 960), (200, 0.3, 960), (300, 0.7, 1920), (150, 0.5, 3840),
                                               (64, 0.2, 640)])
def test_ransac_recovers_inliers_and_least_squares(gpu, n, outliers, extent):
    src, dst, truth, _ = rc.similarity_case(n, outliers, seed=n + int(outliers * 10), extent=extent)
    ok, model, inl, _ = gpu.estimate_affine_partial2d(src, dst)
    assert ok
    assert np.array_equal(inl, truth)
    rc.check_similarity_model(model, src, dst, inl)


def test_ransac_small_and_degenerate(gpu):
    src = np.array([[10, 20], [200, 150]], np.float32)
    dst = ref64.apply_affine([0.98, -0.05, 3, 0.05, 0.98, -2], src).astype(np.float32)
    ok, model, inl, _ = gpu.estimate_affine_partial2d(src, dst)
    assert ok and list(inl) == [1, 1]
    rc.check_similarity_model(model, src, dst, inl, "2 points")
    src3 = np.array([[10, 20], [200, 150], [90, 300]], np.float32)
    dst3 = ref64.apply_affine([1.01, -0.02, -4, 0.02, 1.01, 1.5], src3).astype(np.float32)
    ok, model, inl, _ = gpu.estimate_affine_partial2d(src3, dst3)
    assert ok and list(inl) == [1, 1, 1]
    rc.check_similarity_model(model, src3, dst3, inl, "3 points")
    # collinear points still define a similarity (two distinct points fix one), as in the oracle test
    line = np.stack([np.arange(10) * 30.0, np.arange(10) * 7.0 + 5], 1).astype(np.float32)
    dl = ref64.apply_affine([0.99, -0.03, 2, 0.03, 0.99, -1], line).astype(np.float32)
    ok, model, inl, _ = gpu.estimate_affine_partial2d(line, dl)
    assert ok and inl.all()
    rc.check_similarity_model(model, line, dl, inl, "collinear")
    same = np.tile(np.float32([[40, 50]]), (6, 1))
    ok, model, inl, _ = gpu.estimate_affine_partial2d(same, same + 1)
    assert not ok and not inl.any()


# ---- the batch analysis kernels, through the pipeline ---------------------------------------------------------------
# Every pushed frame is the same picture, so the analysis gray image that debug_arrays() reports is that picture's,
# whichever frame of the batch it came from.


def batch_gray(gpu, frame, w, h, fmt, batch, offset=0, **params):
    s = gpu.stabilizer(gpu.params(smoothing_radius=3, **params))
    s.set_batch(batch)
    s.set_zero_copy(True)
    fb = frame.nbytes
    d_in = capi.DevBuf(gpu, fb + 64)
    d_in.upload(frame, offset)
    n = 2 * batch
    d_out = capi.DevBuf(gpu, fb * n)
    stride = w * 3 if fmt == capi.FMT_BGR8 else w
    k = 0
    for _ in range(n):
        k += s.push_dev(d_in.ptr + offset, w, h, stride, fmt, d_out.ptr + k * fb, stride)
    s.sync()
    assert k > 0
    gray = s.debug_arrays()["gray"].copy()
    s.close()
    d_in.free()
    d_out.free()
    return gray


@pytest.mark.parametrize("offset", [0, 3])
def test_batch_analysis_gray_1080p_bgr(gpu, offset):
    """1920x1080 BGR, batch 64: half_bgr_gray12_kernel (frames on 8-byte boundaries) or half_bgr_gray_kernel (a base 3
    bytes off)."""
    w, h = 1920, 1080
    frame = smooth(h, w, 3, seed=11)
    gray = batch_gray(gpu, frame, w, h, capi.FMT_BGR8, 64, offset)
    assert gray.shape == (540, 960)
    rc.check_resize_gray(gray, frame, 960, 540, what="offset %d" % offset)
    g = np.stack([rc.exact_mean2x2(frame[..., c], 2) for c in range(3)], -1)
    assert np.array_equal(gray, ((g * np.array([3735, 19235, 9798])).sum(-1) + (1 << 14)) >> 15)


def test_batch_analysis_gray_4k_nv12(gpu):
    """3840x2160 NV12, batch 64: quarter_gray_kernel, vector path."""
    w, h = 3840, 2160
    y = noise(h, w, 1, seed=12)
    surf = np.concatenate([y, noise(h // 2, w, 1, seed=13)])
    gray = batch_gray(gpu, surf, w, h, capi.FMT_NV12, 64)
    assert gray.shape == (540, 960)
    assert np.array_equal(gray, rc.exact_mean2x2(y, 4))


def test_batch_analysis_gray_drone_nv12_scalar_tail(gpu):
    """Drone mode, 1128x640 NV12 analysed at 282x160 (hf_analysis_max_width 282): sw == 4 aw, so quarter_gray_kernel runs,
    and its scalar path takes every lane: the analysis pitch is aw = 282, not a multiple of 4, and the source pitch 1128 is
    not a multiple of 16.  (The pipeline's analysis pitch is always aw, so a row that mixes vector and scalar lanes does not
    occur there; the operator test with a 282-wide output covers the same path.)"""
    w, h = 1128, 640
    y = noise(h, w, 1, seed=14)
    surf = np.concatenate([y, noise(h // 2, w, 1, seed=15)])
    gray = batch_gray(gpu, surf, w, h, capi.FMT_NV12, 8, drone_high_freq_mode=1, hf_analysis_max_width=282)
    assert gray.shape == (160, 282) and 282 % 4 == 2
    assert np.array_equal(gray, rc.exact_mean2x2(y, 4))


def test_debug_arrays_gray_larger_than_1080p(gpu):
    """Drone mode analyses 2560x1440 frames at full size: debug_arrays() sizes its gray buffer from the analysis size
    (a fixed 1920x1080 buffer was overrun)."""
    w, h = 2560, 1440
    y = noise(h, w, 1, seed=16)
    gray = batch_gray(gpu, y, w, h, capi.FMT_GRAY8, 4, drone_high_freq_mode=1, hf_analysis_max_width=w)
    assert gray.shape == (h, w)
    assert np.array_equal(gray, y)


# ---- pipeline outputs against the float64 warp of their input, and the reported model against least squares ----------
# The per-frame pipeline reports, after every push, the index of the frame it warped and the matrix it used
# (vs_debug_frame.out_index / warp_matrix), and the analysis it ran: prev / curr / status / inliers and the refined model.
# Batch mode and a vs_batch of 8 streams produce the same frames in the same order from the same pushes (their own
# parity tests), so each of their outputs is held to the float64 warp of its input under the per-frame matrix.

PIPE_W, PIPE_H, PIPE_N = 320, 240, 24


def _pipeline_clip():
    from vsamd import synth
    return synth.make_clip(synth.SEED_CONFIG1 + 5, PIPE_W, PIPE_H, PIPE_N)


def _per_frame_run(gpu, clip, params):
    """Per-frame pipeline: [(out_index, warp_matrix)] per output, flush included; checks each output frame and each
    reported model on the way."""
    s = gpu.stabilizer(params)
    got, n_models = [], 0
    for k, f in enumerate(clip):
        out = s.push(f)
        d, arr = s.debug(), s.debug_arrays()
        if k > 0 and d.n_inliers > 2 and not np.isnan(np.array(d.model)).any():
            st = arr["status"].astype(bool)
            src, dst = arr["prev"][st], arr["curr"][st]
            assert len(src) == d.n_valid == len(arr["inliers"]), k
            assert int(arr["inliers"].sum()) == d.n_inliers, k
            rc.check_similarity_model(np.array(d.model), src, dst, arr["inliers"], what="push %d" % k)
            n_models += 1
        if out is not None:
            assert out.shape == f.shape
            M = np.array(d.warp_matrix, np.float32)
            rc.check_warp(out, clip[d.out_index], M, what="push %d (frame %d)" % (k, d.out_index))
            got.append((d.out_index, M))
    while True:
        out = s.flush(clip[0])
        if out is None:
            break
        d = s.debug()
        M = np.array(d.warp_matrix, np.float32)
        rc.check_warp(out, clip[d.out_index], M, what="flush (frame %d)" % d.out_index)
        got.append((d.out_index, M))
    s.close()
    assert len(got) == len(clip) and n_models >= len(clip) // 2
    # the stream moves: the matrices are not all the identity
    assert max(np.abs(M - np.float32([1, 0, 0, 0, 1, 0])).max() for _, M in got) > 0.5
    return got


def test_pipeline_outputs_and_models_against_float64(gpu):
    _per_frame_run(gpu, _pipeline_clip(), gpu.params(smoothing_radius=5))


def test_batch_mode_outputs_against_float64_warp(gpu):
    clip = _pipeline_clip()
    p = gpu.params(smoothing_radius=5)
    ref = _per_frame_run(gpu, clip, p)
    s = gpu.stabilizer(p)
    s.set_batch(8)
    fb = clip[0].nbytes
    d_in, d_out = capi.DevBuf(gpu, fb * PIPE_N), capi.DevBuf(gpu, fb * PIPE_N)
    k = 0
    for i, f in enumerate(clip):
        d_in.upload(f, i * fb)
        k += s.push_dev(d_in.ptr + i * fb, PIPE_W, PIPE_H, PIPE_W * 3, capi.FMT_BGR8, d_out.ptr + k * fb, PIPE_W * 3)
    while s.flush_dev(d_out.ptr + k * fb, PIPE_W * 3):
        k += 1
    s.sync()
    assert k == len(ref)
    for j, (i, M) in enumerate(ref):
        rc.check_warp(d_out.download((PIPE_H, PIPE_W, 3), np.uint8, j * fb), clip[i], M, what="batch output %d" % j)
    s.close()


def test_vs_batch_of_8_streams_outputs_against_float64_warp(gpu):
    clip = _pipeline_clip()
    p = gpu.params(smoothing_radius=5)
    ref = _per_frame_run(gpu, clip, p)
    S, fb = 8, clip[0].nbytes
    b = gpu.batch(p, S, 8)
    d_in = capi.DevBuf(gpu, fb * PIPE_N)
    for i, f in enumerate(clip):
        d_in.upload(f, i * fb)
    d_out = [capi.DevBuf(gpu, fb * (PIPE_N + 1)) for _ in range(S)]
    k = [0] * S
    for i in range(PIPE_N):
        prod = b.push_dev([d_in.ptr + i * fb] * S, PIPE_W, PIPE_H, PIPE_W * 3, capi.FMT_BGR8,
                          [d_out[g].ptr + k[g] * fb for g in range(S)], PIPE_W * 3)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * fb for g in range(S)], PIPE_W * 3)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    for g in range(S):
        assert k[g] == len(ref), g
        for j, (i, M) in enumerate(ref):
            rc.check_warp(d_out[g].download((PIPE_H, PIPE_W, 3), np.uint8, j * fb), clip[i], M,
                          what="stream %d output %d" % (g, j))
    b.close()
    for buf in d_out + [d_in]:
        buf.free()
