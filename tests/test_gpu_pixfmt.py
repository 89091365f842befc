"""BGRA8, RGBA8 and RGB8 frames on the device, bit for bit against the oracle.

The warp operator with four channels against the oracle's warpAffine; the analysis gray image of the new formats against
the oracle's per-channel resize followed by BGR2GRAY; and the whole stabilizer: a colour frame of any of the new layouts
gives the B, G and R that the oracle's BGR8 stabilizer gives for the same B, G and R (same keypoints, model, path and warp
matrix), and its fourth byte is the oracle's warpAffine of the alpha plane by that frame's warp matrix."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vsamd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD_KW = dict(smoothing_radius=5, max_corners=200, lk_win_size=21, lk_max_level=2)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _alpha(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), np.uint8)


def _as_fmt(bgr, alpha, fmt):
    """The frame of format fmt whose B, G, R are bgr's (and whose fourth byte is alpha)."""
    if fmt == capi.FMT_BGRA8:
        return np.ascontiguousarray(np.dstack([bgr, alpha]))
    if fmt == capi.FMT_RGBA8:
        return np.ascontiguousarray(np.dstack([bgr[..., ::-1], alpha]))
    assert fmt == capi.FMT_RGB8
    return np.ascontiguousarray(bgr[..., ::-1])


def _bgr_of(out, fmt):
    return out[..., :3] if fmt == capi.FMT_BGRA8 else out[..., 2::-1]


def _oracle_run(oracle, clip, **params):
    """The oracle's BGR8 stabilizer over clip, flush included: per result (frame, out_index, warp matrix), and per push its
    debug record (transform, smoothed path, warp matrix)."""
    so = oracle.stabilizer(oracle.params(**params))
    outs, dbg = [], []
    for f in clip:
        o = so.push(f)
        d = so.debug()
        dbg.append((np.array(d.transform), np.array(d.smoothed), np.array(d.warp_matrix), o is not None))
        if o is not None:
            outs.append((o, d.out_index, np.array(d.warp_matrix, np.float32)))
    while True:
        o = so.flush(clip[0])
        if o is None:
            break
        d = so.debug()
        outs.append((o, d.out_index, np.array(d.warp_matrix, np.float32)))
    so.close()
    return outs, dbg


def _check_outputs(oracle, got, ref, fmt, alpha, alpha_of=None):
    """got: the device results in order; ref: _oracle_run's.  alpha_of(plane, M): the expected fourth byte."""
    assert len(got) == len(ref)
    for k, (g, (o, idx, M)) in enumerate(zip(got, ref)):
        assert np.array_equal(_bgr_of(g, fmt), o), k
        if fmt == capi.FMT_RGB8:
            continue
        if idx == len(alpha) - 1:
            # the last frame has no transform: it comes back as it is, unpadded, at the top left of the result
            want = np.zeros(g.shape[:2], np.uint8)
            want[:alpha.shape[1], :alpha.shape[2]] = alpha[idx]
        else:
            want = alpha_of(alpha[idx], M) if alpha_of else oracle.warp_affine(alpha[idx], M)
        assert np.array_equal(g[..., 3], want), k


# ---- 1. / 2. the warp operator ---------------------------------------------------------------------------------------------
_MATS = {
    "identity": [1, 0, 0, 0, 1, 0],
    "int_shift": [1, 0, 7, 0, 1, -3],
    "frac_shift": [1, 0, 3.40625, 0, 1, -2.71875],
    "small_rot": [0.99995, -0.01, 3.25, 0.01, 0.99995, -7.5],
    "rot_zoom_beyond_box": [1.1 * np.cos(0.35), -1.1 * np.sin(0.35), 40.0, 1.1 * np.sin(0.35), 1.1 * np.cos(0.35), -25.0],
    "saturated": [1, 0, -40000.5, 0, 1, 35000.25],
}


def _warp4(gpu, frames, Ms, spitch=None, dpitch=None):
    """vs_op_warp_affine, cn 4, over a stack of frames (b, h, w, 4) with the given row pitches (bytes)."""
    b, h, w, _ = frames.shape
    sp, dp = spitch or w * 4, dpitch or w * 4
    src = np.zeros((b, h, sp), np.uint8)
    src[:, :, :w * 4] = frames.reshape(b, h, w * 4)
    d_in = capi.DevBuf.from_array(gpu, src)
    d_out = capi.DevBuf(gpu, b * h * dp)
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(b, 6))
    gpu.check(gpu.lib.vs_op_warp_affine(d_in.ptr, sp, h * sp, d_out.ptr, dp, h * dp, w, h, 4, capi._p(M, capi.f32p), b, None))
    gpu.sync()
    out = d_out.download((b, h, dp), np.uint8)[:, :, :w * 4].reshape(b, h, w, 4)
    d_in.free(); d_out.free()
    return out


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 23), (130, 17), (1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_warp_affine_cn4_single_frames(gpu, oracle, size):
    w, h = size
    img = np.random.default_rng(w * 7 + h).integers(0, 256, (h, w, 4), np.uint8)
    names = list(_MATS) if w * h < 3840 * 2160 else ["small_rot", "rot_zoom_beyond_box"]
    for name in names:
        got = _warp4(gpu, img[None], [_MATS[name]])[0]
        assert np.array_equal(got, oracle.warp_affine(img, _MATS[name])), (size, name)


@pytest.mark.parametrize("batch,size", [(4, (130, 17)), (4, (3840, 2160)), (33, (37, 23)), (33, (1920, 1080))],
                         ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v)
def test_warp_affine_cn4_batches(gpu, oracle, batch, size):
    """Four frames and more build coordinate tables and take the plane kernel (33: two launches, the second of one frame)."""
    w, h = size
    rng = np.random.default_rng(batch * 1000 + w)
    frames = rng.integers(0, 256, (batch, h, w, 4), np.uint8)
    names = list(_MATS)
    Ms = [_MATS[names[i % len(names)]] for i in range(batch)]
    got = _warp4(gpu, frames, Ms)
    for i in range(batch):
        assert np.array_equal(got[i], oracle.warp_affine(frames[i], Ms[i])), (i, names[i % len(names)])


@pytest.mark.parametrize("spitch,dpitch", [(64, 64), (6, 64), (64, 6), (12, 20)], ids=lambda p: str(p))
def test_warp_affine_cn4_pitched(gpu, oracle, spitch, dpitch):
    """Row pitches past the row: 64 bytes more (16-byte aligned), 6 more (not even 4-byte aligned), 12 / 20 more (4-byte aligned,
    not 16)."""
    w, h, b = 333, 77, 5
    frames = np.random.default_rng(spitch * 31 + dpitch).integers(0, 256, (b, h, w, 4), np.uint8)
    Ms = [_MATS[n] for n in ("small_rot", "frac_shift", "rot_zoom_beyond_box", "identity", "int_shift")]
    got = _warp4(gpu, frames, Ms, w * 4 + spitch, w * 4 + dpitch)
    for i in range(b):
        assert np.array_equal(got[i], oracle.warp_affine(frames[i], Ms[i])), i


@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE])
def test_warp_affine_ex_cn4(gpu, oracle, border):
    w, h = 301, 157
    img = np.random.default_rng(border).integers(0, 256, (h, w, 4), np.uint8)
    for name in ("small_rot", "rot_zoom_beyond_box", "frac_shift", "saturated"):
        M = np.ascontiguousarray(np.asarray(_MATS[name], np.float64))
        d_in = capi.DevBuf.from_array(gpu, img)
        d_out = capi.DevBuf(gpu, img.nbytes)
        gpu.check(gpu.lib.vs_op_warp_affine_ex(d_in.ptr, w * 4, w, h, d_out.ptr, w * 4, w, h, 4, M.ctypes.data_as(capi.f64p),
                                               border, None))
        gpu.sync()
        got = d_out.download(img.shape, np.uint8)
        assert np.array_equal(got, oracle.warp_affine_d(img, M, border)), name


# ---- 3. the analysis gray image ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [capi.FMT_BGRA8, capi.FMT_RGBA8, capi.FMT_RGB8], ids=["bgra", "rgba", "rgb"])
@pytest.mark.parametrize("src,dst", [((1920, 1080), (960, 540)), ((1919, 1079), (960, 540)), ((640, 480), (480, 270))],
                         ids=["2x", "odd", "general"])
def test_resize_gray_of_the_new_formats(gpu, oracle, fmt, src, dst):
    (w, h), (dw, dh) = src, dst
    rng = np.random.default_rng(w + fmt)
    bgr = rng.integers(0, 256, (h, w, 3), np.uint8)
    frame = _as_fmt(bgr, rng.integers(0, 256, (h, w), np.uint8), fmt)
    want = oracle.bgr2gray(np.ascontiguousarray(_bgr_of(oracle.resize(frame, dw, dh), fmt)))
    assert np.array_equal(want, oracle.analysis_gray(bgr, dw, dh))
    assert np.array_equal(gpu.resize_gray(frame, dw, dh, fmt), want)


# ---- 4. / 7. the per-frame pipeline at 320 x 240 -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_clip():
    clip = synth.make_clip(synth.SEED_CONFIG1, 320, 240, 40)
    return clip, _alpha(11, 40, 240, 320)


@pytest.mark.parametrize("fmt", [capi.FMT_BGRA8, capi.FMT_RGBA8, capi.FMT_RGB8], ids=["bgra", "rgba", "rgb"])
def test_pipeline_per_frame(gpu, oracle, small_clip, fmt):
    clip, alpha = small_clip
    params = dict(smoothing_radius=10)
    ref, dbg = _oracle_run(oracle, clip, **params)
    sg = gpu.stabilizer(gpu.params(**params))
    got = []
    for k, f in enumerate(clip):
        o = sg.push(_as_fmt(f, alpha[k], fmt), fmt)
        d = sg.debug()
        t, sm, wm, has = dbg[k]
        assert (o is not None) == has, k
        if k > 0:
            assert np.array_equal(bits(d.transform), bits(t)), k
        if has:
            assert np.array_equal(bits(d.smoothed), bits(sm)), k
            assert np.array_equal(bits(d.warp_matrix), bits(wm)), k
            got.append(o)
    while True:
        o = sg.flush(clip[0], fmt)
        if o is None:
            break
        got.append(o)
    sg.close()
    _check_outputs(oracle, got, ref, fmt, alpha)


# ---- 5. / 7. / 9. the batch pipeline at 1920 x 1080 --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hd(gpu, oracle):
    """72 frames of 1920 x 1080 (rendered on the device), their alpha planes, and the oracle's BGR8 run over them."""
    n = 72
    d = synth.make_clip_dev(gpu, synth.SEED_CONFIG2, 1920, 1080, n)
    clip = list(d.download((n, 1080, 1920, 3), np.uint8))
    d.free()
    oracle.lib.vso_set_threads(8)
    try:
        ref, dbg = _oracle_run(oracle, clip, **HD_KW)
    finally:
        oracle.lib.vso_set_threads(1)
    return clip, _alpha(5, n, 1080, 1920), ref, dbg


def _batch_run(gpu, frames, fmt, batch, spitch=None, opitch=None, zero_copy=True):
    """frames through push_dev with set_batch(batch), drained through flush_dev; returns (results, last debug record)."""
    h, w = frames[0].shape[:2]
    cn = capi.FMT_CHANNELS[fmt]
    sp, op = spitch or w * cn, opitch or w * cn
    s = gpu.stabilizer(gpu.params(**HD_KW) if w == 1920 else gpu.params(smoothing_radius=10))
    s.set_batch(batch)
    s.set_zero_copy(zero_copy)
    n = len(frames)
    src = np.zeros((n, h, sp), np.uint8)
    src[:, :, :w * cn] = np.asarray(frames).reshape(n, h, w * cn)
    d_in = capi.DevBuf.from_array(gpu, src)
    d_out = capi.DevBuf(gpu, (n + 1) * h * op)
    k = 0
    for i in range(n):
        k += s.push_dev(d_in.ptr + i * h * sp, w, h, sp, fmt, d_out.ptr + k * h * op, op)
    s.sync()
    dbg = s.debug()
    dbg = (np.array(dbg.transform), np.array(dbg.smoothed), np.array(dbg.warp_matrix))
    while s.flush_dev(d_out.ptr + k * h * op, op):
        k += 1
    s.sync()
    out = d_out.download((k, h, op), np.uint8)[:, :, :w * cn].reshape(k, h, w, cn)
    s.close(); d_in.free(); d_out.free()
    return list(out), dbg


@pytest.mark.parametrize("fmt", [capi.FMT_BGRA8, capi.FMT_RGB8], ids=["bgra", "rgb"])
def test_pipeline_hd_batch64_with_flush(gpu, oracle, hd, fmt):
    clip, alpha, ref, dbg = hd
    frames = [_as_fmt(f, a, fmt) for f, a in zip(clip, alpha)]
    got, last = _batch_run(gpu, frames, fmt, 64)
    t, sm, wm, _ = dbg[-1]
    assert np.array_equal(bits(last[0]), bits(t)) and np.array_equal(bits(last[1]), bits(sm))
    assert np.array_equal(bits(last[2]), bits(wm))
    _check_outputs(oracle, got, ref, fmt, alpha)


@pytest.mark.parametrize("extra,zero_copy", [(64, True), (6, True), (64, False), (6, False)],
                         ids=["pitch+64-zc", "pitch+6-zc", "pitch+64-copy", "pitch+6-copy"])
def test_pipeline_pitched_bgra(gpu, oracle, small_clip, extra, zero_copy):
    """Device frames with a row pitch of w*4 + 64 and w*4 + 6 (not 4-byte aligned), read in place (zero-copy) or copied into
    the frame ring; results written with the same pitch."""
    clip, alpha = small_clip
    ref, _ = _oracle_run(oracle, clip, smoothing_radius=10)
    frames = [_as_fmt(f, a, capi.FMT_BGRA8) for f, a in zip(clip, alpha)]
    got, _ = _batch_run(gpu, frames, capi.FMT_BGRA8, 8, 320 * 4 + extra, 320 * 4 + extra, zero_copy)
    _check_outputs(oracle, got, ref, capi.FMT_BGRA8, alpha)


# ---- 6. border and crop modes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REFLECT, capi.BORDER_REFLECT_101, capi.BORDER_REPLICATE,
                                    capi.BORDER_WRAP, "crop"], ids=["black", "reflect", "reflect101", "replicate", "wrap", "crop"])
@pytest.mark.parametrize("batch", [1, 8])
def test_pipeline_border_and_crop_modes(gpu, oracle, small_clip, border, batch):
    clip, alpha = small_clip
    clip, alpha = clip[:24], alpha[:24]
    b = 12
    params = dict(smoothing_radius=6, border_size=b)
    if border == "crop":
        params.update(crop_n_zoom=1, border_type=capi.BORDER_BLACK)

        def alpha_of(a, M):
            return oracle.resize(np.ascontiguousarray(oracle.warp_affine(a, M)[b:240 - b, b:320 - b]), 320, 240)
    else:
        params.update(border_type=border)

        def alpha_of(a, M):
            return oracle.warp_affine(oracle.copy_make_border(a, b, border), M)
    ref, _ = _oracle_run(oracle, clip, **params)
    sg = gpu.stabilizer(gpu.params(**params))
    sg.set_batch(batch)
    got = [o for o in (sg.push(_as_fmt(f, a, capi.FMT_BGRA8), capi.FMT_BGRA8) for f, a in zip(clip, alpha)) if o is not None]
    while True:
        o = sg.flush(clip[0], capi.FMT_BGRA8)
        if o is None:
            break
        got.append(o)
    sg.close()
    _check_outputs(oracle, got, ref, capi.FMT_BGRA8, alpha, alpha_of)


def test_pipeline_fade_blends_every_byte(gpu, oracle, small_clip):
    """borderType "fade" blends and updates the fourth byte as it does the other three: with alpha = B the result's alpha is its B."""
    clip, _ = small_clip
    clip = clip[:24]
    params = dict(smoothing_radius=6, border_size=10, border_type=capi.BORDER_FADE, fade_alpha=0.4, fade_duration=5)
    ref, _ = _oracle_run(oracle, clip, **params)
    sg = gpu.stabilizer(gpu.params(**params))
    got = [o for o in (sg.push(_as_fmt(f, f[..., 0], capi.FMT_BGRA8), capi.FMT_BGRA8) for f in clip) if o is not None]
    while True:
        o = sg.flush(clip[0], capi.FMT_BGRA8)
        if o is None:
            break
        got.append(o)
    sg.close()
    assert len(got) == len(ref)
    for k, (g, (o, _, _)) in enumerate(zip(got, ref)):
        assert np.array_equal(g[..., :3], o), k
        assert np.array_equal(g[..., 3], g[..., 0]), k


# ---- 8. vs_batch -----------------------------------------------------------------------------------------------------------
def test_vs_batch_of_four_bgra_streams_at_1080p(gpu, oracle, hd):
    """Four BGRA streams of the same 1080p frames with four different alpha planes: each stream's B, G, R equal the oracle's
    run, its alpha the warp of its own alpha plane."""
    clip, _, _, _ = hd
    n, S, w, h = 24, 4, 1920, 1080
    clip = clip[:n]
    oracle.lib.vso_set_threads(8)
    try:
        ref, _ = _oracle_run(oracle, clip, **HD_KW)
    finally:
        oracle.lib.vso_set_threads(1)
    alphas = [_alpha(100 + g, n, h, w) for g in range(S)]
    fb = w * h * 4
    d_in = [capi.DevBuf.from_array(gpu, np.stack([_as_fmt(f, a, capi.FMT_BGRA8) for f, a in zip(clip, alphas[g])])) for g in range(S)]
    d_out = [capi.DevBuf(gpu, fb * (n + 1)) for _ in range(S)]
    b = gpu.batch(gpu.params(**HD_KW), S, 8)
    b.set_zero_copy(True)
    k = [0] * S
    for i in range(n):
        prod = b.push_dev([d_in[g].ptr + i * fb for g in range(S)], w, h, w * 4, capi.FMT_BGRA8, [d_out[g].ptr + k[g] * fb for g in range(S)], w * 4)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * fb for g in range(S)], w * 4)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    b.close()
    for g in range(S):
        got = list(d_out[g].download((k[g], h, w, 4), np.uint8))
        _check_outputs(oracle, got, ref, capi.FMT_BGRA8, alphas[g])


# ---- 10. the virtual canvas stays BGR8 ----------------------------------------------------------------------------------
def test_canvas_refuses_bgra(gpu):
    sg = gpu.stabilizer(gpu.params(enable_virtual_canvas=1))
    f = np.zeros((240, 320, 4), np.uint8)
    out = np.zeros((240, 320, 4), np.uint8)
    produced = C.c_int32(0)
    rc = gpu.lib.vs_stab_push(sg.h, capi._p(f, capi.u8p), 320, 240, 320 * 4, capi.FMT_BGRA8, capi._p(out, capi.u8p), 320 * 4,
                              C.byref(produced))
    assert rc == 4          # VS_ERR_UNSUPPORTED
    sg.close()


# ---- 11. the C++ class -----------------------------------------------------------------------------------------------------
def test_cpp_class_takes_bgra_mats(gpu):
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "wrapper_bgra")
    csrc = os.path.join(ROOT, "video-stab_amd", "csrc")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "wrapper_bgra.cpp"), os.path.join(ROOT, "video-stab_amd", "host", "Stabilizer.cpp"),
                           "-L" + csrc, "-lvideo-stab", "-Wl,-rpath," + csrc, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout
