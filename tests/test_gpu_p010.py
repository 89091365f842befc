"""P010 surfaces on the device, bit for bit.

The warp operator against tests/ref16.py (which the 8-bit oracle pins: tests/test_p010_cpu.py); the analysis gray image
against the oracle's gray image of the high-byte plane; and the whole stabilizer: a P010 stream's debug records equal those
of the oracle's NV12 run on the clip's high bytes, and every output surface is ref16's warp of input `out_index` under that
record's matrix - flush and the unwarped last frame included."""
import ctypes as C

import numpy as np
import pytest

import ref16
from p010_inputs import MATS, random_surface
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

P010 = capi.FMT_P010
CANARY = 0xA5C3


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. the warp operator ----------------------------------------------------------------------------------------------------
def _warp(gpu, surfs, w, h, Ms, spitch=None, dpitch=None):
    """vs_op_warp_affine_p010 over a stack of surfaces (n, h * 3 / 2, w) uint16 with the given row pitches in BYTES; the chroma
    plane lies h * pitch behind the luma plane.  Returns the results and checks that no padding sample was written."""
    n, rows = surfs.shape[0], h * 3 // 2
    sp, dp = spitch or 2 * w, dpitch or 2 * w
    src = np.full((n, rows, sp // 2), CANARY, np.uint16)
    src[:, :, :w] = surfs
    dst = np.full((n, rows, dp // 2), CANARY, np.uint16)
    d_in, d_out = capi.DevBuf.from_array(gpu, src), capi.DevBuf.from_array(gpu, dst)
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(n, 6))
    gpu.check(gpu.lib.vs_op_warp_affine_p010(d_in.ptr, sp, d_out.ptr, dp, w, h, capi._p(M, capi.f32p), n, rows * sp, rows * dp, None))
    gpu.sync()
    out = d_out.download((n, rows, dp // 2), np.uint16)
    d_in.free(); d_out.free()
    assert np.all(out[:, :, w:] == CANARY), "padding samples were written"
    return out[:, :, :w]


# around the edges of the luma tiles (128 x 32) and of the chroma tiles (128 x 16 chroma pixels = 256 x 32 luma pixels)
_SIZES = [(2, 2), (126, 30), (128, 32), (130, 34), (254, 62), (256, 64), (258, 66), (322, 200), (514, 98)]


@pytest.mark.parametrize("size", _SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ten_bit", [True, False], ids=["ten-bit", "full-range"])
def test_warp_single_surfaces(gpu, size, ten_bit):
    w, h = size
    surf = random_surface(w, w, h, ten_bit)
    for name, M in MATS.items():
        got = _warp(gpu, surf[None], w, h, [M])[0]
        assert np.array_equal(got, ref16.warp_two_planes(surf, w, h, M)), (size, name)


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_warp_single_surfaces_hd_and_4k(gpu, size):
    w, h = size
    surf = random_surface(w, w, h)
    for name in ("small_rot", "rot_zoom_beyond_box"):
        got = _warp(gpu, surf[None], w, h, [MATS[name]])[0]
        assert np.array_equal(got, ref16.warp_two_planes(surf, w, h, MATS[name])), (size, name)


@pytest.mark.parametrize("n,size", [(5, (130, 34)), (33, (322, 200)), (33, (258, 66)), (4, (1920, 1080))],
                         ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v)
def test_warp_batches(gpu, n, size):
    """33 surfaces: a launch of 32 and a launch of one."""
    w, h = size
    surfs = np.stack([random_surface(1000 * n + i, w, h, i % 2 == 0) for i in range(n)])
    names = list(MATS)
    Ms = [MATS[names[i % len(names)]] for i in range(n)]
    got = _warp(gpu, surfs, w, h, Ms)
    for i in range(n):
        assert np.array_equal(got[i], ref16.warp_two_planes(surfs[i], w, h, Ms[i])), (i, names[i % len(names)])


@pytest.mark.parametrize("extra", [(64, 64), (2, 64), (64, 6), (12, 20), (256, 128)], ids=lambda p: "%d-%d" % p)
def test_warp_padded_pitches_leave_the_padding_alone(gpu, extra):
    """Pitches past the row (bytes): 16-byte aligned, only even, 4-byte aligned - the canaries behind every row stay."""
    w, h, n = 322, 78, 5
    surfs = np.stack([random_surface(extra[0] * 7 + extra[1] + i, w, h) for i in range(n)])
    Ms = [MATS[k] for k in ("small_rot", "frac_shift", "rot_zoom_beyond_box", "identity", "saturated")]
    got = _warp(gpu, surfs, w, h, Ms, 2 * w + extra[0], 2 * w + extra[1])
    for i in range(n):
        assert np.array_equal(got[i], ref16.warp_two_planes(surfs[i], w, h, Ms[i])), i


def test_warp_refuses_odd_geometry(gpu):
    d = capi.DevBuf(gpu, 1 << 16)
    M = np.asarray(MATS["identity"], np.float32)
    for w, h, sp, dp, off in ((31, 24, 64, 64, 0), (32, 23, 64, 64, 0), (32, 24, 65, 64, 0), (32, 24, 64, 67, 0), (32, 24, 64, 64, 1)):
        rc = gpu.lib.vs_op_warp_affine_p010(d.ptr + off, sp, d.ptr + 32768, dp, w, h, capi._p(M, capi.f32p), 1, 36 * sp, 36 * dp, None)
        assert rc == 1, (w, h, sp, dp, off)                    # VS_ERR_INVALID_ARG
        assert gpu.lib.vs_last_error()
    d.free()


# ---- 2. the analysis gray image ----------------------------------------------------------------------------------------------
_GRAY = [((1920, 1080), (960, 540)), ((3840, 2160), (960, 540)), ((1280, 720), (960, 540)), ((322, 200), (960, 540))]


@pytest.mark.parametrize("src,dst", _GRAY, ids=["half", "quarter", "general", "upscale"])
def test_resize_gray_single(gpu, oracle, src, dst):
    (w, h), (dw, dh) = src, dst
    surf = random_surface(w + 1, w, h)
    want = oracle.analysis_gray(np.ascontiguousarray((surf[:h] >> 8).astype(np.uint8)), dw, dh)
    assert np.array_equal(gpu.resize_gray(surf, dw, dh, P010), want)


@pytest.mark.parametrize("src", [s for s, _ in _GRAY], ids=["half", "quarter", "general", "upscale"])
def test_resize_gray_through_a_batch_step(gpu, oracle, src):
    """Four frames through one step of the batch schedule: the analysis image of the last one (debug getter)."""
    w, h = src
    n = 4
    surfs = np.stack([random_surface(w + 10 + i, w, h) for i in range(n)])
    fb = surfs[0].nbytes
    s = gpu.stabilizer(gpu.params(smoothing_radius=5))
    s.set_batch(4)
    s.set_zero_copy(True)
    d_in, d_out = capi.DevBuf.from_array(gpu, surfs), capi.DevBuf(gpu, fb)
    for i in range(n):
        assert s.push_dev(d_in.ptr + i * fb, w, h, 2 * w, P010, d_out.ptr, 2 * w) == 0
    s.sync()
    gray = s.debug_arrays()["gray"]
    s.close(); d_in.free(); d_out.free()
    want = oracle.analysis_gray(np.ascontiguousarray((surfs[-1][:h] >> 8).astype(np.uint8)), 960, 540)
    assert np.array_equal(gray, want)


# ---- 3. the stabilizer ---------------------------------------------------------------------------------------------------------
def _oracle_nv12_run(oracle, clip, **params):
    """The oracle's NV12 stabilizer over the clip, flush included: per push its debug record, per result (out_index, matrix)."""
    so = oracle.stabilizer(oracle.params(**params))
    outs, dbg = [], []
    for f in clip:
        o = so.push(f, capi.FMT_NV12)
        d = so.debug()
        dbg.append(dict(transform=np.array(d.transform), smoothed=np.array(d.smoothed), warp=np.array(d.warp_matrix), has=o is not None,
                        counts=(d.n_prev, d.n_valid, d.n_detected, d.detected), out_index=d.out_index))
        if o is not None:
            outs.append((d.out_index, np.array(d.warp_matrix, np.float32)))
    while so.flush(clip[0], capi.FMT_NV12) is not None:
        d = so.debug()
        outs.append((d.out_index, np.array(d.warp_matrix, np.float32)))
    so.close()
    return outs, dbg


def _check_debug(d, want, k):
    assert (d.n_prev, d.n_valid, d.n_detected, d.detected) == want["counts"], k
    if k > 0:
        assert np.array_equal(bits(d.transform), bits(want["transform"])), k
    if want["has"]:
        assert np.array_equal(bits(d.smoothed), bits(want["smoothed"])), k
        assert np.array_equal(bits(d.warp_matrix), bits(want["warp"])), k
        assert d.out_index == want["out_index"], k


def _check_outputs(got, p010, ref, w, h):
    """got: the device results in order; ref: (out_index, matrix) per result.  The last frame of the clip has no transform."""
    assert len(got) == len(ref) == len(p010)
    for k, (g, (idx, M)) in enumerate(zip(got, ref)):
        want = p010[idx] if idx == len(p010) - 1 else ref16.warp_two_planes(p010[idx], w, h, M)
        assert np.array_equal(g, want), (k, idx)


@pytest.fixture(scope="module")
def small(oracle):
    w, h, n = 322, 200, 40
    nv12 = [synth.bgr_to_nv12(f) for f in synth.make_clip(synth.SEED_CONFIG3 + 21, w, h, n)]
    p010 = [synth.nv12_to_p010(f, seed=i) for i, f in enumerate(nv12)]
    return w, h, nv12, p010


@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_GAUSSIAN, capi.SMOOTH_KALMAN], ids=["box", "gaussian", "kalman"])
def test_pipeline_per_frame(gpu, oracle, small, method):
    w, h, nv12, p010 = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = _oracle_nv12_run(oracle, nv12, **params)
    sg = gpu.stabilizer(gpu.params(**params))
    got = []
    for k, f in enumerate(p010):
        o = sg.push(f, P010)
        assert (o is not None) == dbg[k]["has"], k
        _check_debug(sg.debug(), dbg[k], k)
        if o is not None:
            assert o.dtype == np.uint16
            got.append(o)
    while True:
        o = sg.flush(p010[0], P010)
        if o is None:
            break
        got.append(o)
    sg.close()
    _check_outputs(got, p010, ref, w, h)


def _surfaces(frames, w, h, pitch, uv_off):
    """Decoder-style surfaces: rows of `pitch` bytes, the chroma plane uv_off bytes behind the luma plane; canaries elsewhere."""
    n = len(frames)
    size = uv_off + (h // 2) * pitch
    buf = np.full((n, size // 2), CANARY, np.uint16)
    for i, f in enumerate(frames):
        buf[i, :h * pitch // 2].reshape(h, pitch // 2)[:, :w] = f[:h]
        buf[i, uv_off // 2:].reshape(h // 2, pitch // 2)[:, :w] = f[h:]
    return buf, size


def _unpack(buf, w, h, pitch, uv_off):
    out = np.empty((h * 3 // 2, w), np.uint16)
    out[:h] = buf[:h * pitch // 2].reshape(h, pitch // 2)[:, :w]
    out[h:] = buf[uv_off // 2:uv_off // 2 + (h // 2) * pitch // 2].reshape(h // 2, pitch // 2)[:, :w]
    chk = buf.copy()
    chk[:h * pitch // 2].reshape(h, pitch // 2)[:, :w] = CANARY
    chk[uv_off // 2:uv_off // 2 + (h // 2) * pitch // 2].reshape(h // 2, pitch // 2)[:, :w] = CANARY
    assert np.all(chk == CANARY), "samples outside the planes were written"
    return out


def _batch_run(gpu, p010, w, h, batch, params, zero_copy=True, in_layout=None, out_layout=None):
    """The clip through push_dev with set_batch(batch), drained through flush_dev.  Layouts: (pitch, uv offset) in bytes."""
    n = len(p010)
    ip, iuv = in_layout or (2 * w, 2 * w * h)
    op, ouv = out_layout or (2 * w, 2 * w * h)
    src, isz = _surfaces(p010, w, h, ip, iuv)
    osz = ouv + (h // 2) * op
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    s.set_zero_copy(zero_copy)
    if in_layout or out_layout:
        s.set_nv12_layout(iuv if in_layout else 0, ouv if out_layout else 0)
    d_in = capi.DevBuf.from_array(gpu, src)
    d_out = capi.DevBuf.from_array(gpu, np.full((n, osz // 2), CANARY, np.uint16))
    k = 0
    for i in range(n):
        k += s.push_dev(d_in.ptr + i * isz, w, h, ip, P010, d_out.ptr + k * osz, op)
    s.sync()
    last = s.debug()
    last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
    while s.flush_dev(d_out.ptr + k * osz, op):
        k += 1
    s.sync()
    out = d_out.download((n, osz // 2), np.uint16)
    s.close(); d_in.free(); d_out.free()
    return [_unpack(out[i], w, h, op, ouv) for i in range(k)], last


@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_KALMAN], ids=["box", "kalman"])
def test_pipeline_batch_mode_with_partial_batches(gpu, oracle, small, batch, method):
    """40 frames: five steps of 8, or one partial step of a batch of 64; warp launches of fewer than four frames included."""
    w, h, nv12, p010 = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = _oracle_nv12_run(oracle, nv12, **params)
    got, last = _batch_run(gpu, p010, w, h, batch, params)
    assert np.array_equal(bits(last["transform"]), bits(dbg[-1]["transform"]))
    assert np.array_equal(bits(last["smoothed"]), bits(dbg[-1]["smoothed"])) and np.array_equal(bits(last["warp"]), bits(dbg[-1]["warp"]))
    _check_outputs(got, p010, ref, w, h)


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
def test_pipeline_decoder_surfaces_with_different_layouts(gpu, oracle, small, zero_copy):
    """Input: pitch 768 bytes, chroma at pitch x 208 (aligned height).  Output: pitch 704, chroma at pitch x 224."""
    w, h, nv12, p010 = small
    nv12, p010 = nv12[:24], p010[:24]
    params = dict(smoothing_radius=6)
    ref, _ = _oracle_nv12_run(oracle, nv12, **params)
    got, _ = _batch_run(gpu, p010, w, h, 8, params, zero_copy, (768, 768 * 208), (704, 704 * 224))
    _check_outputs(got, p010, ref, w, h)


def test_vs_batch_of_three_streams_against_standalone_instances(gpu, oracle, small):
    w, h, nv12, p010 = small
    n, S = 24, 3
    params = dict(smoothing_radius=6)
    clips = [[np.roll(f, 2 * g, axis=1) for f in p010[:n]] for g in range(S)]        # (an even shift keeps the U, V order)
    fb = clips[0][0].nbytes
    d_in = [capi.DevBuf.from_array(gpu, np.stack(c)) for c in clips]
    d_out = [capi.DevBuf(gpu, fb * n) for _ in range(S)]
    b = gpu.batch(gpu.params(**params), S, 8)
    b.set_zero_copy(True)
    k = [0] * S
    for i in range(n):
        prod = b.push_dev([d_in[g].ptr + i * fb for g in range(S)], w, h, 2 * w, P010, [d_out[g].ptr + k[g] * fb for g in range(S)], 2 * w)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * fb for g in range(S)], 2 * w)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    b.close()
    for g in range(S):
        got = list(d_out[g].download((k[g], h * 3 // 2, w), np.uint16))
        alone, _ = _batch_run(gpu, clips[g], w, h, 8, params)
        assert len(got) == len(alone) == n
        for a, c in zip(got, alone):
            assert np.array_equal(a, c), g
        ref, _ = _oracle_nv12_run(oracle, [np.ascontiguousarray((f >> 8).astype(np.uint8)) for f in clips[g]], **params)
        _check_outputs(got, clips[g], ref, w, h)
    for d in d_in + d_out:
        d.free()


@pytest.mark.parametrize("size,n", [((1920, 1080), 12), ((3840, 2160), 8)], ids=["1080p", "4k"])
def test_pipeline_hd_and_4k_batch_mode(gpu, oracle, size, n):
    w, h = size
    d = synth.make_clip_dev(gpu, synth.SEED_CONFIG3 + 2, w, h, n, nv12=True)
    nv12 = list(d.download((n, h * 3 // 2, w), np.uint8))
    d.free()
    p010 = [synth.nv12_to_p010(f, seed=100 + i) for i, f in enumerate(nv12)]
    params = dict(smoothing_radius=5, max_corners=400)
    oracle.lib.vso_set_threads(8)
    try:
        ref, dbg = _oracle_nv12_run(oracle, nv12, **params)
    finally:
        oracle.lib.vso_set_threads(1)
    got, last = _batch_run(gpu, p010, w, h, 4, params)
    assert np.array_equal(bits(last["transform"]), bits(dbg[-1]["transform"])) and np.array_equal(bits(last["warp"]), bits(dbg[-1]["warp"]))
    _check_outputs(got, p010, ref, w, h)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def _push_status(gpu, params, w, h, pitch, in_off=0, out_pitch=None, ptr_off=0, batch=1, layout=None):
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    if layout:
        s.set_nv12_layout(*layout)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr + ptr_off), w, h, pitch, P010, C.c_void_p(d_out.ptr), out_pitch or pitch, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
def test_refusals(gpu, batch):
    INVALID, UNSUPPORTED = 1, 4
    ok = dict(smoothing_radius=5)
    assert _push_status(gpu, ok, 64, 48, 128, batch=batch)[0] == 0
    for kw in (dict(w=63, h=48, pitch=128), dict(w=64, h=47, pitch=128), dict(w=64, h=48, pitch=129), dict(w=64, h=48, pitch=128, out_pitch=131),
               dict(w=64, h=48, pitch=128, ptr_off=1), dict(w=64, h=48, pitch=128, layout=(128 * 48 + 1, 0)), dict(w=64, h=48, pitch=128, layout=(0, 128 * 48 + 1))):
        rc, msg = _push_status(gpu, ok, batch=batch, **kw)
        assert rc == INVALID and "P010" in msg, (kw, rc, msg)
    for extra in (dict(border_size=8), dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE), dict(enable_virtual_canvas=1)):
        rc, msg = _push_status(gpu, dict(smoothing_radius=5, **extra), 64, 48, 128, batch=batch)
        assert rc == UNSUPPORTED and "P010" in msg, (extra, rc, msg)
