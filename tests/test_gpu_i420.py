"""I420 / YV12 surfaces on the device, bit for bit.

Every expected value is the oracle's NV12 result for the interleaved samples, de-interleaved (tests/test_i420_cpu.py has the
equivalence): the warp operator against oracle.warp_affine_nv12, the whole stabilizer against the oracle's NV12 run - debug
records and every output frame, flush and the unwarped last frame included.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_i420_cpu import MATS, halved
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

I420 = capi.FMT_I420
CANARY = 0xA5


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def random_nv12(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h * 3 // 2, w), np.uint8)


def expected(oracle, nv12, w, h, M, border=capi.BORDER_BLACK):
    """The oracle's NV12 warp.  BORDER_REPLICATE: the same two cv::warpAffine calls - Y under M, the two-channel chroma plane
    under the matrix with the halved translation - through the oracle's entry point that takes a border mode."""
    if border == capi.BORDER_BLACK:
        return oracle.warp_affine_nv12(nv12, w, h, M)
    out = np.empty_like(nv12)
    out[:h] = oracle.warp_affine_d(np.ascontiguousarray(nv12[:h]), np.asarray(M, np.float32).astype(np.float64), border)
    uv = np.ascontiguousarray(nv12[h:].reshape(h // 2, w // 2, 2))
    out[h:] = oracle.warp_affine_d(uv, halved(M).astype(np.float64), border).reshape(h // 2, w)
    return out


class Layout:
    """An I420 surface layout: pitch, chroma pitch, plane offsets and surface size in bytes (None: the packed default)."""

    def __init__(self, w, h, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None):
        self.w, self.h = w, h
        self.given = dict(pitch=pitch, c_pitch=c_pitch, u_off=u_off, v_off=v_off)
        self.pitch, self.c_pitch, self.u_off, self.v_off = synth.i420_layout(w, h, pitch, c_pitch, u_off, v_off)
        end = max(h * self.pitch, self.u_off + (h // 2) * self.c_pitch, self.v_off + (h // 2) * self.c_pitch)
        self.size = size or end
        # what the library is told: 0 for a field left at its default
        self.args = (u_off or 0, v_off or 0, c_pitch or 0)

    def pack(self, nv12):
        return synth.nv12_to_i420(nv12, self.pitch, self.c_pitch, self.u_off, self.v_off, self.size, CANARY)

    def blank(self, n):
        return np.full((n, self.size), CANARY, np.uint8)

    def unpack(self, buf):
        """The surface's samples as NV12; every byte outside the three planes must still be the canary."""
        hole = synth.nv12_to_i420(np.zeros((self.h * 3 // 2, self.w), np.uint8), self.pitch, self.c_pitch, self.u_off, self.v_off, self.size, 1)
        assert np.all(buf.reshape(-1)[hole == 1] == CANARY), "bytes outside the planes were written"
        return synth.i420_to_nv12(buf, self.w, self.h, self.pitch, self.c_pitch, self.u_off, self.v_off)


# ---- 1. the warp operator ----------------------------------------------------------------------------------------------------
def _warp(gpu, nv12s, w, h, Ms, border=capi.BORDER_BLACK, src=None, dst=None):
    """vs_op_warp_affine_i420 over the I420 surfaces holding the given NV12 samples; returns the results as NV12 surfaces."""
    n = len(nv12s)
    src, dst = src or Layout(w, h), dst or Layout(w, h)
    d_in = capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in nv12s]))
    d_out = capi.DevBuf.from_array(gpu, dst.blank(n))
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(n, 6))
    try:
        gpu.check(gpu.lib.vs_op_warp_affine_i420(d_in.ptr, src.pitch, *src.args, d_out.ptr, dst.pitch, *dst.args, w, h, capi._p(M, capi.f32p), n,
                                                 src.size, dst.size, border, None))
        gpu.sync()
        out = d_out.download((n, dst.size), np.uint8)
    finally:
        d_in.free(); d_out.free()
    return [dst.unpack(o) for o in out]


# around the 128-column and 64-row tile edges of the luma plane (first sizes) and of the half-size chroma planes (256 x 128 luma pixels)
_SIZES = [(2, 2), (126, 30), (128, 32), (130, 34), (254, 62), (256, 64), (258, 66), (256, 128), (258, 130), (322, 200), (514, 98)]


@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE], ids=["black", "replicate"])
@pytest.mark.parametrize("size", _SIZES, ids=lambda s: "%dx%d" % s)
def test_warp_single_surfaces(gpu, oracle, size, border):
    w, h = size
    nv12 = random_nv12(w * 7 + h, w, h)
    for name, M in MATS.items():
        got = _warp(gpu, [nv12], w, h, [M], border)[0]
        assert np.array_equal(got, expected(oracle, nv12, w, h, M, border)), (size, name)


@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE], ids=["black", "replicate"])
@pytest.mark.parametrize("n,size", [(5, (130, 34)), (33, (322, 200)), (33, (258, 130))], ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v)
def test_warp_batches(gpu, oracle, n, size, border):
    """33 surfaces: a launch of 32 and a launch of one."""
    w, h = size
    nv12s = [random_nv12(1000 * n + i, w, h) for i in range(n)]
    names = list(MATS)
    Ms = [MATS[names[i % len(names)]] for i in range(n)]
    got = _warp(gpu, nv12s, w, h, Ms, border)
    for i in range(n):
        assert np.array_equal(got[i], expected(oracle, nv12s[i], w, h, Ms[i], border)), (i, names[i % len(names)])


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_warp_hd_and_4k(gpu, oracle, size):
    w, h = size
    nv12s = [random_nv12(w + i, w, h) for i in range(4)]
    Ms = [MATS[k] for k in ("small_rot", "frac_shift", "rot_zoom_beyond_box", "int_shift")]
    got = _warp(gpu, nv12s, w, h, Ms)
    for i in range(4):
        assert np.array_equal(got[i], expected(oracle, nv12s[i], w, h, Ms[i])), i


def _padded_layouts(w, h):
    """(source, destination) layouts: 16-byte aligned pitches; chroma pitch that is not half the luma pitch; odd chroma pitch and
    plane offsets (no aligned path); YV12 order in and out; planes of a pool with gaps between them."""
    cw, ch = w // 2, h // 2
    return {
        "aligned_pitches": (Layout(w, h, pitch=w + 62), Layout(w, h, pitch=w + 30)),
        "chroma_pitch_not_half": (Layout(w, h, pitch=w + 62, c_pitch=cw + 79), Layout(w, h, pitch=w + 14, c_pitch=w + 14)),
        "odd_chroma_pitch": (Layout(w, h, pitch=w + 2, c_pitch=cw + 3, u_off=h * (w + 2) + 1), Layout(w, h, pitch=w + 6, c_pitch=cw + 1, u_off=h * (w + 6) + 3)),
        "yv12": (Layout(w, h, pitch=w + 30, u_off=h * (w + 30) + ch * (cw + 15), v_off=h * (w + 30)), Layout(w, h, u_off=h * w + ch * cw, v_off=h * w)),
        "yv12_to_i420_apart": (Layout(w, h, pitch=384, c_pitch=256, u_off=384 * (h + 8) + 256 * (ch + 4), v_off=384 * (h + 8), size=384 * (h + 8) + 256 * (2 * ch + 8)),
                               Layout(w, h, pitch=352, c_pitch=192, u_off=352 * (h + 16), v_off=352 * (h + 16) + 192 * (ch + 8), size=352 * (h + 16) + 192 * (2 * ch + 16))),
    }


@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE], ids=["black", "replicate"])
@pytest.mark.parametrize("which", ["aligned_pitches", "chroma_pitch_not_half", "odd_chroma_pitch", "yv12", "yv12_to_i420_apart"])
def test_warp_padded_layouts_leave_everything_else_alone(gpu, oracle, which, border):
    w, h, n = 322, 78, 6
    src, dst = _padded_layouts(w, h)[which]
    nv12s = [random_nv12(len(which) * 11 + i, w, h) for i in range(n)]
    Ms = [MATS[k] for k in ("small_rot", "frac_shift", "rot_zoom_beyond_box", "identity", "saturated", "int_shift")]
    got = _warp(gpu, nv12s, w, h, Ms, border, src, dst)
    for i in range(n):
        assert np.array_equal(got[i], expected(oracle, nv12s[i], w, h, Ms[i], border)), i


def test_warp_of_a_surface_wider_than_the_packed_kernel_takes(gpu, oracle):
    """65536 columns: outside what the one-launch kernel packs into 16 bits - the per-plane kernels, the same result."""
    w, h = 65536, 2
    nv12 = random_nv12(9, w, h)
    for name in ("identity", "int_shift", "frac_shift"):
        got = _warp(gpu, [nv12], w, h, [MATS[name]])[0]
        assert np.array_equal(got, expected(oracle, nv12, w, h, MATS[name])), name


def test_warp_refuses_bad_geometry(gpu):
    d = capi.DevBuf(gpu, 1 << 16)
    M = np.asarray(MATS["identity"], np.float32)
    #         w   h   pitch (u, v, c_pitch)
    for w, h, sp, lay in ((31, 24, 64, (0, 0, 0)), (32, 23, 64, (0, 0, 0)), (32, 24, 65, (0, 0, 0)), (32, 24, 64, (0, 0, 15)), (32, 24, 30, (0, 0, 0))):
        rc = gpu.lib.vs_op_warp_affine_i420(d.ptr, sp, *lay, d.ptr + 32768, 64, 0, 0, 0, w, h, capi._p(M, capi.f32p), 1, 36 * 64, 36 * 64, 0, None)
        assert rc == 1, (w, h, sp, lay)                        # VS_ERR_INVALID_ARG
        assert gpu.lib.vs_last_error()
    rc = gpu.lib.vs_op_warp_affine_i420(d.ptr, 64, 0, 0, 0, d.ptr + 32768, 64, 0, 0, 15, 32, 24, capi._p(M, capi.f32p), 1, 36 * 64, 36 * 64, 0, None)
    assert rc == 1
    d.free()


# ---- 2. the stabilizer ---------------------------------------------------------------------------------------------------------
def _oracle_nv12_run(oracle, clip, **params):
    """The oracle's NV12 stabilizer over the clip, flush included: its output frames and, per push, its debug record."""
    so = oracle.stabilizer(oracle.params(**params))
    outs, dbg = [], []
    for f in clip:
        o = so.push(f, capi.FMT_NV12)
        d = so.debug()
        dbg.append(dict(transform=np.array(d.transform), smoothed=np.array(d.smoothed), warp=np.array(d.warp_matrix), has=o is not None,
                        counts=(d.n_prev, d.n_valid, d.n_detected, d.detected), out_index=d.out_index))
        if o is not None:
            outs.append(o)
    while True:
        o = so.flush(clip[0], capi.FMT_NV12)
        if o is None:
            break
        outs.append(o)
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


def _check_outputs(got, ref, clip):
    """got: the device results as NV12 frames, in order; ref: the oracle's.  The last one is the clip's last frame, unwarped."""
    assert len(got) == len(ref) == len(clip)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), k
    assert np.array_equal(got[-1], clip[-1])


@pytest.fixture(scope="module")
def small():
    w, h, n = 322, 200, 40
    return w, h, [synth.bgr_to_nv12(f) for f in synth.make_clip(synth.SEED_CONFIG3 + 21, w, h, n)]


@pytest.fixture(scope="module")
def oracle_runs(oracle, small):
    """The oracle's run of the first n frames of the small clip under the given parameters, computed once per module."""
    cache = {}

    def run(n, **params):
        key = (n, tuple(sorted(params.items())))
        if key not in cache:
            cache[key] = _oracle_nv12_run(oracle, small[2][:n], **params)
        return cache[key]
    return run


@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_GAUSSIAN, capi.SMOOTH_KALMAN], ids=["box", "gaussian", "kalman"])
def test_pipeline_per_frame(gpu, small, oracle_runs, method):
    w, h, nv12 = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = oracle_runs(len(nv12), **params)
    sg = gpu.stabilizer(gpu.params(**params))
    got = []
    for k, f in enumerate(nv12):
        o = sg.push(synth.nv12_to_i420(f), I420)
        assert (o is not None) == dbg[k]["has"], k
        _check_debug(sg.debug(), dbg[k], k)
        if o is not None:
            assert o.dtype == np.uint8 and o.shape == f.shape
            got.append(synth.i420_to_nv12(o, w, h))
    while True:
        o = sg.flush(nv12[0], I420)
        if o is None:
            break
        got.append(synth.i420_to_nv12(o, w, h))
    ow, oh = C.c_int32(), C.c_int32()
    gpu.check(gpu.lib.vs_stab_last_out_dims(sg.h, C.byref(ow), C.byref(oh)), sg.h)
    assert (ow.value, oh.value) == (w, h)
    sg.close()
    _check_outputs(got, ref, nv12)


def _batch_run(gpu, nv12, w, h, batch, params, zero_copy=True, src=None, dst=None, fmt=I420):
    """The clip through push_dev with set_batch(batch), drained through flush_dev; the results as NV12 frames and the last debug record.
    fmt = NV12: the same clip as NV12 surfaces (the sibling path of the same process)."""
    n = len(nv12)
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    s.set_zero_copy(zero_copy)
    if fmt == I420:
        src, dst = src or Layout(w, h), dst or Layout(w, h)
        if any(src.args) or any(dst.args):
            s.set_i420_layout(*src.args, *dst.args)
        frames, isz, osz, ip, op = np.stack([src.pack(f) for f in nv12]), src.size, dst.size, src.pitch, dst.pitch
        blank = dst.blank(n)
    else:
        frames, isz, osz, ip, op = np.stack(nv12), nv12[0].nbytes, nv12[0].nbytes, w, w
        blank = np.full((n, osz), CANARY, np.uint8)
    d_in, d_out = capi.DevBuf.from_array(gpu, frames), capi.DevBuf.from_array(gpu, blank)
    try:
        k = 0
        for i in range(n):
            k += s.push_dev(d_in.ptr + i * isz, w, h, ip, fmt, d_out.ptr + k * osz, op)
        s.sync()
        last = s.debug()
        last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
        while s.flush_dev(d_out.ptr + k * osz, op):
            k += 1
        s.sync()
        out = d_out.download((n, osz), np.uint8)
    finally:
        s.close(); d_in.free(); d_out.free()
    if fmt == I420:
        return [dst.unpack(out[i]) for i in range(k)], last
    return [out[i].reshape(h * 3 // 2, w) for i in range(k)], last


@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_KALMAN], ids=["box", "kalman"])
def test_pipeline_batch_mode_with_partial_batches(gpu, small, oracle_runs, batch, method):
    """40 frames: five steps of 8, or one partial step of a batch of 64; warp launches of fewer than four frames included."""
    w, h, nv12 = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = oracle_runs(len(nv12), **params)
    got, last = _batch_run(gpu, nv12, w, h, batch, params)
    assert np.array_equal(bits(last["transform"]), bits(dbg[-1]["transform"]))
    assert np.array_equal(bits(last["smoothed"]), bits(dbg[-1]["smoothed"])) and np.array_equal(bits(last["warp"]), bits(dbg[-1]["warp"]))
    _check_outputs(got, ref, nv12)


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("which", ["chroma_pitch_not_half", "yv12_to_i420_apart", "odd_chroma_pitch"])
def test_pipeline_with_different_input_and_output_layouts(gpu, small, oracle_runs, zero_copy, which):
    w, h, nv12 = small
    params = dict(smoothing_radius=6)
    ref, _ = oracle_runs(24, **params)
    src, dst = _padded_layouts(w, h)[which]
    got, _ = _batch_run(gpu, nv12[:24], w, h, 8, params, zero_copy, src, dst)
    _check_outputs(got, ref, nv12[:24])


def test_i420_and_nv12_streams_of_the_same_samples_in_one_process(gpu, small):
    w, h, nv12 = small
    params = dict(smoothing_radius=6)
    a, la = _batch_run(gpu, nv12[:24], w, h, 8, params, fmt=capi.FMT_NV12)
    b, lb = _batch_run(gpu, nv12[:24], w, h, 8, params, fmt=I420)
    assert len(a) == len(b) == 24
    for k in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(la[k]), bits(lb[k])), k
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[:h], y[:h]), i
        assert np.array_equal(x[h:, 0::2], y[h:, 0::2]) and np.array_equal(x[h:, 1::2], y[h:, 1::2]), i


def test_vs_batch_of_three_streams_against_standalone_instances(gpu, oracle, small):
    w, h, nv12 = small
    n, S = 24, 3
    params = dict(smoothing_radius=6)
    src, dst = _padded_layouts(w, h)["chroma_pitch_not_half"]
    clips = [[np.roll(f, 2 * g, axis=1) for f in nv12[:n]] for g in range(S)]        # (an even shift keeps the U, V order)
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in c])) for c in clips]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    b = gpu.batch(gpu.params(**params), S, 8)
    b.set_zero_copy(True)
    b.set_i420_layout(*src.args, *dst.args)
    k = [0] * S
    for i in range(n):
        prod = b.push_dev([d_in[g].ptr + i * src.size for g in range(S)], w, h, src.pitch, I420, [d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    b.close()
    for g in range(S):
        raw = d_out[g].download((n, dst.size), np.uint8)
        got = [dst.unpack(raw[i]) for i in range(k[g])]
        alone, _ = _batch_run(gpu, clips[g], w, h, 8, params, True, src, dst)
        assert len(got) == len(alone) == n
        for a, c in zip(got, alone):
            assert np.array_equal(a, c), g
        ref, _ = _oracle_nv12_run(oracle, clips[g], **params)
        _check_outputs(got, ref, clips[g])
    for d in d_in + d_out:
        d.free()


def test_vs_batch_refuses_members_that_disagree_on_the_layout(gpu):
    """A layout change while one member has a frame queued reaches the members in front of it only (VS_ERR_INVALID_ARG); the
    next step finds members with different layouts and refuses them."""
    w, h = 64, 48
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    b = gpu.batch(gpu.params(smoothing_radius=5), 2, 4)
    b.set_zero_copy(True)
    assert b.push_dev([None, d_in.ptr], w, h, w, I420, [None, d_out.ptr], w) == [0, 0]
    with pytest.raises(capi.VsError, match="queue must be empty"):
        b.set_i420_layout(0, 0, 64, 0, 0, 0)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        for _ in range(8):
            b.push_dev([d_in.ptr, d_in.ptr], w, h, w, I420, [d_out.ptr, d_out.ptr + (1 << 19)], w)
    b.close(); d_in.free(); d_out.free()


@pytest.mark.parametrize("size,n", [((1920, 1080), 12), ((3840, 2160), 8)], ids=["1080p", "4k"])
def test_pipeline_hd_and_4k_batch_mode(gpu, oracle, size, n):
    w, h = size
    d = synth.make_clip_dev(gpu, synth.SEED_CONFIG3 + 2, w, h, n, nv12=True)
    nv12 = list(d.download((n, h * 3 // 2, w), np.uint8))
    d.free()
    params = dict(smoothing_radius=5, max_corners=400)
    oracle.lib.vso_set_threads(8)
    try:
        ref, dbg = _oracle_nv12_run(oracle, nv12, **params)
    finally:
        oracle.lib.vso_set_threads(1)
    got, last = _batch_run(gpu, nv12, w, h, 4, params)
    assert np.array_equal(bits(last["transform"]), bits(dbg[-1]["transform"])) and np.array_equal(bits(last["warp"]), bits(dbg[-1]["warp"]))
    _check_outputs(got, ref, nv12)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def _push_status(gpu, params, w, h, pitch, out_pitch=None, batch=1, layout=None):
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    if layout:
        s.set_i420_layout(*layout)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr), w, h, pitch, I420, C.c_void_p(d_out.ptr), out_pitch or pitch, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
def test_refusals(gpu, batch):
    INVALID, UNSUPPORTED = 1, 4
    ok = dict(smoothing_radius=5)
    assert _push_status(gpu, ok, 64, 48, 64, batch=batch)[0] == 0
    assert _push_status(gpu, ok, 64, 48, 128, batch=batch, layout=(0, 0, 32, 0, 0, 32))[0] == 0
    for kw in (dict(w=63, h=48, pitch=64), dict(w=64, h=47, pitch=64), dict(w=64, h=48, pitch=65), dict(w=64, h=48, pitch=64, out_pitch=67),
               dict(w=64, h=48, pitch=64, layout=(0, 0, 31, 0, 0, 0)), dict(w=64, h=48, pitch=64, layout=(0, 0, 0, 0, 0, 31))):
        rc, msg = _push_status(gpu, ok, batch=batch, **kw)
        assert rc == INVALID and "I420" in msg, (kw, rc, msg)
    for extra in (dict(border_size=8), dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE), dict(enable_virtual_canvas=1)):
        rc, msg = _push_status(gpu, dict(smoothing_radius=5, **extra), 64, 48, 64, batch=batch)
        assert rc == UNSUPPORTED and "I420" in msg, (extra, rc, msg)


@pytest.mark.parametrize("batch", [1, 8])
def test_layout_change_with_frames_queued_is_refused(gpu, batch):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5))
    s.set_batch(batch)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    s.set_i420_layout(0, 0, 64, 0, 0, 64)                    # nothing queued: accepted
    assert s.push_dev(d_in.ptr, 64, 48, 64, I420, d_out.ptr, 64) == 0
    rc = gpu.lib.vs_stab_set_i420_layout(s.h, 0, 0, 0, 0, 0, 0)
    assert rc == 1 and "queue must be empty" in (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
