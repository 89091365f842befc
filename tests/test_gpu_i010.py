"""I010 / I012 surfaces on the device, bit for bit.

The warp operator against tests/ref16.py plane by plane (i010_inputs.warp_three_planes; tests/test_i010_cpu.py ties it to the
P010 reference); the analysis gray image against the oracle's gray image of the plane min(sample >> (bits - 8), 255); and the
whole stabilizer: a stream's debug records equal those of the oracle's NV12 run on the analysis bytes, and every output is the
reference warp of input `out_index` under that record's matrix - flush and the unwarped last frame included."""
import ctypes as C

import numpy as np
import pytest

import i010_inputs as ii
from i010_inputs import Layout
from p010_inputs import MATS
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

I010, I012 = capi.FMT_I010, capi.FMT_I012
BORDERS = pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE], ids=["black", "replicate"])


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. the warp operator ----------------------------------------------------------------------------------------------------
def _warp(gpu, frames, w, h, Ms, border=capi.BORDER_BLACK, src=None, dst=None):
    """vs_op_warp_affine_i010 over the surfaces holding the given packed frames; the results as packed frames (unpack checks
    that nothing outside the planes was written)."""
    n = len(frames)
    src, dst = src or Layout(w, h), dst or Layout(w, h)
    d_in = capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in frames]))
    d_out = capi.DevBuf.from_array(gpu, dst.blank(n))
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(n, 6))
    try:
        gpu.check(gpu.lib.vs_op_warp_affine_i010(d_in.ptr, src.pitch, *src.args, d_out.ptr, dst.pitch, *dst.args, w, h, capi._p(M, capi.f32p), n,
                                                 src.size, dst.size, border, None))
        gpu.sync()
        out = d_out.download((n, dst.size // 2), np.uint16)
    finally:
        d_in.free(); d_out.free()
    return [dst.unpack(o) for o in out]


# around the edges of the luma tiles (128 x 32) and of the chroma tiles (128 x 32 chroma pixels = 256 x 64 luma pixels)
_SIZES = [(2, 2), (126, 30), (130, 34), (254, 62), (258, 66), (322, 200), (514, 130)]


@BORDERS
@pytest.mark.parametrize("full_range", [False, True], ids=["ten-bit", "full-range"])
@pytest.mark.parametrize("size", _SIZES, ids=lambda s: "%dx%d" % s)
def test_warp_single_surfaces(gpu, size, full_range, border):
    w, h = size
    frame = ii.random_frame(w, w, h, 10, full_range)        # (258 x 66, ten-bit: the frame whose rounding ties test_i010_cpu.py counts)
    for name, M in MATS.items():
        got = _warp(gpu, [frame], w, h, [M], border)[0]
        assert np.array_equal(got, ii.warp_three_planes(frame, w, h, M, border)), (size, name)


@BORDERS
@pytest.mark.parametrize("n,size", [(5, (130, 34)), (33, (258, 66))], ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v)
def test_warp_batches(gpu, n, size, border):
    """33 surfaces: a launch of 32 and a launch of one."""
    w, h = size
    frames = [ii.random_frame(1000 * n + i, w, h, 10, i % 2 == 1) for i in range(n)]
    names = list(MATS)
    Ms = [MATS[names[i % len(names)]] for i in range(n)]
    got = _warp(gpu, frames, w, h, Ms, border)
    for i in range(n):
        assert np.array_equal(got[i], ii.warp_three_planes(frames[i], w, h, Ms[i], border)), (i, names[i % len(names)])


def test_warp_1080p(gpu):
    w, h = 1920, 1080
    frame = ii.random_frame(w, w, h, 12)
    for name in ("small_rot", "rot_zoom_beyond_box"):
        got = _warp(gpu, [frame], w, h, [MATS[name]])[0]
        assert np.array_equal(got, ii.warp_three_planes(frame, w, h, MATS[name])), name


def _padded_layouts(w, h):
    """(source, destination) layouts, in bytes: 16-byte aligned pitches; pitches and offsets that are only even (no aligned path);
    a chroma pitch that is not half the luma pitch; V before U, in and out; planes of a pool with gaps between them."""
    cw, ch = w, h // 2                                      # bytes of a chroma row, chroma rows
    return {
        "aligned_pitches": (Layout(w, h, pitch=2 * w + 60), Layout(w, h, pitch=2 * w + 28)),
        "only_even": (Layout(w, h, pitch=2 * w + 2, c_pitch=cw + 4, u_off=h * (2 * w + 2) + 2), Layout(w, h, pitch=2 * w + 6, c_pitch=cw + 8, u_off=h * (2 * w + 6) + 6)),
        "chroma_pitch_not_half": (Layout(w, h, pitch=2 * w + 124, c_pitch=cw + 158), Layout(w, h, pitch=2 * w + 28, c_pitch=2 * w + 28)),
        "v_first": (Layout(w, h, pitch=2 * w + 60, u_off=h * (2 * w + 60) + ch * (cw + 30), v_off=h * (2 * w + 60)),
                    Layout(w, h, u_off=h * 2 * w + ch * cw, v_off=h * 2 * w)),
        "v_first_to_u_first_apart": (Layout(w, h, pitch=768, c_pitch=512, u_off=768 * (h + 8) + 512 * (ch + 4), v_off=768 * (h + 8), size=768 * (h + 8) + 512 * (2 * ch + 8)),
                                     Layout(w, h, pitch=704, c_pitch=384, u_off=704 * (h + 16), v_off=704 * (h + 16) + 384 * (ch + 8), size=704 * (h + 16) + 384 * (2 * ch + 16))),
    }


@BORDERS
@pytest.mark.parametrize("which", ["aligned_pitches", "only_even", "chroma_pitch_not_half", "v_first", "v_first_to_u_first_apart"])
def test_warp_padded_layouts_leave_everything_else_alone(gpu, which, border):
    w, h, n = 322, 78, 6
    src, dst = _padded_layouts(w, h)[which]
    frames = [ii.random_frame(len(which) * 11 + i, w, h, 10, i == 5) for i in range(n)]
    Ms = [MATS[k] for k in ("small_rot", "frac_shift", "rot_zoom_beyond_box", "identity", "saturated", "int_shift")]
    got = _warp(gpu, frames, w, h, Ms, border, src, dst)
    for i in range(n):
        assert np.array_equal(got[i], ii.warp_three_planes(frames[i], w, h, Ms[i], border)), i


def test_warp_refuses_odd_geometry(gpu):
    d = capi.DevBuf(gpu, 1 << 16)
    M = np.asarray(MATS["identity"], np.float32)
    ok = dict(w=32, h=24, sp=64, lay=(0, 0, 0), off=0, dp=64, dlay=(0, 0, 0), fb=36 * 64)

    def call(**kw):
        a = dict(ok, **kw)
        return gpu.lib.vs_op_warp_affine_i010(d.ptr + a["off"], a["sp"], *a["lay"], d.ptr + 32768, a["dp"], *a["dlay"], a["w"], a["h"], capi._p(M, capi.f32p), 1,
                                              a["fb"], 36 * 64, 0, None)
    assert call() == 0
    gpu.sync()
    # odd w, h, pointer, pitch, chroma pitch, offsets, frame distance; a default chroma pitch of odd samples; a chroma pitch below w bytes
    for kw in (dict(w=31), dict(h=23), dict(off=1), dict(sp=65), dict(dp=67), dict(lay=(0, 0, 33)), dict(lay=(64 * 24 + 1, 0, 0)), dict(dlay=(0, 64 * 30 + 1, 0)),
               dict(fb=36 * 64 + 1), dict(sp=66), dict(dp=70), dict(lay=(0, 0, 30)), dict(dlay=(0, 0, 30))):
        assert call(**kw) == 1, kw                               # VS_ERR_INVALID_ARG
        assert gpu.lib.vs_last_error()
    d.free()


# ---- 2. the analysis gray image ----------------------------------------------------------------------------------------------
_GRAY = [((1920, 1080), (960, 540)), ((3840, 2160), (960, 540)), ((1280, 720), (960, 540)), ((322, 200), (960, 540))]
_GRAY_IDS = ["half", "quarter", "general", "upscale"]


@pytest.mark.parametrize("fmt,depth", [(I010, 10), (I012, 12)], ids=["I010", "I012"])
@pytest.mark.parametrize("full_range", [False, True], ids=["in-range", "full-range"])
@pytest.mark.parametrize("src,dst", _GRAY, ids=_GRAY_IDS)
def test_resize_gray_single(gpu, oracle, src, dst, full_range, fmt, depth):
    (w, h), (dw, dh) = src, dst
    y = np.random.default_rng(w + depth).integers(0, 65536 if full_range else 1 << depth, (h, w), np.uint16)
    want = oracle.analysis_gray(np.ascontiguousarray(ii.analysis_byte(y, depth)), dw, dh)
    assert np.array_equal(gpu.resize_gray(y, dw, dh, fmt), want)


@pytest.mark.parametrize("src", [s for s, _ in _GRAY], ids=_GRAY_IDS)
def test_resize_gray_through_a_batch_step(gpu, oracle, src):
    """Four frames through one step of the batch schedule: the analysis image of the last one (debug getter).  The last frame is
    full-range I012 content: the saturation of the batch kernels."""
    w, h = src
    n = 4
    frames = np.stack([ii.random_frame(w + 10 + i, w, h, 12, i == n - 1) for i in range(n)])
    fb = frames[0].nbytes
    s = gpu.stabilizer(gpu.params(smoothing_radius=5))
    s.set_batch(4)
    s.set_zero_copy(True)
    d_in, d_out = capi.DevBuf.from_array(gpu, frames), capi.DevBuf(gpu, fb)
    for i in range(n):
        assert s.push_dev(d_in.ptr + i * fb, w, h, 2 * w, I012, d_out.ptr, 2 * w) == 0
    s.sync()
    gray = s.debug_arrays()["gray"]
    s.close(); d_in.free(); d_out.free()
    want = oracle.analysis_gray(np.ascontiguousarray(ii.analysis_byte(frames[-1][:h], 12)), 960, 540)
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


def _check_outputs(got, clip, ref, w, h):
    """got: the device results in order; ref: (out_index, matrix) per result.  The last frame of the clip has no transform."""
    assert len(got) == len(ref) == len(clip)
    for k, (g, (idx, M)) in enumerate(zip(got, ref)):
        want = clip[idx] if idx == len(clip) - 1 else ii.warp_three_planes(clip[idx], w, h, M)
        assert np.array_equal(g, want), (k, idx)


@pytest.fixture(scope="module")
def small():
    """(w, h, NV12 clip, the P010 clip with live low bits, its I010 clip, its I012 clip).  The analysis bytes of all three 16-bit
    clips are the NV12 clip's luma bytes."""
    w, h, n = 322, 200, 40
    nv12 = [synth.bgr_to_nv12(f) for f in synth.make_clip(synth.SEED_CONFIG3 + 21, w, h, n)]
    p010 = [synth.nv12_to_p010(f, seed=i) for i, f in enumerate(nv12)]
    return w, h, nv12, p010, [synth.p010_to_i010(f, w, h, 10) for f in p010], [synth.p010_to_i010(f, w, h, 12) for f in p010]


@pytest.fixture(scope="module")
def oracle_runs(oracle, small):
    """The oracle's NV12 run over the first n frames of the small clip under the given parameters, computed once per module."""
    cache = {}

    def run(n, **params):
        key = (n, tuple(sorted(params.items())))
        if key not in cache:
            cache[key] = _oracle_nv12_run(oracle, small[2][:n], **params)
        return cache[key]
    return run


def _per_frame(gpu, clip, fmt, w, h, params, dbg):
    """The host entry points, frame by frame: every debug record against the oracle's; the results in order."""
    sg = gpu.stabilizer(gpu.params(**params))
    got = []
    for k, f in enumerate(clip):
        o = sg.push(f, fmt)
        assert (o is not None) == dbg[k]["has"], k
        _check_debug(sg.debug(), dbg[k], k)
        if o is not None:
            assert o.dtype == np.uint16 and o.shape == f.shape
            got.append(o)
    while True:
        o = sg.flush(clip[0], fmt)
        if o is None:
            break
        got.append(o)
    ow, oh = C.c_int32(), C.c_int32()
    gpu.check(gpu.lib.vs_stab_last_out_dims(sg.h, C.byref(ow), C.byref(oh)), sg.h)
    assert (ow.value, oh.value) == (w, h)
    sg.close()
    return got


@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_GAUSSIAN, capi.SMOOTH_KALMAN], ids=["box", "gaussian", "kalman"])
def test_pipeline_per_frame(gpu, small, oracle_runs, method):
    w, h, nv12, _, i010, _ = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = oracle_runs(len(nv12), **params)
    _check_outputs(_per_frame(gpu, i010, I010, w, h, params, dbg), i010, ref, w, h)


def test_pipeline_per_frame_i012(gpu, small, oracle_runs):
    w, h, nv12, _, _, i012 = small
    params = dict(smoothing_radius=10, smoothing_method=capi.SMOOTH_BOX)
    ref, dbg = oracle_runs(len(nv12), **params)
    _check_outputs(_per_frame(gpu, i012, I012, w, h, params, dbg), i012, ref, w, h)


def _batch_run(gpu, clip, w, h, batch, params, zero_copy=True, src=None, dst=None, fmt=I010, push_n=0):
    """The clip through push_dev (push_n > 0: push_dev_n, that many frames a call) with set_batch(batch), drained through flush_dev;
    the results as packed frames and the last debug record.  fmt = P010: the clip as P010 surfaces (the sibling path)."""
    n = len(clip)
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    s.set_zero_copy(zero_copy)
    if fmt == capi.FMT_P010:
        frames, isz, osz, ip, op = np.stack(clip), clip[0].nbytes, clip[0].nbytes, 2 * w, 2 * w
        blank = np.full((n, osz // 2), ii.CANARY, np.uint16)
    else:
        src, dst = src or Layout(w, h), dst or Layout(w, h)
        if any(src.args) or any(dst.args):
            s.set_i420_layout(*src.args, *dst.args)
        frames, isz, osz, ip, op = np.stack([src.pack(f) for f in clip]), src.size, dst.size, src.pitch, dst.pitch
        blank = dst.blank(n)
    d_in, d_out = capi.DevBuf.from_array(gpu, frames), capi.DevBuf.from_array(gpu, blank)
    try:
        k = 0
        for i in range(0, n, push_n or 1):
            if push_n:
                m = min(push_n, n - i)
                k += s.push_dev_n([d_in.ptr + (i + j) * isz for j in range(m)], w, h, ip, fmt, [d_out.ptr + (k + j) * osz for j in range(m)], op)
            else:
                k += s.push_dev(d_in.ptr + i * isz, w, h, ip, fmt, d_out.ptr + k * osz, op)
        s.sync()
        last = s.debug()
        last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
        while s.flush_dev(d_out.ptr + k * osz, op):
            k += 1
        s.sync()
        out = d_out.download((n, osz // 2), np.uint16)
    finally:
        s.close(); d_in.free(); d_out.free()
    if fmt == capi.FMT_P010:
        return [out[i].reshape(h * 3 // 2, w) for i in range(k)], last
    return [dst.unpack(out[i]) for i in range(k)], last


def _same_last(last, want):
    for k in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(last[k]), bits(want[k])), k


@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_KALMAN], ids=["box", "kalman"])
def test_pipeline_batch_mode_with_partial_batches(gpu, small, oracle_runs, batch, method):
    """40 frames: five steps of 8, or one partial step of a batch of 64; warp launches of fewer than four frames included."""
    w, h, nv12, _, i010, _ = small
    params = dict(smoothing_radius=10, smoothing_method=method)
    ref, dbg = oracle_runs(len(nv12), **params)
    got, last = _batch_run(gpu, i010, w, h, batch, params)
    _same_last(last, dbg[-1])
    _check_outputs(got, i010, ref, w, h)


def test_pipeline_push_dev_n(gpu, small, oracle_runs):
    w, h, nv12, _, i010, _ = small
    params = dict(smoothing_radius=6)
    ref, dbg = oracle_runs(24, **params)
    got, last = _batch_run(gpu, i010[:24], w, h, 8, params, push_n=5)
    _same_last(last, dbg[23])
    _check_outputs(got, i010[:24], ref, w, h)


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("which", ["chroma_pitch_not_half", "v_first_to_u_first_apart", "only_even"])
def test_pipeline_with_different_input_and_output_layouts(gpu, small, oracle_runs, zero_copy, which):
    w, h, nv12, _, i010, _ = small
    params = dict(smoothing_radius=6)
    ref, _ = oracle_runs(24, **params)
    src, dst = _padded_layouts(w, h)[which]
    got, _ = _batch_run(gpu, i010[:24], w, h, 8, params, zero_copy, src, dst)
    _check_outputs(got, i010[:24], ref, w, h)


def test_i010_and_p010_streams_in_one_process(gpu, small):
    """The P010 stream holds sample << 6: the same analysis bytes, so the same records.  (Not the same pixels: the blend's one
    rounding does not commute with the shift.)"""
    w, h, _, p010, i010, _ = small
    params = dict(smoothing_radius=6)
    a, la = _batch_run(gpu, p010[:24], w, h, 8, params, fmt=capi.FMT_P010)
    b, lb = _batch_run(gpu, i010[:24], w, h, 8, params)
    assert len(a) == len(b) == 24
    _same_last(la, lb)
    s1, s2 = gpu.stabilizer(gpu.params(**params)), gpu.stabilizer(gpu.params(**params))
    for k in range(24):
        s1.push(p010[k], capi.FMT_P010)
        s2.push(i010[k], I010)
        d1, d2 = s1.debug(), s2.debug()
        assert (d1.n_prev, d1.n_valid, d1.n_detected, d1.detected, d1.out_index) == (d2.n_prev, d2.n_valid, d2.n_detected, d2.detected, d2.out_index), k
        for f in ("transform", "smoothed", "warp_matrix"):
            assert np.array_equal(bits(getattr(d1, f)), bits(getattr(d2, f))), (k, f)
    s1.close(); s2.close()


def test_vs_batch_of_three_streams_against_standalone_instances(gpu, oracle, small):
    w, h, nv12, _, i010, _ = small
    n, S = 24, 3
    params = dict(smoothing_radius=6)
    src, dst = _padded_layouts(w, h)["chroma_pitch_not_half"]

    def rolled(f, g):                                   # every plane shifted along its rows: another picture, the same layout
        return np.concatenate([np.roll(p, (2 * g, g)[i > 0], axis=1).reshape(-1) for i, p in enumerate(ii.planes(f, w, h))]).reshape(f.shape)
    clips = [[rolled(f, g) for f in i010[:n]] for g in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in c])) for c in clips]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    b = gpu.batch(gpu.params(**params), S, 8)
    b.set_zero_copy(True)
    b.set_i420_layout(*src.args, *dst.args)
    k = [0] * S
    for i in range(n):
        prod = b.push_dev([d_in[g].ptr + i * src.size for g in range(S)], w, h, src.pitch, I010, [d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    b.close()
    for g in range(S):
        raw = d_out[g].download((n, dst.size // 2), np.uint16)
        got = [dst.unpack(raw[i]) for i in range(k[g])]
        alone, _ = _batch_run(gpu, clips[g], w, h, 8, params, True, src, dst)
        assert len(got) == len(alone) == n
        for a, c in zip(got, alone):
            assert np.array_equal(a, c), g
        # an NV12 frame of the same shape: the analysis bytes as luma (the chroma rows are not looked at)
        ref, _ = _oracle_nv12_run(oracle, [np.ascontiguousarray(ii.analysis_byte(f, 10)) for f in clips[g]], **params)
        _check_outputs(got, clips[g], ref, w, h)
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
    assert b.push_dev([None, d_in.ptr], w, h, 2 * w, I010, [None, d_out.ptr], 2 * w) == [0, 0]
    with pytest.raises(capi.VsError, match="queue must be empty"):
        b.set_i420_layout(0, 0, 128, 0, 0, 0)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        for _ in range(8):
            b.push_dev([d_in.ptr, d_in.ptr], w, h, 2 * w, I010, [d_out.ptr, d_out.ptr + (1 << 19)], 2 * w)
    b.close(); d_in.free(); d_out.free()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def _push_status(gpu, params, w, h, pitch, out_pitch=None, ptr_off=0, batch=1, layout=None, fmt=I010):
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    if layout:
        s.set_i420_layout(*layout)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr + ptr_off), w, h, pitch, fmt, C.c_void_p(d_out.ptr), out_pitch or pitch, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
def test_refusals(gpu, batch):
    INVALID, UNSUPPORTED = 1, 4
    ok = dict(smoothing_radius=5)
    assert _push_status(gpu, ok, 64, 48, 128, batch=batch)[0] == 0
    assert _push_status(gpu, ok, 64, 48, 128, batch=batch, fmt=I012)[0] == 0
    assert _push_status(gpu, ok, 64, 48, 130, batch=batch, layout=(0, 0, 64, 0, 0, 66))[0] == 0        # pitches that are only even
    # odd geometry; odd pitch, output pitch, pointer; a default chroma pitch of odd bytes; odd offsets; a chroma pitch below w bytes
    for kw in (dict(w=63, h=48, pitch=128), dict(w=64, h=47, pitch=128), dict(w=64, h=48, pitch=129), dict(w=64, h=48, pitch=128, out_pitch=131),
               dict(w=64, h=48, pitch=128, ptr_off=1), dict(w=64, h=48, pitch=130), dict(w=64, h=48, pitch=128, out_pitch=134),
               dict(w=64, h=48, pitch=128, layout=(128 * 48 + 1, 0, 0, 0, 0, 0)), dict(w=64, h=48, pitch=128, layout=(0, 0, 0, 0, 128 * 60 + 1, 0)),
               dict(w=64, h=48, pitch=128, layout=(0, 0, 62, 0, 0, 0)), dict(w=64, h=48, pitch=128, layout=(0, 0, 0, 0, 0, 62))):
        rc, msg = _push_status(gpu, ok, batch=batch, **kw)
        assert rc == INVALID and "I010" in msg, (kw, rc, msg)
    for extra in (dict(border_size=8), dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE), dict(enable_virtual_canvas=1)):
        rc, msg = _push_status(gpu, dict(smoothing_radius=5, **extra), 64, 48, 128, batch=batch)
        assert rc == UNSUPPORTED and "I010" in msg, (extra, rc, msg)
