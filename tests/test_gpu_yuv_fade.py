"""The fade border on YUV streams on the device, bit for bit: vs_op_fade_blend_jobs and vs_op_fade_update_jobs against
tests/yuvfaderef.py, and streams with vs_stab_set_yuv_fade against surfaces built without the code under test: the oracle's NV12 run
with border_size = 0 gives out_index and matrix of every result, yuvfaderef pads and blends every plane with the history, every
blended plane is warped under BORDER_REPLICATE by the oracle's double-precision warp (8-bit) or i010_inputs.warp_plane (16-bit) with
the format's chroma matrix, yuvfaderef updates the history, and the recurrence is run frame by frame.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import compref
import planar_inputs as pi
import plane_job_refusals as pjr
import roi
import yuvfaderef as yf
import yuvpadref as yp
from test_gpu_planar import _check_debug
from test_gpu_yuv_border_pad import _decoder_layouts, _padded, _unpack_last, chosen_fill, default_fill
from test_gpu_yuv_cropzoom import Fmt, _same, world  # noqa: F401  (world: the module's clips and oracle runs)
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
F = np.float32
# (w, h), (bx, by): planes smaller than their border, the streams' planes, several tiles across and down, unequal borders, no border
SHAPES = [((1, 1), (3, 3)), ((2, 3), (7, 7)), ((5, 4), (7, 7)), ((126, 92), (2, 2)), ((322, 200), (30, 30)), ((64, 48), (15, 30)), ((40, 40), (0, 0))]
SHAPE_IDS = ["%dx%d+%dx%d" % (s + b) for s, b in SHAPES]
RAMP7 = F(0.1) * (F(7) / F(30))
ALPHAS = [F(0), F(0.5), F(0.1), RAMP7]
# (source, history, destination) sides of tests/roi.py, each aligned by itself
TRIPLES8 = [("packed", "packed", "packed"), ("padded16", "padded16", "padded16"), ("roi_off1", "roi_off3", "roi_off2"), ("odd_pitch", "padded16", "odd_pitch"),
            ("padded16", "odd_pitch", "padded16"), ("roi_off2", "padded16", "roi_off1"), ("tight_end", "tight_end", "tight_end")]
TRIPLES16 = [("packed", "packed", "packed"), ("padded16", "padded16", "padded16"), ("roi_off2", "padded16", "tight_end"), ("tight_end", "roi_off2", "padded16")]
FRAME16 = [0, 1, 63, 64, 1023, 4095, 0x8000, 0xffc0, 65535] + [int(v) for v in np.random.default_rng(16).integers(0, 65536, 7)]


def _weights(alpha):
    return float(alpha), float(F(1) - alpha)


def _samples(surface, w, h, px, dtype, cn):
    rows = surface._view(surface.host)[0]
    a = np.ascontiguousarray(rows[:h, :w * px]).view(dtype)
    return a if cn == 1 else a.reshape(h, w, cn)


# ---- 1. the operators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_blend_on_rois_against_the_numpy_statement(gpu, shape, sb, cn):
    """Source, history and destination are ROIs of larger random surfaces, each aligned by itself.  Every byte outside the padded
    destination plane keeps its prefill; source and history are untouched."""
    (w, h), (bx, by) = shape
    px, dtype = sb * cn, (np.uint8 if sb == 1 else np.uint16)
    dw, dh = w + 2 * bx, h + 2 * by
    top = 256 if sb == 1 else 65536
    for sides in (TRIPLES8 if sb == 1 else TRIPLES16):
        seed = roi.case_seed("yuvfade", shape, sb, cn, sides)
        fill = [int(v) for v in np.random.default_rng(seed).integers(1, top, 2)]
        src, hist = roi.Surface(sides[0], w, h, px, seed=seed).bind(gpu), roi.Surface(sides[1], dw, dh, px, seed=seed + 1).bind(gpu)
        dsts = []
        try:
            plane, hp = _samples(src, w, h, px, dtype, cn), _samples(hist, dw, dh, px, dtype, cn)
            for k, alpha in enumerate(ALPHAS):
                dst = roi.Surface(sides[2], dw, dh, px, seed=seed + 2 + k).bind(gpu)
                dsts.append(dst)
                gpu.fade_blend_jobs([(src.ptr, src.pitch, w, h, hist.ptr, hist.pitch, dst.ptr, dst.pitch, bx, by, cn, fill)], *_weights(alpha), sb)
            gpu.sync()
            for dst, alpha in zip(dsts, ALPHAS):
                got, clean = dst.result((dh, dw * cn), dtype)
                want = yf.blend_plane(plane, hp, bx, by, fill[0] if cn == 1 else fill, alpha, F(1) - alpha)
                assert np.array_equal(got, want.reshape(dh, dw * cn)), (sides, float(alpha))
                assert clean, dst.stray()
            assert src.untouched() and hist.untouched(), sides
        finally:
            src.free(); hist.free()
            for d in dsts:
                d.free()


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_update_on_rois_against_the_numpy_statement(gpu, shape, sb, cn):
    """History (updated in place) and result are ROIs of larger random surfaces, at the padded sizes of the blend's shapes - ragged
    rows at every alignment.  Every history byte outside the plane keeps its prefill; the result is untouched."""
    (w, h), (bx, by) = shape
    px, dtype = sb * cn, (np.uint8 if sb == 1 else np.uint16)
    dw, dh = w + 2 * bx, h + 2 * by
    for sides in (TRIPLES8 if sb == 1 else TRIPLES16):
        seed = roi.case_seed("yuvfade-update", shape, sb, cn, sides)
        hist, res = roi.Surface(sides[1], dw, dh, px, seed=seed).bind(gpu), roi.Surface(sides[2], dw, dh, px, seed=seed + 1).bind(gpu)
        try:
            want = yf.update_plane(_samples(hist, dw, dh, px, dtype, 1), _samples(res, dw, dh, px, dtype, 1))
            gpu.fade_update_jobs([(hist.ptr, hist.pitch, res.ptr, res.pitch, dw, dh, cn)], sb)
            gpu.sync()
            got, clean = hist.result((dh, dw * cn), dtype)
            assert np.array_equal(got, want), sides
            assert clean, hist.stray()
            assert res.untouched(), sides
        finally:
            hist.free(); res.free()


def _value_planes(sb):
    """(history, frame) planes that hold every pair of bytes, or every 16-bit history value against the 16 frame values of FRAME16."""
    if sb == 1:
        return np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    r, c = np.meshgrid(np.arange(256), np.arange(4096), indexing="ij")
    return ((r % 16) * 4096 + c).astype(np.uint16), np.asarray(FRAME16, np.uint16)[r // 16]


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_blend_value_coverage(gpu, sb):
    """All 256 x 256 (history, frame) pairs of bytes, all 65536 history words against 16 frame values; per alpha: 0, 0.5, 0.1f, every
    value of the 0.1 / 30 ramp, and 1 with beta 1 (saturation)."""
    hist, frame = _value_planes(sb)
    h, w = hist.shape
    dtype = hist.dtype
    weights = [_weights(a) for a in [F(0), F(0.5)] + [compref.fade_alpha(0.1, c, 30)[0] for c in range(1, 31)]] + [(1.0, 1.0), (1.0, 0.0)]
    d_h, d_f = capi.DevBuf.from_array(gpu, hist), capi.DevBuf.from_array(gpu, np.ascontiguousarray(frame))
    d_o = capi.DevBuf(gpu, len(weights) * hist.nbytes)
    try:
        for k, (al, be) in enumerate(weights):
            gpu.fade_blend_jobs([(d_f.ptr, w * sb, w, h, d_h.ptr, w * sb, d_o.ptr + k * hist.nbytes, w * sb, 0, 0, 1, (0, 0))], al, be, sb)
        gpu.sync()
        got = d_o.download((len(weights), h, w), dtype)
    finally:
        d_h.free(); d_f.free(); d_o.free()
    for k, (al, be) in enumerate(weights):
        assert np.array_equal(got[k], yf.blend_plane(frame, hist, 0, 0, 0, F(al), F(be))), (al, be)
    assert got[-2].max() == np.iinfo(dtype).max and np.array_equal(got[-1], hist)


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_update_value_coverage(gpu, sb):
    hist, res = _value_planes(sb)
    h, w = hist.shape
    d_h, d_r = capi.DevBuf.from_array(gpu, hist), capi.DevBuf.from_array(gpu, np.ascontiguousarray(res))
    try:
        gpu.fade_update_jobs([(d_h.ptr, w * sb, d_r.ptr, w * sb, w, h, 1)], sb)
        gpu.sync()
        got = d_h.download((h, w), hist.dtype)
    finally:
        d_h.free(); d_r.free()
    assert np.array_equal(got, yf.update_plane(hist, res))


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_32_mixed_jobs_in_one_launch_equal_the_jobs_one_by_one(gpu, sb):
    shapes = [((1, 1), (3, 3)), ((2, 3), (7, 7)), ((5, 4), (7, 7)), ((126, 92), (2, 2)), ((61, 30), (15, 30)), ((300, 9), (0, 4)), ((40, 40), (0, 0))]
    dtype = np.uint8 if sb == 1 else np.uint16
    top = 256 if sb == 1 else 65536
    rng = np.random.default_rng(32 + sb)
    al, be = _weights(RAMP7)
    jobs, so, ho, do = [], 0, 0, 0
    for i in range(32):
        (w, h), (bx, by) = shapes[i % len(shapes)]
        cn = 1 + (i // 2) % 2
        dw, dh = w + 2 * bx, h + 2 * by
        sp, hp = (w * cn + 3) * sb + (sb == 1) * (i % 2), ((dw * cn + 7) * sb if i % 3 else (dw * cn * sb + 15) // 16 * 16)
        dp = (dw * cn + 5) * sb if i % 4 else (dw * cn * sb + 15) // 16 * 16
        fill = [int(v) for v in rng.integers(1, top, 2)]
        do = (do + 15) // 16 * 16 if i % 4 == 0 else do              # (every fourth destination, every third history: 16-byte aligned with a 16-byte pitch)
        ho = (ho + 15) // 16 * 16 if i % 3 == 0 else ho
        jobs.append((so, sp, w, h, ho, hp, do, dp, bx, by, cn, fill))
        so += sp * h + 2 * (i % 5); ho += hp * dh + 2 * (i % 4); do += dp * dh + 2 * (i % 3)
    src, his, pre = rng.integers(0, 256, so, np.uint8), rng.integers(0, 256, ho, np.uint8), rng.integers(0, 256, do, np.uint8)
    d_src, d_his = capi.DevBuf.from_array(gpu, src), capi.DevBuf.from_array(gpu, his)
    d_one, d_all = capi.DevBuf.from_array(gpu, pre), capi.DevBuf.from_array(gpu, pre)
    d_h1, d_h2 = capi.DevBuf.from_array(gpu, his), capi.DevBuf.from_array(gpu, his)

    def view(flat, off, rows, row, pitch):
        return np.lib.stride_tricks.as_strided(flat[off:], (rows, row), (pitch, 1))
    try:
        gpu.fade_blend_jobs([(d_src.ptr + a, sp, w, h, d_his.ptr + c, hp, d_all.ptr + b, dp, bx, by, cn, fl) for a, sp, w, h, c, hp, b, dp, bx, by, cn, fl in jobs], al, be, sb)
        for a, sp, w, h, c, hp, b, dp, bx, by, cn, fl in jobs:
            gpu.fade_blend_jobs([(d_src.ptr + a, sp, w, h, d_his.ptr + c, hp, d_one.ptr + b, dp, bx, by, cn, fl)], al, be, sb)
        # the update: the blended planes into copies of the histories, at once and one by one
        gpu.fade_update_jobs([(d_h2.ptr + c, hp, d_all.ptr + b, dp, w + 2 * bx, h + 2 * by, cn) for a, sp, w, h, c, hp, b, dp, bx, by, cn, fl in jobs], sb)
        for a, sp, w, h, c, hp, b, dp, bx, by, cn, fl in jobs:
            gpu.fade_update_jobs([(d_h1.ptr + c, hp, d_one.ptr + b, dp, w + 2 * bx, h + 2 * by, cn)], sb)
        gpu.sync()
        one, al_ = d_one.download((do,), np.uint8), d_all.download((do,), np.uint8)
        h1, h2 = d_h1.download((ho,), np.uint8), d_h2.download((ho,), np.uint8)
        assert np.array_equal(one, al_) and np.array_equal(h1, h2)
        assert np.array_equal(d_src.download((so,), np.uint8), src) and np.array_equal(d_his.download((ho,), np.uint8), his)
        want, hwant = pre.copy(), his.copy()
        for a, sp, w, h, c, hp, b, dp, bx, by, cn, fl in jobs:
            dw, dh = w + 2 * bx, h + 2 * by
            plane = view(src, a, h, w * cn * sb, sp).copy().view(dtype)
            plane = plane if cn == 1 else plane.reshape(h, w, cn)
            hist = view(his, c, dh, dw * cn * sb, hp).copy().view(dtype)
            hist = hist if cn == 1 else hist.reshape(dh, dw, cn)
            blended = yf.blend_plane(plane, hist, bx, by, fl[0] if cn == 1 else fl, F(al), F(be))
            view(want, b, dh, dw * cn * sb, dp)[...] = np.ascontiguousarray(blended).reshape(dh, dw * cn).view(np.uint8)
            view(hwant, c, dh, dw * cn * sb, hp)[...] = np.ascontiguousarray(yf.update_plane(hist, blended)).reshape(dh, dw * cn).view(np.uint8)
        assert np.array_equal(al_, want) and np.array_equal(h2, hwant)
    finally:
        for d in (d_src, d_his, d_one, d_all, d_h1, d_h2):
            d.free()


def test_operator_refusals(gpu):
    """The tables of tests/plane_job_refusals.py on a real buffer: the accepted calls launch."""
    d = capi.DevBuf(gpu, pjr.REGION)
    d.zero()
    for make in (pjr.fade_blend, pjr.fade_update):
        op = make(d.ptr)
        pjr.check_accepted(gpu.lib, op, pjr.OK)
        pjr.check_refusals(gpu.lib, op)
    gpu.sync()
    d.free()


# ---- 2. streams ---------------------------------------------------------------------------------------------------------------
STREAM_FORMATS = ["NV12", "P010", "I420", "I010", "I422", "I210", "I444", "I412"]
N = 22
FAST = dict(fade_alpha=0.5, fade_duration=4)          # the history weighs in from the second output on and reaches full alpha
_chains = {}


def _split(f, frame, w, h):
    if f.uv:
        return [frame[:h], frame[h:].reshape(h // 2, w // 2, 2)]
    return list(pi.planes(frame, f.name, w, h))


def chain(oracle, world, name, w, h, n, b, fill, fade, state=(None, 0), clip_key=0, outs=None, **params):
    """One clip through the recurrence.  state: (history planes, count) carried in (None: a fresh stream); outs: the (out_index,
    matrix) of every result where they are not those of a fresh stream's run (clip_key names the case).  -> (per result: the
    surface - padded, blended, warped; the last one, which has no transform, is the input frame, unpadded -, the state behind the
    clip).  Computed once per case and left unchanged."""
    key = (name, w, h, n, b, tuple(fill), tuple(sorted(fade.items())), clip_key, tuple(sorted(params.items())))
    if key in _chains:
        return _chains[key]
    clip, run, _ = world
    f, frames = Fmt(name), clip(name, w, h)[:n]
    hist, count = state
    hist = None if hist is None else [p.copy() for p in hist]
    out = []
    for idx, M in (run(w, h, n, **params)[0] if outs is None else outs):
        if idx == n - 1:
            out.append(frames[idx])
            continue
        blended, hist, count, _ = yf.stream_step(hist, count, _split(f, frames[idx], w, h), f.sx, f.sy, b, fill, fade["fade_alpha"], fade["fade_duration"])
        Mc = pi.chroma_matrix(M, f.sx, f.sy)
        py, pu, pv = (blended[0], blended[1][..., 0], blended[1][..., 1]) if f.uv else blended
        wy, wu, wv = pi.warp_plane(oracle, py, M, pi.REPLICATE), pi.warp_plane(oracle, pu, Mc, pi.REPLICATE), pi.warp_plane(oracle, pv, Mc, pi.REPLICATE)
        res = [wy, np.stack([wu, wv], axis=-1)] if f.uv else [wy, wu, wv]
        hist = [yf.update_plane(hp, r) for hp, r in zip(hist, res)]
        out.append(np.vstack([wy, res[1].reshape(wu.shape[0], -1)]) if f.uv else synth.yuv_pack(wy, wu, wv, f.sx, f.sy))
    _chains[key] = out, (hist, count)
    return _chains[key]


def stream_run(gpu, f, frames, w, h, b, fill, params, batch=1, zero_copy=False, src=None, dst=None, dbg=None, clips=1, reset=False):
    """The clip through push_dev / flush_dev of a stream with border_size = b and borderType fade, `clips` times with vs_stab_clean in
    between (reset: and the setter called again); whole output allocations are read back (unpack asserts that nothing outside the
    planes was written).  -> per clip the results."""
    n = len(frames)
    pw, ph = w + 2 * b, h + 2 * b
    s = gpu.stabilizer(gpu.params(border_size=b, border_type=capi.BORDER_FADE, **params))
    src, dst = src or f.layout(w, h), dst or f.layout(pw, ph)
    d_in = capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in frames]))
    d_out = capi.DevBuf.from_array(gpu, dst.blank(n * clips))
    dims = []

    def dim():
        ow, oh = C.c_int32(), C.c_int32()
        gpu.check(gpu.lib.vs_stab_last_out_dims(s.h, C.byref(ow), C.byref(oh)), s.h)
        return ow.value, oh.value
    try:
        if batch > 1:
            s.set_batch(batch)
        s.set_zero_copy(zero_copy)
        s.set_yuv_fade(True, fill)
        f.set_layouts(s, src, dst)
        k = 0
        for c in range(clips):
            if c:
                s.clean()
                if reset:
                    s.set_yuv_fade(True, fill)
            for i in range(n):
                p = s.push_dev(d_in.ptr + i * src.size, w, h, src.pitch, f.fmt, d_out.ptr + k * dst.size, dst.pitch)
                if dbg is not None:
                    assert bool(p) == dbg[i]["has"], i
                    _check_debug(s.debug(), dbg[i], i)
                if p:
                    dims.append(dim())
                k += p
            s.sync()
            while s.flush_dev(d_out.ptr + k * dst.size, dst.pitch):
                dims.append(dim())
                k += 1
            s.sync()
        out = d_out.download((n * clips, dst.size // dst.sb), dst.dtype)
    finally:
        s.close(); d_in.free(); d_out.free()
    assert k == n * clips and dims == ([(pw, ph)] * (n - 1) + [(w, h)]) * clips, dims
    return [[dst.unpack(out[c * n + i]) for i in range(n - 1)] + [_unpack_last(f, dst, out[c * n + n - 1], w, h)] for c in range(clips)]


@pytest.mark.parametrize("size", [(130, 96, 8), (322, 200, 30)], ids=lambda s: "%dx%d+%d" % s)
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_stream_per_frame(gpu, oracle, world, name, size):
    """22 frames, flush included, through the device entry points with padded layouts and copy-in (whole allocations compared, the
    debug records those of the border_size = 0 run); at the small size also zero-copy with decoder-style layouts and the host entry
    points.  The large size has a chosen fill, the small one the default."""
    w, h, b = size
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:N]
    _, dbg = run(w, h, N, **params)
    fill = chosen_fill(f) if b == 30 else None
    want, _ = chain(oracle, world, name, w, h, N, b, fill or default_fill(f), FAST, **params)
    src, dst = _padded(f, w, h, b)
    got, = stream_run(gpu, f, frames, w, h, b, fill, dict(params, **FAST), src=src, dst=dst, dbg=dbg)
    _same(got, want, (name, b))
    assert np.array_equal(got[-1], frames[-1])
    if b == 30:
        return
    src, dst = _decoder_layouts(f, w, h, b)
    got, = stream_run(gpu, f, frames, w, h, b, fill, dict(params, **FAST), zero_copy=True, src=src, dst=dst)
    _same(got, want, (name, "zero-copy"))
    # the host entry points
    pw = w + 2 * b
    s = gpu.stabilizer(gpu.params(border_size=b, border_type=capi.BORDER_FADE, **params, **FAST))
    s.set_yuv_fade(True, fill)
    got = []
    for k, x in enumerate(frames):
        o = s.push(x, f.fmt)
        _check_debug(s.debug(), dbg[k], k)
        if o is not None:
            got.append(o)
    while True:
        o = s.flush(frames[0], f.fmt)
        if o is None:
            break
        got.append(o)
    ow, oh = C.c_int32(), C.c_int32()
    gpu.check(gpu.lib.vs_stab_last_out_dims(s.h, C.byref(ow), C.byref(oh)), s.h)
    assert (ow.value, oh.value) == (w, h)
    s.close()
    _same(got[:-1], want[:-1], (name, "host"))
    # the last frame: unpadded in the caller's padded buffer, the default offsets of w x h at the buffer's pitch, zeros (np.zeros) elsewhere
    flat = got[-1].reshape(-1)
    host = f.layout(w, h, pitch=pw * flat.itemsize)
    hole = host.pack(np.zeros_like(frames[-1])) == host.canary
    held = np.where(hole, 0, host.pack(frames[-1]))
    assert np.array_equal(flat[:held.size], held) and not flat[held.size:].any()


def test_stream_with_the_default_fade_parameters(gpu, oracle, world):
    """fade_alpha 0.1, fade_duration 30: the ramp never ends within the clip."""
    name, w, h, b = "I010", 130, 96, 8
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    want, (_, count) = chain(oracle, world, name, w, h, N, b, default_fill(f), dict(fade_alpha=0.1, fade_duration=30), **params)
    got, = stream_run(gpu, f, clip(name, w, h)[:N], w, h, b, None, params)
    assert count == N - 1
    _same(got, want, name)


# ---- 3. stream state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_batch_mode_runs_per_frame_and_gives_the_same_bytes(gpu, oracle, world, name):
    w, h, b = 130, 96, 8
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:N]
    src, dst = _decoder_layouts(f, w, h, b)
    got, = stream_run(gpu, f, frames, w, h, b, None, dict(params, **FAST), batch=8, zero_copy=True, src=src, dst=dst)
    _same(got, chain(oracle, world, name, w, h, N, b, default_fill(f), FAST, **params)[0], name)


_second = {}


def _second_clip_outs(oracle, nv12, **params):
    """(out_index, matrix) of every result of the clip's SECOND pass through one oracle instance, clean() in between (the analysis of
    a cleaned instance is not a fresh one's: Stabilizer::clean() keeps the detection cadence)."""
    key = (len(nv12), nv12[0].shape, tuple(sorted(params.items())))
    if key not in _second:
        so = oracle.stabilizer(oracle.params(**params))
        for c in range(2):
            outs = []
            if c:
                so.clean()
            for x in nv12:
                if so.push(x, capi.FMT_NV12) is not None:
                    outs.append((so.debug().out_index, np.array(so.debug().warp_matrix, np.float32)))
            while so.flush(nv12[0], capi.FMT_NV12) is not None:
                outs.append((so.debug().out_index, np.array(so.debug().warp_matrix, np.float32)))
        so.close()
        _second[key] = outs
    return _second[key]


@pytest.mark.parametrize("name", ["NV12", "I010"])
def test_clean_keeps_the_history_and_the_setter_drops_it(gpu, oracle, world, name):
    """Two passes of the clip with vs_stab_clean in between: the second pass's outputs are the recurrence carried over (history and
    count), not those of a fresh history; with the setter called again in between they are those of a fresh history."""
    w, h, b = 130, 96, 8
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:N]
    fill = chosen_fill(f)
    outs = _second_clip_outs(oracle, clip("NV12", w, h)[:N], **params)
    first, state = chain(oracle, world, name, w, h, N, b, fill, FAST, **params)
    second, _ = chain(oracle, world, name, w, h, N, b, fill, FAST, state=state, clip_key="second pass, history kept", outs=outs, **params)
    fresh, _ = chain(oracle, world, name, w, h, N, b, fill, FAST, clip_key="second pass, fresh history", outs=outs, **params)
    assert state[1] == 4 and not np.array_equal(fresh[0], second[0])
    got = stream_run(gpu, f, frames, w, h, b, fill, dict(params, **FAST), clips=2)
    _same(got[0], first, (name, "first pass"))
    _same(got[1], second, (name, "second pass"))
    got = stream_run(gpu, f, frames, w, h, b, fill, dict(params, **FAST), clips=2, reset=True)
    _same(got[0], first, (name, "first pass"))
    _same(got[1], fresh, (name, "second pass after the setter"))


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def _first_push(gpu, name, params, fade=None, pad=None, w=64, h=48, batch=1, fill=None, out_pitch=None):
    """fade / pad: None = the setter is never called."""
    f = Fmt(name)
    sb = 1 if f.nbits == 8 else 2
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **params))
    s.set_batch(batch)
    if fade is not None:
        s.set_yuv_fade(fade, fill)
    if pad is not None:
        s.set_yuv_border_pad(pad)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    b = params.get("border_size", 0) if not params.get("crop_n_zoom") else 0
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr), w, h, w * sb, f.fmt, C.c_void_p(d_out.ptr), out_pitch or (w + 2 * b) * sb, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


FADE = dict(border_size=8, border_type=capi.BORDER_FADE)
TEXTS = dict(NV12="NV12", P010="P010", I420="I420", I010="I010 / I012", I422="I422", I210="I210", I444="I444", I412="I412")


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_mode_off_the_fade_is_refused_as_ever(gpu, name, batch):
    """The mode never touched: code and text are those every build before the mode gave."""
    want = "border/crop modes need a colour format (BGR8, BGRA8, RGBA8, RGB8)"
    if name != "NV12":
        want = "border/crop/fade modes need a colour format (BGR8, BGRA8, RGBA8, RGB8), not " + TEXTS[name]
    assert _first_push(gpu, name, FADE, batch=batch) == (UNSUPPORTED, want)
    assert _first_push(gpu, name, dict(border_size=5, border_type=capi.BORDER_FADE), batch=batch) == (UNSUPPORTED, want)


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_refusals_through_the_stream(gpu, name, batch):
    f = Fmt(name)
    never = _first_push(gpu, name, FADE, batch=batch)
    assert _first_push(gpu, name, FADE, fade=False, batch=batch) == never and never[0] == UNSUPPORTED
    assert _first_push(gpu, name, FADE, fade=True, batch=batch)[0] == 0
    odd = _first_push(gpu, name, dict(border_size=5, border_type=capi.BORDER_FADE), fade=True, batch=batch)
    if f.sx or f.sy:
        assert odd[0] == INVALID and name in odd[1] and "fade on" in odd[1] and "even border_size" in odd[1]
    else:
        assert odd[0] == 0
    big = _first_push(gpu, name, FADE, fade=True, batch=batch, fill=(0, 256, 0))
    if f.nbits == 8:
        assert big[0] == INVALID and "above 255" in big[1] and name in big[1] and "vs_stab_set_yuv_fade" in big[1]
    else:
        assert big[0] == 0
    sb = 1 if f.nbits == 8 else 2
    small = _first_push(gpu, name, FADE, fade=True, batch=batch, out_pitch=(64 + 14) * sb)             # holds a frame's row, not a padded one
    assert small[0] == INVALID and "padded row" in small[1]
    # only the border-pad switch on: the fade is refused as ever; only the fade switch on: so is a pad; crop-and-zoom likewise
    assert _first_push(gpu, name, FADE, pad=True, batch=batch) == never
    pad = dict(border_size=8, border_type=yp.REFLECT)
    assert _first_push(gpu, name, pad, fade=True, batch=batch) == _first_push(gpu, name, pad, batch=batch) and _first_push(gpu, name, pad, fade=True, batch=batch)[0] == UNSUPPORTED
    assert _first_push(gpu, name, pad, fade=True, pad=True, batch=batch)[0] == 0 and _first_push(gpu, name, FADE, fade=True, pad=True, batch=batch)[0] == 0
    crop = dict(border_size=8, crop_n_zoom=1, border_type=capi.BORDER_FADE)
    assert _first_push(gpu, name, crop, fade=True, batch=batch) == _first_push(gpu, name, crop, batch=batch)
    # the canvas
    on, off = (_first_push(gpu, name, dict(enable_virtual_canvas=1), fade=m, batch=batch) for m in (True, None))
    assert on == off and on[0] == UNSUPPORTED and "enableVirtualCanvas" in on[1]
    both = _first_push(gpu, name, dict(enable_virtual_canvas=1, **FADE), fade=True, batch=batch)
    assert both[0] == UNSUPPORTED and "enableVirtualCanvas" in both[1]


def test_a_fill_above_255_is_refused_by_the_setter_once_the_format_is_known(gpu):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **FADE))
    s.set_zero_copy(True)
    s.set_yuv_fade(True, (300, 0, 0))                     # no format yet: accepted, refused by the push
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    with pytest.raises(capi.VsError, match="above 255 on NV12"):
        s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 80)
    s.set_yuv_fade(True, (30, 0, 0))
    assert s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 80) == 0
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_fade: the frame queue must be empty"):
        s.set_yuv_fade(False)
    s.sync()
    while s.flush_dev(d_out.ptr, 80):
        pass
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_fade: a fill sample above 255 on NV12"):
        s.set_yuv_fade(True, (0, 0, 256))
    with pytest.raises(capi.VsError, match="reserved"):
        gpu.check(gpu.lib.vs_stab_set_yuv_fade(s.h, 1, C.byref(capi.VsYuvFill(1, 2, 3, 4))), s.h)
    s.set_yuv_fade(True, (0, 0, 255))
    s.close(); d_in.free(); d_out.free()


@pytest.mark.parametrize("batch", [1, 8])
def test_setter_with_frames_queued_is_refused(gpu, batch):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **FADE))
    s.set_batch(batch)
    s.set_zero_copy(True)
    s.set_yuv_fade(True)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    assert s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 80) == 0
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_fade: the frame queue must be empty"):
        s.set_yuv_fade(False)
    s.sync()
    s.close(); d_in.free(); d_out.free()


def test_vs_batch_create_still_refuses_the_fade(gpu):
    with pytest.raises(capi.VsError, match="fade border"):
        gpu.batch(gpu.params(smoothing_radius=5, **FADE), 2, 4)
    assert not hasattr(gpu.lib, "vs_batch_set_yuv_fade")
