"""Border pad on YUV streams on the device, bit for bit: vs_op_pad_jobs against tests/yuvpadref.py, and streams with
vs_stab_set_yuv_border_pad - per frame, in batch mode and in a vs_batch group - against surfaces built without the code under test:
the oracle's NV12 run with border_size = 0 gives out_index and matrix of every result, yuvpadref pads every plane of the input, and
every padded plane is warped under BORDER_REPLICATE by the oracle's double-precision warp (8-bit) or i010_inputs.warp_plane (16-bit)
with the format's chroma matrix.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import planar_inputs as pi
import plane_job_refusals as pjr
import roi
import yuvpadref as yp
from test_gpu_planar import _check_debug, _oracle_nv12_run, bits
from test_gpu_yuv_cropzoom import Fmt, UVLayout, _same, world  # noqa: F401  (world: the module's clips and oracle runs)
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
NAMES = {yp.BLACK: "black", yp.REFLECT: "reflect", yp.REFLECT_101: "reflect101", yp.REPLICATE: "replicate", yp.WRAP: "wrap"}
# (w, h), (bx, by): planes smaller than their border, the streams' planes, several tiles across and down (128 bytes x 256 rows of bytes, 256 x 128 of words), unequal borders
SHAPES = [((1, 1), (3, 3)), ((2, 3), (7, 7)), ((5, 4), (7, 7)), ((126, 92), (2, 2)), ((322, 200), (30, 30)), ((704, 400), (6, 6)), ((64, 48), (15, 30))]
SHAPE_IDS = ["%dx%d+%dx%d" % (s + b) for s, b in SHAPES]


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------
def _samples(surface, w, h, px, dtype, cn):
    rows = surface._view(surface.host)[0]
    a = np.ascontiguousarray(rows[:h, :w * px]).view(dtype)
    return a if cn == 1 else a.reshape(h, w, cn)


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_operator_on_rois_against_the_numpy_statement(gpu, shape, sb, cn):
    """Sources and destinations are ROIs of larger random surfaces, with odd and padded pitches at every base alignment the sample
    size allows, for all five modes.  Every byte outside the padded plane keeps its prefill, the sources are untouched."""
    (w, h), (bx, by) = shape
    px, dtype = sb * cn, (np.uint8 if sb == 1 else np.uint16)
    dw, dh = w + 2 * bx, h + 2 * by
    layouts = roi.LAYOUT_NAMES if sb == 1 else ["packed", "padded16", "roi_off2", "tight_end"]       # (16-bit: even addresses and pitches)
    top = 256 if sb == 1 else 65536
    for layout in layouts:
        for mode in yp.MODES:
            seed = roi.case_seed("yuvpad", shape, sb, cn, layout, mode)
            fill = [int(v) for v in np.random.default_rng(seed).integers(1, top, 2)]
            src, dst = roi.pair(layout, seed, (w, h, px), (dw, dh, px))
            src.bind(gpu); dst.bind(gpu)
            try:
                plane = _samples(src, w, h, px, dtype, cn)
                gpu.pad_jobs([(src.ptr, src.pitch, w, h, dst.ptr, dst.pitch, bx, by, cn, mode, fill)], sb)
                gpu.sync()
                got, clean = dst.result((dh, dw * cn), dtype)
                want = yp.pad_plane(plane, bx, by, mode, fill[0] if cn == 1 else fill)
                assert np.array_equal(got, want.reshape(dh, dw * cn)), (layout, NAMES[mode])
                assert clean, dst.stray()
                assert src.untouched(), layout
            finally:
                src.free(); dst.free()


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_operator_96_mixed_jobs_in_one_launch_equal_the_jobs_one_by_one(gpu, sb):
    shapes = [((1, 1), (3, 3)), ((2, 3), (7, 7)), ((5, 4), (7, 7)), ((126, 92), (2, 2)), ((61, 30), (15, 30)), ((300, 9), (0, 4)), ((40, 40), (0, 0))]
    dtype = np.uint8 if sb == 1 else np.uint16
    top = 256 if sb == 1 else 65536
    rng = np.random.default_rng(96 + sb)
    jobs, so, do = [], 0, 0
    for i in range(96):
        (w, h), (bx, by) = shapes[i % len(shapes)]
        cn = 1 + (i // 2) % 2
        dw, dh = w + 2 * bx, h + 2 * by
        sp, dp = (w * cn + 3) * sb + (sb == 1) * (i % 2), ((dw * cn + 5) * sb if i % 4 else (dw * cn * sb + 15) // 16 * 16)
        fill = [int(v) for v in rng.integers(1, top, 2)]
        do = (do + 15) // 16 * 16 if i % 4 == 0 else do              # (every fourth destination 16-byte aligned with a 16-byte pitch)
        jobs.append((so, sp, w, h, do, dp, bx, by, cn, i % 5, fill))
        so += sp * h + 2 * (i % 5); do += dp * dh + 2 * (i % 3)
    src = rng.integers(0, 256, so, np.uint8)
    pre = rng.integers(0, 256, do, np.uint8)
    d_src, d_one, d_all = capi.DevBuf.from_array(gpu, src), capi.DevBuf.from_array(gpu, pre), capi.DevBuf.from_array(gpu, pre)
    try:
        gpu.pad_jobs([(d_src.ptr + a, sp, w, h, d_all.ptr + b, dp, bx, by, cn, m, fl) for a, sp, w, h, b, dp, bx, by, cn, m, fl in jobs], sb)
        for a, sp, w, h, b, dp, bx, by, cn, m, fl in jobs:
            gpu.pad_jobs([(d_src.ptr + a, sp, w, h, d_one.ptr + b, dp, bx, by, cn, m, fl)], sb)
        gpu.sync()
        one, al = d_one.download((do,), np.uint8), d_all.download((do,), np.uint8)
        assert np.array_equal(one, al)
        assert np.array_equal(d_src.download((so,), np.uint8), src)
        want = pre.copy()
        for a, sp, w, h, b, dp, bx, by, cn, m, fl in jobs:
            plane = np.lib.stride_tricks.as_strided(src[a:], (h, w * cn * sb), (sp, 1)).copy().view(dtype)
            plane = plane if cn == 1 else plane.reshape(h, w, cn)
            padded = yp.pad_plane(plane, bx, by, m, fl[0] if cn == 1 else fl)
            dw, dh = w + 2 * bx, h + 2 * by
            np.lib.stride_tricks.as_strided(want[b:], (dh, dw * cn * sb), (dp, 1))[...] = np.ascontiguousarray(padded).reshape(dh, dw * cn).view(np.uint8)
        assert np.array_equal(al, want)
    finally:
        d_src.free(); d_one.free(); d_all.free()


def test_operator_refusals(gpu):
    """The tables of tests/plane_job_refusals.py on a real buffer: the accepted calls launch."""
    d = capi.DevBuf(gpu, pjr.REGION)
    d.zero()
    for make in (pjr.pad,):
        op = make(d.ptr)
        pjr.check_accepted(gpu.lib, op, pjr.OK)
        pjr.check_refusals(gpu.lib, op)
    gpu.sync()
    d.free()


# ---- 2. streams ---------------------------------------------------------------------------------------------------------------
STREAM_FORMATS = ["NV12", "P010", "I420", "I010", "I422", "I210", "I444", "I412"]
N = 22
_expected = {}


def chosen_fill(f):
    """A colour of the caller's, as the samples lie in memory."""
    return (81, 90, 240) if f.nbits == 8 else (0x2340, 0x8100, 0x7fc0) if f.name == "P010" else (0x0123, 0x0234, 0x0345)


def default_fill(f):
    return yp.video_black(f.nbits, f.name == "P010")


def pad_warp(oracle, f, frame, w, h, b, mode, fill, M):
    """The expected result of one frame: every plane padded (yuvpadref) and warped under BORDER_REPLICATE, Y under M, chroma under
    the format's chroma matrix."""
    if f.uv:
        uv = frame[h:].reshape(h // 2, w // 2, 2)
        y, u, v = frame[:h], uv[..., 0], uv[..., 1]
    else:
        y, u, v = pi.planes(frame, f.name, w, h)
    py, pu, pv = yp.pad_surface([y, u, v], f.sx, f.sy, b, mode, fill)
    Mc = pi.chroma_matrix(M, f.sx, f.sy)
    wy, wu, wv = pi.warp_plane(oracle, py, M, pi.REPLICATE), pi.warp_plane(oracle, pu, Mc, pi.REPLICATE), pi.warp_plane(oracle, pv, Mc, pi.REPLICATE)
    if f.uv:
        return np.vstack([wy, np.stack([wu, wv], axis=-1).reshape(wu.shape[0], -1)])
    return synth.yuv_pack(wy, wu, wv, f.sx, f.sy)


def expected(oracle, world, name, w, h, n, b, mode, fill, **params):
    """Per result: the padded, warped surface; the last one (no transform) is the input frame, unpadded.  Computed once per case."""
    key = (name, w, h, n, b, mode, tuple(fill), tuple(sorted(params.items())))
    if key not in _expected:
        clip, run, _ = world
        f, frames = Fmt(name), clip(name, w, h)
        _expected[key] = [frames[idx] if idx == n - 1 else pad_warp(oracle, f, frames[idx], w, h, b, mode, fill, M) for idx, M in run(w, h, n, **params)[0]]
    return _expected[key]


def _padded(f, w, h, b):
    """Distinct input (w x h) and output (padded size) layouts with padding everywhere."""
    sb = 1 if f.nbits == 8 else 2
    pw, ph = w + 2 * b, h + 2 * b
    if f.uv:
        return f.layout(w, h, pitch=(w + 30) * sb, uv_off=(w + 30) * sb * (h + 6)), f.layout(pw, ph, pitch=(pw + 62) * sb, uv_off=(pw + 62) * sb * (ph + 2))
    return f.layout(w, h, pitch=(w + 62) * sb, c_pitch=((w >> f.sx) + 40) * sb), f.layout(pw, ph, pitch=(pw + 14) * sb, c_pitch=(pw + 14) * sb)


def _decoder_layouts(f, w, h, b):
    """Distinct layouts: a decoder-style uv_offset (NV12 / P010); V before U in, a chroma pitch of its own out."""
    sb = 1 if f.nbits == 8 else 2
    pw, ph = w + 2 * b, h + 2 * b
    if f.uv:
        return f.layout(w, h, pitch=256 * sb, uv_off=256 * sb * (h + 8)), f.layout(pw, ph, pitch=192 * sb, uv_off=192 * sb * (ph + 16))
    ch = h >> f.sy
    return (f.layout(w, h, pitch=512, c_pitch=384, u_off=512 * (h + 8) + 384 * (ch + 4), v_off=512 * (h + 8), size=512 * (h + 8) + 384 * (2 * ch + 8)),
            f.layout(pw, ph, pitch=(pw + 14) * sb, c_pitch=(pw + 30) * sb))


def _unpack_last(f, dst, raw, w, h):
    """The last frame of a flush inside an output allocation of layout `dst`: w x h with the default offsets of that size at
    dst.pitch, and nothing else written."""
    if f.uv:
        own = UVLayout(f.name, w, h, pitch=dst.pitch)
        raw = np.asarray(raw).reshape(-1)
        assert np.all(raw[own.size // own.sb:] == own.canary), "samples behind the unpadded frame were written"
        return own.unpack(raw[:own.size // own.sb])
    return pi.Layout(f.name, w, h, pitch=dst.pitch, size=dst.size).unpack(raw)


def stream_run(gpu, f, frames, w, h, b, mode, fill, params, batch=1, zero_copy=False, src=None, dst=None, dbg=None):
    """The clip through push_dev / flush_dev of a stream with border_size = b and border_type = mode; whole output allocations are
    read back (unpack asserts that nothing outside the planes was written).  fill: None = the default.  dbg: the oracle's records,
    checked at every push (per frame).  -> the results, the last debug record, the reported size of every result."""
    n = len(frames)
    pw, ph = w + 2 * b, h + 2 * b
    s = gpu.stabilizer(gpu.params(border_size=b, border_type=mode, **params))
    src, dst = src or f.layout(w, h), dst or f.layout(pw, ph)
    d_in, d_out = capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in frames])), capi.DevBuf.from_array(gpu, dst.blank(n))
    dims = []

    def dim():
        ow, oh = C.c_int32(), C.c_int32()
        gpu.check(gpu.lib.vs_stab_last_out_dims(s.h, C.byref(ow), C.byref(oh)), s.h)
        return ow.value, oh.value
    try:
        if batch > 1:
            s.set_batch(batch)
        s.set_zero_copy(zero_copy)
        s.set_yuv_border_pad(True, fill)
        f.set_layouts(s, src, dst)
        k = 0
        for i in range(n):
            p = s.push_dev(d_in.ptr + i * src.size, w, h, src.pitch, f.fmt, d_out.ptr + k * dst.size, dst.pitch)
            if dbg is not None:
                assert bool(p) == dbg[i]["has"], i
                _check_debug(s.debug(), dbg[i], i)
            if p:
                dims.append(dim())
            k += p
        s.sync()
        last = s.debug()
        last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
        while s.flush_dev(d_out.ptr + k * dst.size, dst.pitch):
            dims.append(dim())
            k += 1
        s.sync()
        out = d_out.download((n, dst.size // dst.sb), dst.dtype)
    finally:
        s.close(); d_in.free(); d_out.free()
    assert k == n and dims == [(pw, ph)] * (n - 1) + [(w, h)], dims
    return [dst.unpack(out[i]) for i in range(n - 1)] + [_unpack_last(f, dst, out[n - 1], w, h)], last


@pytest.mark.parametrize("size", [(130, 96), (322, 200)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_stream_per_frame(gpu, oracle, world, name, size):
    """Frame by frame through the device entry points (padded layouts, whole allocations compared) for every border, the default and
    a chosen fill, and once through the host entry points; the debug records are those of the border_size = 0 run, the last flushed
    frame is the input frame at w x h."""
    w, h = size
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:14]
    _, dbg = run(w, h, 14, **params)
    cases = [(2, yp.BLACK, None), (6, yp.REFLECT_101, None), (30, yp.BLACK, chosen_fill(f))] + ([(5, yp.WRAP, None)] if (f.sx, f.sy) == (0, 0) else [])
    for b, mode, fill in cases:
        want = expected(oracle, world, name, w, h, 14, b, mode, fill or default_fill(f), **params)
        src, dst = _padded(f, w, h, b)
        got, _ = stream_run(gpu, f, frames, w, h, b, mode, fill, params, src=src, dst=dst, dbg=dbg)
        _same(got, want, (name, b))
        assert np.array_equal(got[-1], frames[-1])
    # the host entry points
    b, mode, fill = cases[2]
    pw, ph = w + 2 * b, h + 2 * b
    want = expected(oracle, world, name, w, h, 14, b, mode, fill, **params)
    s = gpu.stabilizer(gpu.params(border_size=b, border_type=mode, **params))
    s.set_yuv_border_pad(True, fill)
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


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("batch", [8, 40])
@pytest.mark.parametrize("name", ["NV12", "P010", "I420", "I210", "I444"])
def test_stream_batch_mode_equals_the_per_frame_path(gpu, oracle, world, name, batch, zero_copy):
    """22 frames in batches of 8 (two whole steps and one of six) and of 40 (one partial step), decoder-style layouts that differ
    between input and output (YV12 order in): the results equal the per-frame path's and the expected surfaces."""
    w, h, b, mode = 130, 96, 6, yp.REFLECT
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:N]
    src, dst = _decoder_layouts(f, w, h, b)
    per_frame, last1 = stream_run(gpu, f, frames, w, h, b, mode, None, params, 1, zero_copy, src, dst)
    got, last = stream_run(gpu, f, frames, w, h, b, mode, None, params, batch, zero_copy, src, dst)
    _same(got, per_frame, (name, "batch vs per frame"))
    _same(got, expected(oracle, world, name, w, h, N, b, mode, default_fill(f), **params), name)
    for key in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(last[key]), bits(last1[key])) and np.array_equal(bits(last[key]), bits(run(w, h, N, **params)[1][-1][key])), key


@pytest.mark.parametrize("name", ["NV12", "I420"])
def test_stream_batch_of_32_with_several_tiles_in_every_plane(gpu, oracle, name):
    """704 x 400, batch 32: one pad launch of 64 / 96 jobs in front of one warp launch of 32 surfaces; every plane has several tiles
    across and down."""
    w, h, b, n, mode = 704, 400, 30, 40, yp.BLACK
    f, params = Fmt(name), dict(smoothing_radius=5)
    bgr = synth.make_clip(synth.SEED_CONFIG3 + 34, w, h, n)
    nv12 = [synth.bgr_to_nv12(x) for x in bgr]
    frames = f.frames(bgr, nv12)
    got, _ = stream_run(gpu, f, frames, w, h, b, mode, chosen_fill(f), params, 32, True)
    per_frame, _ = stream_run(gpu, f, frames, w, h, b, mode, chosen_fill(f), params, 1, True)
    _same(got, per_frame, name)
    ref, _ = _oracle_nv12_run(oracle, nv12, **params)
    assert len(got) == len(ref) == n
    for k, (idx, M) in enumerate(ref):
        if k % 4 == 0 or idx == n - 1:          # (every result equals the per-frame path's; every fourth is rebuilt from the oracle)
            want = frames[idx] if idx == n - 1 else pad_warp(oracle, f, frames[idx], w, h, b, mode, chosen_fill(f), M)
            assert np.array_equal(got[k], want), (name, k)


@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_vs_batch_of_three_streams_against_standalone_instances(gpu, oracle, world, name):
    w, h, b, n, S, mode = 130, 96, 6, N, 3, yp.REFLECT
    pw, ph = w + 2 * b, h + 2 * b
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:n]
    src, dst = _decoder_layouts(f, w, h, b)
    # another picture per stream, the same layout: every frame rolled along its rows by an even number of samples
    cl = [[np.roll(x, 4 * g, axis=1) for x in frames] for g in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in c])) for c in cl]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    g = gpu.batch(gpu.params(border_size=b, border_type=mode, **params), S, 8)
    try:
        g.set_zero_copy(True)
        g.set_yuv_border_pad(True)
        f.set_layouts(g, src, dst)
        with pytest.raises(capi.VsError, match="belongs to a vs_batch"):
            g.stream(0).set_yuv_border_pad(False)
        k = [0] * S
        for i in range(n):
            prod = g.push_dev([d_in[j].ptr + i * src.size for j in range(S)], w, h, src.pitch, f.fmt, [d_out[j].ptr + k[j] * dst.size for j in range(S)], dst.pitch)
            k = [k[j] + prod[j] for j in range(S)]
        while True:
            prod = g.flush_dev([d_out[j].ptr + k[j] * dst.size for j in range(S)], dst.pitch)
            k = [k[j] + prod[j] for j in range(S)]
            if not any(prod):
                break
        g.sync()
    finally:
        g.close()
    assert k == [n] * S
    for j in range(S):
        raw = d_out[j].download((n, dst.size // dst.sb), dst.dtype)
        got = [dst.unpack(raw[i]) for i in range(n - 1)] + [_unpack_last(f, dst, raw[n - 1], w, h)]
        alone, _ = stream_run(gpu, f, cl[j], w, h, b, mode, None, params, 8, True, src, dst)
        _same(got, alone, (name, j))
        if j == 0:                                           # (stream 0 has the clip itself)
            _same(got, expected(oracle, world, name, w, h, n, b, mode, default_fill(f), **params), name)
    for d in d_in + d_out:
        d.free()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def _first_push(gpu, name, params, mode, w=64, h=48, batch=1, fill=None, out_pitch=None):
    f = Fmt(name)
    sb = 1 if f.nbits == 8 else 2
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **params))
    s.set_batch(batch)
    s.set_yuv_border_pad(mode, fill)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    b = params.get("border_size", 0) if mode and not params.get("crop_n_zoom") else 0
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr), w, h, w * sb, f.fmt, C.c_void_p(d_out.ptr), out_pitch or (w + 2 * b) * sb, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_refusals_through_the_stream(gpu, name, batch):
    f = Fmt(name)
    pad = dict(border_size=8, border_type=yp.REFLECT)
    off = _first_push(gpu, name, pad, False, batch=batch)
    assert off[0] == UNSUPPORTED and "modes need a colour format" in off[1]                    # mode off: today's refusal and text
    assert _first_push(gpu, name, pad, True, batch=batch)[0] == 0
    odd = _first_push(gpu, name, dict(border_size=5), True, batch=batch)
    if f.sx or f.sy:
        assert odd[0] == INVALID and name in odd[1] and "even border_size" in odd[1]
    else:
        assert odd[0] == 0
    big = _first_push(gpu, name, pad, True, batch=batch, fill=(256, 0, 0))
    if f.nbits == 8:
        assert big[0] == INVALID and "above 255" in big[1] and name in big[1]
    else:
        assert big[0] == 0
    sb = 1 if f.nbits == 8 else 2
    small = _first_push(gpu, name, pad, True, batch=batch, out_pitch=(64 + 14) * sb)            # holds a frame's row, not a padded one
    assert small[0] == INVALID and "padded row" in small[1]
    for params in (dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE)):   # crop-and-zoom, fade: as with the mode off
        assert _first_push(gpu, name, params, True, batch=batch) == _first_push(gpu, name, params, False, batch=batch)
        assert _first_push(gpu, name, params, True, batch=batch)[0] == UNSUPPORTED
    on, offc = (_first_push(gpu, name, dict(enable_virtual_canvas=1), m, batch=batch) for m in (True, False))
    assert on == offc and on[0] == UNSUPPORTED and "enableVirtualCanvas" in on[1]
    padcanvas = _first_push(gpu, name, dict(enable_virtual_canvas=1, **pad), True, batch=batch)
    assert padcanvas[0] == UNSUPPORTED and "enableVirtualCanvas" in padcanvas[1]


@pytest.mark.parametrize("batch", [1, 8])
def test_setter_with_frames_queued_is_refused(gpu, batch):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, border_size=8))
    s.set_batch(batch)
    s.set_zero_copy(True)
    s.set_yuv_border_pad(True)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    assert s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 80) == 0
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_border_pad: the frame queue must be empty"):
        s.set_yuv_border_pad(False)
    s.sync()
    s.close(); d_in.free(); d_out.free()


def test_vs_batch_refuses_members_that_disagree(gpu):
    """A step refuses group members that differ in border_size (as ever) or in the fill colour their pad launch would write - one
    launch pads the planes of all members with ONE colour.  The setter reaches all members through the group; a member with a frame
    queued refuses the change and the group reports it, which is how members come to hold different colours.  The same sequence with
    equal colours is accepted, and a member that is left with the mode off is refused by its own push."""
    w, h = 64, 48
    A, B = (30, 100, 200), (31, 100, 200)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()

    def push_both(g, n=8):
        for _ in range(n):
            g.push_dev([d_in.ptr, d_in.ptr], w, h, w, capi.FMT_NV12, [d_out.ptr, d_out.ptr + (1 << 19)], w + 16)

    def group_with_member_1_queued(first, second):
        """Both members get `first`; member 1 queues a frame; the setter comes again with `second`: member 0 takes it, member 1 refuses."""
        g = gpu.batch(gpu.params(smoothing_radius=5, border_size=8), 2, 4)
        g.set_zero_copy(True)
        g.set_yuv_border_pad(*first)
        assert g.push_dev([None, d_in.ptr], w, h, w, capi.FMT_NV12, [None, d_out.ptr + (1 << 19)], w + 16) == [0, 0]
        with pytest.raises(capi.VsError, match="queue must be empty"):
            g.set_yuv_border_pad(*second)
        return g
    # border_size
    p = [gpu.params(smoothing_radius=5, border_size=8), gpu.params(smoothing_radius=5, border_size=6)]
    g = gpu.batch(p, 2, 4)
    g.set_zero_copy(True)
    g.set_yuv_border_pad(True)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        push_both(g)
    g.close()
    # the fill colour: a chosen one against another, and a chosen one against the default
    for first, second in (((True, A), (True, B)), ((True, A), (True, None)), ((True, None), (True, B))):
        g = group_with_member_1_queued(first, second)
        with pytest.raises(capi.VsError, match="share one frame geometry"):
            push_both(g)
        g.close()
    # equal colours - the same one again, and video black spelled out against the default: every step runs
    for first, second in (((True, A), (True, A)), ((True, None), (True, yp.video_black(8)))):
        g = group_with_member_1_queued(first, second)
        push_both(g)
        g.sync()
        g.close()
    # the mode itself: member 0 is switched off and member 1 is not; member 0's push is then refused as a stream without the mode is
    g = group_with_member_1_queued((True, A), (False, None))
    with pytest.raises(capi.VsError, match="modes need a colour format"):
        push_both(g)
    g.close(); d_in.free(); d_out.free()
