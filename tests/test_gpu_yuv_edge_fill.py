"""Edge fill on YUV streams on the device, bit for bit: vs_op_warp_affine_yuv_fill against tests/yuvfillref.py, and streams with
vs_stab_set_yuv_edge_fill - per frame, with crop-and-zoom, in batch mode and in a vs_batch group - against surfaces built without the
code under test: the oracle's NV12 run with border_size = 0 gives out_index and matrix of every result, and yuvfillref warps every
plane of the input under M / the format's chroma matrix with the fill outside.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import planar_inputs as pi
import yuvfillref as yf
from test_gpu_planar import _check_debug, bits
from test_gpu_yuv_cropzoom import Fmt, UVLayout, _same, world  # noqa: F401  (world: the module's clips and oracle runs)
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
FORMATS = ["NV12", "P010", "I420", "I010", "I422", "I210", "I444", "I412"]
N = 22


def chosen_fill(f):
    """A colour of the caller's, as the samples lie in memory: Y, U and V distinct, and in 16-bit samples the two bytes distinct - a
    swapped byte or a swapped pair shows."""
    return (81, 90, 240) if f.nbits == 8 else (0x2340, 0x8100, 0x7fc0) if f.name == "P010" else (0x0123, 0x0234, 0x0345)


def default_fill(f):
    sh = 8 if f.name == "P010" else f.nbits - 8
    return (16 << sh, 128 << sh, 128 << sh)


def fill_warp(f, frame, w, h, M, fill):
    """The expected warp of one packed frame."""
    if f.uv:
        wy, wuv = yf.warp_surface([frame[:h], frame[h:].reshape(h // 2, w // 2, 2)], 1, 1, M, fill)
        return np.vstack([wy, wuv.reshape(h // 2, w)])
    return synth.yuv_pack(*yf.warp_surface(list(pi.planes(frame, f.name, w, h)), f.sx, f.sy, M, fill), f.sx, f.sy)


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------
def matrices(w, h):
    """identity; sub-pixel shifts that straddle each of the four edges; shifts that put whole tiles outside the picture, either way;
    a shift by more than the picture (the fill everywhere); 1 and 3 degrees (staged); 10 degrees and zoom 0.5 (direct: the source
    box of a tile outgrows the staging area); a translation that saturates the coordinates."""
    return {
        "identity": [1, 0, 0, 0, 1, 0],
        "left": [1, 0, 3.40625, 0, 1, 0], "right": [1, 0, -2.71875, 0, 1, 0], "top": [1, 0, 0, 0, 1, 5.28125], "bottom": [1, 0, 0, 0, 1, -4.59375],
        "tiles_out": [1, 0, w * 0.45 + 0.25, 0, 1, h * 0.7 + 0.5], "tiles_out_back": [1, 0, -(w * 0.45 + 0.75), 0, 1, -(h * 0.7 + 0.25)],
        "beyond": [1, 0, w + 7.5, 0, 1, -(h + 3.25)],
        "rot_1deg": pi.rotation(1.0, 2.25, -1.5), "rot_3deg": pi.rotation(3.0, -3.5, 2.75),
        "rot_10deg": pi.rotation(10.0, 6.0, -9.5), "zoom_0.5": [0.5, 0, 10.25, 0, 0.5, 5.5],
        "saturated": [1, 0, -40000.5, 0, 1, 35000.25],
    }


def op_layouts(f, w, h):
    """(source, destination) layouts: the packed defaults; padded pitches; odd pitches (8-bit) or pitches that are no multiple of 4
    (16-bit) with plane bases off their alignment, so that no plane of either side is aligned."""
    sb = 1 if f.nbits == 8 else 2
    odd = (w + 31 if w % 2 == 0 else w + 30) * sb          # an odd number of samples
    cw, ch = w >> f.sx, h >> f.sy
    if f.uv:
        return [(f.layout(w, h), f.layout(w, h)),
                (f.layout(w, h, pitch=(w + 30) * sb, uv_off=(w + 30) * sb * (h + 6)), f.layout(w, h, pitch=(w + 62) * sb, uv_off=(w + 62) * sb * (h + 2))),
                (f.layout(w, h, pitch=odd, uv_off=odd * (h + 3) + sb), f.layout(w, h, pitch=odd + 2 * sb, uv_off=(odd + 2 * sb) * (h + 1) + sb))]
    codd = (cw + 21 if cw % 2 == 0 else cw + 20) * sb

    def off(p, c, extra):          # Y, then U and V, every plane `extra` samples off where the last one ended
        u = p * h + extra * sb
        v = u + c * ch + extra * sb
        return dict(pitch=p, c_pitch=c, u_off=u, v_off=v, size=v + c * ch + 16)
    return [(f.layout(w, h), f.layout(w, h)),
            (f.layout(w, h, pitch=(w + 62) * sb, c_pitch=(cw + 40) * sb), f.layout(w, h, pitch=(w + 14) * sb, c_pitch=(w + 14) * sb)),
            (f.layout(w, h, **off(odd, codd, 1)), f.layout(w, h, **off(odd + 2 * sb, codd + 2 * sb, 3)))]


def op_frame(f, seed, w, h):
    """Random samples over the whole range of the sample type."""
    rows = h * 3 // 2 if f.uv else pi.frame_rows(h, f.sx, f.sy)
    return np.random.default_rng(seed).integers(0, 256 if f.nbits == 8 else 65536, (rows, w), np.uint8 if f.nbits == 8 else np.uint16)


def op_run(gpu, f, frames, w, h, Ms, fill, src=None, dst=None, one_source=False):
    """vs_op_warp_affine_yuv_fill over len(Ms) surfaces (one_source: all of them the one source surface, frame distance 0); whole
    output allocations are read back and unpack asserts that nothing outside the planes was written."""
    n = len(Ms)
    src, dst = src or f.layout(w, h), dst or f.layout(w, h)
    d_in = capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in frames]))
    d_out = capi.DevBuf.from_array(gpu, dst.blank(n))
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(n, 6))
    c = C.byref(capi.VsYuvFill(*fill, 0)) if fill is not None else None
    sargs, dargs = ((src.uv_arg, 0, 0), (dst.uv_arg, 0, 0)) if f.uv else (src.args, dst.args)
    try:
        gpu.check(gpu.lib.vs_op_warp_affine_yuv_fill(f.fmt, d_in.ptr, src.pitch, *sargs, d_out.ptr, dst.pitch, *dargs, w, h, capi._p(M, capi.f32p), n,
                                                     0 if one_source else src.size, dst.size, c, None))
        gpu.sync()
        out = d_out.download((n, dst.size // dst.sb), dst.dtype)
        back = d_in.download((len(frames), src.size // src.sb), src.dtype)
    finally:
        d_in.free(); d_out.free()
    assert all(np.array_equal(back[i], src.pack(x)) for i, x in enumerate(frames)), "the sources were written"
    return [dst.unpack(out[i]) for i in range(n)]


def op_sizes(name):
    # several tiles per plane with partial last tiles; 4:4:4 also at an odd width, where the rows are no multiple of 4 bytes
    return [(130, 96), (322, 200)] + ([(131, 97)] if name in ("I444", "I412") else [])


@pytest.mark.parametrize("name,size", [(n, s) for n in FORMATS for s in op_sizes(n)], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_operator_against_the_numpy_statement(gpu, name, size):
    w, h = size
    f = Fmt(name)
    frame, fill = op_frame(f, w * 7 + h, w, h), chosen_fill(f)
    mats = matrices(w, h)
    want = {k: fill_warp(f, frame, w, h, M, fill) for k, M in mats.items()}
    assert np.all(want["beyond"][:h] == fill[0]) and not np.array_equal(want["identity"], want["left"])
    assert np.array_equal(want["identity"], frame)
    for i, (src, dst) in enumerate(op_layouts(f, w, h)):
        got = op_run(gpu, f, [frame], w, h, list(mats.values()), fill, src, dst, one_source=True)
        for k, g in zip(mats, got):
            assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (name, size, i, k)
    # one surface per call: the launch a stream makes per frame
    for k in ("left", "rot_3deg", "rot_10deg"):
        assert np.array_equal(op_run(gpu, f, [frame], w, h, [mats[k]], fill)[0], want[k]), (name, size, k)


@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_operator_32_surfaces_in_one_launch(gpu, name):
    w, h, n = 130, 96, 32
    f = Fmt(name)
    frames = [op_frame(f, 100 + i, w, h) for i in range(n)]
    mats = list(matrices(w, h).values())
    Ms = [mats[i % len(mats)] for i in range(n)]
    got = op_run(gpu, f, frames, w, h, Ms, chosen_fill(f))
    for i in range(n):
        assert np.array_equal(got[i], fill_warp(f, frames[i], w, h, Ms[i], chosen_fill(f))), (name, i)


@pytest.mark.parametrize("name", FORMATS)
def test_operator_default_fill_and_fill_zero(gpu, name):
    """fill NULL is the format's video black; fill (0, 0, 0) gives the bytes of the VS_BORDER_BLACK warp of the same surfaces."""
    w, h = 130, 96
    f = Fmt(name)
    frame = op_frame(f, 9, w, h)
    mats = matrices(w, h)
    Ms = list(mats.values())
    stack = np.stack([frame] * len(Ms))
    got = gpu.warp_affine_yuv_fill(f.fmt, stack, w, h, Ms, None)
    for k, g in zip(mats, got):
        assert np.array_equal(g, fill_warp(f, frame, w, h, mats[k], default_fill(f))), (name, k)
    assert gpu.yuv_video_black(f.fmt) == default_fill(f)
    zero = gpu.warp_affine_yuv_fill(f.fmt, stack, w, h, Ms, (0, 0, 0))
    black = gpu.warp_affine_nv12(stack, w, h, Ms) if name == "NV12" else gpu.warp_affine_p010(stack, w, h, Ms) if name == "P010" else \
        gpu.warp_affine_planar(f.fmt, stack, w, h, Ms, capi.BORDER_BLACK)
    assert zero.dtype == black.dtype and np.array_equal(zero, black), name


def test_operator_refusals_behind_the_host_checks(gpu):
    """What the launchers refuse: geometry, pitches and 16-bit alignment, as for the sibling operators."""
    d = capi.DevBuf(gpu, 1 << 16)
    d.zero()
    M = np.array([1, 0, 0, 0, 1, 0], np.float32)

    def rc(fmt, w=64, h=48, ss=128, ds=128, su=0, fill=None):
        c = C.byref(capi.VsYuvFill(*fill, 0)) if fill is not None else None
        return gpu.lib.vs_op_warp_affine_yuv_fill(fmt, d.ptr, ss, su, 0, 0, d.ptr + 32768, ds, 0, 0, 0, w, h, capi._p(M, capi.f32p), 1, 0, 0, c, None)
    assert rc(capi.FMT_NV12) == 0 and rc(capi.FMT_I420) == 0 and rc(capi.FMT_P010, ss=256, ds=256) == 0
    assert rc(capi.FMT_NV12, w=63) == INVALID and rc(capi.FMT_I420, h=47) == INVALID and rc(capi.FMT_I422, w=63) == INVALID
    assert rc(capi.FMT_I444, w=63, h=47) == 0
    assert rc(capi.FMT_NV12, ss=60) == INVALID                       # a pitch below a row
    assert rc(capi.FMT_P010, ss=255, ds=256) == INVALID              # an odd 16-bit pitch
    assert rc(capi.FMT_P010, ss=256, ds=256, su=256 * 48 + 1) == INVALID
    assert rc(capi.FMT_I010, ss=128, ds=128, fill=(65535, 65535, 65535)) == 0
    assert rc(capi.FMT_I420, fill=(255, 255, 256)) == INVALID
    gpu.sync()
    d.free()


# ---- 2. streams ---------------------------------------------------------------------------------------------------------------
_expected = {}
OFF = "off"            # fill argument of stream_run: the mode is not touched


def expected(world, name, w, h, n, fill, cz=0, **params):
    """Per result: the input frame warped with the fill outside (and, cz = b > 0, its crop zoomed back by cropzoomref); the last one
    (no transform) is the input frame.  Computed once per case."""
    key = (name, w, h, n, tuple(fill), cz, tuple(sorted(params.items())))
    if key not in _expected:
        clip, run, _ = world
        f, frames = Fmt(name), clip(name, w, h)

        def one(idx, M):
            if idx == n - 1:
                return frames[idx]
            wp = fill_warp(f, frames[idx], w, h, M, fill)
            return f.crop_zoom(wp, w, h, cz) if cz else wp
        _expected[key] = [one(idx, M) for idx, M in run(w, h, n, **params)[0]]
    return _expected[key]


def _padded(f, w, h):
    sb = 1 if f.nbits == 8 else 2
    if f.uv:
        return f.layout(w, h, pitch=(w + 30) * sb, uv_off=(w + 30) * sb * (h + 6)), f.layout(w, h, pitch=(w + 62) * sb, uv_off=(w + 62) * sb * (h + 2))
    return f.layout(w, h, pitch=(w + 62) * sb, c_pitch=((w >> f.sx) + 40) * sb), f.layout(w, h, pitch=(w + 14) * sb, c_pitch=(w + 14) * sb)


def _decoder_layouts(f, w, h):
    """Distinct layouts: a decoder-style uv_offset (NV12 / P010); V before U in, a chroma pitch of its own out."""
    sb = 1 if f.nbits == 8 else 2
    if f.uv:
        return f.layout(w, h, pitch=256 * sb, uv_off=256 * sb * (h + 8)), f.layout(w, h, pitch=192 * sb, uv_off=192 * sb * (h + 16))
    ch = h >> f.sy
    return (f.layout(w, h, pitch=512, c_pitch=384, u_off=512 * (h + 8) + 384 * (ch + 4), v_off=512 * (h + 8), size=512 * (h + 8) + 384 * (2 * ch + 8)),
            f.layout(w, h, pitch=(w + 14) * sb, c_pitch=(w + 30) * sb))


def stream_run(gpu, f, frames, w, h, fill, params, batch=1, zero_copy=False, src=None, dst=None, dbg=None, cz=0):
    """The clip through push_dev / flush_dev of a stream with border_size = 0 (cz = b > 0: crop-and-zoom with border_size = b); whole
    output allocations are read back (unpack asserts that nothing outside the planes was written).  fill: OFF = the mode is left
    alone, None = the mode with the default colour, or a colour.  dbg: the oracle's records, checked at every push (per frame)."""
    n = len(frames)
    s = gpu.stabilizer(gpu.params(border_size=cz, crop_n_zoom=1 if cz else 0, **params))
    src, dst = src or f.layout(w, h), dst or f.layout(w, h)
    d_in, d_out = capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in frames])), capi.DevBuf.from_array(gpu, dst.blank(n))
    try:
        if batch > 1:
            s.set_batch(batch)
        s.set_zero_copy(zero_copy)
        if cz:
            s.set_yuv_crop_zoom(True)
        if fill is not OFF:
            s.set_yuv_edge_fill(True, fill)
        f.set_layouts(s, src, dst)
        k = 0
        for i in range(n):
            p = s.push_dev(d_in.ptr + i * src.size, w, h, src.pitch, f.fmt, d_out.ptr + k * dst.size, dst.pitch)
            if dbg is not None:
                assert bool(p) == dbg[i]["has"], i
                _check_debug(s.debug(), dbg[i], i)
            k += p
        s.sync()
        last = s.debug()
        last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
        while s.flush_dev(d_out.ptr + k * dst.size, dst.pitch):
            k += 1
        s.sync()
        ow, oh = C.c_int32(), C.c_int32()
        gpu.check(gpu.lib.vs_stab_last_out_dims(s.h, C.byref(ow), C.byref(oh)), s.h)
        assert (ow.value, oh.value) == (w, h)
        out = d_out.download((n, dst.size // dst.sb), dst.dtype)
    finally:
        s.close(); d_in.free(); d_out.free()
    assert k == n
    return [dst.unpack(out[i]) for i in range(n)], last


@pytest.mark.parametrize("name", FORMATS)
def test_stream_per_frame(gpu, world, name):
    """Frame by frame through the device entry points (padded layouts, whole allocations compared) with the default and a chosen
    fill, and once through the host entry points; the debug records are those of the border_size = 0 run, the last flushed frame is
    the input frame."""
    w, h = 130, 96
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:14]
    _, dbg = run(w, h, 14, **params)
    for fill in (None, chosen_fill(f)):
        want = expected(world, name, w, h, 14, fill or default_fill(f), **params)
        src, dst = _padded(f, w, h)
        got, _ = stream_run(gpu, f, frames, w, h, fill, params, src=src, dst=dst, dbg=dbg)
        _same(got, want, (name, fill))
        assert np.array_equal(got[-1], frames[-1])
    # the picture does leave the frame in this clip: the fill shows, and the stream without the mode differs there
    plain = [x if wp is None else wp for (_, wp), x in zip(world[2](name, w, h, 14, **params), want)]
    assert any(not np.array_equal(a, b) for a, b in zip(plain, want)), "no tap of this clip leaves the picture: the case shows nothing"
    # the host entry points
    fill = chosen_fill(f)
    s = gpu.stabilizer(gpu.params(**params))
    s.set_yuv_edge_fill(True, fill)
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
    s.close()
    _same(got, want, (name, "host"))


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_stream_crop_and_zoom_crops_the_fill_warped_surface(gpu, world, name, batch):
    """border_size 30 with crop_n_zoom: the warp into the scratch surface reads the fill outside the picture, and cropzoomref crops
    and zooms that surface."""
    w, h, b = 130, 96, 30
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:14]
    fill = chosen_fill(f)
    src, dst = _decoder_layouts(f, w, h)
    got, _ = stream_run(gpu, f, frames, w, h, fill, params, batch, True, src, dst, cz=b)
    _same(got, expected(world, name, w, h, 14, fill, cz=b, **params), (name, "crop-and-zoom"))


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("batch", [8, 40])
@pytest.mark.parametrize("name", ["NV12", "P010", "I444"])
def test_stream_batch_mode_equals_the_per_frame_path(gpu, world, name, batch, zero_copy):
    """22 frames in batches of 8 (two whole steps and one of six) and of 40 (one partial step), decoder-style layouts that differ
    between input and output: the results equal the per-frame path's and the expected surfaces.  The warps of a step are issued two
    steps later, and launches of fewer than four surfaces go plane by plane through the general fill kernel."""
    w, h = 130, 96
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:N]
    fill = chosen_fill(f)
    src, dst = _decoder_layouts(f, w, h)
    per_frame, last1 = stream_run(gpu, f, frames, w, h, fill, params, 1, zero_copy, src, dst)
    got, last = stream_run(gpu, f, frames, w, h, fill, params, batch, zero_copy, src, dst)
    _same(got, per_frame, (name, "batch vs per frame"))
    _same(got, expected(world, name, w, h, N, fill, **params), name)
    for key in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(last[key]), bits(last1[key])) and np.array_equal(bits(last[key]), bits(run(w, h, N, **params)[1][-1][key])), key


@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_vs_batch_of_three_streams_against_standalone_instances(gpu, world, name):
    w, h, n, S = 130, 96, N, 3
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:n]
    fill = chosen_fill(f)
    src, dst = _decoder_layouts(f, w, h)
    # another picture per stream, the same layout: every frame rolled along its rows by an even number of samples
    cl = [[np.roll(x, 4 * g, axis=1) for x in frames] for g in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in c])) for c in cl]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    g = gpu.batch(gpu.params(**params), S, 8)
    try:
        g.set_zero_copy(True)
        g.set_yuv_edge_fill(True, fill)
        f.set_layouts(g, src, dst)
        with pytest.raises(capi.VsError, match="belongs to a vs_batch"):
            g.stream(0).set_yuv_edge_fill(False)
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
        got = [dst.unpack(raw[i]) for i in range(n)]
        alone, _ = stream_run(gpu, f, cl[j], w, h, fill, params, 8, True, src, dst)
        _same(got, alone, (name, j))
        if j == 0:                                           # (stream 0 has the clip itself)
            _same(got, expected(world, name, w, h, n, fill, **params), name)
    for d in d_in + d_out:
        d.free()


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", ["NV12", "P010", "I422", "I412"])
def test_opt_in(gpu, world, name, batch):
    """The mode off is today's stream - the oracle's warp with zeros outside -, and the mode on with fill (0, 0, 0) equals it."""
    w, h, n = 130, 96, 14
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, warps = world
    frames = clip(name, w, h)[:n]
    today = [frames[idx] if wp is None else wp for idx, wp in warps(name, w, h, n, **params)]
    off, _ = stream_run(gpu, f, frames, w, h, OFF, params, batch, True)
    zero, _ = stream_run(gpu, f, frames, w, h, (0, 0, 0), params, batch, True)
    _same(off, today, (name, "mode off"))
    _same(zero, today, (name, "fill 0"))


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def _first_push(gpu, name, params, mode, w=64, h=48, batch=1, fill=None, pad=False):
    f = Fmt(name) if name not in ("GRAY8", "BGR8") else None
    fmt = f.fmt if f else getattr(capi, "FMT_" + name)
    px = capi.fmt_px_bytes(fmt)
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **params))
    s.set_batch(batch)
    if mode is not OFF:
        s.set_yuv_edge_fill(mode, fill)
    if pad:
        s.set_yuv_border_pad(True)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    b = params.get("border_size", 0) if pad else 0
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr), w, h, w * px, fmt, C.c_void_p(d_out.ptr), (w + 2 * b) * px, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", FORMATS)
def test_refusals_through_the_stream(gpu, name, batch):
    f = Fmt(name)
    assert _first_push(gpu, name, {}, True, batch=batch)[0] == 0
    # a border_size without a pad mode opted in, crop-and-zoom without its mode, the fade, the canvas: as with the mode off
    for params in (dict(border_size=8), dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE), dict(enable_virtual_canvas=1)):
        on, off = _first_push(gpu, name, params, True, batch=batch), _first_push(gpu, name, params, OFF, batch=batch)
        assert on == off and on[0] == UNSUPPORTED, params
    # border pad opted in: the mode is independent of it and does nothing there
    assert _first_push(gpu, name, dict(border_size=8), True, batch=batch, pad=True)[0] == 0
    big = _first_push(gpu, name, {}, True, batch=batch, fill=(256, 0, 0))          # (the format is not known at the setter: the push answers)
    if f.nbits == 8:
        assert big[0] == INVALID and "above 255" in big[1] and name in big[1] and "vs_stab_set_yuv_edge_fill" in big[1]
    else:
        assert big[0] == 0
    assert _first_push(gpu, name, {}, False, batch=batch, fill=(256, 0, 0))[0] == 0       # (switched off: the colour is not looked at)


def test_setter_refusals(gpu):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5))
    rc = gpu.lib.vs_stab_set_yuv_edge_fill(s.h, 1, C.byref(capi.VsYuvFill(16, 128, 128, 1)))
    assert rc == INVALID and b"vs_stab_set_yuv_edge_fill: fill->reserved must be 0" in gpu.lib.vs_stab_last_error(s.h)
    s.set_zero_copy(True)
    s.set_yuv_edge_fill(True, (300, 0, 0))                   # no format yet
    s.set_yuv_edge_fill(True)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    assert s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 64) == 0
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_edge_fill: the frame queue must be empty"):
        s.set_yuv_edge_fill(False)
    while s.flush_dev(d_out.ptr, 64):
        pass
    s.sync()
    with pytest.raises(capi.VsError, match="above 255 on NV12"):      # the format is known now
        s.set_yuv_edge_fill(True, (16, 128, 300))
    s.set_yuv_edge_fill(True, (16, 128, 255))
    s.set_yuv_edge_fill(False)
    s.close(); d_in.free(); d_out.free()


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", ["GRAY8", "BGR8"])
def test_gray8_and_bgr8_are_not_touched(gpu, name, batch):
    """The same frames through a stream with the mode on and through one without: the same bytes."""
    w, h, n = 64, 48, 12
    bgr = synth.make_clip(synth.SEED_CONFIG3 + 35, w, h, n)
    frames = bgr if name == "BGR8" else [np.ascontiguousarray(x[..., 1]) for x in bgr]
    fmt = getattr(capi, "FMT_" + name)
    outs = []
    for mode in (False, True):
        s = gpu.stabilizer(gpu.params(smoothing_radius=5))
        s.set_batch(batch)
        if mode:
            s.set_yuv_edge_fill(True, (81, 90, 240))
        got = [o for o in (s.push(x, fmt) for x in frames) if o is not None]
        while True:
            o = s.flush(frames[0], fmt)
            if o is None:
                break
            got.append(o)
        s.close()
        outs.append(got)
    assert len(outs[0]) == n
    _same(outs[1], outs[0], name)


def test_vs_batch_refuses_members_that_disagree(gpu):
    """One warp launch serves the frames of all members with ONE colour: a step refuses members that differ in the mode or in the
    resolved fill.  The setter reaches all members through the group; a member with a frame queued refuses the change and the group
    reports it, which is how members come to differ.  Equal colours - video black spelled out against the default - are accepted."""
    w, h = 64, 48
    A, B = (30, 100, 200), (31, 100, 200)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()

    def push_both(g, n=8):
        for _ in range(n):
            g.push_dev([d_in.ptr, d_in.ptr], w, h, w, capi.FMT_NV12, [d_out.ptr, d_out.ptr + (1 << 19)], w)

    def group_with_member_1_queued(first, second):
        """Both members get `first`; member 1 queues a frame; the setter comes again with `second`: member 0 takes it, member 1 refuses."""
        g = gpu.batch(gpu.params(smoothing_radius=5), 2, 4)
        g.set_zero_copy(True)
        g.set_yuv_edge_fill(*first)
        assert g.push_dev([None, d_in.ptr], w, h, w, capi.FMT_NV12, [None, d_out.ptr + (1 << 19)], w) == [0, 0]
        with pytest.raises(capi.VsError, match="queue must be empty"):
            g.set_yuv_edge_fill(*second)
        return g
    for first, second in (((True, A), (True, B)), ((True, A), (True, None)), ((True, None), (True, B)), ((True, A), (False, None)), ((False, None), (True, None))):
        g = group_with_member_1_queued(first, second)
        with pytest.raises(capi.VsError, match="share one frame geometry"):
            push_both(g)
        g.close()
    for first, second in (((True, A), (True, A)), ((True, None), (True, (16, 128, 128))), ((False, None), (False, A))):
        g = group_with_member_1_queued(first, second)
        push_both(g)
        g.sync()
        g.close()
    d_in.free(); d_out.free()
