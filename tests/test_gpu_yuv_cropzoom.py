"""Crop-and-zoom on YUV streams on the device, bit for bit: vs_op_resize_jobs against tests/cropzoomref.py, and streams with
vs_stab_set_yuv_crop_zoom - per frame, in batch mode and in a vs_batch group - against surfaces built without the code under test:
the warped surfaces the formats' existing stream tests derive from the oracle for the same clip with border_size = 0 (the oracle's
NV12 run gives out_index and matrix of every result; oracle.warp_affine_nv12, ref16.warp_two_planes and planar_inputs.warp_frame the
warp), every plane cropped and zoomed by cropzoomref.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import cropzoomref as cz
import planar_inputs as pi
import plane_job_refusals as pjr
import ref16
import roi
from test_gpu_planar import _check_debug, _oracle_nv12_run, bits
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
SIZES = [((126, 92), (130, 96)), ((310, 188), (322, 200)), ((20, 4), (64, 48)), ((2, 2), (64, 48)), ((1, 3), (32, 48)), ((644, 340), (704, 400))]
SIZE_IDS = ["%dx%d-%dx%d" % (s + d) for s, d in SIZES]


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------
def _crop_view(surface, x, y, sw, sh, px, dtype):
    """The crop at pixel (x, y) of the source surface's ROI, as samples, from the surface's prefill."""
    rows = surface._view(surface.host)[0]
    return np.ascontiguousarray(rows[y:y + sh, x * px:(x + sw) * px]).view(dtype)


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_operator_on_rois_against_the_numpy_statement(gpu, size, sb, cn):
    """Sources: crops at x = 1, 2, 3 samples inside larger random pictures that are themselves ROIs; destinations: ROIs with odd and
    padded pitches at every base alignment the sample size allows.  Every byte outside the destination ROI keeps its prefill, the
    sources are untouched."""
    (sw, sh), (dw, dh) = size
    px, dtype = sb * cn, (np.uint8 if sb == 1 else np.uint16)
    layouts = roi.LAYOUT_NAMES if sb == 1 else ["packed", "padded16", "roi_off2", "tight_end"]       # (16-bit: even addresses and pitches)
    for i, layout in enumerate(layouts):
        x = 1 + i % 3
        seed = roi.case_seed("cropzoom", size, sb, cn, layout)
        src, dst = roi.pair(layout, seed, (sw + 4, sh + 2, px), (dw, dh, px))
        src.bind(gpu); dst.bind(gpu)
        try:
            crop = _crop_view(src, x, 1, sw, sh, px, dtype)
            gpu.resize_jobs([(src.ptr + src.pitch + x * px, src.pitch, sw, sh, dst.ptr, dst.pitch, dw, dh, cn)], sb)
            gpu.sync()
            got, clean = dst.result((dh, dw * cn), dtype)
            assert np.array_equal(got, cz.resize(crop, cn, dw, dh)), (layout, x)
            assert clean, dst.stray()
            assert src.untouched(), layout
        finally:
            src.free(); dst.free()


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_operator_96_mixed_jobs_in_one_launch_equal_the_jobs_one_by_one(gpu, sb):
    shapes = [((20, 4), (64, 48)), ((2, 2), (64, 48)), ((1, 3), (32, 48)), ((126, 92), (130, 96)), ((61, 30), (67, 33)), ((300, 9), (301, 40))]
    dtype = np.uint8 if sb == 1 else np.uint16
    rng = np.random.default_rng(96 + sb)
    jobs, so, do = [], 0, 0
    for i in range(96):
        (sw, sh), (dw, dh) = shapes[i % len(shapes)]
        cn = 1 + (i // 2) % 2
        sp, dp = (sw * cn + 3) * sb + (sb == 1) * (i % 2), (dw * cn + 5) * sb
        jobs.append((so, sp, sw, sh, do, dp, dw, dh, cn))
        so += sp * sh + 2 * (i % 5); do += dp * dh + 2 * (i % 3)
    src = rng.integers(0, 256, so, np.uint8)
    fill = rng.integers(0, 256, do, np.uint8)
    d_src, d_one, d_all = capi.DevBuf.from_array(gpu, src), capi.DevBuf.from_array(gpu, fill), capi.DevBuf.from_array(gpu, fill)
    try:
        gpu.resize_jobs([(d_src.ptr + a, sp, sw, sh, d_all.ptr + b, dp, dw, dh, cn) for a, sp, sw, sh, b, dp, dw, dh, cn in jobs], sb)
        for a, sp, sw, sh, b, dp, dw, dh, cn in jobs:
            gpu.resize_jobs([(d_src.ptr + a, sp, sw, sh, d_one.ptr + b, dp, dw, dh, cn)], sb)
        gpu.sync()
        one, al = d_one.download((do,), np.uint8), d_all.download((do,), np.uint8)
        assert np.array_equal(one, al)
        assert np.array_equal(d_src.download((so,), np.uint8), src)
        want = fill.copy()
        for a, sp, sw, sh, b, dp, dw, dh, cn in jobs:
            crop = np.lib.stride_tricks.as_strided(src[a:], (sh, sw * cn * sb), (sp, 1)).copy().view(dtype)
            np.lib.stride_tricks.as_strided(want[b:], (dh, dw * cn * sb), (dp, 1))[...] = cz.resize(crop, cn, dw, dh).view(np.uint8)
        assert np.array_equal(al, want)
    finally:
        d_src.free(); d_one.free(); d_all.free()


def test_operator_refusals(gpu):
    """The tables of tests/plane_job_refusals.py on a real buffer: the accepted calls launch."""
    d = capi.DevBuf(gpu, pjr.REGION)
    d.zero()
    for make in (pjr.resize,):
        op = make(d.ptr)
        pjr.check_accepted(gpu.lib, op, pjr.OK)
        pjr.check_refusals(gpu.lib, op)
    gpu.sync()
    d.free()


# ---- 2. streams ---------------------------------------------------------------------------------------------------------------
class UVLayout:
    """An NV12 / P010 surface: rows of `pitch` bytes, the interleaved chroma plane uv_off bytes behind the luma plane (None: the
    packed default); canaries wherever no sample lies.  The interface of planar_inputs.Layout."""

    def __init__(self, name, w, h, pitch=None, uv_off=None):
        self.name, self.w, self.h = name, w, h
        self.sb = 1 if name == "NV12" else 2
        self.dtype = np.uint8 if self.sb == 1 else np.uint16
        self.canary = 0xA5 if self.sb == 1 else 0xA5C3
        self.pitch = pitch or w * self.sb
        self.uv_off = uv_off or h * self.pitch
        self.size = self.uv_off + (h // 2) * self.pitch
        self.uv_arg = uv_off or 0

    def _planes(self, buf):
        p = self.pitch // self.sb
        return (buf[:self.h * p].reshape(self.h, p)[:, :self.w], buf[self.uv_off // self.sb:][:(self.h // 2) * p].reshape(self.h // 2, p)[:, :self.w])

    def pack(self, frame):
        buf = np.full(self.size // self.sb, self.canary, self.dtype)
        y, uv = self._planes(buf)
        y[...] = frame[:self.h]; uv[...] = frame[self.h:]
        return buf

    def blank(self, n):
        return np.full((n, self.size // self.sb), self.canary, self.dtype)

    def unpack(self, buf):
        buf = np.asarray(buf, self.dtype).reshape(-1).copy()
        y, uv = self._planes(buf)
        out = np.vstack([y, uv])
        y[...] = self.canary; uv[...] = self.canary
        assert np.all(buf == self.canary), "samples outside the planes were written"
        return out


class Fmt:
    """One of the stream formats under test: its clip, its layouts, the reference warp, and its planes for cropzoomref."""

    def __init__(self, name):
        self.name = name
        self.uv = name in ("NV12", "P010")
        if self.uv:
            self.fmt, self.sx, self.sy, self.nbits = getattr(capi, "FMT_" + name), 1, 1, 8 if name == "NV12" else 10
        else:
            self.fmt, self.sx, self.sy, self.nbits = dict(pi.FORMATS, **pi.OLD)[name]
        self.kind = ("uv" if self.uv else "planar", self.sx, self.sy)

    def frames(self, bgr, nv12):
        if self.name == "NV12":
            return nv12
        if self.name == "P010":
            return [synth.nv12_to_p010(f, seed=i) for i, f in enumerate(nv12)]
        return [synth.bgr_to_planar(f, self.sx, self.sy, self.nbits, seed=i) for i, f in enumerate(bgr)]

    def layout(self, w, h, **kw):
        return UVLayout(self.name, w, h, **kw) if self.uv else pi.Layout(self.name, w, h, **kw)

    def set_layouts(self, s, src, dst):
        if self.uv:
            if src.uv_arg or dst.uv_arg:
                s.set_nv12_layout(src.uv_arg, dst.uv_arg)
        elif any(src.args) or any(dst.args):
            s.set_i420_layout(*src.args, *dst.args)

    def warp(self, oracle, frame, w, h, M):
        if self.name == "NV12":
            return oracle.warp_affine_nv12(frame, w, h, M)
        if self.name == "P010":
            return ref16.warp_two_planes(frame, w, h, M)
        return pi.warp_frame(oracle, frame, self.name, w, h, M)

    def crop_zoom(self, warped, w, h, b):
        if self.uv:
            return np.vstack(cz.crop_zoom_surface(self.kind, [warped[:h], warped[h:]], b))
        return synth.yuv_pack(*cz.crop_zoom_surface(self.kind, list(pi.planes(warped, self.name, w, h)), b), self.sx, self.sy)


STREAM_FORMATS = ["NV12", "P010", "I420", "I010", "I422", "I210", "I444", "I412"]
N = 22


@pytest.fixture(scope="module")
def world(oracle):
    """Per size: the clip in every format, the oracle's runs (border_size = 0) and the warped surfaces of every result - each computed
    once and left unchanged."""
    clips, runs, warped = {}, {}, {}

    def clip(name, w, h):
        if (w, h) not in clips:
            bgr = synth.make_clip(synth.SEED_CONFIG3 + 33, w, h, N)
            clips[(w, h)] = dict(bgr=bgr, nv12=[synth.bgr_to_nv12(f) for f in bgr])
        c = clips[(w, h)]
        if name not in c:
            c[name] = Fmt(name).frames(c["bgr"], c["nv12"])
        return c[name]

    def run(w, h, n, **params):
        key = (w, h, n, tuple(sorted(params.items())))
        if key not in runs:
            clip("NV12", w, h)
            runs[key] = _oracle_nv12_run(oracle, clips[(w, h)]["nv12"][:n], **params)
        return runs[key]

    def warps(name, w, h, n, **params):
        """Per result of the run: the warped surface (None for the last frame, which has no transform) and its input's index."""
        key = (name, w, h, n, tuple(sorted(params.items())))
        if key not in warped:
            f, frames = Fmt(name), clip(name, w, h)[:n]
            warped[key] = [(idx, None if idx == n - 1 else f.warp(oracle, frames[idx], w, h, M)) for idx, M in run(w, h, n, **params)[0]]
        return warped[key]
    return clip, run, warps


def expected(world, name, w, h, n, b, **params):
    clip, _, warps = world
    f, frames = Fmt(name), clip(name, w, h)
    return [frames[idx] if wp is None else f.crop_zoom(wp, w, h, b) for idx, wp in warps(name, w, h, n, **params)]


def _padded(f, w, h):
    """Distinct input and output layouts with padding everywhere."""
    sb = 1 if f.nbits == 8 else 2
    if f.uv:
        return f.layout(w, h, pitch=(w + 30) * sb, uv_off=(w + 30) * sb * (h + 6)), f.layout(w, h, pitch=(w + 62) * sb, uv_off=(w + 62) * sb * (h + 2))
    return f.layout(w, h, pitch=(w + 62) * sb, c_pitch=((w >> f.sx) + 40) * sb), f.layout(w, h, pitch=(w + 14) * sb, c_pitch=(w + 14) * sb)


def stream_run(gpu, f, frames, w, h, b, params, batch=1, zero_copy=False, src=None, dst=None, dbg=None, mode=True):
    """The clip through push_dev / flush_dev of a stream with crop_n_zoom and border_size = b; whole output allocations are read back
    (unpack asserts that nothing outside the planes was written).  dbg: the oracle's records, checked at every push (per frame)."""
    n = len(frames)
    s = gpu.stabilizer(gpu.params(border_size=b, crop_n_zoom=1, **params))
    src, dst = src or f.layout(w, h), dst or f.layout(w, h)
    d_in, d_out = capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in frames])), capi.DevBuf.from_array(gpu, dst.blank(n))
    try:
        if batch > 1:
            s.set_batch(batch)
        s.set_zero_copy(zero_copy)
        s.set_yuv_crop_zoom(mode)
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
        out = d_out.download((n, dst.size // dst.sb), dst.dtype)
    finally:
        s.close(); d_in.free(); d_out.free()
    return [dst.unpack(out[i]) for i in range(k)], last


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.dtype == r.dtype and np.array_equal(g, r), (what, k)


@pytest.mark.parametrize("size", [(130, 96), (322, 200)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_stream_per_frame(gpu, world, name, size):
    """Frame by frame through the device entry points (padded layouts, whole allocations compared) for every border, and once through
    the host entry points; the debug records are those of the border_size = 0 run, the last flushed frame is the input frame."""
    w, h = size
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:14]
    _, dbg = run(w, h, 14, **params)
    borders = [2, 6, 30] + ([5] if (f.sx, f.sy) == (0, 0) else [])
    for b in borders:
        want = expected(world, name, w, h, 14, b, **params)
        src, dst = _padded(f, w, h)
        got, _ = stream_run(gpu, f, frames, w, h, b, params, src=src, dst=dst, dbg=dbg)
        _same(got, want, (name, b))
        assert np.array_equal(got[-1], frames[-1])
    # the host entry points
    b = borders[1]
    want = expected(world, name, w, h, 14, b, **params)
    s = gpu.stabilizer(gpu.params(border_size=b, crop_n_zoom=1, **params))
    s.set_yuv_crop_zoom(True)
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
    _same(got, want, (name, "host"))


def _decoder_layouts(f, w, h):
    """Distinct input and output layouts: a decoder-style uv_offset (NV12 / P010); V before U in, a chroma pitch of its own out."""
    sb = 1 if f.nbits == 8 else 2
    if f.uv:
        return f.layout(w, h, pitch=256 * sb, uv_off=256 * sb * (h + 8)), f.layout(w, h, pitch=192 * sb, uv_off=192 * sb * (h + 16))
    ch = h >> f.sy
    return (f.layout(w, h, pitch=512, c_pitch=384, u_off=512 * (h + 8) + 384 * (ch + 4), v_off=512 * (h + 8), size=512 * (h + 8) + 384 * (2 * ch + 8)),
            f.layout(w, h, pitch=(w + 14) * sb, c_pitch=(w + 30) * sb))


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("batch", [8, 40])
@pytest.mark.parametrize("name", ["NV12", "P010", "I420", "I210", "I444"])
def test_stream_batch_mode_equals_the_per_frame_path(gpu, world, name, batch, zero_copy):
    """22 frames in batches of 8 (two whole steps and one of six) and of 40 (one partial step), decoder-style layouts that differ
    between input and output (YV12 order in): the results equal the per-frame path's and the expected surfaces."""
    w, h, b = 130, 96, 6
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, run, _ = world
    frames = clip(name, w, h)[:N]
    src, dst = _decoder_layouts(f, w, h)
    per_frame, last1 = stream_run(gpu, f, frames, w, h, b, params, 1, zero_copy, src, dst)
    got, last = stream_run(gpu, f, frames, w, h, b, params, batch, zero_copy, src, dst)
    _same(got, per_frame, (name, "batch vs per frame"))
    _same(got, expected(world, name, w, h, N, b, **params), name)
    for key in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(last[key]), bits(last1[key])) and np.array_equal(bits(last[key]), bits(run(w, h, N, **params)[1][-1][key])), key


@pytest.mark.parametrize("name", ["NV12", "I420"])
def test_stream_batch_of_32_with_several_tiles_in_every_plane(gpu, oracle, name):
    """704 x 400, batch 32: one warp launch of 32 surfaces, one zoom launch of 64 / 96 jobs; every plane has several tiles across and
    down (256 bytes x 64 rows)."""
    w, h, b, n = 704, 400, 30, 40
    f, params = Fmt(name), dict(smoothing_radius=5)
    bgr = synth.make_clip(synth.SEED_CONFIG3 + 34, w, h, n)
    nv12 = [synth.bgr_to_nv12(x) for x in bgr]
    frames = f.frames(bgr, nv12)
    got, _ = stream_run(gpu, f, frames, w, h, b, params, 32, True)
    per_frame, _ = stream_run(gpu, f, frames, w, h, b, params, 1, True)
    _same(got, per_frame, name)
    ref, _ = _oracle_nv12_run(oracle, nv12, **params)
    assert len(got) == len(ref) == n
    for k, (idx, M) in enumerate(ref):
        want = frames[idx] if idx == n - 1 else f.crop_zoom(f.warp(oracle, frames[idx], w, h, M), w, h, b)
        assert np.array_equal(got[k], want), (name, k)


@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_vs_batch_of_three_streams_against_standalone_instances(gpu, world, name):
    w, h, b, n, S = 130, 96, 6, N, 3
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, _ = world
    frames = clip(name, w, h)[:n]
    src, dst = _decoder_layouts(f, w, h)
    # another picture per stream, the same layout: every frame rolled along its rows by an even number of samples
    cl = [[np.roll(x, 4 * g, axis=1) for x in frames] for g in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(x) for x in c])) for c in cl]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    g = gpu.batch(gpu.params(border_size=b, crop_n_zoom=1, **params), S, 8)
    try:
        g.set_zero_copy(True)
        g.set_yuv_crop_zoom(True)
        f.set_layouts(g, src, dst)
        with pytest.raises(capi.VsError, match="belongs to a vs_batch"):
            g.stream(0).set_yuv_crop_zoom(False)
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
    for j in range(S):
        raw = d_out[j].download((n, dst.size // dst.sb), dst.dtype)
        got = [dst.unpack(raw[i]) for i in range(k[j])]
        alone, _ = stream_run(gpu, f, cl[j], w, h, b, params, 8, True, src, dst)
        _same(got, alone, (name, j))
        if j == 0:                                           # (stream 0 has the clip itself)
            _same(got, expected(world, name, w, h, n, b, **params), name)
    for d in d_in + d_out:
        d.free()


# ---- 3. refusals and the empty crop ---------------------------------------------------------------------------------------------
def _first_push(gpu, name, params, mode, w=64, h=48, batch=1):
    f = Fmt(name)
    sb = 1 if f.nbits == 8 else 2
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, **params))
    s.set_batch(batch)
    s.set_yuv_crop_zoom(mode)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    produced = C.c_int32(0)
    rc = gpu.lib.vs_stab_push_dev(s.h, C.c_void_p(d_in.ptr), w, h, w * sb, f.fmt, C.c_void_p(d_out.ptr), w * sb, C.byref(produced))
    msg = (gpu.lib.vs_stab_last_error(s.h) or b"").decode()
    s.close(); d_in.free(); d_out.free()
    return rc, msg


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", STREAM_FORMATS)
def test_refusals_through_the_stream(gpu, name, batch):
    f = Fmt(name)
    crop = dict(border_size=8, crop_n_zoom=1)
    off = _first_push(gpu, name, crop, False, batch=batch)
    assert off[0] == UNSUPPORTED and "modes need a colour format" in off[1]                    # mode off: today's refusal and text
    assert _first_push(gpu, name, crop, True, batch=batch)[0] == 0
    odd = _first_push(gpu, name, dict(border_size=5, crop_n_zoom=1), True, batch=batch)
    if f.sx or f.sy:
        assert odd[0] == INVALID and name in odd[1] and "even border_size" in odd[1]
    else:
        assert odd[0] == 0
    for params in (dict(border_size=8), dict(border_size=8, border_type=capi.BORDER_FADE)):   # pad, fade: as with the mode off
        assert _first_push(gpu, name, params, True, batch=batch) == _first_push(gpu, name, params, False, batch=batch)
        assert _first_push(gpu, name, params, True, batch=batch)[0] == UNSUPPORTED
    on, offc = (_first_push(gpu, name, dict(enable_virtual_canvas=1), m, batch=batch) for m in (True, False))
    assert on == offc and on[0] == UNSUPPORTED and "enableVirtualCanvas" in on[1]


@pytest.mark.parametrize("batch", [1, 8])
def test_setter_with_frames_queued_is_refused(gpu, batch):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5, border_size=8, crop_n_zoom=1))
    s.set_batch(batch)
    s.set_zero_copy(True)
    s.set_yuv_crop_zoom(True)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    assert s.push_dev(d_in.ptr, 64, 48, 64, capi.FMT_NV12, d_out.ptr, 64) == 0
    with pytest.raises(capi.VsError, match="vs_stab_set_yuv_crop_zoom: the frame queue must be empty"):
        s.set_yuv_crop_zoom(False)
    s.sync()
    s.close(); d_in.free(); d_out.free()


def test_vs_batch_refuses_members_that_disagree(gpu):
    """Members of a group agree on border_size and crop_n_zoom as ever: a step refuses those that differ.  The mode is set for all
    members through the group; a member with a frame queued refuses the change, and the group reports it."""
    w, h = 64, 48
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    p = [gpu.params(smoothing_radius=5, border_size=8, crop_n_zoom=1), gpu.params(smoothing_radius=5, border_size=6, crop_n_zoom=1)]
    g = gpu.batch(p, 2, 4)
    g.set_zero_copy(True)
    g.set_yuv_crop_zoom(True)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        for _ in range(8):
            g.push_dev([d_in.ptr, d_in.ptr], w, h, w, capi.FMT_NV12, [d_out.ptr, d_out.ptr + (1 << 19)], w)
    g.close()
    # the mode itself: member 1 has a frame queued when the group's setter comes, so member 0 is switched off and member 1 is not
    g = gpu.batch(gpu.params(smoothing_radius=5, border_size=48, crop_n_zoom=1), 2, 4)       # (an empty crop: both modes accept the push)
    g.set_zero_copy(True)
    g.set_yuv_crop_zoom(True)
    assert g.push_dev([None, d_in.ptr], w, h, w, capi.FMT_NV12, [None, d_out.ptr], w) == [0, 0]
    with pytest.raises(capi.VsError, match="queue must be empty"):
        g.set_yuv_crop_zoom(False)
    g.close(); d_in.free(); d_out.free()


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("name", ["NV12", "I210"])
def test_a_border_that_leaves_no_crop_only_warps(gpu, world, name, batch):
    """w - 2b <= 0 (or h - 2b <= 0) with the mode on: the plain warped surface, as for BGR8."""
    w, h, n = 130, 96, 14
    f, params = Fmt(name), dict(smoothing_radius=6)
    clip, _, warps = world
    frames = clip(name, w, h)[:n]
    want = [frames[idx] if wp is None else wp for idx, wp in warps(name, w, h, n, **params)]
    for b in (48, 66):
        got, _ = stream_run(gpu, f, frames, w, h, b, params, batch, True)
        _same(got, want, (name, b))
