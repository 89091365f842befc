"""Planar 4:2:2 / 4:4:4 surfaces (I422, I444, I210, I212, I410, I412) on the device, bit for bit.

The warp operator against per-plane references - Y under M, U and V under the chroma matrix Mc = S^-1 M S (planar_inputs.warp_frame:
the oracle's cv::warpAffine for 8-bit planes, tests/ref16.py for 16-bit planes; tests/test_planar_cpu.py ties the two together for
the sheared matrix of 4:2:2); the analysis gray image against the oracle's gray image of min(sample >> (bits - 8), 255); and the
whole stabilizer: a stream's debug records equal those of the oracle's NV12 run on the analysis bytes, and every output is the
reference warp of input `out_index` under that record's matrix - flush and the unwarped last frame included.

Which tiles leave the staging area (planar_inputs.STAGING has the arithmetic): a full-width (128-column) tile is staged below 3.61
degrees and direct from 4.07 degrees for Y and for 4:4:4 chroma, but staged below 1.80 and direct from 2.04 degrees for 4:2:2 chroma,
whose inverse map has 2 sin(a) in m3.  A 4:2:2 chroma tile of 65 columns (the 130-wide surfaces): staged below 3.58, direct from 4.05."""
import ctypes as C

import numpy as np
import pytest

import i010_inputs as ii
import planar_inputs as pi
from planar_inputs import ALL_MATS, FORMATS, Layout
from p010_inputs import MATS
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

NAMES = list(FORMATS)
FMTS = pytest.mark.parametrize("name", NAMES)
BORDERS = pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE], ids=["black", "replicate"])


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def fmt_of(name):
    return dict(FORMATS, **pi.OLD)[name][0]


# ---- 1. the warp operator ----------------------------------------------------------------------------------------------------
def _warp(gpu, name, frames, w, h, Ms, border=capi.BORDER_BLACK, src=None, dst=None):
    """vs_op_warp_affine_planar over the surfaces holding the given packed frames; the results as packed frames (unpack checks that
    nothing outside the planes was written)."""
    n = len(frames)
    src, dst = src or Layout(name, w, h), dst or Layout(name, w, h)
    d_in = capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in frames]))
    d_out = capi.DevBuf.from_array(gpu, dst.blank(n))
    M = np.ascontiguousarray(np.asarray(Ms, np.float32).reshape(n, 6))
    try:
        gpu.check(gpu.lib.vs_op_warp_affine_planar(fmt_of(name), d_in.ptr, src.pitch, *src.args, d_out.ptr, dst.pitch, *dst.args, w, h, capi._p(M, capi.f32p),
                                                   n, src.size, dst.size, border, None))
        gpu.sync()
        out = d_out.download((n, dst.size // dst.sb), dst.dtype)
    finally:
        d_in.free(); d_out.free()
    return [dst.unpack(o) for o in out]


# one tile column and one tile row crossed in Y (tiles of 128 x 64 pixels, 128 x 32 for 16-bit samples); the 4:2:2 chroma planes of
# 65 / 129 columns then have a ragged last tile of their own.  258 x 33: a full-width 4:2:2 chroma tile (direct at 2.5 degrees and up).
_SIZES = {0: [(1, 1), (131, 67), (258, 34)], 1: [(2, 1), (130, 67), (258, 33)]}


@BORDERS
@pytest.mark.parametrize("k", [0, 1, 2], ids=["tiny", "one-tile-column", "two-tile-columns"])
@FMTS
def test_warp_single_surfaces(gpu, oracle, name, k, border):
    w, h = _SIZES[FORMATS[name][1]][k]
    frame = pi.random_frame(w, name, w, h)          # (the 16-bit frames whose rounding ties test_planar_cpu.py counts)
    for m, M in ALL_MATS.items():
        got = _warp(gpu, name, [frame], w, h, [M], border)[0]
        assert np.array_equal(got, pi.warp_frame(oracle, frame, name, w, h, M, border)), (name, (w, h), m)


# 130 x 66: Y has a 128-column and a 2-column tile, the 4:2:2 chroma planes one tile of 65 columns, 4:4:4 chroma the tiles of Y.
# rot_1.5deg, rot_2.5deg, rot_3.4deg: every tile staged.  rot_5deg: the 128-column tiles of Y (and of 4:4:4 chroma) and the 65-column
# tiles of 4:2:2 chroma go direct (64 x 2 sin(5 deg) = 11.2 rows more than the staging area's 9); the 2-column tiles stay staged.
# rot_zoom_beyond_box (20 degrees) and saturated: direct everywhere.  So 3.4 and 5 degrees lie on either side of the limit of these
# surfaces' chroma tiles, and surfaces 0 and 1 of every batch are that pair.
_BATCH_ORDER = ["rot_3.4deg", "rot_5deg", "rot_1.5deg", "rot_2.5deg"] + list(MATS)


@BORDERS
@pytest.mark.parametrize("n", [2, 5, 32])
@FMTS
def test_warp_batches(gpu, oracle, name, n, border):
    w, h = 130, 66
    frames = [pi.random_frame(1000 * n + i, name, w, h, i % 3 == 2) for i in range(n)]
    Ms = [ALL_MATS[_BATCH_ORDER[i % len(_BATCH_ORDER)]] for i in range(n)]
    got = _warp(gpu, name, frames, w, h, Ms, border)
    for i in range(n):
        assert np.array_equal(got[i], pi.warp_frame(oracle, frames[i], name, w, h, Ms[i], border)), (i, _BATCH_ORDER[i % len(_BATCH_ORDER)])


def _padded_layouts(name, w, h):
    """(source, destination) layouts, in bytes: padded pitches; a chroma pitch of its own; V before U, in and out; planes of a pool
    with gaps between them and another order on the way out."""
    _, sx, sy, nbits = FORMATS[name]
    sb = 1 if nbits == 8 else 2
    row, crow, ch = sb * w, sb * (w >> sx), h >> sy
    p1, p2 = row + 60, row + 28
    return {
        "padded_pitches": (Layout(name, w, h, pitch=p1), Layout(name, w, h, pitch=p2)),
        "unaligned": (Layout(name, w, h, pitch=row + 2, c_pitch=crow + 6, u_off=h * (row + 2) + 2), Layout(name, w, h, pitch=row + 6, c_pitch=crow + 2, u_off=h * (row + 6) + 6)),
        "chroma_pitch_of_its_own": (Layout(name, w, h, pitch=row + 124, c_pitch=crow + 158), Layout(name, w, h, pitch=p2, c_pitch=p2)),
        "v_first": (Layout(name, w, h, pitch=p1, c_pitch=crow + 30, u_off=h * p1 + ch * (crow + 30), v_off=h * p1),
                    Layout(name, w, h, u_off=h * row + ch * crow, v_off=h * row)),
        "v_first_to_u_first_apart": (Layout(name, w, h, pitch=768, c_pitch=640, u_off=768 * (h + 8) + 640 * (ch + 4), v_off=768 * (h + 8), size=768 * (h + 8) + 640 * (2 * ch + 8)),
                                     Layout(name, w, h, pitch=704, c_pitch=576, u_off=704 * (h + 16), v_off=704 * (h + 16) + 576 * (ch + 8), size=704 * (h + 16) + 576 * (2 * ch + 16))),
    }


@BORDERS
@pytest.mark.parametrize("which", ["padded_pitches", "unaligned", "chroma_pitch_of_its_own", "v_first", "v_first_to_u_first_apart"])
@FMTS
def test_warp_padded_layouts_leave_everything_else_alone(gpu, oracle, name, which, border):
    w, h, n = 258, 67, 4
    src, dst = _padded_layouts(name, w, h)[which]
    frames = [pi.random_frame(len(which) * 11 + i, name, w, h, i == 3) for i in range(n)]
    Ms = [ALL_MATS[k] for k in ("rot_2.5deg", "frac_shift", "rot_zoom_beyond_box", "small_rot")]
    got = _warp(gpu, name, frames, w, h, Ms, border, src, dst)
    for i in range(n):
        assert np.array_equal(got[i], pi.warp_frame(oracle, frames[i], name, w, h, Ms[i], border)), i


@BORDERS
@pytest.mark.parametrize("name", ["I420", "I010"])
def test_planar_operator_on_the_old_formats_is_the_old_operators(gpu, name, border):
    w, h, n = 258, 66, 5
    frames = np.stack([pi.random_frame(70 + i, name, w, h, i == 4) for i in range(n)])
    Ms = [ALL_MATS[k] for k in ("small_rot", "rot_5deg", "frac_shift", "rot_zoom_beyond_box", "saturated")]
    old = gpu.warp_affine_i420(frames, w, h, Ms, border) if name == "I420" else gpu.warp_affine_i010(frames, w, h, Ms, border)
    assert np.array_equal(gpu.warp_affine_planar(fmt_of(name), frames, w, h, Ms, border), old)
    if name == "I010":
        assert np.array_equal(gpu.warp_affine_planar(capi.FMT_I012, frames, w, h, Ms, border), old)


def test_warp_refuses_bad_geometry(gpu):
    d = capi.DevBuf(gpu, 1 << 16)
    M = np.asarray(MATS["identity"], np.float32)

    def call(fmt, w=32, h=24, sp=64, lay=(0, 0, 0), off=0, dp=64, dlay=(0, 0, 0), fb=4096):
        return gpu.lib.vs_op_warp_affine_planar(fmt, d.ptr + off, sp, *lay, d.ptr + 32768, dp, *dlay, w, h, capi._p(M, capi.f32p), 1, fb, 4096, 0, None)
    for fmt in (capi.FMT_I422, capi.FMT_I444, capi.FMT_I210, capi.FMT_I410):
        assert call(fmt) == 0
    assert call(capi.FMT_I444, w=31, h=23, sp=31, dp=33) == 0 and call(capi.FMT_I422, h=23) == 0 and call(capi.FMT_I410, w=31, h=23, sp=62) == 0
    gpu.sync()
    bad = [(capi.FMT_I422, dict(w=31)), (capi.FMT_I422, dict(sp=65)), (capi.FMT_I422, dict(lay=(0, 0, 15))), (capi.FMT_I422, dict(dlay=(0, 0, 15))),
           (capi.FMT_I444, dict(lay=(0, 0, 31))), (capi.FMT_I210, dict(w=31)), (capi.FMT_I210, dict(off=1)), (capi.FMT_I210, dict(sp=66)),
           (capi.FMT_I210, dict(dp=70)), (capi.FMT_I210, dict(lay=(0, 0, 30))), (capi.FMT_I210, dict(lay=(64 * 24 + 1, 0, 0))), (capi.FMT_I210, dict(fb=4097)),
           (capi.FMT_I410, dict(sp=65)), (capi.FMT_I410, dict(lay=(0, 0, 62))), (capi.FMT_I410, dict(dlay=(0, 64 * 50 + 1, 0))), (6, dict()), (16, dict())]
    for fmt, kw in bad:
        assert call(fmt, **kw) == 1, (fmt, kw)                     # VS_ERR_INVALID_ARG
        assert gpu.lib.vs_last_error()
    d.free()


# ---- 2. the analysis gray image ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["I210", "I212", "I410", "I412"])
@pytest.mark.parametrize("full_range", [False, True], ids=["in-range", "full-range"])
@pytest.mark.parametrize("src,dst", [((1920, 1080), (960, 540)), ((1280, 720), (960, 540)), ((322, 201), (960, 540))], ids=["half", "general", "upscale"])
def test_resize_gray(gpu, oracle, src, dst, full_range, name):
    (w, h), (dw, dh) = src, dst
    fmt, _, _, depth = FORMATS[name]
    y = np.random.default_rng(w + depth).integers(0, 65536 if full_range else 1 << depth, (h, w), np.uint16)
    want = oracle.analysis_gray(np.ascontiguousarray(ii.analysis_byte(y, depth)), dw, dh)
    assert np.array_equal(gpu.resize_gray(y, dw, dh, fmt), want)


# ---- 3. the stabilizer ---------------------------------------------------------------------------------------------------------
W, H, N = 320, 240, 24
PIPE = ["I422", "I444", "I210", "I412"]


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


@pytest.fixture(scope="module")
def clips():
    """The BGR clip of the generator, its luma bytes as NV12 frames (what the analysis of every format below sees: the chroma rows are
    not looked at) and its packed planar frames per format - real chroma, live low bits in the 10- and 12-bit forms."""
    bgr = synth.make_clip(synth.SEED_CONFIG3 + 33, W, H, N)
    nv12 = [synth.bgr_to_nv12(f) for f in bgr]
    per = {}
    for name in PIPE:
        _, sx, sy, nbits = FORMATS[name]
        per[name] = [synth.bgr_to_planar(f, sx, sy, nbits, seed=i) for i, f in enumerate(bgr)]
        assert all(np.array_equal(pi.analysis_byte(pi.planes(f, name, W, H)[0], nbits), g[:H]) for f, g in zip(per[name], nv12))
    return nv12, per


@pytest.fixture(scope="module")
def oracle_runs(oracle, clips):
    cache = {}

    def run(n, **params):
        key = (n, tuple(sorted(params.items())))
        if key not in cache:
            cache[key] = _oracle_nv12_run(oracle, clips[0][:n], **params)
        return cache[key]
    return run


def _check_debug(d, want, k):
    assert (d.n_prev, d.n_valid, d.n_detected, d.detected) == want["counts"], k
    if k > 0:
        assert np.array_equal(bits(d.transform), bits(want["transform"])), k
    if want["has"]:
        assert np.array_equal(bits(d.smoothed), bits(want["smoothed"])), k
        assert np.array_equal(bits(d.warp_matrix), bits(want["warp"])), k
        assert d.out_index == want["out_index"], k


def _check_outputs(oracle, name, got, clip, ref):
    """got: the device results in order; ref: (out_index, matrix) per result.  The last frame of the clip has no transform: it comes
    back unwarped, all three planes."""
    assert len(got) == len(ref) == len(clip)
    for k, (g, (idx, M)) in enumerate(zip(got, ref)):
        want = clip[idx] if idx == len(clip) - 1 else pi.warp_frame(oracle, clip[idx], name, W, H, M)
        assert np.array_equal(g, want), (name, k, idx)


@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_GAUSSIAN, capi.SMOOTH_KALMAN], ids=["box", "gaussian", "kalman"])
@pytest.mark.parametrize("name", PIPE)
def test_pipeline_per_frame(gpu, oracle, clips, oracle_runs, name, method):
    """The host entry points, frame by frame: every debug record against the oracle's; the results in order."""
    clip, fmt = clips[1][name], fmt_of(name)
    params = dict(smoothing_radius=8, smoothing_method=method)
    ref, dbg = oracle_runs(N, **params)
    sg = gpu.stabilizer(gpu.params(**params))
    got = []
    for k, f in enumerate(clip):
        o = sg.push(f, fmt)
        assert (o is not None) == dbg[k]["has"], k
        _check_debug(sg.debug(), dbg[k], k)
        if o is not None:
            assert o.dtype == f.dtype and o.shape == f.shape
            got.append(o)
    while True:
        o = sg.flush(clip[0], fmt)
        if o is None:
            break
        got.append(o)
    ow, oh = C.c_int32(), C.c_int32()
    gpu.check(gpu.lib.vs_stab_last_out_dims(sg.h, C.byref(ow), C.byref(oh)), sg.h)
    assert (ow.value, oh.value) == (W, H)
    sg.close()
    _check_outputs(oracle, name, got, clip, ref)


def _batch_run(gpu, name, clip, batch, params, zero_copy=True, src=None, dst=None, push_n=0):
    """The clip through push_dev (push_n > 0: push_dev_n, that many frames a call) with set_batch(batch), drained through flush_dev;
    the results as packed frames and the last debug record."""
    n, fmt = len(clip), fmt_of(name)
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(batch)
    s.set_zero_copy(zero_copy)
    src, dst = src or Layout(name, W, H), dst or Layout(name, W, H)
    if any(src.args) or any(dst.args):
        s.set_i420_layout(*src.args, *dst.args)
    d_in, d_out = capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in clip])), capi.DevBuf.from_array(gpu, dst.blank(n))
    isz, osz, ip, op = src.size, dst.size, src.pitch, dst.pitch
    try:
        k = 0
        for i in range(0, n, push_n or 1):
            if push_n:
                m = min(push_n, n - i)
                k += s.push_dev_n([d_in.ptr + (i + j) * isz for j in range(m)], W, H, ip, fmt, [d_out.ptr + (k + j) * osz for j in range(m)], op)
            else:
                k += s.push_dev(d_in.ptr + i * isz, W, H, ip, fmt, d_out.ptr + k * osz, op)
        s.sync()
        last = s.debug()
        last = dict(transform=np.array(last.transform), smoothed=np.array(last.smoothed), warp=np.array(last.warp_matrix))
        while s.flush_dev(d_out.ptr + k * osz, op):
            k += 1
        s.sync()
        out = d_out.download((n, osz // dst.sb), dst.dtype)
    finally:
        s.close(); d_in.free(); d_out.free()
    return [dst.unpack(out[i]) for i in range(k)], last


def _same_last(last, want):
    for k in ("transform", "smoothed", "warp"):
        assert np.array_equal(bits(last[k]), bits(want[k])), k


@pytest.mark.parametrize("method", [capi.SMOOTH_BOX, capi.SMOOTH_KALMAN], ids=["box", "kalman"])
@pytest.mark.parametrize("name", PIPE)
def test_pipeline_batch_mode_with_partial_batches(gpu, oracle, clips, oracle_runs, name, method):
    """22 frames in batches of 8: two whole steps and one of six frames (box: the release kernel builds the tables; kalman: the
    one-kernel tail)."""
    clip = clips[1][name][:22]
    params = dict(smoothing_radius=6, smoothing_method=method)
    ref, dbg = oracle_runs(22, **params)
    got, last = _batch_run(gpu, name, clip, 8, params)
    _same_last(last, dbg[-1])
    _check_outputs(oracle, name, got, clip, ref)


@pytest.mark.parametrize("name", ["I422", "I412"])
def test_pipeline_push_dev_n(gpu, oracle, clips, oracle_runs, name):
    clip = clips[1][name]
    params = dict(smoothing_radius=6)
    ref, dbg = oracle_runs(N, **params)
    got, last = _batch_run(gpu, name, clip, 8, params, push_n=5)
    _same_last(last, dbg[-1])
    _check_outputs(oracle, name, got, clip, ref)


def _pipe_layouts(name, which):
    _, sx, sy, nbits = FORMATS[name]
    sb = 1 if nbits == 8 else 2
    row, crow, ch = sb * W, sb * (W >> sx), H >> sy
    return {
        "chroma_pitch_of_its_own": (Layout(name, W, H, pitch=row + 124, c_pitch=crow + 158), Layout(name, W, H, pitch=row + 28, c_pitch=row + 28)),
        "v_first_to_u_first_apart": (Layout(name, W, H, pitch=768, c_pitch=704, u_off=768 * (H + 8) + 704 * (ch + 4), v_off=768 * (H + 8), size=768 * (H + 8) + 704 * (2 * ch + 8)),
                                     Layout(name, W, H, pitch=704, c_pitch=640, u_off=704 * (H + 16), v_off=704 * (H + 16) + 640 * (ch + 8), size=704 * (H + 16) + 640 * (2 * ch + 16))),
    }[which]


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero-copy", "copy-in"])
@pytest.mark.parametrize("which", ["chroma_pitch_of_its_own", "v_first_to_u_first_apart"])
@pytest.mark.parametrize("name", ["I422", "I444", "I210", "I412"])
def test_pipeline_with_different_input_and_output_layouts(gpu, oracle, clips, oracle_runs, name, which, zero_copy):
    clip = clips[1][name][:22]
    params = dict(smoothing_radius=6)
    ref, _ = oracle_runs(22, **params)
    src, dst = _pipe_layouts(name, which)
    got, _ = _batch_run(gpu, name, clip, 8, params, zero_copy, src, dst)
    _check_outputs(oracle, name, got, clip, ref)


@pytest.mark.parametrize("name", ["I444", "I210"])
def test_pipeline_host_entry_points_in_batch_mode(gpu, oracle, clips, oracle_runs, name):
    clip, fmt = clips[1][name][:22], fmt_of(name)
    params = dict(smoothing_radius=6)
    ref, _ = oracle_runs(22, **params)
    s = gpu.stabilizer(gpu.params(**params))
    s.set_batch(8)
    got = [o for o in (s.push(f, fmt) for f in clip) if o is not None]
    while True:
        o = s.flush(clip[0], fmt)
        if o is None:
            break
        got.append(o)
    s.close()
    _check_outputs(oracle, name, got, clip, ref)


@pytest.mark.parametrize("name", ["I422", "I210"])
def test_vs_batch_of_three_streams_against_standalone_instances(gpu, oracle, clips, name):
    n, S, fmt = 22, 3, fmt_of(name)
    params = dict(smoothing_radius=6)
    src, dst = _pipe_layouts(name, "chroma_pitch_of_its_own")
    _, sx, sy, nbits = FORMATS[name]

    def rolled(f, g):                                   # every plane shifted along its rows: another picture, the same layout
        return synth.yuv_pack(*[np.roll(p, (2 * g, g)[i > 0], axis=1) for i, p in enumerate(pi.planes(f, name, W, H))], sx, sy)
    cl = [[rolled(f, g) for f in clips[1][name][:n]] for g in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, np.stack([src.pack(f) for f in c])) for c in cl]
    d_out = [capi.DevBuf.from_array(gpu, dst.blank(n)) for _ in range(S)]
    b = gpu.batch(gpu.params(**params), S, 8)
    b.set_zero_copy(True)
    b.set_i420_layout(*src.args, *dst.args)
    k = [0] * S
    for i in range(n):
        prod = b.push_dev([d_in[g].ptr + i * src.size for g in range(S)], W, H, src.pitch, fmt, [d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
    while True:
        prod = b.flush_dev([d_out[g].ptr + k[g] * dst.size for g in range(S)], dst.pitch)
        k = [k[g] + prod[g] for g in range(S)]
        if not any(prod):
            break
    b.sync()
    b.close()
    for g in range(S):
        raw = d_out[g].download((n, dst.size // dst.sb), dst.dtype)
        got = [dst.unpack(raw[i]) for i in range(k[g])]
        alone, _ = _batch_run(gpu, name, cl[g], 8, params, True, src, dst)
        assert len(got) == len(alone) == n
        for a, c in zip(got, alone):
            assert np.array_equal(a, c), g
        # an NV12 frame per input: the analysis bytes as luma (the chroma rows are not looked at)
        nv = [np.vstack([pi.analysis_byte(pi.planes(f, name, W, H)[0], nbits), np.full((H // 2, W), 128, np.uint8)]) for f in cl[g]]
        ref, _ = _oracle_nv12_run(oracle, nv, **params)
        _check_outputs(oracle, name, got, cl[g], ref)
    for d in d_in + d_out:
        d.free()


def test_vs_batch_refuses_members_that_disagree(gpu):
    """A layout change while one member has a frame queued reaches the members in front of it only (VS_ERR_INVALID_ARG); the next
    step finds members with different layouts and refuses them.  So it does members of different formats."""
    w, h = 64, 48
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    b = gpu.batch(gpu.params(smoothing_radius=5), 2, 4)
    b.set_zero_copy(True)
    assert b.push_dev([None, d_in.ptr], w, h, 2 * w, capi.FMT_I210, [None, d_out.ptr], 2 * w) == [0, 0]
    with pytest.raises(capi.VsError, match="queue must be empty"):
        b.set_i420_layout(0, 0, 128, 0, 0, 0)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        for _ in range(8):
            b.push_dev([d_in.ptr, d_in.ptr], w, h, 2 * w, capi.FMT_I210, [d_out.ptr, d_out.ptr + (1 << 19)], 2 * w)
    b.close()
    # two members that each start fresh, one with I210 frames and one with I212 frames (the same bytes, another analysis shift): the
    # step that finds both queued compares the members' formats and refuses them
    b = gpu.batch(gpu.params(smoothing_radius=5), 2, 4)
    b.set_zero_copy(True)
    with pytest.raises(capi.VsError, match="share one frame geometry"):
        for _ in range(8):
            b.push_dev([d_in.ptr, None], w, h, 2 * w, capi.FMT_I210, [d_out.ptr, None], 2 * w)
            b.push_dev([None, d_in.ptr], w, h, 2 * w, capi.FMT_I212, [None, d_out.ptr + (1 << 19)], 2 * w)
    b.close(); d_in.free(); d_out.free()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def _push_status(gpu, params, fmt, w, h, pitch, out_pitch=None, ptr_off=0, batch=1, layout=None):
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
@FMTS
def test_refusals(gpu, name, batch):
    INVALID, UNSUPPORTED = 1, 4
    fmt, sx, sy, nbits = FORMATS[name]
    sb = 1 if nbits == 8 else 2
    ok = dict(smoothing_radius=5)
    p = 64 * sb
    crow = (64 >> sx) * sb
    assert _push_status(gpu, ok, fmt, 64, 48, p, batch=batch)[0] == 0
    assert _push_status(gpu, ok, fmt, 64, 47, p, batch=batch)[0] == 0                              # an odd h is fine
    assert _push_status(gpu, ok, fmt, 64, 48, p + 2, batch=batch, layout=(0, 0, crow, 0, 0, crow + 2))[0] == 0
    bad = [dict(w=64, h=48, pitch=p, layout=(0, 0, crow - sb, 0, 0, 0)), dict(w=64, h=48, pitch=p, layout=(0, 0, 0, 0, 0, crow - sb))]   # a chroma pitch that is too small
    if sx:
        bad += [dict(w=63, h=48, pitch=p)]                                                       # an odd w for 4:2:2
    else:
        assert _push_status(gpu, ok, fmt, 63, 47, p, batch=batch)[0] == 0
    if sb == 2:                                                                                  # an odd pitch, output pitch, pointer, offset
        bad += [dict(w=64, h=48, pitch=p + 1), dict(w=64, h=48, pitch=p, out_pitch=p + 3), dict(w=64, h=48, pitch=p, ptr_off=1),
                dict(w=64, h=48, pitch=p, layout=(p * 48 + 1, 0, 0, 0, 0, 0)), dict(w=64, h=48, pitch=p, layout=(0, 0, 0, 0, p * 60 + 1, 0))]
        if sx:                                                                                   # a default chroma pitch of odd bytes
            bad += [dict(w=64, h=48, pitch=p + 2), dict(w=64, h=48, pitch=p, out_pitch=p + 6)]
    elif sx:
        bad += [dict(w=64, h=48, pitch=p + 1), dict(w=64, h=48, pitch=p, out_pitch=p + 3)]
    for kw in bad:
        rc, msg = _push_status(gpu, ok, fmt, batch=batch, **kw)
        assert rc == INVALID and name in msg, (kw, rc, msg)
    for extra in (dict(border_size=8), dict(border_size=8, crop_n_zoom=1), dict(border_size=8, border_type=capi.BORDER_FADE), dict(enable_virtual_canvas=1)):
        rc, msg = _push_status(gpu, dict(smoothing_radius=5, **extra), fmt, 64, 48, p, batch=batch)
        assert rc == UNSUPPORTED and name in msg, (extra, rc, msg)


@pytest.mark.parametrize("batch", [1, 8])
def test_layout_change_with_frames_queued_is_refused(gpu, batch):
    s = gpu.stabilizer(gpu.params(smoothing_radius=5))
    s.set_batch(batch)
    d_in, d_out = capi.DevBuf(gpu, 1 << 20), capi.DevBuf(gpu, 1 << 20)
    d_in.zero()
    assert s.push_dev(d_in.ptr, 64, 48, 128, capi.FMT_I210, d_out.ptr, 128) == 0
    with pytest.raises(capi.VsError, match="queue must be empty"):
        s.set_i420_layout(0, 0, 128, 0, 0, 0)
    s.sync()
    while s.flush_dev(d_out.ptr, 128):
        pass
    s.sync()
    with pytest.raises(capi.VsError, match="I210"):
        s.set_i420_layout(0, 0, 62, 0, 0, 0)                 # now the queue is empty and the geometry known: the pitch is too small
    s.set_i420_layout(0, 0, 128, 0, 0, 0)
    s.close(); d_in.free(); d_out.free()


# ---- 5. a real tile count ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("I422", 6), ("I210", 2)])
def test_warp_1080p_batch(gpu, oracle, name, n):
    """1080p: 15 x 17 (16-bit: 15 x 34) tiles of Y and 2 x 8 x 17 (34) chroma tiles per surface in the XCD-aware order.  At 2.5
    degrees the seven full-width chroma tiles of every tile row go direct while Y is staged."""
    w, h = 1920, 1080
    frames = [pi.random_frame(w + i, name, w, h) for i in range(n)]
    Ms = [ALL_MATS[k] for k in ("rot_2.5deg", "small_rot", "rot_1.5deg", "rot_5deg", "frac_shift", "rot_zoom_beyond_box")][:n]
    got = _warp(gpu, name, frames, w, h, Ms)
    for i in range(n):
        assert np.array_equal(got[i], pi.warp_frame(oracle, frames[i], name, w, h, Ms[i])), i
