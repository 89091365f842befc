"""Asynchronous roll correction and auto zoom/crop on interleaved colour frames (BGR8, RGB8, BGRA8, RGBA8), bit for bit.

The reference is tests/rgb_chain_inputs.py (angle, state and info8 from the oracle's BGR operators on the frame's BGR permutation, the
pixels of every channel through ref16_geom.warp; pinned to the oracle by tests/test_rgb_chain_cpu.py).  Every frame and every result
is a region of a larger surface (tests/roi.py): padded and odd strides, first bytes at +1, +2, +3, and every byte outside a result -
the part of a result buffer that a smaller outcome leaves alone included - is compared with its prefill."""
import ctypes as C

import numpy as np
import pytest

import azc_size_inputs as sizes
import ref16_geom as geom
import rgb_chain_inputs as inputs
import roi
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID = 1
LAYOUTS = ["packed", "padded16", "roi_off1", "roi_off2", "roi_off3", "odd_pitch", "mixed"]
FMT_IDS = [inputs.FMT_NAMES[f] for f in inputs.FORMATS]


def _pair(gpu, layout, key, frames, out_w, out_h):
    """The frames as ROIs of one source allocation and a destination of out_w x out_h ROIs, both on the device."""
    n = len(frames)
    h, w, cn = frames[0].shape
    src, dst = roi.pair(layout, roi.case_seed("rgb_chain", *key), (w, h, cn, n), (out_w, out_h, cn, n))
    src.put(np.stack(frames)).bind(gpu)
    dst.bind(gpu)
    return src, dst


def _results(src, dst, shapes):
    """The destination's ROIs after the calls: per frame its (oh, ow) part; asserts that nothing else changed - outside the ROIs, in
    the rest of each ROI, and in the source."""
    n, cn = dst.frames, dst.px
    got, clean = dst.result((n, dst.rows, dst.w, cn))
    assert clean, dst.stray()
    before = np.ascontiguousarray(dst._view(dst.host)).reshape(got.shape)
    out = []
    for i, (oh, ow) in enumerate(shapes):
        rest = np.ones(got.shape[1:3], bool)
        rest[:oh, :ow] = False
        assert np.array_equal(got[i][rest], before[i][rest]), ("bytes of the result buffer beyond the result were written", i)
        out.append(got[i, :oh, :ow].copy())
    assert src.untouched(), "the source was written"
    src.free()
    dst.free()
    return out


# ---- 1. roll ---------------------------------------------------------------------------------------------------------------------
def _roll_run(gpu, frames, fmt, thr, layout, key, array_form):
    n = len(frames)
    h, w, cn = frames[0].shape
    src, dst = _pair(gpu, layout, key, frames, w, h)
    ins, outs = [src.frame_ptr(i) for i in range(n)], [dst.frame_ptr(i) for i in range(n)]
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    try:
        if array_form:
            rg.correct_rgb_dev_n(fmt, ins, w, h, src.pitch, outs, dst.pitch)
        else:       # single calls between array calls: 2 + 4 + 1 + the rest
            for a, b in ((0, 2), (2, 6), (6, 7), (7, n)):
                if b - a <= 2:
                    for i in range(a, b):
                        rg.correct_rgb_dev(fmt, ins[i], w, h, src.pitch, outs[i], dst.pitch)
                else:
                    rg.correct_rgb_dev_n(fmt, ins[a:b], w, h, src.pitch, outs[a:b], dst.pitch)
        rg.sync()
        state = rg.state()
    finally:
        rg.close()
    return _results(src, dst, [(h, w)] * n), state


@pytest.mark.parametrize("case", range(len(inputs.ROLL_CASES)), ids=["640x360", "322x242"])
@pytest.mark.parametrize("fmt", inputs.FORMATS, ids=FMT_IDS)
def test_roll_correct_rgb_matches_the_reference(gpu, oracle, fmt, case):
    """Eleven frames (8 + 3, the flat one in the middle): every channel of every result, the angle bits and the line counts after
    sync; the array form and single calls mixed with it; two surface layouts per case."""
    size, slope, _ = inputs.ROLL_CASES[case]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    frames = inputs.roll_frames(size, slope, fmt)
    refs, states = inputs.roll_refs(oracle, size, slope, fmt)
    k = 2 * (inputs.FORMATS.index(fmt) * 2 + case)
    for j, array_form in enumerate((True, False)):
        layout = LAYOUTS[(k + j) % len(LAYOUTS)]
        got, state = _roll_run(gpu, frames, fmt, thr, layout, (fmt, case, j), array_form)
        assert state == states[-1] and state[0] != 0.0, (layout, state, states[-1])
        assert np.float64(state[0]).view(np.uint64) == np.float64(states[-1][0]).view(np.uint64)
        for i in range(len(frames)):
            assert np.array_equal(got[i], refs[i]), (layout, array_form, i)


@pytest.mark.parametrize("case", range(len(inputs.ROLL_CASES)), ids=["640x360", "322x242"])
def test_roll_correct_rgb_bgr8_equals_the_synchronous_call(gpu, case):
    size, slope, _ = inputs.ROLL_CASES[case]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    frames = inputs.roll_frames(size, slope, inputs.BGR8)
    got, state = _roll_run(gpu, frames, inputs.BGR8, thr, "padded16", ("sync", case), True)
    rs = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    d_in, d_out = capi.DevBuf(gpu, w * h * 3), capi.DevBuf(gpu, w * h * 3)
    try:
        for i, f in enumerate(frames):
            d_in.upload(f)
            rs.correct_dev(d_in.ptr, w, h, w * 3, d_out.ptr, w * 3)
            rs.sync()
            assert np.array_equal(d_out.download((h, w, 3), np.uint8), got[i]), i
        assert rs.state() == state
    finally:
        rs.close()
        d_in.free()
        d_out.free()


# ---- 2. zoom ---------------------------------------------------------------------------------------------------------------------
def _zoom_run(gpu, frames, fmt, out_size, layout, key):
    """Thirteen frames through one zoom object: five single calls, then the array form.  Returns per frame (ow, oh, info8, pixels)."""
    n = len(frames)
    h, w, cn = frames[0].shape
    ow, oh = sizes.resolved(tuple(out_size), w, h)
    src, dst = _pair(gpu, layout, key, frames, max(w, ow), max(h, oh))
    ins, outs = [src.frame_ptr(i) for i in range(n)], [dst.frame_ptr(i) for i in range(n)]
    az = gpu.auto_zoom_crop()
    try:
        az.set_output_size(*out_size)
        tickets = [az.apply_rgb_dev(fmt, ins[i], w, h, src.pitch, outs[i], dst.pitch) for i in range(5)]
        tickets += az.apply_rgb_dev_n(fmt, ins[5:], w, h, src.pitch, outs[5:], dst.pitch)
        assert tickets == list(range(n))
        az.sync()
        res = [az.result(t) for t in tickets]
        wt = az.worker_times()
    finally:
        az.close()
    px = _results(src, dst, [(r[1], r[0]) for r in res])
    assert wt[0] == n and wt[5] == 2                         # two batches: 8 + 5
    return [(r[0], r[1], r[2].tolist(), p) for r, p in zip(res, px)]


@pytest.mark.parametrize("out_size", inputs.OUT_SIZES, ids=lambda s: "out_%dx%d" % s)
@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", inputs.FORMATS, ids=FMT_IDS)
def test_auto_zoom_crop_rgb_matches_the_reference(gpu, oracle, fmt, size, out_size):
    """Every ticket's out_w, out_h, info8 and bytes; the fall-back frames (no contour; empty crop) come back whole, fourth channel
    included."""
    w, h = size
    frames = inputs.zoom_frames(oracle, size, fmt)
    refs = inputs.zoom_refs(oracle, size, fmt, out_size)
    case = (inputs.FORMATS.index(fmt) * 3 + inputs.ZOOM_SIZES.index(size)) * 3 + inputs.OUT_SIZES.index(out_size)
    layout = LAYOUTS[case % len(LAYOUTS)]
    got = _zoom_run(gpu, frames, fmt, out_size, layout, (fmt, size, out_size))
    whole = 0
    for i, ((ow, oh, info, px), (want, winfo)) in enumerate(zip(got, refs)):
        assert info == winfo.tolist(), (layout, i)
        assert (ow, oh) == (sizes.resolved(tuple(out_size), w, h) if winfo[7] else (w, h)), (layout, i)
        assert px.shape == want.shape and np.array_equal(px, want), (layout, i)
        if not winfo[7]:
            assert np.array_equal(px, frames[i])
            whole += 1
    assert whole >= 2


# ---- 3. vs_op_scale_jobs_rgb -----------------------------------------------------------------------------------------------------
def _stride_of(row_bytes, variant, cn):
    """0: a multiple of 48 (of 12 and of 16) with slack; 1: row bytes + 5 or + 6, no multiple of 4; 2: a multiple of 4 that is no
    multiple of 4 * cn."""
    if variant == 0:
        return (row_bytes + 47) // 48 * 48 + 48
    if variant == 1:
        return row_bytes + 5 if (row_bytes + 5) % 4 else row_bytes + 6
    s = (row_bytes + 3) // 4 * 4 + 4
    return s if s % (4 * cn) else s + 4


def _place(items, cn, seed):
    """items: [(row_bytes, rows, base residue mod 4, stride variant)] -> (prefilled host bytes, [(offset, stride)]): every item on a
    64-byte boundary plus its residue, 64 random bytes at least between two of them."""
    where, off = [], 64
    for rb, rows, res, var in items:
        stride = _stride_of(rb, var, cn)
        off = (off + 63) // 64 * 64 + res
        where.append((off, stride))
        off += stride * rows + 64
    host = np.random.default_rng(seed).integers(1, 256, off + 64, dtype=np.uint8)
    return host, where


@pytest.mark.parametrize("path", [0, 1], ids=["staged_and_direct", "all_direct"])
@pytest.mark.parametrize("cn", [3, 4])
def test_scale_jobs_rgb_matches_the_reference(gpu, cn, path):
    """The 24 jobs of azc_size_inputs.OP_CASES in one call: source bases at every residue mod 4 and strides that are and are not
    multiples of 12 / 16, in every combination; the rows around a crop are random non-zero bytes (a tap outside the crop is 0)."""
    cases = sizes.OP_CASES
    assert gpu.scale_jobs_rgb_plan([(4096, sw * cn, sw, sh, 8192, dw * cn, dw, dh, cn) for (sw, sh), (dw, dh) in cases]).tolist() == sizes.OP_STAGED
    crops = [sizes.random_plane(c, cn, np.uint8, 100 * cn + i) for i, (c, _) in enumerate(cases)]
    refs = sizes.cache("rgb_op").setdefault(cn, [sizes.reference(crop, d) for crop, (_, d) in zip(crops, cases)])
    src_host, src_at = _place([(sw * cn, sh, i % 4, i % 3) for i, ((sw, sh), _) in enumerate(cases)], cn, 7 + cn)
    dst_host, dst_at = _place([(dw * cn, dh, (i + 1) % 4, (i + 2) % 3) for i, (_, (dw, dh)) in enumerate(cases)], cn, 9 + cn)
    assert {(o % 4, s % (4 * cn) == 0, s % 4 == 0) for o, s in src_at} >= {(r, a, b) for r in range(4) for a, b in ((True, True), (False, True), (False, False))}
    roi_mask = np.zeros(dst_host.size, bool)
    for crop, ((sw, sh), (dw, dh)), (so, ss), (do, ds) in zip(crops, cases, src_at, dst_at):
        for y in range(sh):
            src_host[so + y * ss:so + y * ss + sw * cn] = crop[y].reshape(-1)
        for y in range(dh):
            roi_mask[do + y * ds:do + y * ds + dw * cn] = True
    d_src, d_dst = capi.DevBuf.from_array(gpu, src_host), capi.DevBuf.from_array(gpu, dst_host)
    try:
        gpu.scale_jobs_rgb([(d_src.ptr + so, ss, sw, sh, d_dst.ptr + do, ds, dw, dh, cn)
                            for ((sw, sh), (dw, dh)), (so, ss), (do, ds) in zip(cases, src_at, dst_at)], path=path)
        gpu.sync()
        after = d_dst.download((dst_host.size,), np.uint8)
    finally:
        d_src.free()
        d_dst.free()
    assert np.array_equal(after[~roi_mask], dst_host[~roi_mask]), "bytes outside the destinations were written"
    for i, ((_, (dw, dh)), (do, ds), want) in enumerate(zip(cases, dst_at, refs)):
        got = np.stack([after[do + y * ds:do + y * ds + dw * cn] for y in range(dh)]).reshape(dh, dw, cn)
        assert np.array_equal(got, want), (i, cases[i], path)


# ---- 4. one object, three kinds of frame -------------------------------------------------------------------------------------------
def _kind(i, n):
    return inputs.BGRA8 if i < n // 3 else capi.FMT_NV12 if i < 2 * n // 3 + 1 else inputs.RGB8


def test_roll_object_takes_bgra_nv12_and_rgb8_without_a_sync(gpu, oracle):
    """BGRA8, then NV12, then RGB8 frames of one scene: each change closes the pending batch, the angle carries across - its sequence is
    the oracle's over the whole sequence - and every result is complete and correct."""
    size, slope, _ = inputs.ROLL_CASES[1]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    bgr = inputs.roll_bgr(size, slope)
    n = len(bgr)
    ro = oracle.roll_correction(oracle.roll_params(hough_threshold=thr))
    frames, want = [], []
    for i, f in enumerate(bgr):
        k = _kind(i, n)
        if k == capi.FMT_NV12:
            frames.append(synth.bgr_to_nv12(f))
            want.append(ro.correct_nv12(frames[-1], w, h))
        else:
            frames.append(inputs.pack(f, inputs.alpha_plane(h, w, 50 + i), k))
            want.append(inputs.roll_ref([frames[-1]], k, ro)[0][0])
    state = ro.state()
    ro.close()
    d_in = [capi.DevBuf.from_array(gpu, f) for f in frames]
    d_out = [capi.DevBuf.from_array(gpu, np.full(f.shape, 0xA5, np.uint8)) for f in frames]
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    try:
        for i in range(n):
            k = _kind(i, n)
            if k == capi.FMT_NV12:
                rg.correct_nv12_dev(d_in[i].ptr, w, h, w, d_out[i].ptr, w)
            else:
                rg.correct_rgb_dev(k, d_in[i].ptr, w, h, w * inputs.CN[k], d_out[i].ptr, w * inputs.CN[k])
        rg.sync()
        assert rg.state() == state and state[0] != 0.0
        for i in range(n):
            assert np.array_equal(d_out[i].download(frames[i].shape, np.uint8), want[i]), (i, _kind(i, n))
    finally:
        rg.close()
        for d in d_in + d_out:
            d.free()


def test_zoom_object_takes_bgra_nv12_and_rgb8_without_a_sync(gpu, oracle):
    size = inputs.ZOOM_SIZES[2]
    w, h = size
    bgr = inputs.zoom_bgr(oracle, size)
    n = len(bgr)
    W, H = max(w, 640), max(h, 360)
    frames, want = [], []
    for i, f in enumerate(bgr):
        k = _kind(i, n)
        if k == capi.FMT_NV12:
            frames.append(synth.bgr_to_nv12(f))
            want.append(oracle.auto_zoom_crop_nv12(frames[-1], w, h))
        else:
            frames.append(inputs.pack(f, inputs.alpha_plane(h, w, 70 + i), k))
            want.append(inputs.azc_ref(frames[-1], k, oracle))
    d_in = [capi.DevBuf.from_array(gpu, f) for f in frames]
    d_out = [capi.DevBuf.from_array(gpu, np.full(W * H * 4, 0xA5, np.uint8)) for _ in frames]
    az = gpu.auto_zoom_crop()
    try:
        tickets = []
        for i in range(n):
            k = _kind(i, n)
            if k == capi.FMT_NV12:
                tickets.append(az.apply_nv12_dev(d_in[i].ptr, w, h, w, d_out[i].ptr, W, W * H))
            else:
                tickets.append(az.apply_rgb_dev(k, d_in[i].ptr, w, h, w * inputs.CN[k], d_out[i].ptr, W * inputs.CN[k]))
        az.sync()
        assert az.worker_times()[5] == 3                    # a batch per kind
        for i, t in enumerate(tickets):
            k = _kind(i, n)
            ow, oh, info = az.result(t)
            ref, winfo = want[i]
            assert info.tolist() == winfo.tolist() and (ow, oh) == ((640, 360) if winfo[7] else (w, h)), (i, k)
            if k == capi.FMT_NV12:
                g = d_out[i].download((H * 3 // 2, W), np.uint8)
                got = np.concatenate([g[:oh, :ow], g[H:H + oh // 2, :ow]])
            else:
                cn = inputs.CN[k]
                got = d_out[i].download((H, W, cn), np.uint8)[:oh, :ow]
            assert got.shape == ref.shape and np.array_equal(got, ref), (i, k)
    finally:
        az.close()
        for d in d_in + d_out:
            d.free()


# ---- 5. the chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [inputs.BGR8, inputs.BGRA8], ids=["BGR8", "BGRA8"])
def test_rgb_chain_equals_the_oracle_chain(gpu, oracle, fmt):
    """704 x 400, 24 frames: roll (array form) -> stabilizer (batch 8, push_dev_n, the same fmt) -> zoom (array form), against the
    oracle's roll, the oracle's stabilizer on the BGR permutation (a fourth channel: the oracle's warp of that plane by the frame's
    matrix; the clip's last frame comes back unwarped) and the zoom reference."""
    from test_gpu_pixfmt import _oracle_run
    W, H = inputs.CHAIN_SIZE
    N, CH = 24, 8
    cn = inputs.CN[fmt]
    params = dict(smoothing_radius=5, max_corners=400)
    frames = inputs.chain_frames(N, fmt)
    ro = oracle.roll_correction()
    rolled, states = inputs.roll_ref(frames, fmt, ro)
    ro.close()
    outs, _ = _oracle_run(oracle, [inputs.unpack(r, fmt)[0] for r in rolled], **params)
    want = []
    for o, idx, M in outs:
        a = None
        if cn == 4:
            a = rolled[idx][..., 3] if idx == N - 1 else oracle.warp_affine(np.ascontiguousarray(rolled[idx][..., 3]), M)
        want.append(inputs.azc_ref(inputs.pack(o, a, fmt), fmt, oracle))
    assert len(want) == N and states[-1][0] != 0.0 and any(i[7] for _, i in want)

    fb, pitch = W * H * cn, W * cn
    d_in, d_roll = capi.DevBuf.from_array(gpu, np.stack(frames)), capi.DevBuf(gpu, fb * N)
    d_stab, d_zoom = capi.DevBuf(gpu, fb * N), capi.DevBuf.from_array(gpu, np.full(fb * N, 0xA5, np.uint8))
    rc, st, az = gpu.roll_correction(), gpu.stabilizer(gpu.params(**params)), gpu.auto_zoom_crop()
    try:
        rc.correct_rgb_dev_n(fmt, [d_in.ptr + i * fb for i in range(N)], W, H, pitch, [d_roll.ptr + i * fb for i in range(N)], pitch)
        rc.sync()
        assert rc.state() == states[-1]
        st.set_batch(CH)
        k = 0
        for c in range(N // CH):
            k += st.push_dev_n([d_roll.ptr + (c * CH + i) * fb for i in range(CH)], W, H, pitch, fmt, [d_stab.ptr + (k + j) * fb for j in range(CH)], pitch)
        while k < N and st.flush_dev(d_stab.ptr + k * fb, pitch):
            k += 1
        st.sync()
        assert k == N
        tickets = az.apply_rgb_dev_n(fmt, [d_stab.ptr + i * fb for i in range(N)], W, H, pitch, [d_zoom.ptr + i * fb for i in range(N)], pitch)
        az.sync()
        for i, t in enumerate(tickets):
            ow, oh, info = az.result(t)
            ref, winfo = want[i]
            assert info.tolist() == winfo.tolist() and (ow, oh) == ((640, 360) if winfo[7] else (W, H)), i
            got = d_zoom.download((H, W, cn), np.uint8, i * fb)[:oh, :ow]
            assert got.shape == ref.shape and np.array_equal(got, ref), i
    finally:
        for o in (rc, st, az):
            o.close()
        for d in (d_in, d_roll, d_stab, d_zoom):
            d.free()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def _names_the_formats(text, call):
    return call in text and all(n in text for n in ("VS_FMT_BGR8", "VS_FMT_RGB8", "VS_FMT_BGRA8", "VS_FMT_RGBA8"))


def test_refusals_on_live_objects_and_the_objects_still_work(gpu, oracle):
    size, slope, _ = inputs.ROLL_CASES[1]
    w, h = size
    frame = inputs.roll_frames(size, slope, inputs.BGRA8)[0]
    d_in = capi.DevBuf.from_array(gpu, frame)
    d_out = capi.DevBuf.from_array(gpu, np.full(640 * 360 * 4, 0x5A, np.uint8))
    rg, az = gpu.roll_correction(gpu.roll_params(hough_threshold=inputs.roll_hough_threshold(w))), gpu.auto_zoom_crop()
    L = gpu.lib
    pin, pout = C.c_void_p(d_in.ptr), C.c_void_p(d_out.ptr)
    lin, lout = (C.c_void_p * 1)(d_in.ptr), (C.c_void_p * 1)(d_out.ptr)
    t = C.c_int64(-1)
    bad_fmts = [capi.FMT_GRAY8, capi.FMT_NV12, capi.FMT_P010, capi.FMT_I420, capi.FMT_I444, capi.FMT_I412, -1, 99]
    try:
        roll_calls = [lambda f=f: L.vs_roll_correct_rgb_dev(rg.h, f, pin, w, h, w * 4, pout, w * 4) for f in bad_fmts]
        roll_calls += [lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGRA8, pin, w, h, w * 4 - 1, pout, w * 4),
                       lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGRA8, pin, w, h, w * 4, pout, w * 4 - 1),
                       lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGR8, pin, w, h, w * 3 - 1, pout, w * 3),
                       lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGRA8, None, w, h, w * 4, pout, w * 4),
                       lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGRA8, pin, w, h, w * 4, None, w * 4),
                       lambda: L.vs_roll_correct_rgb_dev(rg.h, inputs.BGRA8, pin, 0, h, w * 4, pout, w * 4)]
        for i, call in enumerate(roll_calls):
            assert call() == INVALID, i
            assert _names_the_formats(L.vs_roll_last_error(rg.h).decode(), "vs_roll_correct_rgb_dev"), i
        for args in ((lin, lout, 0), (lin, lout, -1), (None, lout, 1), (lin, None, 1)):
            assert L.vs_roll_correct_rgb_dev_n(rg.h, inputs.BGRA8, args[0], args[1], args[2], w, h, w * 4, w * 4) == INVALID, args[2]
            assert _names_the_formats(L.vs_roll_last_error(rg.h).decode(), "vs_roll_correct_rgb_dev_n")
        assert L.vs_roll_correct_rgb_dev_n(rg.h, capi.FMT_NV12, lin, lout, 1, w, h, w * 4, w * 4) == INVALID

        zoom_calls = [lambda f=f: L.vs_azc_apply_rgb_dev(az.h, f, pin, w, h, w * 4, pout, 640 * 4, C.byref(t)) for f in bad_fmts]
        zoom_calls += [lambda: L.vs_azc_apply_rgb_dev(az.h, inputs.BGRA8, pin, w, h, w * 4 - 1, pout, 640 * 4, C.byref(t)),
                       lambda: L.vs_azc_apply_rgb_dev(az.h, inputs.BGRA8, pin, w, h, w * 4, pout, 640 * 4 - 1, C.byref(t)),
                       lambda: L.vs_azc_apply_rgb_dev(az.h, inputs.BGRA8, None, w, h, w * 4, pout, 640 * 4, C.byref(t)),
                       lambda: L.vs_azc_apply_rgb_dev(az.h, inputs.BGRA8, pin, w, h, w * 4, None, 640 * 4, C.byref(t)),
                       lambda: L.vs_azc_apply_rgb_dev(az.h, inputs.BGRA8, pin, w, 0, w * 4, pout, 640 * 4, C.byref(t))]
        for i, call in enumerate(zoom_calls):
            assert call() == INVALID and t.value == -1, i
            assert _names_the_formats(L.vs_azc_last_error(az.h).decode(), "vs_azc_apply_rgb_dev"), i
        for args in ((lin, lout, 0), (None, lout, 1), (lin, None, 1)):
            assert L.vs_azc_apply_rgb_dev_n(az.h, inputs.BGRA8, args[0], args[1], args[2], w, h, w * 4, 640 * 4, C.byref(t)) == INVALID
            assert _names_the_formats(L.vs_azc_last_error(az.h).decode(), "vs_azc_apply_rgb_dev_n")
        rg.sync()
        az.sync()
        assert (d_out.download((640 * 360 * 4,), np.uint8) == 0x5A).all(), "a refused call wrote"
        # the operator: what the plan refuses, and a null stream argument is the default stream
        assert L.vs_op_scale_jobs_rgb(gpu._scale_job_array([(d_in.ptr, w * 4, w, h, d_out.ptr, 640 * 4, 640, 360, 2)]), 1, 0, None) == INVALID
        assert L.vs_op_scale_jobs_rgb(gpu._scale_job_array([(d_in.ptr, w * 4, w, h, d_out.ptr, 640 * 4, 640, 360, 4)]), 1, 2, None) == INVALID
        assert b"scale_jobs_rgb" in L.vs_last_error()
        # ... and both objects still work
        ro = oracle.roll_correction(oracle.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
        want, states = inputs.roll_ref([frame], inputs.BGRA8, ro)
        ro.close()
        rg.correct_rgb_dev(inputs.BGRA8, d_in.ptr, w, h, w * 4, d_out.ptr, w * 4)
        rg.sync()
        assert rg.state() == states[0] and np.array_equal(d_out.download((h, w, 4), np.uint8), want[0])
        zref, zinfo = inputs.azc_ref(frame, inputs.BGRA8, oracle)
        ticket = az.apply_rgb_dev(inputs.BGRA8, d_in.ptr, w, h, w * 4, d_out.ptr, 640 * 4)
        az.sync()
        ow, oh, info = az.result(ticket)
        assert ticket == 0 and info.tolist() == zinfo.tolist()
        assert np.array_equal(d_out.download((max(h, 360), 640, 4), np.uint8)[:oh, :ow], zref)
    finally:
        rg.close()
        az.close()
        d_in.free()
        d_out.free()
