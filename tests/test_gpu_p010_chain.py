"""Roll correction and auto zoom/crop on P010 surfaces, and the 10-bit chain roll -> stabilize -> zoom, bit for bit.

The reference is tests/ref16_geom.py (numpy integers; pinned against the 8-bit oracle by tests/test_p010_geom_cpu.py, which also
asserts that the inputs used here hold rounding ties: a kernel that rounds half up fails these tests).  Angle, line counts, info8
and the crop rectangle come from the oracle's NV12 objects run on the surfaces' high bytes - the definition of the analysis plane."""
import ctypes as C
import threading

import numpy as np
import pytest

import p010_chain_inputs as inputs
import ref16
import ref16_geom as geom
from vsamd import capi

pytestmark = pytest.mark.gpu

P010 = capi.FMT_P010
CANARY = 0xA5C3
INVALID = 1


# ---- 1. vs_op_warp_affine16_ex ---------------------------------------------------------------------------------------------------
def _warp16(gpu, img, M, dsize, border, extra_src=3, extra_dst=5):
    """The operator on a plane whose rows are padded by an ODD number of samples (pitches in bytes stay even); canaries in the padding."""
    sh, sw = img.shape[:2]
    cn = 1 if img.ndim == 2 else img.shape[2]
    dw, dh = dsize
    sp, dp = sw * cn + extra_src, dw * cn + extra_dst              # samples per row
    src = np.full((sh, sp), CANARY, np.uint16)
    src[:, :sw * cn] = img.reshape(sh, sw * cn)
    d_in, d_out = capi.DevBuf.from_array(gpu, src), capi.DevBuf.from_array(gpu, np.full((dh, dp), CANARY, np.uint16))
    M = np.ascontiguousarray(M, np.float64).reshape(6)
    gpu.check(gpu.lib.vs_op_warp_affine16_ex(d_in.ptr, 2 * sp, sw, sh, d_out.ptr, 2 * dp, dw, dh, cn, capi._p(M, capi.f64p), border, None))
    gpu.sync()
    out = d_out.download((dh, dp), np.uint16)
    d_in.free(); d_out.free()
    assert np.all(out[:, dw * cn:] == CANARY), "padding samples were written"
    return out[:, :dw * cn].reshape((dh, dw) if cn == 1 else (dh, dw, cn))


@pytest.mark.parametrize("border", [geom.CONSTANT, geom.REPLICATE], ids=["constant", "replicate"])
@pytest.mark.parametrize("dsize", inputs.WARP16_DSTS, ids=lambda s: "into_%dx%d" % s)
@pytest.mark.parametrize("cn", [1, 2])
def test_warp_affine16_ex(gpu, cn, dsize, border):
    img = inputs.warp16_plane(cn)
    for name, M in inputs.warp16_matrices(dsize).items():
        assert np.array_equal(_warp16(gpu, img, M, dsize, border), geom.warp(img, M, dsize, border)), name


def test_warp_affine16_ex_refuses_odd_pointers_and_strides(gpu):
    d = capi.DevBuf(gpu, 1 << 16)
    M = np.asarray([1.0, 0, 0, 0, 1.0, 0], np.float64)
    ok = dict(so=0, sp=64, do=32768, dp=64, cn=1, border=0)
    for kw in (dict(), dict(so=1), dict(do=32769), dict(sp=65), dict(dp=67), dict(cn=3), dict(border=1)):
        a = dict(ok, **kw)
        rc = gpu.lib.vs_op_warp_affine16_ex(d.ptr + a["so"], a["sp"], 32, 24, d.ptr + a["do"], a["dp"], 32, 24, a["cn"], capi._p(M, capi.f64p), a["border"], None)
        assert rc == (INVALID if kw else 0), (kw, rc)
        if kw:
            assert gpu.lib.vs_last_error()
    gpu.sync()
    d.free()


# ---- surfaces in decoder layout ------------------------------------------------------------------------------------------------------
def _pack(surfs, w, h, ps, hal):
    """(n, hal + h / 2, ps) uint16: rows of ps samples, the chroma plane behind hal rows; canaries elsewhere."""
    host = np.full((len(surfs), hal + h // 2, ps), CANARY, np.uint16)
    for i, s in enumerate(surfs):
        host[i, :h, :w] = s[:h]
        host[i, hal:, :w] = s[h:]
    return host


def _unpack(got, w, h, hal):
    return np.concatenate([got[:h, :w], got[hal:hal + h // 2, :w]])


# ---- 2. roll ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def roll_refs(oracle):
    """Per case: the reference results, the oracle's NV12 results on the high bytes, and the oracle's state after the last frame."""
    out = {}
    for size, slope, _ in inputs.ROLL_CASES:
        w, h = size
        ro = oracle.roll_correction(oracle.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
        refs, nv = [], []
        for s in inputs.roll_surfaces(size, slope):
            hi = geom.high_bytes(s)
            nv.append(ro.correct_nv12(hi, w, h))
            refs.append(geom.rotate_surface(s, w, h, ro.state()[0]))
        out[(size, slope)] = (refs, nv, ro.state())
        ro.close()
    return out


def _roll_run(gpu, surfs, w, h, thr, padded, fmt_of=lambda i: 2, array_form=False):
    """The surfaces through one roll object; fmt_of(i) = 2: surface i as P010, 1: its high bytes as NV12 (same buffer geometry in
    samples).  Returns the unpacked results (uint16 / uint8 per surface) and the state."""
    ps = (w + 63) // 64 * 64 + 64 if padded else w
    hal = h + 6 if padded else h
    n = len(surfs)
    host16 = _pack(surfs, w, h, ps, hal)
    host8 = np.full(host16.shape, 0xA5, np.uint8)
    for i, s in enumerate(surfs):
        hi = geom.high_bytes(s)
        host8[i, :h, :w] = hi[:h]
        host8[i, hal:, :w] = hi[h:]
    d16, d8 = capi.DevBuf.from_array(gpu, host16), capi.DevBuf.from_array(gpu, host8)
    o16 = capi.DevBuf.from_array(gpu, np.full(host16.shape, CANARY, np.uint16))
    o8 = capi.DevBuf.from_array(gpu, np.full(host8.shape, 0x5A, np.uint8))
    sb16, sb8 = host16[0].nbytes, host8[0].nbytes
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    if array_form:
        assert all(fmt_of(i) == 2 for i in range(n))
        rg.correct_p010_dev_n([d16.ptr + i * sb16 for i in range(n)], w, h, 2 * ps, [o16.ptr + i * sb16 for i in range(n)], 2 * ps,
                              uv_offset=2 * ps * hal, out_uv_offset=2 * ps * hal)
    else:
        for i in range(n):
            if fmt_of(i) == 2:
                rg.correct_p010_dev(d16.ptr + i * sb16, w, h, 2 * ps, o16.ptr + i * sb16, 2 * ps, uv_offset=2 * ps * hal, out_uv_offset=2 * ps * hal)
            else:
                rg.correct_nv12_dev(d8.ptr + i * sb8, w, h, ps, o8.ptr + i * sb8, ps, uv_offset=ps * hal, out_uv_offset=ps * hal)
    rg.sync()
    state = rg.state()
    g16, g8 = o16.download(host16.shape, np.uint16), o8.download(host8.shape, np.uint8)
    rg.close()
    for d in (d16, d8, o16, o8):
        d.free()
    res = []
    for i in range(n):
        g, pad = (g16[i], CANARY) if fmt_of(i) == 2 else (g8[i], 0x5A)
        res.append(_unpack(g, w, h, hal))
        assert (g[:h, w:] == pad).all() and (g[h:hal] == pad).all() and (g[hal:, w:] == pad).all(), "padding was written"
        other = g8[i] if fmt_of(i) == 2 else g16[i]
        assert (other == (0x5A if fmt_of(i) == 2 else CANARY)).all(), "the other format's buffer was written"
    return res, state


@pytest.mark.parametrize("size,slope,padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_roll_correct_p010_matches_the_reference(gpu, roll_refs, size, slope, padded):
    """Eleven frames, the flat one included: both planes equal the reference, the state equals the oracle's NV12 state on the high
    bytes and is non-zero, the padding is untouched, and the array form equals the calls."""
    w, h = size
    surfs = inputs.roll_surfaces(size, slope)
    refs, _, state = roll_refs[(size, slope)]
    got, gstate = _roll_run(gpu, surfs, w, h, inputs.roll_hough_threshold(w), padded)
    for i in range(len(surfs)):
        assert np.array_equal(got[i][:h], refs[i][:h]), ("luma", i)
        assert np.array_equal(got[i][h:], refs[i][h:]), ("chroma", i)
    assert gstate == state and state[0] != 0.0
    got_n, state_n = _roll_run(gpu, surfs, w, h, inputs.roll_hough_threshold(w), padded, array_form=True)
    assert state_n == gstate and all(np.array_equal(a, b) for a, b in zip(got, got_n))


def test_roll_correct_p010_refuses_odd_geometry(gpu):
    d = capi.DevBuf(gpu, 1 << 18)
    rg = gpu.roll_correction()
    ok = dict(off=0, w=64, h=48, pitch=128, uv=0, ooff=1 << 17, opitch=128, ouv=0)
    for kw in (dict(off=1), dict(ooff=(1 << 17) + 1), dict(pitch=129), dict(opitch=131), dict(uv=128 * 48 + 1), dict(ouv=128 * 48 + 1)):
        a = dict(ok, **kw)
        rc = gpu.lib.vs_roll_correct_p010_dev(rg.h, C.c_void_p(d.ptr + a["off"]), a["w"], a["h"], a["pitch"], a["uv"], C.c_void_p(d.ptr + a["ooff"]), a["opitch"], a["ouv"])
        assert rc == INVALID and "P010" in (gpu.lib.vs_roll_last_error(rg.h) or b"").decode(), kw
    for kw in (dict(w=63), dict(h=47), dict(pitch=126), dict(opitch=126)):
        a = dict(ok, **kw)
        assert gpu.lib.vs_roll_correct_p010_dev(rg.h, C.c_void_p(d.ptr), a["w"], a["h"], a["pitch"], 0, C.c_void_p(d.ptr + a["ooff"]), a["opitch"], 0) == INVALID, kw
    rg.sync()
    rg.close()
    d.free()


# ---- 3. zoom ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoom_refs(oracle):
    return {size: [geom.azc_p010(s, size[0], size[1], oracle) for s in inputs.zoom_surfaces(oracle, size)] for size in inputs.ZOOM_SIZES}


def _zoom_run(gpu, surfs, w, h, fmt_of=lambda i: 2):
    """The surfaces through one zoom object (the first five one by one, the rest - when all are P010 - through the array form).
    Returns per surface (ticket, ow, oh, info8, packed result) and the worker times."""
    n = len(surfs)
    stack16 = np.stack(surfs)
    stack8 = np.stack([geom.high_bytes(s) for s in surfs])
    d16, d8 = capi.DevBuf.from_array(gpu, stack16), capi.DevBuf.from_array(gpu, stack8)
    o16 = capi.DevBuf.from_array(gpu, np.full(stack16.shape, CANARY, np.uint16))
    o8 = capi.DevBuf.from_array(gpu, np.full(stack8.shape, 0x5A, np.uint8))
    sb16, sb8 = stack16[0].nbytes, stack8[0].nbytes
    az = gpu.auto_zoom_crop()
    all16 = all(fmt_of(i) == 2 for i in range(n))
    tickets = []
    for i in range(5 if all16 else n):
        if fmt_of(i) == 2:
            tickets.append(az.apply_p010_dev(d16.ptr + i * sb16, w, h, 2 * w, o16.ptr + i * sb16, 2 * w, 2 * w * h))
        else:
            tickets.append(az.apply_nv12_dev(d8.ptr + i * sb8, w, h, w, o8.ptr + i * sb8, w, w * h))
    if all16:
        tickets += az.apply_p010_dev_n([d16.ptr + i * sb16 for i in range(5, n)], w, h, 2 * w, [o16.ptr + i * sb16 for i in range(5, n)], 2 * w, 2 * w * h)
    assert tickets == list(range(n))
    az.sync()
    g16, g8 = o16.download(stack16.shape, np.uint16), o8.download(stack8.shape, np.uint8)
    res = []
    for i, t in enumerate(tickets):
        ow, oh, info = az.result(t)
        g = g16[i] if fmt_of(i) == 2 else g8[i]
        res.append((t, ow, oh, info.tolist(), np.concatenate([g[:oh, :ow], g[h:h + oh // 2, :ow]])))
    wt = az.worker_times()
    az.close()
    for d in (d16, d8, o16, o8):
        d.free()
    return res, wt


@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=["wide_mask_800", "wide_mask_808", "general_mask_804"])
def test_auto_zoom_crop_p010_matches_the_reference(gpu, oracle, zoom_refs, size):
    """Twelve surfaces pushed without waiting: tickets, info8 and sizes equal the oracle's on the high bytes, planes equal the
    reference (the unchanged surface, all 16 bits, on the fall-back paths); between 9 and 11 are cropped."""
    w, h = size
    surfs = inputs.zoom_surfaces(oracle, size)
    res, wt = _zoom_run(gpu, surfs, w, h)
    cropped = 0
    for i, ((t, ow, oh, ginfo, px), (want, info)) in enumerate(zip(res, zoom_refs[size])):
        assert ginfo == info.tolist(), i
        assert (ow, oh) == ((640, 360) if info[7] else (w, h)), i
        assert px.shape == want.shape and np.array_equal(px[:oh], want[:oh]), ("luma", i)
        assert np.array_equal(px[oh:], want[oh:]), ("chroma", i)
        cropped += int(info[7])
    assert 9 <= cropped <= 11
    assert wt[0] == len(surfs) and wt[5] == 2 and wt[3] > 0 and all(v >= 0 for v in wt)      # two batches: 8 + 4


def test_auto_zoom_crop_p010_refuses_odd_geometry(gpu):
    d = capi.DevBuf(gpu, 4 << 20)
    az = gpu.auto_zoom_crop()
    half = 2 << 20
    ok = dict(off=0, w=64, h=48, pitch=128, uv=0, ooff=half, opitch=1280, ouv=1280 * 360)
    t = C.c_int64(-1)
    for kw in (dict(off=1), dict(ooff=half + 1), dict(pitch=129), dict(opitch=1281, ouv=1281 * 360 + 1), dict(uv=128 * 48 + 1), dict(ouv=1280 * 360 + 1)):
        a = dict(ok, **kw)
        rc = gpu.lib.vs_azc_apply_p010_dev(az.h, C.c_void_p(d.ptr + a["off"]), a["w"], a["h"], a["pitch"], a["uv"], C.c_void_p(d.ptr + a["ooff"]), a["opitch"], a["ouv"], C.byref(t))
        assert rc == INVALID and "P010" in (gpu.lib.vs_azc_last_error(az.h) or b"").decode(), kw
    for kw in (dict(w=63), dict(h=47), dict(pitch=126), dict(opitch=1278), dict(ouv=1280 * 359)):      # (out_pitch >= 2 * max(w, 640), chroma behind 360 rows)
        a = dict(ok, **kw)
        assert gpu.lib.vs_azc_apply_p010_dev(az.h, C.c_void_p(d.ptr), a["w"], a["h"], a["pitch"], 0, C.c_void_p(d.ptr + a["ooff"]), a["opitch"], a["ouv"], C.byref(t)) == INVALID, kw
    az.sync()
    az.close()
    d.free()


# ---- 4. NV12 and P010 through one object -----------------------------------------------------------------------------------------------
def test_roll_object_takes_nv12_and_p010_alternately(gpu, roll_refs):
    """Every change of sample size closes the pending batch; each result equals the unmixed run's and the smoothed angle carries
    across (the analysis plane of a P010 surface is its high-byte surface: one angle sequence for all three runs)."""
    size, slope, padded = inputs.ROLL_CASES[1]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    surfs = inputs.roll_surfaces(size, slope)
    refs, nv, state = roll_refs[(size, slope)]
    only16, s16 = _roll_run(gpu, surfs, w, h, thr, padded)
    only8, s8 = _roll_run(gpu, surfs, w, h, thr, padded, fmt_of=lambda i: 1)
    mixed, sm = _roll_run(gpu, surfs, w, h, thr, padded, fmt_of=lambda i: 1 + i % 2)
    assert s16 == s8 == sm == state and sm[0] != 0.0
    for i in range(len(surfs)):
        assert np.array_equal(only8[i], nv[i]), i
        assert np.array_equal(mixed[i], only16[i] if i % 2 else only8[i]), i
        assert mixed[i].dtype == (np.uint16 if i % 2 else np.uint8)


def test_zoom_object_takes_nv12_and_p010_alternately(gpu, oracle, zoom_refs):
    size = inputs.ZOOM_SIZES[1]
    w, h = size
    surfs = inputs.zoom_surfaces(oracle, size)
    only16, _ = _zoom_run(gpu, surfs, w, h)
    only8, _ = _zoom_run(gpu, surfs, w, h, fmt_of=lambda i: 1)
    mixed, wt = _zoom_run(gpu, surfs, w, h, fmt_of=lambda i: 1 + i % 2)
    assert wt[0] == len(surfs) and wt[5] == len(surfs)           # (every call closed the batch of the one before)
    for i in range(len(surfs)):
        want = only16[i] if i % 2 else only8[i]
        assert mixed[i][:4] == want[:4], i
        assert mixed[i][4].dtype == want[4].dtype and np.array_equal(mixed[i][4], want[4]), i
        assert only8[i][3] == only16[i][3] == zoom_refs[size][i][1].tolist(), i


# ---- 5. the chain ----------------------------------------------------------------------------------------------------------------------
def run_chain_p010(vs, W, H, CH, batch, params, rings, lags, n_chunks, src, overlap=True):
    """tests/test_gpu_chain.py::run_chain (the schedule of bench.py's config2_chain; keep the two in step) for P010 surfaces: roll(c)
    writes ring slot c % R, stab(c) pushes those (batch `batch`, zero-copy) into slot c % S, zoom(c) crops those into slot c % Z.
    overlap=True: one thread per stage, roll(c) after stab(c - lags[0]), stab(c) after zoom(c - lags[1]); overlap=False: one stage at
    a time.  One chunk more than n_chunks: the stabilizer's flush.  Returns [(ow, oh, info, P010 rows of the output)], the roll
    stage's state and the stabilizer's frames_out."""
    R, S, Z = rings
    lag_r, lag_s = lags
    pitch = 2 * W
    sb = pitch * H * 3 // 2
    bufs = [capi.DevBuf(vs, sb * CH) for _ in range(R + S + Z)]
    d_roll, d_stab, d_zoom = bufs[:R], bufs[R:R + S], bufs[R + S:]
    rc, az, st = vs.roll_correction(), vs.auto_zoom_crop(), vs.stabilizer(params)
    st.set_batch(batch)
    st.set_zero_copy(True)
    produced = {}
    results = []
    total = n_chunks + 1

    def roll_stage(c):
        if c == n_chunks:
            return
        assert sum(produced[j] for j in range(c - lag_r + 1)) >= (c - R + 1) * CH, ("R ring reused too early", c)
        rc.correct_p010_dev_n([src(c * CH + i) for i in range(CH)], W, H, pitch, [d_roll[c % R].ptr + i * sb for i in range(CH)], pitch)
        rc.sync()

    def stab_stage(c):
        assert sum(produced[j] for j in range(c - lag_s + 1)) >= sum(produced[j] for j in range(c - S + 1)), ("S ring reused too early", c)
        out = d_stab[c % S].ptr
        if c < n_chunks:
            produced[c] = st.push_dev_n([d_roll[c % R].ptr + i * sb for i in range(CH)], W, H, pitch, P010, [out + j * sb for j in range(CH)], pitch)
        else:
            k = 0
            while True:
                assert k < CH, "the flush holds more than a chunk"
                if not st.flush_dev(out + k * sb, pitch):
                    break
                k += 1
            produced[c] = k
        st.sync()

    def zoom_stage(c):
        k = produced[c]
        if not k:
            return
        slot = d_zoom[c % Z]
        tickets = az.apply_p010_dev_n([d_stab[c % S].ptr + j * sb for j in range(k)], W, H, pitch, [slot.ptr + j * sb for j in range(k)], pitch, pitch * H)
        az.sync()
        for j, t in enumerate(tickets):
            ow, oh, info = az.result(t)
            y = slot.download((oh, W), np.uint16, j * sb)[:, :ow]
            uv = slot.download((oh // 2, W), np.uint16, j * sb + pitch * H)[:, :ow]
            results.append((ow, oh, info.tolist(), np.concatenate([y, uv])))

    try:
        if not overlap:
            for c in range(total):
                roll_stage(c)
                stab_stage(c)
                zoom_stage(c)
        else:
            done = {"roll": -1, "stab": -1, "zoom": -1}
            cond = threading.Condition()
            failed = []

            def wait_for(stage, c):
                with cond:
                    cond.wait_for(lambda: done[stage] >= c or failed)
                return not failed

            def stage_loop(name, f, before, after, lag):
                try:
                    for c in range(total):
                        if before and not wait_for(before, c):
                            return
                        if after and not wait_for(after, c - lag):
                            return
                        f(c)
                        with cond:
                            done[name] = c
                            cond.notify_all()
                except BaseException as e:          # (a failed stage must not leave the others waiting)
                    with cond:
                        failed.append(e)
                        cond.notify_all()

            ths = [threading.Thread(target=stage_loop, args=a) for a in (("roll", roll_stage, None, "stab", lag_r),
                                                                         ("stab", stab_stage, "roll", "zoom", lag_s),
                                                                         ("zoom", zoom_stage, "stab", None, 0))]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            if failed:
                raise failed[0]
        return results, rc.state(), st.counters().frames_out
    finally:
        for o in (st, rc, az):
            o.close()
        for b in bufs:
            b.free()


def _reference_chain(oracle, surfs, W, H, params):
    """Stage by stage: ref16_geom roll; the oracle's stabilizer on the high bytes of the rolled surfaces for the matrices and
    ref16.warp_two_planes for the pixels (the last frame of the clip comes back unwarped); ref16_geom zoom."""
    from test_gpu_p010 import _oracle_nv12_run
    ro = oracle.roll_correction()
    rolled = [geom.roll_p010(s, W, H, ro) for s in surfs]
    state = ro.state()
    ro.close()
    outs, _ = _oracle_nv12_run(oracle, [geom.high_bytes(r) for r in rolled], **params)
    res = []
    ties = [0, 0]
    for idx, M in outs:
        stab = rolled[idx] if idx == len(rolled) - 1 else ref16.warp_two_planes(rolled[idx], W, H, M)
        z, info = geom.azc_p010(stab, W, H, oracle)
        res.append((z, info))
        if idx != len(rolled) - 1 and len(res) % 8 == 1:         # (the inputs of the two later stages hold ties too: a sample of them)
            ties[0] += int(ref16.tie_mask(rolled[idx][:H], M).sum())
            if info[7]:
                x, y, cw, ch, dw, dh, My = geom.zoom_jobs(info)[0]
                ties[1] += int(geom.tie_mask(stab[:H][y:y + ch, x:x + cw], My, (dw, dh)).sum())
    assert ties[0] > 0 and ties[1] > 0, ties
    return res, state


def test_p010_chain_overlapped_equals_serial_equals_the_reference(gpu, oracle):
    """704 x 400, chunks of 8, stabilizer batch 8 zero-copy, rings 4 / 3 / 2 with lags 3 / 3 (every slot is rewritten while the other
    stages run), five chunks plus the flush."""
    W, H = inputs.CHAIN_SIZE
    CH, n_chunks = 8, 5
    N = CH * n_chunks
    surfs = inputs.chain_surfaces(N)
    params = dict(smoothing_radius=5, max_corners=400)
    sb = surfs[0].nbytes
    d_in = capi.DevBuf(gpu, sb * 7)
    try:
        for i in range(7):
            d_in.upload(surfs[i], i * sb)
        runs = [run_chain_p010(gpu, W, H, CH, 8, gpu.params(**params), (4, 3, 2), (3, 3), n_chunks, lambda i: d_in.ptr + (i % 7) * sb, overlap=o)
                for o in (False, True)]
    finally:
        d_in.free()
    (ser, ser_state, ser_out), (got, state, out) = runs
    assert len(got) == len(ser) == N and out == ser_out == N
    for j, (a, b) in enumerate(zip(got, ser)):
        assert a[:3] == b[:3], j
        assert a[3].shape == b[3].shape and np.array_equal(a[3], b[3]), j
    assert state == ser_state
    ref, ref_state = _reference_chain(oracle, surfs, W, H, params)
    assert len(ref) == N and ser_state == ref_state and ref_state[0] != 0.0
    n_crop = 0
    for j, ((ow, oh, info, px), (want, winfo)) in enumerate(zip(ser, ref)):
        assert info == winfo.tolist(), j
        assert (ow, oh) == ((640, 360) if winfo[7] else (W, H)), j
        assert px.shape == want.shape and np.array_equal(px, want), j
        n_crop += int(winfo[7])
    assert n_crop > 0
