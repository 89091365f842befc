"""Auto zoom/crop at a chosen output size on the device (vs_azc_set_output_size, vs_op_scale_jobs).

1. the operator, bit for bit against azc_size_inputs.reference (pinned to the oracle in tests/test_azc_size_cpu.py).  The staged kernel
   works on tiles of T_w x T_h = 128 x 16 output samples and stages at most 160 x 24 source samples; azc_size_inputs states which of
   the 24 (crop, destination) pairs cross what: destinations of one tile, of a ragged second tile column and row (130 x 19) and of two
   full tile columns plus two samples (258); crops of 1 x 1, 3 x 2, a prime size, the exact 2 x zoom, the identity and downscales on
   either side of the staging limit, across and down.  All 24 go in ONE call, 8-bit and 16-bit, cn 1 and 2; the crops sit at unaligned
   origins inside planes whose samples are all non-zero (so a border that is not 0 shows), half of them in a plane whose base and
   pitch keep no alignment at all; the destinations have padded pitches, half of them unaligned, and every byte outside dw x dh must
   still be the canary.  path 1 (the direct kernels) and vs_op_warp_affine_ex / vs_op_warp_affine16_ex give the same bytes.
2. the stage: NV12, P010, I420 and I010 surfaces of two sizes at four output sizes; info8 is the oracle's, out_w / out_h as defined,
   every plane equals the per-plane reference, a fall-back surface comes back unchanged, and nothing outside the planes is written.
   An explicit (640, 360) equals a fresh object that never called the setter, byte for byte.
3. a change of size between calls closes the batch; every ticket keeps the size it was issued under.
4. refusals: the setter's bad values; result pitches, offsets and layouts that hold the surface but not ow x oh, and the reverse.
5. the synchronous forms, BGR and gray, at (0, 0) and (1280, 720)."""
import ctypes as C

import numpy as np
import pytest

import azc_size_inputs as inp
import p010_chain_inputs as inputs
import ref16_geom as geom
from test_azc import rotated_frame
from test_gpu_i420_chain import I010, I420, NV12, P010, Layout, _dtype, _sb, check_planes, surface_planes, zoom_run
from vsamd import capi

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY = 0x5A


# ---- 1. the operator -------------------------------------------------------------------------------------------------------------------
SRC_SIZE = (320, 36)          # holds the largest crop (310 x 28) at the largest origin (7, 5)


def _up(v, a):
    return (v + a - 1) // a * a


def _op_setup(sb, cn):
    """Two copies of one random plane in one source buffer - A: base and pitch multiples of 16; B: base one sample off, pitch one pixel
    more (no alignment survives from row to row) - the 24 jobs as (byte offsets and geometry), and the expected destination buffer."""
    key = (sb, cn)
    memo = inp.cache("op_setup")
    if key in memo:
        return memo[key]
    dtype = np.uint8 if sb == 1 else np.uint16
    px = cn * sb
    W, H = SRC_SIZE
    plane = inp.random_plane(SRC_SIZE, cn, dtype, 300 + 10 * sb + cn)
    rows = plane.reshape(H, W * cn).view(np.uint8)                      # (H, W * px) bytes
    pitch_a = _up(W * px, 16)
    pitch_b = pitch_a + px
    off_b = _up(pitch_a * H, 256) + sb
    src = np.full(off_b + pitch_b * H + 64, CANARY | 1, np.uint8)       # (non-zero around the planes too)
    for base, pitch in ((0, pitch_a), (off_b, pitch_b)):
        for y in range(H):
            src[base + y * pitch: base + y * pitch + W * px] = rows[y]
    jobs, cursor, writes = [], 0, []
    for i, ((sw, sh), (dw, dh)) in enumerate(inp.OP_CASES):
        x0, y0 = 1 + i % 7, 1 + i % 5
        base, pitch = ((0, pitch_a), (off_b, pitch_b))[i % 2]
        unaligned = (i // 2) % 2
        dpitch = dw * px + 3 * px if unaligned else _up(dw * px, 16) + 16
        dstart = cursor + (sb if unaligned else 0)
        cursor = _up(dstart + dpitch * dh + 64, 256)
        jobs.append((base + y0 * pitch + x0 * px, pitch, sw, sh, dstart, dpitch, dw, dh, cn))
        roi = plane[y0:y0 + sh, x0:x0 + sw]
        want = inp.reference(roi, (dw, dh))
        writes.append((dstart, dpitch, want.reshape(dh, dw * cn).view(np.uint8), roi, want))
    expect = np.full(cursor, CANARY, np.uint8)
    for dstart, dpitch, wb, _, _ in writes:
        for y in range(wb.shape[0]):
            expect[dstart + y * dpitch: dstart + y * dpitch + wb.shape[1]] = wb[y]
    memo[key] = (src, jobs, expect, writes)
    return memo[key]


def _op_run(gpu, sb, cn, path):
    src, jobs, expect, _ = _op_setup(sb, cn)
    d_src = capi.DevBuf.from_array(gpu, src)
    d_dst = capi.DevBuf.from_array(gpu, np.full(expect.size, CANARY, np.uint8))
    try:
        gpu.scale_jobs([(d_src.ptr + so, sp, sw, sh, d_dst.ptr + do, dp, dw, dh, c) for so, sp, sw, sh, do, dp, dw, dh, c in jobs], sb, path)
        gpu.sync()
        return d_dst.download((expect.size,), np.uint8)
    finally:
        d_src.free()
        d_dst.free()


def _first_bad_job(got, sb, cn):
    _, jobs, _, writes = _op_setup(sb, cn)
    for i, ((dstart, dpitch, wb, _, _), case) in enumerate(zip(writes, inp.OP_CASES)):
        for y in range(wb.shape[0]):
            row = got[dstart + y * dpitch: dstart + y * dpitch + wb.shape[1]]
            if not np.array_equal(row, wb[y]):
                return "job %d %s row %d: %d bytes differ" % (i, case, y, int((row != wb[y]).sum()))
    return "bytes outside the destinations were written"


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("sb", [1, 2], ids=["8bit", "16bit"])
def test_scale_jobs_both_paths_equal_the_reference(gpu, sb, cn):
    _, jobs, expect, _ = _op_setup(sb, cn)
    plan = gpu.scale_jobs_plan([(4096 + so, sp, sw, sh, (1 << 30) + do, dp, dw, dh, c) for so, sp, sw, sh, do, dp, dw, dh, c in jobs], sb).tolist()
    assert plan == inp.OP_STAGED and len(jobs) == 24                   # one call, both classes: two launches
    staged = _op_run(gpu, sb, cn, 0)
    assert np.array_equal(staged, expect), _first_bad_job(staged, sb, cn)
    direct = _op_run(gpu, sb, cn, 1)
    assert np.array_equal(direct, expect), _first_bad_job(direct, sb, cn)
    assert np.array_equal(staged, direct)
    # the plane warp with the same matrix (vs_op_warp_affine_ex / vs_op_warp_affine16_ex) gives the same bytes
    _, _, _, writes = _op_setup(sb, cn)
    f = gpu.warp_affine_ex if sb == 1 else gpu.warp_affine16_ex
    for i, ((_, _, _, roi, want), (ssize, dsize)) in enumerate(zip(writes, inp.OP_CASES)):
        got = f(np.ascontiguousarray(roi), inp.scale_matrix(ssize, dsize), capi.BORDER_BLACK, dsize)
        assert np.array_equal(got, want), (i, ssize, dsize)


# ---- 2. the stage ----------------------------------------------------------------------------------------------------------------------
KINDS = [NV12, P010, I420, I010]
KIND_IDS = ["nv12", "p010", "i420", "i010"]


def _orc(oracle, size):
    memo = inp.cache("orc")
    if size not in memo:
        memo[size] = [oracle.auto_zoom_crop_nv12(geom.high_bytes(s), size[0], size[1])[1] for s in inputs.zoom_surfaces(oracle, size)]
    return memo[size]


def _planes(oracle, kind, size):
    """NV12 and I420 hold the same planes, so they share them and the references below."""
    pk = {NV12: I420}.get(kind, kind)
    memo = inp.cache("planes")
    if (pk, size) not in memo:
        memo[(pk, size)] = [surface_planes(s, size[0], size[1], pk) for s in inputs.zoom_surfaces(oracle, size)]
    return pk, memo[(pk, size)]


def _want(oracle, kind, size, out_size, idx=None):
    """Per surface the reference's (Y, U, V) at the resolved output size; idx: only those surfaces (the others None)."""
    pk, planes = _planes(oracle, kind, size)
    memo = inp.cache("want")
    osz = inp.resolved(out_size, *size)
    out = []
    for i, (p, info) in enumerate(zip(planes, _orc(oracle, size))):
        if idx is not None and i not in idx:
            out.append(None)
            continue
        k = (pk, size, osz, i)
        if k not in memo:
            memo[k] = inp.stage_planes(p, info, osz)
        out.append(memo[k])
    return out


def _stage_run(gpu, oracle, kind, size, out_size, set_size=True, out_style="packed"):
    w, h = size
    _, planes = _planes(oracle, kind, size)
    ow, oh = inp.resolved(out_size, w, h)
    li, lo = Layout(kind, w, h), Layout(kind, max(w, ow), max(h, oh), out_style)
    az = gpu.auto_zoom_crop()
    try:
        if set_size:
            az.set_output_size(*out_size)
            assert az.output_size == out_size
        else:
            assert az.output_size == (640, 360)
        res, bufs = zoom_run(gpu, az, [(kind, w, h, p, li, lo) for p in planes])
    finally:
        az.close()
    return res, bufs, lo


@pytest.mark.parametrize("out_size", inp.OUT_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", inp.STAGE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_stage_at_a_chosen_output_size(gpu, oracle, kind, size, out_size):
    w, h = size
    orc = _orc(oracle, size)
    want = _want(oracle, kind, size, out_size)
    style = "padded" if kind in (I420, I010) and out_size[0] in (0, 322) else "packed"
    res, bufs, lo = _stage_run(gpu, oracle, kind, size, out_size, out_style=style)
    osz = inp.resolved(out_size, w, h)
    cropped = 0
    for i, ((t, ow, oh, ginfo), info) in enumerate(zip(res, orc)):
        assert t == i and ginfo == info.tolist(), i
        assert (ow, oh) == (osz if info[7] else (w, h)), i
        check_planes(bufs[i], lo, want[i], i)
        cropped += int(info[7])
    assert cropped >= 10 and not orc[3][7]          # (the cap of tests/test_azc_size_cpu.py: only the oracle's fall-back surfaces fall back)
    _, planes = _planes(oracle, kind, size)
    assert all(np.array_equal(a, b) for a, b in zip(want[3], planes[3]))        # the all-black surface: unchanged
    if out_size == (640, 360):                      # the explicit default equals an object that never called the setter
        res0, bufs0, _ = _stage_run(gpu, oracle, kind, size, out_size, set_size=False, out_style=style)
        assert res0 == res
        for a, b in zip(bufs0, bufs):
            assert np.array_equal(a, b)


# ---- 3. a change of size between calls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [NV12, I010], ids=["nv12", "i010"])
def test_a_change_of_size_closes_the_batch_and_tickets_keep_their_size(gpu, oracle, kind):
    size = inp.STAGE_SIZES[1]
    w, h = size
    a_size, b_size = (640, 360), (322, 182)
    sizes = [a_size] * 3 + [b_size] * 3 + [a_size] * 2
    _, planes = _planes(oracle, kind, size)
    orc = _orc(oracle, size)
    want_a, want_b = _want(oracle, kind, size, a_size, idx=(0, 1, 2, 6, 7)), _want(oracle, kind, size, b_size, idx=(3, 4, 5))
    li, lo = Layout(kind, w, h), Layout(kind, max(w, 640), max(h, 360))
    d_in = [capi.DevBuf.from_array(gpu, li.pack(p)) for p in planes[:8]]
    d_out = [capi.DevBuf.from_array(gpu, lo.blank()) for _ in range(8)]
    az = gpu.auto_zoom_crop()
    try:
        tickets = []
        for i in range(8):
            if i in (3, 6):
                az.set_output_size(*sizes[i])
            if kind == NV12:
                tickets.append(az.apply_nv12_dev(d_in[i].ptr, w, h, w, d_out[i].ptr, lo.w, lo.w * lo.h))
            else:
                tickets.append(az.apply_i420_dev(kind, d_in[i].ptr, w, h, li.c, d_out[i].ptr, lo.c))
        az.sync()
        assert tickets == list(range(8))
        for i, t in enumerate(tickets):
            ow, oh, info = az.result(t)
            assert info.tolist() == orc[i].tolist(), i
            assert (ow, oh) == (sizes[i] if orc[i][7] else (w, h)), i
            want = (want_b if sizes[i] == b_size else want_a)[i]
            check_planes(d_out[i].download((lo.size // lo.sb,), _dtype(kind)), lo, want, i)
        wt = az.worker_times()
        assert wt[0] == 8 and wt[5] == 3            # 3 + 3 + 2: each change closed the pending batch
        assert sum(int(orc[i][7]) for i in range(8)) >= 6
    finally:
        az.close()
        for d in d_in + d_out:
            d.free()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_setter_refuses_bad_values_and_keeps_the_size(gpu):
    az = gpu.auto_zoom_crop()
    try:
        assert az.output_size == (640, 360)
        for bad in [(641, 360), (640, 361), (-2, 360), (640, -2), (0, 360), (640, 0), (8194, 360), (640, 8194), (1, 1)]:
            assert gpu.lib.vs_azc_set_output_size(az.h, *bad) == INVALID, bad
            assert b"output size" in gpu.lib.vs_azc_last_error(az.h), bad
            assert az.output_size == (640, 360), bad
        for good in [(2, 2), (8192, 8192), (0, 0), (1280, 720)]:
            az.set_output_size(*good)
            assert az.output_size == good
    finally:
        az.close()


def _lay(**kw):
    return capi.i420_layout(kw.get("pitch", 0), kw.get("c_pitch", 0), kw.get("u_off", 0), kw.get("v_off", 0))


@pytest.mark.parametrize("sb", [1, 2], ids=["8bit", "16bit"])
def test_result_buffers_must_hold_the_surface_and_the_output_size(gpu, sb):
    """w x h = 64 x 48.  At (128, 96) the result rules read 128 and 96, at (32, 24) they read the surface's 64 and 48: a layout that
    holds only one of the two is refused (the planar texts name the format), the one that holds both is taken."""
    w, h = 64, 48
    d = capi.DevBuf(gpu, 4 << 20)
    half = 2 << 20
    az = gpu.auto_zoom_crop()
    t = C.c_int64(-1)
    two = gpu.lib.vs_azc_apply_nv12_dev if sb == 1 else gpu.lib.vs_azc_apply_p010_dev
    fmt, name = (I420, "I420") if sb == 1 else (I010, "I010")

    def two_plane(out_pitch, out_uv):
        return two(az.h, C.c_void_p(d.ptr), w, h, w * sb, 0, C.c_void_p(d.ptr + half), out_pitch, out_uv, C.byref(t))

    def planar(**lout):
        rc = gpu.lib.vs_azc_apply_i420_dev(az.h, fmt, C.c_void_p(d.ptr), w, h, C.byref(_lay(pitch=w * sb)), C.c_void_p(d.ptr + half), C.byref(_lay(**lout)), C.byref(t))
        return rc, (gpu.lib.vs_azc_last_error(az.h) or b"").decode()

    try:
        issued = 0
        for (ow, oh), (nw, nh) in (((128, 96), (128, 96)), ((32, 24), (64, 48)), ((0, 0), (64, 48))):
            az.set_output_size(ow, oh)
            p = nw * sb
            assert two_plane(p - 2, p * nh) == INVALID and two_plane(p, p * nh - 2) == INVALID, (ow, oh)
            if (ow, oh) == (128, 96):               # holds the surface, not ow x oh
                assert two_plane(w * sb, w * sb * h) == INVALID
            if (ow, oh) == (32, 24):                # holds ow x oh, not the surface
                assert two_plane(32 * sb, 32 * sb * 24) == INVALID
            for lout in (dict(pitch=p - 2), dict(pitch=p, c_pitch=p // 2 - 2), dict(pitch=p, u_off=p * (nh - 1)),
                         dict(pitch=p, u_off=p * nh, v_off=p * nh + p // 2 * (nh // 2 - 1))):
                rc, msg = planar(**lout)
                assert rc == INVALID and name in msg, ((ow, oh), lout, rc, msg)
            if (ow, oh) == (128, 96):
                rc, msg = planar(pitch=w * sb)
                assert rc == INVALID and name in msg and "128" in msg and "96" in msg, msg
            assert two_plane(p, p * nh) == 0 and t.value == issued
            rc, msg = planar(pitch=p)
            assert rc == 0 and t.value == issued + 1, msg
            issued += 2
        az.sync()
    finally:
        az.close()
        d.free()


# ---- 5. the synchronous forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", [(0, 0), (1280, 720)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cn", [3, 1], ids=["bgr", "gray"])
def test_synchronous_forms_at_a_chosen_output_size(gpu, oracle, cn, out_size):
    w, h = 804, 452
    frame = rotated_frame(oracle, w, h, 4.0, seed=5, cn=cn)
    black = np.zeros_like(frame)
    _, info = oracle.auto_zoom_crop(frame)
    assert info[7] and not oracle.auto_zoom_crop(black)[1][7]
    cx, cy, cw, ch = (int(v) for v in info[2:6])
    ow, oh = inp.resolved(out_size, w, h)
    want = inp.reference(frame[cy:cy + ch, cx:cx + cw], (ow, oh))
    az = gpu.auto_zoom_crop()
    d_in, d_out = capi.DevBuf.from_array(gpu, frame), capi.DevBuf(gpu, max(w, ow) * max(h, oh) * cn + 64)
    try:
        az.set_output_size(*out_size)
        got = az.apply(frame)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert az.info().tolist() == info.tolist()
        assert np.array_equal(az.apply(black), black)                                   # the fall-back path: w x h, unchanged
        stride = max(w, ow) * cn
        assert az.apply_dev(d_in.ptr, w, h, w * cn, cn, d_out.ptr, stride) == (ow, oh)
        az.sync()
        rows = d_out.download((oh, stride), np.uint8)[:, :ow * cn]
        assert np.array_equal(rows.reshape(want.shape), want)
        wv, hv = C.c_int(), C.c_int()
        assert gpu.lib.vs_azc_apply_dev(az.h, d_in.ptr, w, h, w * cn, cn, d_out.ptr, stride - 1, C.byref(wv), C.byref(hv)) == INVALID
    finally:
        az.close()
        d_in.free()
        d_out.free()
