"""The 8-bit operators on regions of interest of larger surfaces, every byte guarded (tests/roi.py), on a real MI355X.

For every operator and every layout of roi.LAYOUTS two assertions:
  (a) the ROI of the result equals, bit for bit, what the CPU oracle gives for the picture alone;
  (b) nothing outside the ROI changed - guards, parent rows above and below, the bytes beside every ROI row, the gaps between
      the frames of a batch - and the inputs are untouched.
No tolerance appears anywhere, and the expectation never comes from a packed run of the library.  No layout is refused: the header
states no alignment rule for an 8-bit operator.

Which alignment-dependent paths the layouts reach (from the kernels' own conditions; GUARD and the pad64 pitches are multiples
of 64, so an ROI's address modulo 16 is (ox * px + lead) modulo 16):
  k_pyr.hip `inside` (pitch % 4 == 0 and base % 4 == 0, tile at x0 >= 4, y0 >= 2 that ends 4 columns / 2 rows before the edge):
      136 x 36, tile (64, 16), in padded16, mixed (source side), tight_end (120 bytes left of the ROI) and packed (pitch 136);
      false by the base in roi_off1..3, by the pitch in odd_pitch and mixed_rev, by the geometry at 131 x 35 and 64 x 16.  The
      16-byte derivative store: every group of 136 x 36 and 64 x 16 (the derivative image is no picture: 256-byte aligned); the
      dword stores at 131 (odd rows start 4 bytes off).
  k_gray.hip: vs_op_resize_gray reaches the vector path of half_bgr_gray_kernel (vec_ok: source base and pitch multiples of 8,
      destination base and pitch multiples of 4) at the exact 2 x decimation of a colour picture, 132 x 98 -> 66 x 49 BGR8: true in
      padded16 (and the scalar tail group at x = 64), false in roi_off1..3, odd_pitch, mixed, mixed_rev (one side fails) and in packed
      (pitch 396 / 66); the other sizes and formats take resize_gray_kernel, a pixel per lane with byte loads and stores.  The
      quarter_gray / half_bgr_gray12 kernels (`vec` from (src | pitch) & 15) are launched by the batch schedule's table launcher
      only (streams in batch mode): no operator of this file reaches them.
  k_enhance.hip aligned4 (single-frame entry, per side): true in padded16 (101 x 77: 303-byte rows at pitch 384) and packed 64 x 32,
      false in roi_off1..3, odd_pitch, packed 101 x 77; (true, false) in mixed, (false, true) in mixed_rev.  The batch entry takes
      its table launch (which presumes alignment) only when every frame and both pitches are multiples of 4 and the stage list has
      no per-frame statistics - shipped and vibrance_only in padded16 and, at 64 x 32, in packed and tight_end - and goes frame by
      frame otherwise.
  k_warp.hip src_aligned / dst_aligned (pitch and every frame's base multiples of 4; cn 2: of 8; cn 4: the destination's of 16): (1, 1) padded16 and packed 128 /
      260 wide, (0, 0) roi_off1..3 and odd_pitch and packed 131 x 19, (1, 0) mixed, (0, 1) mixed_rev; in a batch the frame
      distance of the unaligned layouts is no multiple of 4, so the frames' bases differ modulo 4.
"""
import math

import numpy as np
import pytest

import roi
import roll_scene
from test_azc import rotated_frame
from test_enhance import CONFIGS, scene
from test_gpu_parity import MATS
from vsamd import capi, synth

pytestmark = pytest.mark.gpu
LAYOUTS = roi.LAYOUT_NAMES
F32P = capi.f32p
_cache = {}


def cached(key, fn):
    """References are computed once and shared by the layouts; they are never written to."""
    if key not in _cache:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def picture(key, shape, lo=0, hi=256):
    return cached(("pic", key, shape, lo, hi), lambda: np.random.default_rng(roi.case_seed("pic", key, shape)).integers(lo, hi, shape, dtype=np.uint8))


class Call:
    """The surfaces of one operator call: bound to device memory on entry, all checked and freed on exit."""

    def __init__(self, gpu, ins, outs):
        self.gpu, self.ins, self.outs = gpu, list(ins), list(outs)

    def __enter__(self):
        for s in self.ins + self.outs:
            s.bind(self.gpu)
        return self

    def done(self, status, what):
        """After the launch: status VS_OK, inputs untouched; -> the outputs' ROIs, after asserting (b) for each."""
        self.gpu.check(status)
        self.gpu.sync()
        for i, s in enumerate(self.ins):
            assert s.untouched(), (what, "input %d was written" % i)
        res = []
        for i, s in enumerate(self.outs):
            r, clean = s.result()
            assert clean, (what, "output %d" % i, s.stray())
            res.append(r)
        return res

    def __exit__(self, *exc):
        for s in self.ins + self.outs:
            s.free()


def same(got, want, what):
    got = np.asarray(got).reshape(np.asarray(want).shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


# ---- vs_op_warp_affine ---------------------------------------------------------------------------------------------------------
WARP_MATS = [MATS[0], MATS[2], MATS[3], MATS[4], MATS[6], MATS[7]]   # identity, fractional shift, 3 deg (fast path), 45 deg (direct
#                                                                      path), zoom out, everything out of frame
WARP_SIZES = [(131, 19), (128, 16), (260, 35), (1, 1)]


def warp_ref(oracle, cn, w, h, k, m):
    img = picture(("warp", k), (h, w, cn))
    return cached(("warp", cn, w, h, k, m), lambda: oracle.warp_affine(img if cn > 1 else img[..., 0], WARP_MATS[m]).reshape(h, w * cn))


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("cn", [1, 2, 3, 4])           # (4: a lane's four pixels are one 16-byte store where the destination allows it)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_warp_affine(gpu, oracle, layout, cn, batch):
    for w, h in WARP_SIZES:
        # batch 1: every matrix in a launch of its own; batch 5: two launches that cover the six matrices between them
        groups = [[m] for m in range(6)] if batch == 1 else [[0, 1, 2, 3, 4], [5, 4, 3, 2, 1]]
        for g in groups:
            what = (layout, cn, w, h, g)
            src, dst = roi.pair(layout, roi.case_seed(what), (w, h, cn, batch), (w, h, cn, batch))
            src.put(np.stack([picture(("warp", k), (h, w, cn)) for k in range(batch)]))
            M = np.ascontiguousarray([WARP_MATS[m] for m in g], np.float32)
            with Call(gpu, [src], [dst]) as c:
                out, = c.done(gpu.lib.vs_op_warp_affine(src.ptr, src.pitch, src.frame_bytes, dst.ptr, dst.pitch, dst.frame_bytes, w, h, cn,
                                                        capi._p(M, F32P), batch, None), what)
            out = out.reshape(batch, h, w * cn)
            for k, m in enumerate(g):
                same(out[k], warp_ref(oracle, cn, w, h, k, m), what + (k,))
                if m == 5:
                    assert not out[k].any()             # out of frame: the ROI is written black (and nothing else touched)


# ---- vs_op_warp_affine_ex ------------------------------------------------------------------------------------------------------
def _rot(deg, cx, cy, tx=0.0, ty=0.0):
    a = math.radians(deg)
    al, be = math.cos(a), math.sin(a)
    return [al, be, (1 - al) * cx - be * cy + tx, -be, al, be * cx + (1 - al) * cy + ty]


@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REPLICATE])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_warp_affine_ex(gpu, oracle, layout, cn, border):
    (sw, sh), (dw, dh) = (131, 19), (70, 33)
    img = picture("warp_ex", (sh, sw, cn))
    for i, M in enumerate([_rot(0.0, 0, 0), _rot(2.3, 65.5, 9.5, -3.25, 4.5), _rot(45.0, 65.5, 9.5), [0.5, 0, 2.0, 0, 0.5, 1.0]]):
        what = (layout, cn, border, i)
        src, dst = roi.pair(layout, roi.case_seed("ex", what), (sw, sh, cn), (dw, dh, cn))
        src.put(img)
        Md = np.ascontiguousarray(M, np.float64)
        with Call(gpu, [src], [dst]) as c:
            out, = c.done(gpu.lib.vs_op_warp_affine_ex(src.ptr, src.pitch, sw, sh, dst.ptr, dst.pitch, dw, dh, cn, capi._p(Md, capi.f64p), border, None), what)
        want = cached(("ex", cn, border, i), lambda: warp_ex_ref(oracle, img, Md, border, dw, dh))
        same(out, want.reshape(dh, dw * cn), what)


def warp_ex_ref(oracle, img, M, border, dw, dh):
    """The oracle's warp has dsize = the source's size.  A destination pixel depends on the matrix, its own coordinates and the
    taps alone, and a tap outside the source is 0 (BORDER_BLACK) or the nearest edge pixel (BORDER_REPLICATE).  So the source is
    extended to max(sw, dw) x max(sh, dh) by black / by replicating its last row and column - every tap then reads what it read
    before, inside the extension or beyond it - warped at that size under the same M, and cropped to dw x dh."""
    sh, sw = img.shape[:2]
    big = np.pad(img, ((0, max(dh - sh, 0)), (0, max(dw - sw, 0)), (0, 0)), mode="constant" if border == capi.BORDER_BLACK else "edge")
    big = np.ascontiguousarray(big if img.shape[2] > 1 else big[..., 0])
    out = oracle.warp_affine_d(big, M, border).reshape(big.shape[0], big.shape[1], -1)
    return np.ascontiguousarray(out[:dh, :dw])


# ---- vs_op_warp_affine_nv12 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_warp_affine_nv12(gpu, oracle, layout, batch):
    """The operator takes the interleaved plane at h * pitch behind the luma plane (it has no offset argument), so a surface is
    an ROI of h * 3 / 2 rows; the parent's padding lies beside the rows of both planes."""
    for w, h in ((130, 18), (256, 32)):
        rows = h * 3 // 2
        groups = [[m] for m in range(6)] if batch == 1 else [[0, 1, 2, 3, 4], [5, 4, 3, 2, 1]]
        for g in groups:
            what = (layout, w, h, g)
            src, dst = roi.pair(layout, roi.case_seed("nv12", what), (w, rows, 1, batch), (w, rows, 1, batch))
            surfs = np.stack([picture(("nv12", k), (rows, w)) for k in range(batch)])
            src.put(surfs)
            M = np.ascontiguousarray([WARP_MATS[m] for m in g], np.float32)
            with Call(gpu, [src], [dst]) as c:
                out, = c.done(gpu.lib.vs_op_warp_affine_nv12(src.ptr, src.pitch, dst.ptr, dst.pitch, w, h, capi._p(M, F32P), batch,
                                                             src.frame_bytes, dst.frame_bytes, None), what)
            out = out.reshape(batch, rows, w)
            for k, m in enumerate(g):
                same(out[k], cached(("nv12", w, h, k, m), lambda: oracle.warp_affine_nv12(surfs[k], w, h, WARP_MATS[m])), what + (k,))


# ---- vs_op_resize_gray ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [capi.FMT_BGR8, capi.FMT_GRAY8, capi.FMT_NV12], ids=["bgr8", "gray8", "nv12"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_resize_gray(gpu, oracle, layout, fmt):
    for (sw, sh), (dw, dh) in (((131, 97), (60, 44)), ((64, 48), (96, 72)), ((132, 98), (66, 49))):      # the last: the exact 2 x path
        if fmt == capi.FMT_NV12:
            sw, sh = sw & ~1, sh & ~1
        cn = 3 if fmt == capi.FMT_BGR8 else 1
        rows = sh * 3 // 2 if fmt == capi.FMT_NV12 else sh
        what = (layout, fmt, sw, sh)
        img = picture(("resize", fmt), (rows, sw, cn))
        src, dst = roi.pair(layout, roi.case_seed("resize", what), (sw, rows, cn), (dw, dh))
        src.put(img)
        with Call(gpu, [src], [dst]) as c:
            out, = c.done(gpu.lib.vs_op_resize_gray(src.ptr, src.pitch, sw, sh, fmt, dst.ptr, dst.pitch, dw, dh, None), what)
        want = cached(("resize", fmt, sw, sh), lambda: oracle.analysis_gray(img[:sh] if cn == 3 else np.ascontiguousarray(img[:sh, :, 0]), dw, dh))
        same(out, want, what)


# ---- vs_op_pyr_down, vs_op_scharr, vs_op_pyr_level -----------------------------------------------------------------------------
PYR_SIZES = [(131, 35), (136, 36), (64, 16)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pyr_down_and_scharr(gpu, oracle, layout):
    for w, h in PYR_SIZES:
        g = picture("pyr0", (h, w))
        dw, dh = (w + 1) // 2, (h + 1) // 2
        what = (layout, w, h)
        src, dst = roi.pair(layout, roi.case_seed("pyr_down", what), (w, h), (dw, dh))
        src.put(g)
        with Call(gpu, [src], [dst]) as c:
            out, = c.done(gpu.lib.vs_op_pyr_down(src.ptr, src.pitch, w, h, dst.ptr, dst.pitch, None), what)
        same(out, cached(("pyr_down", w, h, 0), lambda: oracle.pyr_down(g)), what)
        src, _ = roi.pair(layout, roi.case_seed("scharr", what), (w, h), (1, 1))
        src.put(g)
        der = roi.blob(w * h * 4, roi.case_seed("scharr_der", what))
        with Call(gpu, [src], [der]) as c:
            out, = c.done(gpu.lib.vs_op_scharr(src.ptr, src.pitch, w, h, der.ptr, None), what)
        same(out.view(np.int16), cached(("scharr", w, h, 0), lambda: oracle.scharr(g)), what)


@pytest.mark.parametrize("down", [True, False], ids=["with_next", "derivatives_only"])
@pytest.mark.parametrize("items", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pyr_level(gpu, oracle, layout, items, down):
    for w, h in PYR_SIZES:
        dw, dh = (w + 1) // 2, (h + 1) // 2
        what = (layout, items, down, w, h)
        gs = [picture("pyr%d" % k, (h, w)) for k in range(items)]
        src, nxt = roi.pair(layout, roi.case_seed("pyr_level", what), (w, h, 1, items), (dw, dh, 1, items))
        src.put(np.stack(gs))
        der = roi.blob(items * w * h * 4, roi.case_seed("pyr_level_der", what))
        with Call(gpu, [src], [der] + ([nxt] if down else [])) as c:
            outs = c.done(gpu.lib.vs_op_pyr_level(src.ptr, src.pitch, src.frame_bytes, w, h, der.ptr, nxt.ptr if down else None,
                                                  nxt.pitch, nxt.frame_bytes, items, None), what)
        d = outs[0].view(np.int16).reshape(items, h, w, 2)
        for k in range(items):
            same(d[k], cached(("scharr", w, h, k), lambda: oracle.scharr(gs[k])), what + (k, "der"))
            if down:
                same(outs[1].reshape(items, dh, dw)[k], cached(("pyr_down", w, h, k), lambda: oracle.pyr_down(gs[k])), what + (k, "next"))


# ---- vs_op_pyr_lk ----------------------------------------------------------------------------------------------------------------
def lk_inputs(oracle):
    def make():
        clip = synth.make_clip(synth.SEED_CONFIG1, 320, 240, 2)
        g0, g1 = [oracle.analysis_gray(f, 480, 360) for f in clip]
        pts, _ = oracle.gftt(g0, 120, 0.02, 15.0, 3)
        w, h = 480, 360
        # within half a window of each edge (and outside, and on the corners): reflected padding, status 0 paths
        edge = [[3.5, 180.2], [w - 4.25, 170.0], [240.3, 2.75], [230.0, h - 3.5], [0.5, 0.5], [w - 1.0, h - 1.0], [7.0, 9.0],
                [w - 9.5, h - 8.0], [-30.0, 10.0], [600.0, 20.0], [10.0, 100.5], [w - 10.5, 260.0]]
        return g0, g1, np.ascontiguousarray(np.vstack([pts, np.array(edge, np.float32)]), np.float32)
    return cached("lk_inputs", make)


@pytest.mark.parametrize("win,levels,iters,eps", [(15, 2, 20, 0.03), (21, 2, 20, 0.03), (21, 3, 30, 0.01)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pyr_lk(gpu, oracle, layout, win, levels, iters, eps):
    g0, g1, pts = lk_inputs(oracle)
    h, w = g0.shape
    n = len(pts)
    what = (layout, win, levels)
    # both images are ROIs of one pitch: two frames of one surface (the source side of the layout)
    src = roi.Surface(roi.LAYOUTS[layout][0], w, h, 1, 2, seed=roi.case_seed("lk", what))
    src.put(np.stack([g0, g1]))
    d_pts = roi.blob(n * 8, 1).put(pts)
    o_pts, o_st, o_err = roi.blob(n * 8, 2), roi.blob(n, 3), roi.blob(n * 4, 4)
    with Call(gpu, [src, d_pts], [o_pts, o_st, o_err]) as c:
        got_p, got_s, got_e = c.done(gpu.lib.vs_op_pyr_lk(src.frame_ptr(0), src.frame_ptr(1), src.pitch, w, h, d_pts.ptr, n, o_pts.ptr, o_st.ptr, o_err.ptr,
                                                          win, levels, iters, eps, None), what)
    no, so, eo = cached(("lk", win, levels, iters, eps), lambda: oracle.pyr_lk(g0, g1, pts, win, levels, iters, eps))
    assert 20 < so.sum() < n
    same(got_s, so, what + ("status",))
    same(got_p.view(np.uint32), no.view(np.uint32), what + ("points",))
    same(got_e.view(np.uint32), eo.view(np.uint32), what + ("err",))


# ---- vs_op_gftt ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_eig", [True, False], ids=["eig", "no_eig"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gftt(gpu, oracle, layout, want_eig):
    max_corners = 60
    for w, h in ((135, 97), (160, 64)):
        g = cached(("gftt_img", w, h), lambda: np.ascontiguousarray(oracle.analysis_gray(synth.make_clip(synth.SEED_CONFIG1, 320, 240, 1)[0], 480, 360)[100:100 + h, 150:150 + w]))
        what = (layout, want_eig, w, h)
        src = roi.Surface(roi.LAYOUTS[layout][0], w, h, seed=roi.case_seed("gftt", what)).put(g)
        d_pts, d_cnt = roi.blob(max_corners * 8, 5), roi.blob(4, 6)
        d_eig = roi.blob(w * h * 4, 7)
        with Call(gpu, [src], [d_pts, d_cnt] + ([d_eig] if want_eig else [])) as c:
            outs = c.done(gpu.lib.vs_op_gftt(src.ptr, src.pitch, w, h, max_corners, 0.02, 6.0, 3, d_pts.ptr, d_cnt.ptr,
                                             d_eig.ptr if want_eig else None, None), what)
        ref_pts, _ = cached(("gftt", w, h), lambda: oracle.gftt(g, max_corners, 0.02, 6.0, 3))
        n = int(outs[1].view(np.int32).reshape(-1)[0])
        assert 5 < len(ref_pts) and n == len(ref_pts), what
        same(outs[0].view(np.float32).reshape(-1, 2)[:n].view(np.uint32), ref_pts.view(np.uint32), what)
        if want_eig:
            same(outs[2].view(np.uint32), cached(("min_eigen", w, h), lambda: oracle.min_eigen(g, 3)).view(np.uint32), what + ("eig",))

# ---- vs_op_estimate_affine_partial2d: no picture on either side, the three result buffers guarded -----------------------------
@pytest.mark.parametrize("n,n_out", [(200, 60), (57, 20), (3, 0), (2, 0)])
def test_ransac_result_buffers(gpu, oracle, n, n_out):
    from test_gpu_parity import _correspondences
    a, b = _correspondences(n * 7 + n_out, n, n_out)
    d_a, d_b = roi.blob(n * 8, 11).put(a), roi.blob(n * 8, 12).put(b)
    model, inl, info = roi.blob(48, 13), roi.blob(n, 14), roi.blob(16, 15)
    with Call(gpu, [d_a, d_b], [model, inl, info]) as c:
        gm, gi, gf = c.done(gpu.lib.vs_op_estimate_affine_partial2d(d_a.ptr, d_b.ptr, n, 5.0, 500, model.ptr, inl.ptr, info.ptr, None), (n, n_out))
    ok, mo, io, fo = oracle.estimate_affine_partial2d(a, b)
    same(gf.view(np.int32), fo, (n, "info"))
    same(gi, io, (n, "inliers"))
    if ok:
        same(gm.view(np.uint64), mo.view(np.uint64), (n, "model"))
    else:
        assert np.all(np.isnan(gm.view(np.float64)))


# ---- vs_op_canny, vs_op_hough_lines, vs_op_content_mask ------------------------------------------------------------------------
MASK_SIZES = [(135, 62), (128, 64), (67, 5)]
THETA = np.float32(math.pi / 180)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_canny(gpu, oracle, layout):
    for w, h in MASK_SIZES:
        g = cached(("noisy", w, h), lambda: roll_scene.noisy_gray(w, h, 3))
        for lo, hi in ((50, 150), (10, 30)):
            what = (layout, w, h, lo, hi)
            src, dst = roi.pair(layout, roi.case_seed("canny", what), (w, h), (w, h))
            src.put(g)
            with Call(gpu, [src], [dst]) as c:
                out, = c.done(gpu.lib.vs_op_canny(src.ptr, src.pitch, w, h, lo, hi, dst.ptr, dst.pitch, None), what)
            same(out, cached(("canny", w, h, lo, hi), lambda: oracle.canny(g, lo, hi)), what)
    assert cached(("canny", 135, 62, 10, 30), lambda: None).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hough_lines(gpu, oracle, layout):
    max_lines = 64                                           # 67 x 5 finds 212 lines: the list is cut at the guard
    for w, h in MASK_SIZES:
        def edges():
            e = np.zeros((h, w), np.uint8)
            e[h // 2, :] = 255                               # lines that reach the first and the last column and row
            e[:, w // 3] = 255
            e[np.arange(h), np.arange(h) * (w - 1) // max(h - 1, 1)] = 255
            e[0, :] = 255
            return e
        e = cached(("edges", w, h), edges)
        thr = 4 if h < 10 else 40
        what = (layout, w, h)
        src = roi.Surface(roi.LAYOUTS[layout][0], w, h, seed=roi.case_seed("hough", what)).put(e)
        lines, cnt = roi.blob(max_lines * 8, 8), roi.blob(4, 9)
        with Call(gpu, [src], [lines, cnt]) as c:
            got_l, got_n = c.done(gpu.lib.vs_op_hough_lines(src.ptr, src.pitch, w, h, 1.0, THETA, thr, lines.ptr, max_lines, cnt.ptr, None), what)
        ref = cached(("hough", w, h), lambda: oracle.hough_lines(e, 1.0, THETA, thr))
        n = int(got_n.view(np.int32).reshape(-1)[0])
        assert len(ref) >= 3 and n == min(len(ref), max_lines), (what, n, len(ref))
        assert (len(ref) > max_lines) == (h < 10)
        same(got_l.view(np.uint32).reshape(-1, 2)[:n], ref[:n].view(np.uint32), what)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_content_mask(gpu, oracle, layout, cn):
    for w, h in MASK_SIZES:
        def make():
            rng = np.random.default_rng(w * 7 + cn)
            img = rng.integers(0, 4, (h, w, 3), dtype=np.uint8)      # around the threshold: a busy mask up to every edge
            img[rng.random((h, w)) < 0.6] = 0
            img[h // 4:h // 2, w // 4:w // 2] = 180
            return np.ascontiguousarray(img if cn == 3 else img[..., 1:2])
        img = cached(("mask_img", w, h, cn), make)
        what = (layout, cn, w, h)
        src, dst = roi.pair(layout, roi.case_seed("mask", what), (w, h, cn), (w, h))
        src.put(img)
        with Call(gpu, [src], [dst]) as c:
            out, = c.done(gpu.lib.vs_op_content_mask(src.ptr, src.pitch, w, h, cn, dst.ptr, dst.pitch, None), what)
        same(out, cached(("mask", w, h, cn), lambda: oracle.content_mask(img if cn == 3 else img[..., 0])), what)


# ---- vs_op_copy_make_border, vs_op_fade_update ---------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [capi.BORDER_BLACK, capi.BORDER_REFLECT, capi.BORDER_REFLECT_101, capi.BORDER_REPLICATE, capi.BORDER_WRAP],
                         ids=["black", "reflect", "reflect101", "replicate", "wrap"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_copy_make_border(gpu, oracle, layout, border):
    for (w, h, cn) in ((131, 19, 3), (128, 16, 1), (67, 20, 4)):
        img = picture("border", (h, w, cn))
        for b in (9, 16):
            what = (layout, border, w, h, cn, b)
            ow, oh = w + 2 * b, h + 2 * b
            src, dst = roi.pair(layout, roi.case_seed("border", what), (w, h, cn), (ow, oh, cn))
            src.put(img)
            with Call(gpu, [src], [dst]) as c:
                out, = c.done(gpu.lib.vs_op_copy_make_border(src.ptr, src.pitch, w, h, cn, dst.ptr, dst.pitch, b, border, None), what)
            same(out, cached(("border", w, h, cn, b, border), lambda: oracle.copy_make_border(img if cn > 1 else img[..., 0], b, border)).reshape(oh, ow * cn), what)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fade_update(gpu, layout):
    """The history is packed by definition (a guarded blob); the stabilized frame is the ROI."""
    import compref
    for row_bytes, rows in ((131 * 3, 19), (128, 16), (1, 1)):
        what = (layout, row_bytes, rows)
        hist0, stab = picture("hist", (rows, row_bytes)), picture("stab", (rows, row_bytes))
        src = roi.Surface(roi.LAYOUTS[layout][0], row_bytes, rows, seed=roi.case_seed("fade", what)).put(stab)
        hist = roi.blob(rows * row_bytes, 10).put(hist0)
        with Call(gpu, [src], [hist]) as c:
            out, = c.done(gpu.lib.vs_op_fade_update(hist.ptr, src.ptr, src.pitch, row_bytes, rows, None), what)
        same(out, cached(("fade", row_bytes, rows), lambda: compref.fade_update(hist0, stab)), what)


# ---- vs_enh_apply_dev, vs_enh_apply_batch_dev ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enh(gpu):
    e = capi.Enhancer(gpu)
    yield e
    e.close()


@pytest.mark.parametrize("cfg", ["shipped", "vibrance_only", "wb_only", "clahe_3x3", "denoise_after_unsharp"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_enhancer(gpu, oracle, enh, layout, cfg):
    """The unsharp and NLM windows and the CLAHE histogram see the reflected picture, not the parent: any pixel of the parent that
    entered a window, a white-balance mean or a histogram changes ROI bytes."""
    p = oracle.enh_params(**CONFIGS[cfg])
    n = 3
    for w, h in ((101, 77), (64, 32)):
        frames = [cached(("scene", w, h, s), lambda: scene(w, h, seed=s)) for s in range(n)]
        want = [cached(("enh", cfg, w, h, s), lambda: oracle.enhance(frames[s], p)) for s in range(n)]
        what = (layout, cfg, w, h)
        src, dst = roi.pair(layout, roi.case_seed("enh1", what), (w, h, 3), (w, h, 3))
        src.put(frames[0])
        with Call(gpu, [src], [dst]) as c:
            st = gpu.lib.vs_enh_apply_dev(enh.h, capi.C.byref(p), src.ptr, w, h, src.pitch, dst.ptr, dst.pitch)
            enh._check(st)
            enh.sync()
            out, = c.done(st, what)
        same(out, want[0].reshape(h, w * 3), what)
        src, dst = roi.pair(layout, roi.case_seed("enh3", what), (w, h, 3, n), (w, h, 3, n))
        src.put(np.stack(frames))
        with Call(gpu, [src], [dst]) as c:
            a = (capi.C.c_void_p * n)(*[src.frame_ptr(k) for k in range(n)])
            b = (capi.C.c_void_p * n)(*[dst.frame_ptr(k) for k in range(n)])
            st = gpu.lib.vs_enh_apply_batch_dev(enh.h, capi.C.byref(p), a, b, n, w, h, src.pitch, dst.pitch)
            enh._check(st)
            enh.sync()
            out, = c.done(st, what + ("batch",))
        for k in range(n):
            same(out.reshape(n, h, w * 3)[k], want[k].reshape(h, w * 3), what + ("batch", k))


# ---- vs_roll_correct_dev, vs_azc_apply_dev -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["padded16", "roi_off1", "odd_pitch"])
def test_roll_correct_dev(gpu, oracle, layout):
    w, h, thr = 322, 242, 40                                        # the smallest scene of test_roll.py, its threshold
    ro = oracle.roll_correction(oracle.roll_params(hough_threshold=thr))
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    moved = False
    for i in range(3):
        f = cached(("horizon", i), lambda: roll_scene.horizon_frame(w, h, 20 + i, seed=i, offset=i - 3))
        want = ro.correct(f)
        what = (layout, i)
        src, dst = roi.pair(layout, roi.case_seed("roll", what), (w, h, 3), (w, h, 3))
        src.put(f)
        with Call(gpu, [src], [dst]) as c:
            st = gpu.lib.vs_roll_correct_dev(rg.h, src.ptr, w, h, src.pitch, dst.ptr, dst.pitch)
            rg._check(st)
            rg.sync()
            out, = c.done(st, what)
        assert ro.state() == rg.state(), what
        same(out, want.reshape(h, w * 3), what)
        moved |= ro.state()[0] != 0.0
    assert moved


@pytest.mark.parametrize("layout", ["padded16", "roi_off1", "odd_pitch"])
def test_azc_apply_dev(gpu, oracle, layout):
    w, h = 333, 201                                                 # the smallest scene of test_azc.py
    f = cached("azc_frame", lambda: rotated_frame(oracle, w, h, 3.0, seed=w))
    ref, info = cached("azc_ref", lambda: oracle.auto_zoom_crop(f))
    assert info[7] == 1 and ref.shape == (360, 640, 3)
    az = gpu.auto_zoom_crop()
    src, dst = roi.pair(layout, roi.case_seed("azc", layout), (w, h, 3), (640, 360, 3))
    src.put(f)
    ow, oh = capi.C.c_int(), capi.C.c_int()
    with Call(gpu, [src], [dst]) as c:
        st = gpu.lib.vs_azc_apply_dev(az.h, src.ptr, w, h, src.pitch, 3, dst.ptr, dst.pitch, capi.C.byref(ow), capi.C.byref(oh))
        az._check(st)
        az.sync()
        out, = c.done(st, layout)
    assert (ow.value, oh.value) == (640, 360) and az.info().tolist() == info.tolist()     # the crop rectangle is the oracle's
    same(out, ref.reshape(360, 640 * 3), layout)
