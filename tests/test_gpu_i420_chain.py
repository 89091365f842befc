"""Roll correction and auto zoom/crop on I420 / YV12 / I010 / I012 surfaces, and the chain roll -> stabilize -> zoom on planar
surfaces, bit for bit.

References (include/vs_stab.h, vs_pixfmt_planar / vs_pixfmt_planar16):
  8-bit   the oracle's NV12 functions on the same samples, de-interleaved (vso_roll_correct_nv12, vso_azc_apply_nv12);
  16-bit  tests/ref16_geom.py per plane - warp(plane, M or Mc, BORDER_REPLICATE) for the rotation, crop_scale_surface for the zoom
          (a warp treats channels independently: tests/test_i420_chain_cpu.py) - with angle, line counts, info8 and the rectangle
          from the oracle's NV12 objects run on the analysis bytes min(sample >> (bits - 8), 255).
Inputs: the designs of tests/p010_chain_inputs.py.  Their P010 samples become I420 through the high bytes, I010 / I012 through
synth.p010_to_i010 (sample >> 6 / >> 4): one analysis plane - the high bytes - for every format, so one oracle run serves all.
Whole output buffers are compared, canaries included: a byte written outside the planes fails the comparison."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import i010_inputs
import p010_chain_inputs as inputs
import ref16_geom as geom
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

I420, I010, I012 = capi.FMT_I420, capi.FMT_I010, capi.FMT_I012
NV12, P010 = "nv12", "p010"                # (the two-plane surfaces of the mixed tests)
PLANAR = (I420, I010, I012)
BITS = {I420: 8, I010: 10, I012: 12}
INVALID = 1


def _sb(kind):
    return 1 if kind in (I420, NV12) else 2


def _dtype(kind):
    return np.uint8 if _sb(kind) == 1 else np.uint16


def _canary(kind):
    return 0x5A if _sb(kind) == 1 else 0xA5C3


def surface_planes(p010, w, h, kind):
    """(Y, U, V) of the surface that holds a P010 input's samples in format `kind`."""
    if kind in (I420, NV12):
        return synth.planar_planes(synth.nv12_to_i420(geom.high_bytes(p010)), w, h)
    if kind == P010:
        return np.array(p010[:h]), np.array(p010[h:, 0::2]), np.array(p010[h:, 1::2])
    return synth.planar_planes(synth.p010_to_i010(p010, w, h, BITS[kind]), w, h)


def analysis_nv12(planes, kind):
    """The NV12 surface of the analysis bytes: what the oracle's objects are run on."""
    if kind in (I420, NV12):
        b = planes
    elif kind == P010:
        b = [(p >> 8).astype(np.uint8) for p in planes]
    else:
        b = [i010_inputs.analysis_byte(p, BITS[kind]) for p in planes]
    return interleave(*b)


def interleave(y, u, v):
    """The packed two-plane surface (h * 3 / 2, w) of three planes."""
    h, w = y.shape
    out = np.empty((h * 3 // 2, w), y.dtype)
    out[:h] = y
    out[h:, 0::2] = u
    out[h:, 1::2] = v
    return out


def deinterleave(surf, w, h):
    surf = np.asarray(surf)
    return np.array(surf[:h, :w]), np.array(surf[h:h + h // 2, 0:w:2]), np.array(surf[h:h + h // 2, 1:w:2])


class Layout:
    """Where the planes of a w x h planar surface lie, in bytes, and what is handed to the C ABI for it (zeros: its defaults)."""

    def __init__(self, kind, w, h, style="packed"):
        sb = _sb(kind)
        self.kind, self.w, self.h, self.sb = kind, w, h, sb
        if style == "packed":
            self.pitch, self.c_pitch = w * sb, w * sb // 2
            self.u_off = h * self.pitch
            self.v_off = self.u_off + (h // 2) * self.c_pitch
            self.size = self.v_off + (h // 2) * self.c_pitch
            self.c = capi.i420_layout(self.pitch)                                       # every default
        else:                         # decoder style: padded rows, a gap behind every plane, a chroma pitch of its own; yv12: V before U
            self.pitch = ((w + 63) // 64 * 64 + 64) * sb
            self.c_pitch = ((w // 2 + 31) // 32 * 32 + 32) * sb
            a = self.pitch * (h + 6)
            b = a + self.c_pitch * (h // 2 + 3)
            self.u_off, self.v_off = (b, a) if style == "yv12" else (a, b)
            self.size = b + self.c_pitch * (h // 2 + 2)
            self.c = capi.i420_layout(self.pitch, self.c_pitch, self.u_off, self.v_off)
        if kind in (NV12, P010):      # two planes: packed, the interleaved chroma plane behind the luma rows
            assert style == "packed"
            self.size = w * h * 3 // 2 * sb

    def kw(self):
        return dict(pitch=self.pitch, c_pitch=self.c_pitch, u_off=self.u_off, v_off=self.v_off, size=self.size)

    def pack(self, planes):
        if self.kind in (NV12, P010):
            return interleave(*planes).reshape(-1)
        return synth.planar_from_planes(*planes, fill=_canary(self.kind), **self.kw())

    def blank(self):
        return np.full(self.size // self.sb, _canary(self.kind), _dtype(self.kind))

    def expect(self, planes):
        """The whole buffer after a call that wrote `planes` (of any size that fits) into a blank one."""
        if self.kind in (NV12, P010):
            buf = self.blank().reshape(self.h * 3 // 2, self.w)
            ph, pw = planes[0].shape
            buf[:ph, :pw] = planes[0]
            buf[self.h:self.h + ph // 2, :pw] = interleave(*planes)[ph:]
            return buf.reshape(-1)
        return synth.planar_from_planes(*planes, fill=_canary(self.kind), **self.kw())


# ---- references --------------------------------------------------------------------------------------------------------------------
def rotate_planes(planes, w, h, angle):
    """The roll stage's rotation of three 16-bit planes: ref16_geom.warp per plane, Y under M, U and V under Mc, BORDER_REPLICATE."""
    M, Mc = geom.roll_matrices(w, h, angle)
    return [geom.warp(planes[0], M, None, geom.REPLICATE), geom.warp(planes[1], Mc, None, geom.REPLICATE), geom.warp(planes[2], Mc, None, geom.REPLICATE)]


def oracle_roll(oracle, analysis, w, h, ro=None, **params):
    """The oracle's NV12 roll object over the analysis surfaces: per frame (its NV12 result, its state after the frame)."""
    own = ro is None
    ro = ro or oracle.roll_correction(oracle.roll_params(**params))
    out = []
    for a in analysis:
        r = ro.correct_nv12(a, w, h)
        out.append((r, ro.state()))
    if own:
        ro.close()
    return out


def roll_want(kind, planes, orc, w, h):
    """What the device must give for the surfaces `planes` of format `kind`, given the oracle's run on their analysis bytes."""
    if _sb(kind) == 1:
        return [deinterleave(r, w, h) for r, _ in orc]
    return [rotate_planes(p, w, h, st[0]) for p, (_, st) in zip(planes, orc)]


N_ROLL = 10          # one full batch of eight and a partial one that vs_roll_sync closes; the flat frame (the decay branch) is the sixth


@functools.lru_cache(maxsize=None)
def _roll_case(size, slope):
    return inputs.roll_surfaces(size, slope)[:N_ROLL]


@pytest.fixture(scope="module")
def roll_orc(oracle):
    """Per ROLL_CASES entry: the oracle's run on the high-byte surfaces (the analysis plane of every format here)."""
    out = {}
    for size, slope, _ in inputs.ROLL_CASES:
        w, h = size
        out[(size, slope)] = oracle_roll(oracle, [geom.high_bytes(s) for s in _roll_case(size, slope)], w, h, hough_threshold=inputs.roll_hough_threshold(w))
    return out


_roll_want_cache = {}


def _roll_wanted(kind, size, slope, roll_orc):
    key = (kind, size, slope)
    if key not in _roll_want_cache:
        w, h = size
        planes = [surface_planes(s, w, h, kind) for s in _roll_case(size, slope)]
        _roll_want_cache[key] = (planes, roll_want(kind, planes, roll_orc[(size, slope)], w, h))
    return _roll_want_cache[key]


def roll_run(gpu, rg, frames, array_form=False):
    """frames: [(kind, w, h, planes, Layout in, Layout out)] through the roll object in order; returns the whole result buffers."""
    d_in = [capi.DevBuf.from_array(gpu, li.pack(p)) for _, _, _, p, li, _ in frames]
    d_out = [capi.DevBuf.from_array(gpu, lo.blank()) for _, _, _, _, _, lo in frames]
    try:
        if array_form:
            kind, w, h, _, li, lo = frames[0]
            rg.correct_i420_dev_n(kind, [d.ptr for d in d_in], w, h, li.c, [d.ptr for d in d_out], lo.c)
        else:
            for (kind, w, h, _, li, lo), di, do in zip(frames, d_in, d_out):
                if kind == NV12:
                    rg.correct_nv12_dev(di.ptr, w, h, w, do.ptr, w)
                elif kind == P010:
                    rg.correct_p010_dev(di.ptr, w, h, 2 * w, do.ptr, 2 * w)
                else:
                    rg.correct_i420_dev(kind, di.ptr, w, h, li.c, do.ptr, lo.c)
        rg.sync()
        return [do.download((lo.size // lo.sb,), _dtype(kind)) for (kind, _, _, _, _, lo), do in zip(frames, d_out)]
    finally:
        for d in d_in + d_out:
            d.free()


def check_planes(got_buf, lo, want, what):
    """Plane by plane first (the message names the plane), then the whole buffer: nothing outside the planes was written."""
    if lo.kind in PLANAR:
        ph, pw = want[0].shape
        lay = {k: v for k, v in lo.kw().items() if k != "size"}
        flat = got_buf.reshape(-1)

        def plane(off, pitch, w_, h_):
            return flat[off // lo.sb:(off + h_ * pitch) // lo.sb].reshape(h_, pitch // lo.sb)[:, :w_]
        got = (plane(0, lay["pitch"], pw, ph), plane(lay["u_off"], lay["c_pitch"], pw // 2, ph // 2), plane(lay["v_off"], lay["c_pitch"], pw // 2, ph // 2))
        for name, g, wnt in zip("YUV", got, want):
            assert np.array_equal(g, wnt), (what, name, int((g != wnt).sum()))
    assert np.array_equal(got_buf, lo.expect(want)), (what, "bytes outside the planes were written")


# ---- 1. roll ---------------------------------------------------------------------------------------------------------------------------
ROLL_LAYOUTS = [("packed", "packed"), ("padded", "padded")]


def _roll_test(gpu, roll_orc, kind, size, slope, styles, array_form=False):
    w, h = size
    planes, want = _roll_wanted(kind, size, slope, roll_orc)
    li, lo = Layout(kind, w, h, styles[0]), Layout(kind, w, h, styles[1])
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
    try:
        got = roll_run(gpu, rg, [(kind, w, h, p, li, lo) for p in planes], array_form)
        state = rg.state()
    finally:
        rg.close()
    for i in range(len(planes)):
        check_planes(got[i], lo, want[i], i)
    orc = roll_orc[(size, slope)]
    assert state == orc[-1][1] and state[0] != 0.0                        # smoothed and detected angle, lines found and used
    assert any(st[2] > 0 for _, st in orc) and any(st[2] == 0 for _, st in orc)       # (frames with lines, and the decay branch)
    return got


@pytest.mark.parametrize("styles", ROLL_LAYOUTS, ids=lambda s: s[0])
@pytest.mark.parametrize("size,slope,_padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
@pytest.mark.parametrize("kind", PLANAR, ids=["i420", "i010", "i012"])
def test_roll_correct_planar_matches_the_reference(gpu, roll_orc, kind, size, slope, _padded, styles):
    _roll_test(gpu, roll_orc, kind, size, slope, styles)


@pytest.mark.parametrize("styles", [("yv12", "yv12"), ("packed", "padded")], ids=["yv12", "layouts_differ"])
@pytest.mark.parametrize("kind", PLANAR, ids=["i420", "i010", "i012"])
def test_roll_correct_planar_yv12_and_differing_layouts(gpu, roll_orc, kind, styles):
    size, slope, _ = inputs.ROLL_CASES[1]
    got = _roll_test(gpu, roll_orc, kind, size, slope, styles)
    got_n = _roll_test(gpu, roll_orc, kind, size, slope, styles, array_form=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, got_n))


def test_roll_correct_results_of_one_batch_in_different_layouts(gpu, roll_orc):
    """The results of a batch do not share a layout: the rotation goes frame by frame, the results are the same."""
    size, slope, _ = inputs.ROLL_CASES[1]
    w, h = size
    for kind in (I420, I010):
        planes, want = _roll_wanted(kind, size, slope, roll_orc)
        li = Layout(kind, w, h)
        los = [Layout(kind, w, h, ("packed", "padded", "yv12")[i % 3]) for i in range(len(planes))]
        rg = gpu.roll_correction(gpu.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
        try:
            got = roll_run(gpu, rg, [(kind, w, h, p, li, lo) for p, lo in zip(planes, los)])
            assert rg.state() == roll_orc[(size, slope)][-1][1]
        finally:
            rg.close()
        for i, lo in enumerate(los):
            check_planes(got[i], lo, want[i], (kind, i))


@pytest.mark.parametrize("kind", [I010, I012], ids=["i010", "i012"])
def test_roll_correct_out_of_range_samples_saturate_the_analysis_byte(gpu, oracle, kind):
    """Samples >= 2^bits in a block of Y and in stripes of U: the analysis byte there is 255 (not the wrapped low bits), the rotation
    blends all sixteen bits."""
    size, slope, _ = inputs.ROLL_CASES[1]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    planes = []
    for s in _roll_case(size, slope):
        y, u, v = surface_planes(s, w, h, kind)
        y[h // 5:h // 2, w // 3:w // 3 + 90] |= 1 << BITS[kind]           # (bit `bits` set: min(sample >> shift, 255) = 255; wrapped it would be the low byte)
        y[0:9, :] |= 0x8000
        u[::5] |= 0xC000
        planes.append((y, u, v))
    analysis = [analysis_nv12(p, kind) for p in planes]
    assert all((a[h // 5:h // 2, w // 3:w // 3 + 90] == 255).all() for a in analysis)
    wrapped = [interleave(*[(q >> (BITS[kind] - 8)).astype(np.uint8) for q in p]) for p in planes]
    orc = oracle_roll(oracle, analysis, w, h, hough_threshold=thr)
    assert orc[-1][1] != oracle_roll(oracle, wrapped, w, h, hough_threshold=thr)[-1][1], "the saturation does not show in the state"
    want = roll_want(kind, planes, orc, w, h)
    lay = Layout(kind, w, h, "padded")
    rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
    try:
        got = roll_run(gpu, rg, [(kind, w, h, p, lay, lay) for p in planes])
        assert rg.state() == orc[-1][1]
    finally:
        rg.close()
    for i in range(len(planes)):
        check_planes(got[i], lay, want[i], i)


@pytest.mark.parametrize("size", [(34, 18), (260, 66)], ids=["narrower_than_a_tile", "straddles_the_tiles_of_both_plane_sizes"])
@pytest.mark.parametrize("kind", PLANAR, ids=["i420", "i010", "i012"])
def test_roll_correct_small_pictures_on_the_tile_staging(gpu, oracle, kind, size):
    """16-bit tiles are 128 x 32: 34 x 18 (chroma 17 x 9) is narrower than one, 260 x 66 (chroma 130 x 33) ends four / two columns and
    two / one rows into a new one in either plane size.  Pictures this small hold no line, so three frames of a ROLL_CASES scene go
    first through the same object, with a smoothing that follows the detected angle at once: the small pictures are rotated by degrees."""
    w, h = size
    big, slope, _ = inputs.ROLL_CASES[0]
    bw, bh = big
    par = dict(hough_threshold=inputs.roll_hough_threshold(bw), angle_smoothing_alpha=0.9, max_angle_change_deg=10.0)
    lead = [surface_planes(s, bw, bh, kind) for s in _roll_case(big, slope)[:3]]
    rng = np.random.default_rng(w * 100 + h + BITS[kind])
    hi = 1 << (16 if kind != I420 else 8)
    small = [tuple(rng.integers(0, hi, shp, _dtype(kind)) for shp in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for _ in range(9)]
    ro = oracle.roll_correction(oracle.roll_params(**par))
    orc_lead = oracle_roll(oracle, [analysis_nv12(p, kind) for p in lead], bw, bh, ro=ro)
    orc = oracle_roll(oracle, [analysis_nv12(p, kind) for p in small], w, h, ro=ro)
    ro.close()
    assert abs(orc[0][1][0]) > 1.0 and abs(orc[-1][1][0]) > 1.0, "the small pictures are not rotated"
    want_lead, want = roll_want(kind, lead, orc_lead, bw, bh), roll_want(kind, small, orc, w, h)
    lb, ls = Layout(kind, bw, bh), Layout(kind, w, h, "padded")
    rg = gpu.roll_correction(gpu.roll_params(**par))
    try:
        got = roll_run(gpu, rg, [(kind, bw, bh, p, lb, lb) for p in lead] + [(kind, w, h, p, ls, ls) for p in small])
        assert rg.state() == orc[-1][1]
    finally:
        rg.close()
    for i in range(3):
        check_planes(got[i], lb, want_lead[i], ("lead", i))
    for i in range(len(small)):
        check_planes(got[3 + i], ls, want[i], i)


# ---- 2. zoom ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoom_orc(oracle):
    """Per size: the oracle's NV12 auto zoom/crop on the high-byte surfaces - (NV12 result, info8) per surface."""
    return {size: [oracle.auto_zoom_crop_nv12(geom.high_bytes(s), size[0], size[1]) for s in inputs.zoom_surfaces(oracle, size)] for size in inputs.ZOOM_SIZES}


def zoom_want(kind, planes, orc, w, h):
    out = []
    for p, (res, info) in zip(planes, orc):
        ow, oh = (640, 360) if info[7] else (w, h)
        if _sb(kind) == 1:
            out.append(deinterleave(res, ow, oh))
        else:
            out.append(deinterleave(geom.crop_scale_surface(interleave(*p), w, h, info), ow, oh))
    return out


def zoom_run(gpu, az, frames, n_single=None):
    """frames: [(kind, w, h, planes, Layout in, Layout out)]; the first n_single one by one, the rest (planar, one layout) through the
    array form.  Returns per frame (ticket, ow, oh, info8) and the whole result buffers."""
    n = len(frames)
    n_single = n if n_single is None else n_single
    d_in = [capi.DevBuf.from_array(gpu, li.pack(p)) for _, _, _, p, li, _ in frames]
    d_out = [capi.DevBuf.from_array(gpu, lo.blank()) for _, _, _, _, _, lo in frames]
    try:
        tickets = []
        for (kind, w, h, _, li, lo), di, do in list(zip(frames, d_in, d_out))[:n_single]:
            if kind == NV12:
                tickets.append(az.apply_nv12_dev(di.ptr, w, h, w, do.ptr, lo.w, lo.w * lo.h))
            elif kind == P010:
                tickets.append(az.apply_p010_dev(di.ptr, w, h, 2 * w, do.ptr, 2 * lo.w, 2 * lo.w * lo.h))
            else:
                tickets.append(az.apply_i420_dev(kind, di.ptr, w, h, li.c, do.ptr, lo.c))
        if n_single < n:
            kind, w, h, _, li, lo = frames[n_single]
            tickets += az.apply_i420_dev_n(kind, [d.ptr for d in d_in[n_single:]], w, h, li.c, [d.ptr for d in d_out[n_single:]], lo.c)
        az.sync()
        res = []
        for t in tickets:
            ow, oh, info = az.result(t)
            res.append((t, ow, oh, info.tolist()))
        return res, [do.download((lo.size // lo.sb,), _dtype(kind)) for (kind, _, _, _, _, lo), do in zip(frames, d_out)]
    finally:
        for d in d_in + d_out:
            d.free()


@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=["wide_mask_800", "wide_mask_808", "general_mask_804"])
@pytest.mark.parametrize("kind", PLANAR, ids=["i420", "i010", "i012"])
def test_auto_zoom_crop_planar_matches_the_reference(gpu, oracle, zoom_orc, kind, size):
    """Twelve surfaces pushed without waiting (a batch of eight and one of four): tickets, info8 and sizes equal the oracle's on the
    analysis bytes; the planes equal the reference - 640 x 360 / 320 x 180 / 320 x 180, or the unchanged surface on the fall-back
    paths (the all-black surface and whatever else the oracle does not crop).  800: the wide mask path of both sample sizes; 808: wide
    for 16-bit samples, general for 8-bit; 804: general for both.  The padded result layout at 804."""
    w, h = size
    orc = zoom_orc[size]
    planes = [surface_planes(s, w, h, kind) for s in inputs.zoom_surfaces(oracle, size)]
    want = zoom_want(kind, planes, orc, w, h)
    li = Layout(kind, w, h, "padded" if w == 808 else "packed")
    lo = Layout(kind, max(w, 640), max(h, 360), "yv12" if w == 804 else "packed")
    az = gpu.auto_zoom_crop()
    try:
        res, bufs = zoom_run(gpu, az, [(kind, w, h, p, li, lo) for p in planes], n_single=5)
        wt = az.worker_times()
    finally:
        az.close()
    cropped = 0
    for i, ((t, ow, oh, ginfo), (_, info)) in enumerate(zip(res, orc)):
        assert t == i and ginfo == info.tolist(), i
        assert (ow, oh) == ((640, 360) if info[7] else (w, h)), i
        check_planes(bufs[i], lo, want[i], i)
        cropped += int(info[7])
    assert 9 <= cropped <= 11 and not orc[3][1][7]              # (both outcomes occur; the all-black surface comes back unchanged)
    assert wt[0] == len(planes) and wt[5] == 2                  # two batches: 8 + 4


@pytest.mark.parametrize("kind", PLANAR, ids=["i420", "i010", "i012"])
def test_auto_zoom_crop_planar_fall_back_paths_return_the_surface_unchanged(gpu, oracle, kind):
    """Both fall-back paths of the reference: no contour (an all-black Y plane) and an empty crop (one row of content: a contour, but
    no rectangle).  The w x h surface comes back unchanged, all three planes with their live chroma and low bits; then a cropped one."""
    w, h = inputs.ZOOM_SIZES[2]
    base = surface_planes(inputs.zoom_surfaces(oracle, (w, h))[0], w, h, kind)
    shift = BITS[kind] - 8
    planes = []
    for case in range(3):
        y, u, v = (np.array(q) for q in base)
        if case < 2:
            y[:] = 1 << shift if case else 0              # (analysis byte 1 is not content either)
        if case == 1:
            y[100, 100:300] = 200 << shift
        planes.append((y, u, v))
    orc = [oracle.auto_zoom_crop_nv12(analysis_nv12(p, kind), w, h) for p in planes]
    assert [(int(i[0]) > 0, int(i[7])) for _, i in orc] == [(False, 0), (True, 0), (True, 1)]
    want = zoom_want(kind, planes, orc, w, h)
    assert all(np.array_equal(a, b) for k in range(2) for a, b in zip(want[k], planes[k]))
    li, lo = Layout(kind, w, h, "padded"), Layout(kind, max(w, 640), max(h, 360), "padded")
    az = gpu.auto_zoom_crop()
    try:
        res, bufs = zoom_run(gpu, az, [(kind, w, h, p, li, lo) for p in planes])
    finally:
        az.close()
    for i in range(3):
        assert res[i][1:] == ((640, 360) if orc[i][1][7] else (w, h)) + (orc[i][1].tolist(),), i
        check_planes(bufs[i], lo, want[i], i)


@pytest.mark.parametrize("kind", [I010, I012], ids=["i010", "i012"])
def test_auto_zoom_crop_out_of_range_samples_are_content(gpu, oracle, kind):
    """A Y plane of zeros with a block of samples whose value bits are 0 or 1 but whose higher bits are set: min(sample >> shift, 255)
    = 255 > 1, content, and the surface is cropped to it; taken modulo 256 the byte would be 0 and the picture all black."""
    w, h = inputs.ZOOM_SIZES[2]
    base = surface_planes(inputs.zoom_surfaces(oracle, (w, h))[0], w, h, kind)
    shift = BITS[kind] - 8
    planes = []
    for k in range(2):
        y, u, v = (np.array(q) for q in base)
        y[:] = 0
        y[40:h - 60, 30:w - 200] = (0x100 << shift << k) | k
        planes.append((y, u, v))
    orc = [oracle.auto_zoom_crop_nv12(analysis_nv12(p, kind), w, h) for p in planes]
    assert all(info[7] for _, info in orc)
    assert not oracle.auto_zoom_crop_nv12(interleave(*[(q >> shift).astype(np.uint8) for q in planes[0]]), w, h)[1][7]
    want = zoom_want(kind, planes, orc, w, h)
    li, lo = Layout(kind, w, h), Layout(kind, max(w, 640), max(h, 360))
    az = gpu.auto_zoom_crop()
    try:
        res, bufs = zoom_run(gpu, az, [(kind, w, h, p, li, lo) for p in planes])
    finally:
        az.close()
    for i in range(2):
        assert res[i][3] == orc[i][1].tolist()
        check_planes(bufs[i], lo, want[i], i)


# ---- 3. NV12, I420, P010 and I010 through one object ---------------------------------------------------------------------------------
MIX = [NV12, I420, P010, I010]


def test_roll_object_takes_two_plane_and_planar_surfaces_alternately(gpu, oracle, roll_orc):
    """Every call changes the format and closes the pending batch.  All four formats share one analysis plane, so the smoothed angle
    of the mixed run must follow the oracle's one sequence across every change, and frame i must come out as it does from an
    object that saw the same i frames before it in its own format: the unmixed run of that format."""
    size, slope, _ = inputs.ROLL_CASES[1]
    w, h = size
    thr = inputs.roll_hough_threshold(w)
    surfs = _roll_case(size, slope)
    orc = roll_orc[(size, slope)]

    def run(kind_of):
        rg = gpu.roll_correction(gpu.roll_params(hough_threshold=thr))
        try:
            frames = []
            for i, s in enumerate(surfs):
                k = kind_of(i)
                lay = Layout(k, w, h)
                frames.append((k, w, h, surface_planes(s, w, h, k), lay, lay))
            return roll_run(gpu, rg, frames), rg.state()
        finally:
            rg.close()

    mixed, sm = run(lambda i: MIX[i % 4])
    assert sm == orc[-1][1] and sm[0] != 0.0
    for j, k in enumerate(MIX):
        only, so = run(lambda i, k=k: k)
        assert so == sm, k
        for i in range(j, len(surfs), 4):
            assert mixed[i].dtype == only[i].dtype and np.array_equal(mixed[i], only[i]), (k, i)
        if k in (NV12, I420):
            for i in range(len(surfs)):
                assert np.array_equal(only[i], Layout(k, w, h).expect(deinterleave(orc[i][0], w, h))), (k, i)


def test_zoom_object_takes_two_plane_and_planar_surfaces_alternately(gpu, oracle, zoom_orc):
    size = inputs.ZOOM_SIZES[1]
    w, h = size
    surfs = inputs.zoom_surfaces(oracle, size)
    orc = zoom_orc[size]

    def run(kind_of):
        az = gpu.auto_zoom_crop()
        try:
            frames = []
            for i, s in enumerate(surfs):
                k = kind_of(i)
                frames.append((k, w, h, surface_planes(s, w, h, k), Layout(k, w, h), Layout(k, max(w, 640), max(h, 360))))
            res, bufs = zoom_run(gpu, az, frames)
            return res, bufs, az.worker_times()
        finally:
            az.close()

    mres, mbufs, wt = run(lambda i: MIX[i % 4])
    assert wt[0] == len(surfs) and wt[5] == len(surfs)           # (every call closed the batch of the one before)
    for j, k in enumerate(MIX):
        ores, obufs, _ = run(lambda i, k=k: k)
        for i in range(len(surfs)):
            assert ores[i][3] == orc[i][1].tolist(), (k, i)
        for i in range(j, len(surfs), 4):
            assert mres[i] == ores[i], (k, i)
            assert mbufs[i].dtype == obufs[i].dtype and np.array_equal(mbufs[i], obufs[i]), (k, i)


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------------
def run_chain_planar(vs, kind, W, H, CH, batch, params, n_chunks, src, overlap):
    """tests/test_gpu_chain.py::run_chain for planar surfaces in the packed layout (kind NV12: the two-plane entry points, for the
    reference run), rings of two slots and lags of one: roll(c) writes
    ring slot c % 2, stab(c) pushes those (batch mode, zero-copy) into its slot c % 2, zoom(c) crops those into its slot c % 2.
    overlap: one host thread per stage.  One chunk more than n_chunks: the stabilizer's flush.  Returns [(ow, oh, info8, Y, U, V)],
    the roll stage's state and the stabilizer's frames_out."""
    lay = Layout(kind, W, H)
    sb = lay.size
    bufs = [capi.DevBuf(vs, sb * CH) for _ in range(6)]
    d_roll, d_stab, d_zoom = bufs[:2], bufs[2:4], bufs[4:]
    rc, az, st = vs.roll_correction(), vs.auto_zoom_crop(), vs.stabilizer(params)
    st.set_batch(batch)
    st.set_zero_copy(True)
    produced, results = {}, []
    total = n_chunks + 1

    def roll_stage(c):
        if c < n_chunks:
            ins, outs = [src(c * CH + i) for i in range(CH)], [d_roll[c % 2].ptr + i * sb for i in range(CH)]
            if kind == NV12:
                rc.correct_nv12_dev_n(ins, W, H, W, outs, W)
            else:
                rc.correct_i420_dev_n(kind, ins, W, H, lay.c, outs, lay.c)
            rc.sync()

    def stab_stage(c):
        out = d_stab[c % 2].ptr
        if c < n_chunks:
            produced[c] = st.push_dev_n([d_roll[c % 2].ptr + i * sb for i in range(CH)], W, H, lay.pitch, capi.FMT_NV12 if kind == NV12 else kind,
                                        [out + j * sb for j in range(CH)], lay.pitch)
        else:
            k = 0
            while st.flush_dev(out + k * sb, lay.pitch):
                k += 1
                assert k <= CH, "the flush holds more than a chunk"
            produced[c] = k
        st.sync()

    def zoom_stage(c):
        k = produced[c]
        if not k:
            return
        slot = d_zoom[c % 2]
        ins, outs = [d_stab[c % 2].ptr + j * sb for j in range(k)], [slot.ptr + j * sb for j in range(k)]
        if kind == NV12:
            tickets = az.apply_nv12_dev_n(ins, W, H, W, outs, W, W * H)
        else:
            tickets = az.apply_i420_dev_n(kind, ins, W, H, lay.c, outs, lay.c)
        az.sync()
        for j, t in enumerate(tickets):
            ow, oh, info = az.result(t)
            buf = slot.download((sb // lay.sb,), _dtype(kind), j * sb)
            if kind == NV12:
                surf = buf.reshape(H * 3 // 2, W)
                y, u, v = surf[:H], surf[H:, 0::2], surf[H:, 1::2]
            else:
                y, u, v = synth.planar_planes(buf, W, H)
            results.append((ow, oh, info.tolist(), y[:oh, :ow], u[:oh // 2, :ow // 2], v[:oh // 2, :ow // 2]))

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

            def stage_loop(name, f, before, after):
                try:
                    for c in range(total):
                        if before and not wait_for(before, c):
                            return
                        if after and not wait_for(after, c - 1):
                            return
                        f(c)
                        with cond:
                            done[name] = c
                            cond.notify_all()
                except BaseException as e:          # (a failed stage must not leave the others waiting)
                    with cond:
                        failed.append(e)
                        cond.notify_all()

            ths = [threading.Thread(target=stage_loop, args=a) for a in (("roll", roll_stage, None, "stab"), ("stab", stab_stage, "roll", "zoom"),
                                                                         ("zoom", zoom_stage, "stab", None))]
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


CHAIN_N, CHAIN_CH = 8, 4
CHAIN_PARAMS = dict(smoothing_radius=2, max_corners=400)


def _chain_runs(gpu, kind, W, H):
    surfs = inputs.chain_surfaces(CHAIN_N)
    lay = Layout(kind, W, H)
    d_in = [capi.DevBuf.from_array(gpu, lay.pack(surface_planes(s, W, H, kind))) for s in surfs]
    try:
        runs = [run_chain_planar(gpu, kind, W, H, CHAIN_CH, CHAIN_CH, gpu.params(**CHAIN_PARAMS), CHAIN_N // CHAIN_CH, lambda i: d_in[i].ptr, o)
                for o in (False, True)]
    finally:
        for d in d_in:
            d.free()
    (ser, ser_state, ser_out), (got, state, out) = runs
    assert len(got) == len(ser) == CHAIN_N and out == ser_out == CHAIN_N and state == ser_state
    for j, (a, b) in enumerate(zip(got, ser)):
        assert a[:3] == b[:3], j
        assert all(np.array_equal(p, q) for p, q in zip(a[3:], b[3:])), j
    return ser, ser_state


def test_i420_chain_overlapped_equals_serial_equals_the_nv12_chain(gpu):
    """roll -> stabilize (batch mode, VS_FMT_I420) -> zoom on eight 704 x 400 surfaces in two chunks plus the flush: serial and
    overlapped give identical bytes, and they are the NV12 chain's on the same samples, de-interleaved."""
    W, H = inputs.CHAIN_SIZE
    ser, state = _chain_runs(gpu, I420, W, H)
    lay = Layout(NV12, W, H)
    d_in = [capi.DevBuf.from_array(gpu, lay.pack(surface_planes(s, W, H, NV12))) for s in inputs.chain_surfaces(CHAIN_N)]
    try:
        ref, ref_state, ref_out = run_chain_planar(gpu, NV12, W, H, CHAIN_CH, CHAIN_CH, gpu.params(**CHAIN_PARAMS), CHAIN_N // CHAIN_CH, lambda i: d_in[i].ptr, False)
    finally:
        for d in d_in:
            d.free()
    assert ref_out == CHAIN_N and len(ref) == CHAIN_N and state == ref_state and state[0] != 0.0
    assert sum(r[2][7] for r in ref) > 0
    for j, (a, b) in enumerate(zip(ser, ref)):
        assert a[:3] == b[:3], j
        for name, g, wnt in zip("YUV", a[3:], b[3:]):
            assert g.dtype == wnt.dtype and np.array_equal(g, wnt), (j, name)


def test_i010_chain_overlapped_equals_serial_equals_the_composed_references(gpu, oracle):
    """The same chain on I010 surfaces against the references composed stage by stage: ref16_geom rotation per plane with the
    oracle's angle; the oracle's stabilizer on the analysis bytes of the rolled surfaces for the matrices and
    i010_inputs.warp_three_planes for the pixels (the last frame comes back unwarped); ref16_geom crop-and-scale with the oracle's
    info8 on the analysis bytes of the stabilized surfaces."""
    from test_gpu_p010 import _oracle_nv12_run
    W, H = inputs.CHAIN_SIZE
    ser, state = _chain_runs(gpu, I010, W, H)
    planes = [surface_planes(s, W, H, I010) for s in inputs.chain_surfaces(CHAIN_N)]
    ro = oracle.roll_correction()
    rolled = []
    for p in planes:
        ro.correct_nv12(analysis_nv12(p, I010), W, H)
        rolled.append(rotate_planes(p, W, H, ro.state()[0]))
    ref_state = ro.state()
    ro.close()
    assert state == ref_state and ref_state[0] != 0.0
    outs, _ = _oracle_nv12_run(oracle, [analysis_nv12(p, I010) for p in rolled], **CHAIN_PARAMS)
    assert len(outs) == CHAIN_N
    n_crop = 0
    for j, ((idx, M), (ow, oh, info, y, u, v)) in enumerate(zip(outs, ser)):
        if idx == CHAIN_N - 1:
            stab = rolled[idx]
        else:
            packed = np.concatenate([q.reshape(-1) for q in rolled[idx]]).reshape(H * 3 // 2, W)
            stab = i010_inputs.planes(i010_inputs.warp_three_planes(packed, W, H, M), W, H)
        _, winfo = oracle.auto_zoom_crop_nv12(analysis_nv12(stab, I010), W, H)
        assert info == winfo.tolist(), j
        assert (ow, oh) == ((640, 360) if winfo[7] else (W, H)), j
        for name, g, wnt in zip("YUV", (y, u, v), zoom_want(I010, [stab], [(None, winfo)], W, H)[0]):
            assert np.array_equal(g, wnt), (j, name)
        n_crop += int(winfo[7])
    assert n_crop > 0


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _lay(**kw):
    return capi.i420_layout(kw.get("pitch", 0), kw.get("c_pitch", 0), kw.get("u_off", 0), kw.get("v_off", 0))


@pytest.mark.parametrize("kind,name", [(I420, "I420"), (I010, "I010"), (I012, "I012")], ids=["i420", "i010", "i012"])
def test_planar_entry_points_refuse_bad_geometry_and_layouts(gpu, kind, name):
    """VS_ERR_INVALID_ARG with a text that names the format, for both stages; nothing is queued by a refused call."""
    sb = _sb(kind)
    w, h = 64, 48
    d = capi.DevBuf(gpu, 4 << 20)
    half = 2 << 20
    rg, az = gpu.roll_correction(), gpu.auto_zoom_crop()
    t = C.c_int64(-1)
    good_in = dict(pitch=w * sb)
    good_roll_out = dict(pitch=w * sb)
    good_zoom_out = dict(pitch=640 * sb)

    def roll(w_=w, h_=h, lin=good_in, lout=good_roll_out, off=0, ooff=0):
        rc = gpu.lib.vs_roll_correct_i420_dev(rg.h, kind, C.c_void_p(d.ptr + off), w_, h_, C.byref(_lay(**lin)), C.c_void_p(d.ptr + half + ooff), C.byref(_lay(**lout)))
        return rc, (gpu.lib.vs_roll_last_error(rg.h) or b"").decode()

    def zoom(w_=w, h_=h, lin=good_in, lout=good_zoom_out, off=0, ooff=0):
        rc = gpu.lib.vs_azc_apply_i420_dev(az.h, kind, C.c_void_p(d.ptr + off), w_, h_, C.byref(_lay(**lin)), C.c_void_p(d.ptr + half + ooff), C.byref(_lay(**lout)),
                                           C.byref(t))
        return rc, (gpu.lib.vs_azc_last_error(az.h) or b"").decode()

    bad = [dict(w_=63), dict(h_=47),                                                        # odd geometry
           dict(lin=dict(pitch=w * sb - 2)), dict(lin=dict(pitch=w * sb, c_pitch=w * sb // 2 - 2)),      # a pitch below a row; I010: a chroma pitch below w bytes
           dict(lin=dict(pitch=w * sb, u_off=w * sb * h - 2))]                                # U inside the luma rows
    if sb == 2:
        bad += [dict(lin=dict(pitch=2 * w + 1)), dict(lin=dict(pitch=2 * w, c_pitch=w + 1)), dict(lin=dict(pitch=2 * w, u_off=2 * w * h + 1)),
                dict(lin=dict(pitch=2 * w, v_off=2 * w * h * 2 + 1)), dict(off=1), dict(ooff=1),
                dict(lin=dict(pitch=2 * w + 2))]                                              # (the default chroma pitch needs a multiple of 4)
    else:
        bad += [dict(lin=dict(pitch=w + 1))]                                                  # (the default chroma pitch needs an even pitch)
    for f, good_out, small_out in ((roll, good_roll_out, dict(pitch=w * sb - 2)), (zoom, good_zoom_out, dict(pitch=640 * sb - 2))):
        cases = bad + [dict(lout=small_out),                                                  # an undersized result layout: the pitch,
                       dict(lout=dict(good_out, c_pitch=good_out["pitch"] // 2 - 2))]         # the chroma pitch,
        if f is zoom:
            cases += [dict(lout=dict(good_out, u_off=good_out["pitch"] * 359)),               # U less than max(h, 360) rows behind Y,
                      dict(lout=dict(good_out, u_off=good_out["pitch"] * 360, v_off=good_out["pitch"] * 360 + good_out["pitch"] // 2 * 179))]   # V inside U
        for kw in cases:
            rc, msg = f(**kw)
            assert rc == INVALID and name in msg, (f.__name__, kw, rc, msg)
    rc, msg = roll()
    assert rc == 0, msg
    rc, msg = zoom()
    assert rc == 0 and t.value == 0, msg
    assert gpu.lib.vs_roll_correct_i420_dev(rg.h, capi.FMT_NV12, C.c_void_p(d.ptr), w, h, C.byref(_lay(**good_in)), C.c_void_p(d.ptr + half), C.byref(_lay(**good_roll_out))) == INVALID
    assert gpu.lib.vs_azc_apply_i420_dev(az.h, capi.FMT_P010, C.c_void_p(d.ptr), w, h, C.byref(_lay(**good_in)), C.c_void_p(d.ptr + half), C.byref(_lay(**good_zoom_out)), C.byref(t)) == INVALID
    rg.sync()
    az.sync()
    rg.close()
    az.close()
    d.free()
