"""Roll correction and auto zoom/crop on planar 4:2:2 / 4:4:4 surfaces (I422, I444, I210, I212, I410, I412), and the chain
roll -> stabilize -> zoom on them, bit for bit.

Reference: tests/planar_chain_ref.py - include/vs_stab.h's definitions with the chroma shifts explicit, on ref16_geom.warp; angle and
info8 come from the oracle's NV12 objects run on the analysis plane of Y.  tests/test_planar_chain_cpu.py pins that reference to the
oracle's cv::warpAffine and to the 4:2:0 references, and asserts what the inputs (tests/planar_chain_inputs.py) must hold: angles near
1, 3 and 8 degrees and never 0, cropped zoom scenes, rounding ties in the chroma of the 16-bit surfaces.
Whole result buffers are compared, canaries included: a sample written outside the planes fails the comparison.
The last section holds vs_op_warp_affine_planar with BORDER_REPLICATE on I422 / I210 at angles on both sides of the two staging limits of
4:2:2 chroma tiles (the launcher's choice between the kernel instances must not show in a single sample).
Layouts go with the geometry: 130 x 96 packed; 322 x 200 padded pitches with the planes apart, the result V before U; 704 x 400 a
chroma pitch of its own (default offsets), the result padded."""
import ctypes as C

import numpy as np
import pytest

import planar_chain_inputs as inp
import planar_chain_ref as ref
import planar_inputs as pin
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

INVALID = 1
FMTV = {n: capi.PIXFMT_BY_NAME[n].fmt for n in ref.ALL}
SIZE_IDS = ["130x96", "322x200", "704x400"]
STYLES = {(130, 96): ("packed", "packed"), (322, 200): ("padded", "vfirst"), (704, 400): ("cpitch", "padded")}


class Lay:
    """Where the planes of a w x h surface of format `fmt` lie, in bytes, and what the C ABI is told about it (zeros: its defaults)."""

    def __init__(self, fmt, w, h, style="packed"):
        sx, sy = ref.shifts(fmt)
        sb = 1 if ref.bits(fmt) == 8 else 2
        self.fmt, self.w, self.h, self.sb, self.sx, self.sy = fmt, w, h, sb, sx, sy
        self.dtype = np.uint8 if sb == 1 else np.uint16
        self.canary = 0x5A if sb == 1 else 0xA5C3
        cw, ch = w >> sx, h >> sy
        if style in ("packed", "cpitch"):
            self.pitch = w * sb
            self.c_pitch = self.pitch >> sx if style == "packed" else (cw + 10) * sb
            self.u_off = h * self.pitch
            self.v_off = self.u_off + ch * self.c_pitch
            self.size = self.v_off + ch * self.c_pitch
            self.c = capi.i420_layout(self.pitch, 0 if style == "packed" else self.c_pitch)
        else:                         # padded rows, a gap behind every plane, a chroma pitch of its own; vfirst: V before U
            self.pitch = ((w + 63) // 64 * 64 + 64) * sb
            self.c_pitch = ((cw + 31) // 32 * 32 + 32) * sb
            a = self.pitch * (h + 6)
            b = a + self.c_pitch * (ch + 3)
            self.u_off, self.v_off = (b, a) if style == "vfirst" else (a, b)
            self.size = b + self.c_pitch * (ch + 2)
            self.c = capi.i420_layout(self.pitch, self.c_pitch, self.u_off, self.v_off)

    def buffer(self, planes):
        """The whole buffer that holds `planes` (of any size that fits) where the layout puts them, canaries everywhere else."""
        return synth.yuv_pack(*planes, self.sx, self.sy, self.pitch, self.c_pitch, self.u_off, self.v_off, self.size, self.canary)

    def blank(self):
        return np.full(self.size // self.sb, self.canary, self.dtype)

    def planes(self, buf, pw, ph):
        return synth.yuv_unpack(np.asarray(buf, self.dtype), pw, ph, self.sx, self.sy, self.pitch, self.c_pitch, self.u_off, self.v_off)


def check(got_buf, lo, want, what):
    """Plane by plane first (the message names the plane), then the whole buffer: nothing outside the planes was written."""
    ph, pw = want[0].shape
    for name, g, wnt in zip("YUV", lo.planes(got_buf, pw, ph), want):
        assert g.shape == wnt.shape and np.array_equal(g, wnt), (what, name, int((g != wnt).sum()))
    assert np.array_equal(got_buf, lo.buffer(want)), (what, "samples outside the planes were written")


def roll_run(gpu, rg, frames, array_form=False):
    """frames: [(fmt, planes, Lay in, Lay out)] through the roll object in order; returns the whole result buffers."""
    d_in = [capi.DevBuf.from_array(gpu, li.buffer(p)) for _, p, li, _ in frames]
    d_out = [capi.DevBuf.from_array(gpu, lo.blank()) for _, _, _, lo in frames]
    try:
        if array_form:
            fmt, _, li, lo = frames[0]
            rg.correct_i420_dev_n(FMTV[fmt], [d.ptr for d in d_in], li.w, li.h, li.c, [d.ptr for d in d_out], lo.c)
        else:
            for (fmt, _, li, lo), di, do in zip(frames, d_in, d_out):
                rg.correct_i420_dev(FMTV[fmt], di.ptr, li.w, li.h, li.c, do.ptr, lo.c)
        rg.sync()
        return [do.download((lo.size // lo.sb,), lo.dtype) for (_, _, _, lo), do in zip(frames, d_out)]
    finally:
        for d in d_in + d_out:
            d.free()


def zoom_run(gpu, az, frames, n_single=None):
    """frames: [(fmt, planes, Lay in, Lay out)]; the first n_single one by one, the rest (one format and layout) through the array form.
    Returns per frame (ticket, ow, oh, info8) and the whole result buffers."""
    n = len(frames)
    n_single = n if n_single is None else n_single
    d_in = [capi.DevBuf.from_array(gpu, li.buffer(p)) for _, p, li, _ in frames]
    d_out = [capi.DevBuf.from_array(gpu, lo.blank()) for _, _, _, lo in frames]
    try:
        tickets = []
        for (fmt, _, li, lo), di, do in list(zip(frames, d_in, d_out))[:n_single]:
            tickets.append(az.apply_i420_dev(FMTV[fmt], di.ptr, li.w, li.h, li.c, do.ptr, lo.c))
        if n_single < n:
            fmt, _, li, lo = frames[n_single]
            tickets += az.apply_i420_dev_n(FMTV[fmt], [d.ptr for d in d_in[n_single:]], li.w, li.h, li.c, [d.ptr for d in d_out[n_single:]], lo.c)
        az.sync()
        res = []
        for t in tickets:
            ow, oh, info = az.result(t)
            res.append((t, ow, oh, info.tolist()))
        return res, [do.download((lo.size // lo.sb,), lo.dtype) for (_, _, _, lo), do in zip(frames, d_out)]
    finally:
        for d in d_in + d_out:
            d.free()


# ---- 1. roll ---------------------------------------------------------------------------------------------------------------------------
_roll_want = {}


def roll_wanted(oracle, fmt, size, tilt):
    key = (fmt, size, tilt)
    if key not in _roll_want:
        states = inp.roll_oracle(oracle, size, tilt)
        _roll_want[key] = [ref.rotate_planar(p, fmt, st[0]) for p, st in zip(inp.roll_planes(fmt, size, tilt), states)]
    return _roll_want[key]


@pytest.mark.parametrize("tilt", list(inp.TILTS))
@pytest.mark.parametrize("size", inp.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("fmt", inp.FORMATS)
def test_roll_correct_matches_the_reference(gpu, oracle, fmt, size, tilt):
    """A single surface, a batch of eight (the array form) and eleven surfaces (8 + 3, the three closed by vs_roll_sync), each on a
    new object whose smoothed angle follows the detected one at once: every surface is rotated by the oracle's angle for it."""
    w, h = size
    states = inp.roll_oracle(oracle, size, tilt)
    assert all(st[0] != 0.0 for st in states), "a surface would pass by not being rotated"
    planes, want = inp.roll_planes(fmt, size, tilt), roll_wanted(oracle, fmt, size, tilt)
    li, lo = Lay(fmt, w, h, STYLES[size][0]), Lay(fmt, w, h, STYLES[size][1])
    for n in (1, 8, inp.N_ROLL):
        rg = gpu.roll_correction(inp.roll_params(gpu, size, **inp.FOLLOW))
        try:
            got = roll_run(gpu, rg, [(fmt, p, li, lo) for p in planes[:n]], array_form=n == 8)
            state = rg.state()
        finally:
            rg.close()
        assert state == states[n - 1], n
        for i in range(n):
            check(got[i], lo, want[i], (n, i))


def _rows_buffer(planes, offs, pitches, size, canary=0x5A):
    """A buffer of `size` bytes, canaries everywhere but the rows of the 2-D byte planes at their offsets and pitches."""
    buf = np.full(size, canary, np.uint8)
    for p, off, pitch in zip(planes, offs, pitches):
        rows, rb = p.shape
        view = np.lib.stride_tricks.as_strided(buf[off:], (rows, rb), (pitch, 1))
        view[:] = p
    return buf


@pytest.mark.parametrize("kind", ["NV12", "I422", "BGRA8"])
def test_roll_correct_results_of_one_batch_in_three_layouts(gpu, oracle, kind):
    """Three surfaces of the smallest size handed over one by one with three result layouts: one batch (one format, geometry and source
    layout) whose rotations go frame by frame.  Every result is the reference's for the oracle's angle, the whole buffer compared.
    NV12: the planes of the I420 form with U and V interleaved (an I420 result is the de-interleaved NV12 result); BGRA8: the angles of
    the oracle's BGR object, every channel - the fourth too - a plane of its own under M (4:4:4)."""
    size, tilt = inp.SIZES[0], "3deg"
    w, h = size
    rg = gpu.roll_correction(inp.roll_params(gpu, size, **inp.FOLLOW))
    try:
        if kind == "I422":
            states = inp.roll_oracle(oracle, size, tilt)[:3]
            planes = inp.roll_planes(kind, size, tilt)[:3]
            li, los = Lay(kind, w, h), [Lay(kind, w, h, s) for s in ("packed", "padded", "vfirst")]
            got = roll_run(gpu, rg, [(kind, p, li, lo) for p, lo in zip(planes, los)])
            assert rg.state() == states[-1] and all(st[0] != 0.0 for st in states)
            for i, lo in enumerate(los):
                check(got[i], lo, ref.rotate_planar(planes[i], kind, states[i][0]), (kind, i))
            return
        if kind == "NV12":
            states = inp.roll_oracle(oracle, size, tilt)[:3]
            yuv = inp.roll_planes("I420", size, tilt)[:3]
            want = [ref.rotate_planar(p, "I420", st[0]) for p, st in zip(yuv, states)]
            two = lambda p: [p[0], np.stack([p[1], p[2]], axis=2).reshape(h // 2, w)]       # Y rows, interleaved (U, V) rows
            srcs, want = [two(p) for p in yuv], [two(p) for p in want]
            # (out_pitch, out_uv_offset, bytes): packed with the default offset; padded rows; the chroma plane apart
            outs = [(w, 0, w * h * 3 // 2), (w + 64, 0, (w + 64) * h * 3 // 2), (w, w * h + 128, w * h + 128 + w * h // 2)]
            lay = [((0, ouv or h * op), (op, op)) for op, ouv, _ in outs]
            call = lambda di, do, i: rg.correct_nv12_dev(di.ptr, w, h, w, do.ptr, outs[i][0], 0, outs[i][1])
        else:
            frames = inp.roll_frames(size, tilt)[:3]
            ro = oracle.roll_correction(inp.roll_params(oracle, size, **inp.FOLLOW))
            states = []
            for f in frames:
                ro.correct(f)
                states.append(ro.state())
            ro.close()
            alpha = [np.roll(f[:, :, 1], 7 + i, axis=1) ^ 0x55 for i, f in enumerate(frames)]
            chans = [[f[:, :, 0], f[:, :, 1], f[:, :, 2], a] for f, a in zip(frames, alpha)]
            rot = [ref.rotate_planar(c[:3], "I444", st[0]) + [ref.rotate_planar([c[3]] * 3, "I444", st[0])[0]] for c, st in zip(chans, states)]
            srcs, want = [[np.stack(c, axis=2).reshape(h, w * 4)] for c in chans], [[np.stack(c, axis=2).reshape(h, w * 4)] for c in rot]
            outs = [(w * 4, 0, w * 4 * h), (w * 4 + 64, 0, (w * 4 + 64) * h), (w * 4 + 128, 0, (w * 4 + 128) * h)]
            lay = [((0,), (op,)) for op, _, _ in outs]
            call = lambda di, do, i: rg.correct_rgb_dev(capi.FMT_BGRA8, di.ptr, w, h, w * 4, do.ptr, outs[i][0])
        assert all(st[0] != 0.0 for st in states), "a surface would pass by not being rotated"
        d_in = [capi.DevBuf.from_array(gpu, np.concatenate([p.reshape(-1) for p in s])) for s in srcs]
        d_out = [capi.DevBuf.from_array(gpu, np.full(size_, 0x5A, np.uint8)) for _, _, size_ in outs]
        try:
            for i in range(3):
                call(d_in[i], d_out[i], i)
            rg.sync()
            assert rg.state() == states[-1]
            for i, (_, _, size_) in enumerate(outs):
                got = d_out[i].download((size_,), np.uint8)
                assert np.array_equal(got, _rows_buffer(want[i], lay[i][0], lay[i][1], size_)), (kind, i, int((got != _rows_buffer(want[i], lay[i][0], lay[i][1], size_)).sum()))
        finally:
            for d in d_in + d_out:
                d.free()
    finally:
        rg.close()


# ---- 2. zoom ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", inp.ZOOM_OUT, ids=["default_640x360", "own_size", "416x232"])
@pytest.mark.parametrize("size", inp.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("fmt", inp.FORMATS)
def test_auto_zoom_crop_matches_the_reference(gpu, oracle, fmt, size, out):
    """Three cropped surfaces (one by one, then two through the array form): info8 is the oracle's, all eight values; Y comes out at
    ow x oh, U and V at (ow >> sx) x (oh >> sy), where the result layout - sized for max(w, ow) x max(h, oh) - puts them."""
    w, h = size
    ow, oh = out[0] or w, out[1] or h
    infos = inp.zoom_info(oracle, size)
    planes = inp.zoom_planes(oracle, fmt, size)
    want = [ref.crop_scale_planar(p, fmt, info, ow, oh) for p, info in zip(planes, infos)]
    li, lo = Lay(fmt, w, h, STYLES[size][0]), Lay(fmt, max(w, ow), max(h, oh), STYLES[size][1])
    az = gpu.auto_zoom_crop()
    try:
        if out != (640, 360):
            az.set_output_size(*out)
        res, bufs = zoom_run(gpu, az, [(fmt, p, li, lo) for p in planes], n_single=1)
    finally:
        az.close()
    for i, ((t, gw, gh, ginfo), info) in enumerate(zip(res, infos)):
        assert t == i and ginfo == info.tolist() and ginfo[7] == 1, i
        assert (gw, gh) == (ow, oh), i
        assert want[i][1].shape == (oh >> ref.shifts(fmt)[1], ow >> ref.shifts(fmt)[0])
        check(bufs[i], lo, want[i], i)


@pytest.mark.parametrize("fmt", inp.FORMATS)
def test_auto_zoom_crop_fall_back_returns_the_three_planes_unchanged(gpu, oracle, fmt):
    """An all-dark Y plane has no contour: the w x h surface comes back unchanged - every plane at its own size, with its live chroma
    and low bits - where the result layout (sized for 640 x 360) puts it."""
    w, h = 322, 200
    y, u, v = (np.array(p) for p in inp.zoom_planes(oracle, fmt, (w, h))[0])
    y[:] = 1 << (ref.bits(fmt) - 8)               # (analysis byte 1 is not content)
    y[::3] = 0
    _, info = oracle.auto_zoom_crop_nv12(ref.analysis_nv12((y, u, v), fmt), w, h)
    assert int(info[7]) == 0
    li, lo = Lay(fmt, w, h, "padded"), Lay(fmt, 640, 360, "padded")
    az = gpu.auto_zoom_crop()
    try:
        res, bufs = zoom_run(gpu, az, [(fmt, (y, u, v), li, lo)])
    finally:
        az.close()
    assert res[0][1:] == (w, h, info.tolist())
    check(bufs[0], lo, (y, u, v), fmt)


# ---- 3. I420, I422 and I210 through one object ---------------------------------------------------------------------------------------
MIX = ["I420", "I422", "I210"]
MIX_SIZE, MIX_TILT, MIX_N = (322, 200), "3deg", 9


def test_roll_object_takes_formats_alternately_and_carries_the_angle(gpu, oracle):
    """Every call changes the format and closes the pending batch.  With the default smoothing the angle of a frame depends on all
    frames before it: the mixed run follows the oracle's one sequence across every change, every surface is rotated by the oracle's
    angle for it, and surface i comes out as it does from an object that saw the same i surfaces before it in its own format."""
    w, h = MIX_SIZE
    ro = oracle.roll_correction(inp.roll_params(oracle, MIX_SIZE))
    states = []
    for p in inp.roll_planes("I444", MIX_SIZE, MIX_TILT)[:MIX_N]:
        ro.correct_nv12(ref.analysis_nv12(p, "I444"), w, h)
        states.append(ro.state())
    ro.close()
    assert all(st[0] != 0.0 for st in states) and len({st[0] for st in states}) == MIX_N         # (the angle moves from frame to frame)

    def run(fmt_of):
        rg = gpu.roll_correction(inp.roll_params(gpu, MIX_SIZE))
        try:
            frames = []
            for i in range(MIX_N):
                f = fmt_of(i)
                lay = Lay(f, w, h)
                frames.append((f, inp.roll_planes(f, MIX_SIZE, MIX_TILT)[i], lay, lay))
            return roll_run(gpu, rg, frames), rg.state()
        finally:
            rg.close()

    mixed, sm = run(lambda i: MIX[i % 3])
    assert sm == states[-1]
    for i in range(MIX_N):
        f = MIX[i % 3]
        check(mixed[i], Lay(f, w, h), ref.rotate_planar(inp.roll_planes(f, MIX_SIZE, MIX_TILT)[i], f, states[i][0]), (f, i))
    for j, f in enumerate(MIX):
        only, so = run(lambda i, f=f: f)
        assert so == sm, f
        for i in range(j, MIX_N, 3):
            assert mixed[i].dtype == only[i].dtype and np.array_equal(mixed[i], only[i]), (f, i)


def test_zoom_object_takes_formats_alternately(gpu, oracle):
    size = (322, 200)
    w, h = size
    infos = inp.zoom_info(oracle, size)
    n = 6

    def run(fmt_of):
        az = gpu.auto_zoom_crop()
        try:
            frames = [(fmt_of(i), inp.zoom_planes(oracle, fmt_of(i), size)[i % 3], Lay(fmt_of(i), w, h), Lay(fmt_of(i), 640, 360)) for i in range(n)]
            res, bufs = zoom_run(gpu, az, frames)
            return res, bufs, az.worker_times()
        finally:
            az.close()

    mres, mbufs, wt = run(lambda i: MIX[i % 3])
    assert wt[0] == n and wt[5] == n                              # (every call closed the batch of the one before)
    for i in range(n):
        f = MIX[i % 3]
        assert mres[i][1:] == (640, 360, infos[i % 3].tolist()), i
        check(mbufs[i], Lay(f, 640, 360), ref.crop_scale_planar(inp.zoom_planes(oracle, f, size)[i % 3], f, infos[i % 3], 640, 360), (f, i))
    for j, f in enumerate(MIX):
        ores, obufs, _ = run(lambda i, f=f: f)
        for i in range(j, n, 3):
            assert mres[i] == ores[i], (f, i)
            assert mbufs[i].dtype == obufs[i].dtype and np.array_equal(mbufs[i], obufs[i]), (f, i)


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------------
CHAIN_CH = 4
CHAIN_PARAMS = dict(smoothing_radius=2, max_corners=400)


def run_chain(gpu, fmt, surfaces):
    """roll -> stabilizer (batch mode, zero-copy, the stream of format `fmt`) -> zoom, chunk by chunk, one chunk more for the
    stabilizer's flush; packed layouts, serial.  Returns [(ow, oh, info8, Y, U, V)], the roll stage's state and the stabilizer's frames_out."""
    W, H = inp.CHAIN_SIZE
    lay = Lay(fmt, W, H)
    sb = lay.size
    n_chunks = len(surfaces) // CHAIN_CH
    d_src = [capi.DevBuf.from_array(gpu, lay.buffer(p)) for p in surfaces]
    # (zero-copy: the stabilizer reads a pushed surface until its result is out, a chunk later - the rolled surfaces go to a ring of two)
    d_roll, d_stab, d_zoom = capi.DevBuf(gpu, 2 * sb * CHAIN_CH), capi.DevBuf(gpu, sb * CHAIN_CH), capi.DevBuf(gpu, sb * CHAIN_CH)
    rc, az, st = gpu.roll_correction(), gpu.auto_zoom_crop(), gpu.stabilizer(gpu.params(**CHAIN_PARAMS))
    st.set_batch(CHAIN_CH)
    st.set_zero_copy(True)
    results = []
    try:
        for c in range(n_chunks + 1):
            if c < n_chunks:
                rolled = [d_roll.ptr + ((c % 2) * CHAIN_CH + i) * sb for i in range(CHAIN_CH)]
                rc.correct_i420_dev_n(FMTV[fmt], [d_src[c * CHAIN_CH + i].ptr for i in range(CHAIN_CH)], W, H, lay.c, rolled, lay.c)
                rc.sync()
                k = st.push_dev_n(rolled, W, H, lay.pitch, FMTV[fmt], [d_stab.ptr + j * sb for j in range(CHAIN_CH)], lay.pitch)
            else:
                k = 0
                while st.flush_dev(d_stab.ptr + k * sb, lay.pitch):
                    k += 1
                    assert k <= CHAIN_CH, "the flush holds more than a chunk"
            st.sync()
            if not k:
                continue
            tickets = az.apply_i420_dev_n(FMTV[fmt], [d_stab.ptr + j * sb for j in range(k)], W, H, lay.c, [d_zoom.ptr + j * sb for j in range(k)], lay.c)
            az.sync()
            for j, t in enumerate(tickets):
                ow, oh, info = az.result(t)
                results.append((ow, oh, info.tolist()) + tuple(lay.planes(d_zoom.download((sb // lay.sb,), lay.dtype, j * sb), ow, oh)))
        return results, rc.state(), st.counters().frames_out
    finally:
        for o in (st, rc, az):
            o.close()
        for b in d_src + [d_roll, d_stab, d_zoom]:
            b.free()


@pytest.mark.parametrize("fmt", ["I422", "I210", "I444"])
def test_chain_equals_the_composed_references(gpu, oracle, fmt):
    """Eight 704 x 400 surfaces in two chunks plus the flush, against the references composed stage by stage: rotate_planar with the
    oracle's angle; the oracle's stabilizer on the analysis bytes of the rolled surfaces for the matrices and planar_inputs.warp_frame
    for the pixels (the last frame comes back unwarped); crop_scale_planar with the oracle's info8 on the analysis bytes of the
    stabilized surfaces."""
    from test_gpu_planar import _oracle_nv12_run
    W, H = inp.CHAIN_SIZE
    sx, sy = ref.shifts(fmt)
    planes = inp.chain_planes(fmt)
    got, state, n_out = run_chain(gpu, fmt, planes)
    ro = oracle.roll_correction()
    rolled = [ref.roll_planar(p, fmt, ro) for p in planes]
    ref_state = ro.state()
    ro.close()
    assert state == ref_state and ref_state[0] != 0.0
    outs, _ = _oracle_nv12_run(oracle, [ref.analysis_nv12(p, fmt) for p in rolled], **CHAIN_PARAMS)
    assert len(outs) == len(got) == n_out == inp.CHAIN_N
    n_crop = 0
    for j, ((idx, M), (ow, oh, info, y, u, v)) in enumerate(zip(outs, got)):
        if idx == inp.CHAIN_N - 1:
            stab = rolled[idx]
        else:
            stab = pin.planes(pin.warp_frame(oracle, synth.yuv_pack(*rolled[idx], sx, sy), fmt, W, H, M), fmt, W, H)
        want, winfo = ref.azc_planar(stab, fmt, oracle)
        assert info == winfo.tolist(), j
        assert (ow, oh) == ((640, 360) if winfo[7] else (W, H)), j
        for name, g, wnt in zip("YUV", (y, u, v), want):
            assert g.shape == wnt.shape and np.array_equal(g, wnt), (j, name)
        n_crop += int(winfo[7])
    assert n_crop > 0


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _lay(**kw):
    return capi.i420_layout(kw.get("pitch", 0), kw.get("c_pitch", 0), kw.get("u_off", 0), kw.get("v_off", 0))


@pytest.mark.parametrize("fmt", inp.FORMATS)
def test_entry_points_refuse_bad_geometry_and_layouts(gpu, fmt):
    """VS_ERR_INVALID_ARG with a text that names the format, for both stages - one case per rule that the chroma shifts change, and the
    rules they share with 4:2:0; the accepted calls beside them return VS_OK.  NV12 and P010 stay refused."""
    sx, sy = ref.shifts(fmt)
    sb = 1 if ref.bits(fmt) == 8 else 2
    w, h = 64, 48
    cw, ch = w >> sx, h >> sy
    d = capi.DevBuf(gpu, 8 << 20)
    half = 4 << 20
    rg, az = gpu.roll_correction(), gpu.auto_zoom_crop()
    t = C.c_int64(-1)
    good_in, good_roll_out, good_zoom_out = dict(pitch=w * sb), dict(pitch=w * sb), dict(pitch=640 * sb)

    def roll(w_=w, h_=h, lin=good_in, lout=good_roll_out, off=0, ooff=0, kind=FMTV[fmt]):
        rc = gpu.lib.vs_roll_correct_i420_dev(rg.h, kind, C.c_void_p(d.ptr + off), w_, h_, C.byref(_lay(**lin)), C.c_void_p(d.ptr + half + ooff), C.byref(_lay(**lout)))
        return rc, (gpu.lib.vs_roll_last_error(rg.h) or b"").decode()

    def zoom(w_=w, h_=h, lin=good_in, lout=good_zoom_out, off=0, ooff=0, kind=FMTV[fmt]):
        rc = gpu.lib.vs_azc_apply_i420_dev(az.h, kind, C.c_void_p(d.ptr + off), w_, h_, C.byref(_lay(**lin)), C.c_void_p(d.ptr + half + ooff), C.byref(_lay(**lout)),
                                           C.byref(t))
        return rc, (gpu.lib.vs_azc_last_error(az.h) or b"").decode()

    P = w * sb
    bad = [(dict(w_=63), "w and h must be even"), (dict(h_=47), "w and h must be even"),
           (dict(lin=dict(pitch=P - 2)), "the pitch must hold a row"),
           (dict(lin=dict(pitch=P, c_pitch=cw * sb - 2 * sb)), "the chroma pitch must hold a chroma row (%d bytes)" % (cw * sb)),
           (dict(lin=dict(pitch=P, u_off=P * h - 2)), "behind the luma rows"),
           # the chroma planes hold h >> sy rows: V one row short of the end of U, and U one row short of the end of V (V first)
           (dict(lin=dict(pitch=P, u_off=P * h, v_off=P * h + (P >> sx) * (ch - 1))), "the U and V planes overlap"),
           (dict(lin=dict(pitch=P, v_off=P * h, u_off=P * h + (P >> sx) * (ch - 1))), "the U and V planes overlap")]
    if sx:
        bad += [(dict(lin=dict(pitch=P + sb)), "the default chroma pitch needs")]          # pitch >> 1 must be whole samples
    if sb == 2:
        bad += [(dict(lin=dict(pitch=P + 1)), "must be even"), (dict(lin=dict(pitch=P, c_pitch=cw * 2 + 1)), "must be even"), (dict(off=1), "must be even"),
                (dict(ooff=1), "must be even")]
    for f, good_out in ((roll, good_roll_out), (zoom, good_zoom_out)):
        OP = good_out["pitch"]
        orows = h if f is roll else 360
        ocw = (OP // sb) >> sx
        cases = bad + [(dict(lout=dict(pitch=OP - 2)), "the pitch must hold a row"),
                       (dict(lout=dict(pitch=OP, c_pitch=ocw * sb - 2 * sb)), "the chroma pitch must hold a chroma row (%d bytes)" % (ocw * sb)),
                       (dict(lout=dict(pitch=OP, u_off=OP * (orows - 1))), "behind the luma rows"),
                       (dict(lout=dict(pitch=OP, u_off=OP * orows, v_off=OP * orows + (OP >> sx) * ((orows >> sy) - 1))), "the U and V planes overlap")]
        for kw, text in cases:
            rc, msg = f(**kw)
            assert rc == INVALID and fmt in msg and text in msg, (f.__name__, kw, rc, msg)
    # accepted: the defaults; V first; 4:4:4: an odd pitch (in samples) with the default chroma pitch
    accepted = [dict(), dict(lin=dict(pitch=P, v_off=P * h, u_off=P * h + (P >> sx) * ch))]
    if not sx:
        accepted.append(dict(lin=dict(pitch=P + sb)))
    for kw in accepted:
        rc, msg = roll(**kw)
        assert rc == 0, (kw, msg)
        rc, msg = zoom(**kw)
        assert rc == 0, (kw, msg)
    assert t.value == len(accepted) - 1
    for kind in (capi.FMT_NV12, capi.FMT_P010, 16):
        rc, msg = roll(kind=kind)
        assert rc == INVALID and "three-plane" in msg, kind
        rc, msg = zoom(kind=kind)
        assert rc == INVALID and "three-plane" in msg, kind
    rg.sync()
    az.sync()
    rg.close()
    az.close()
    d.free()


# ---- 6. 4:2:2 chroma tiles on both sides of the staging limits ---------------------------------------------------------------------------
# Under host maps with BORDER_REPLICATE a launch of 4:2:2 surfaces takes the instances with the taller staged box (THP + 17 source rows
# in place of THP + 9) when a full-width chroma tile may outgrow the smaller one and can fit the taller: with 128-column chroma tiles
# between about 1.8 and 3.7 degrees.  1.5: every tile staged in the box it always had; 1.9, 2.5, 3.4: the taller box, every tile staged;
# 3.7: the taller box, tiles on both paths; 5: direct either way, the old instance.  65-column tiles (130 wide) move all limits up.
TALL_DEGS = [1.5, 1.9, 2.5, 3.4, 3.7, 5.0]
TALL_SIZES = [(130, 96), (322, 200), (3840, 64)]


@pytest.mark.parametrize("size", TALL_SIZES, ids=["130x96", "322x200", "3840x64"])
@pytest.mark.parametrize("fmt", ["I422", "I210"])
def test_warp_affine_planar_replicate_around_the_staging_limits(gpu, oracle, fmt, size):
    """vs_op_warp_affine_planar, BORDER_REPLICATE, one surface per angle and all six angles as one batch: equal to the per-plane
    reference (the oracle's cv::warpAffine for 8-bit planes, ref16 for 16-bit planes), both signs of the angle."""
    w, h = size
    frame = pin.random_frame(w * 7 + h, fmt, w, h, full_range=True)
    mats = [pin.rotation(d if i % 2 == 0 else -d, 1.25 - i, 0.5 * i - 1.75) for i, d in enumerate(TALL_DEGS)]
    want = [pin.warp_frame(oracle, frame, fmt, w, h, M, pin.REPLICATE) for M in mats]
    for d, M, wnt in zip(TALL_DEGS, mats, want):
        got = gpu.warp_affine_planar(FMTV[fmt], frame, w, h, M, capi.BORDER_REPLICATE)
        assert np.array_equal(got, wnt), (d, int((got != wnt).sum()))
    got = gpu.warp_affine_planar(FMTV[fmt], np.stack([frame] * len(mats)), w, h, mats, capi.BORDER_REPLICATE)
    for d, g, wnt in zip(TALL_DEGS, got, want):
        assert np.array_equal(g, wnt), ("batch", d, int((g != wnt).sum()))
