"""The compositing kernels held to the numpy statements of tests/compref.py, each through the operator that calls what the stream
calls (vs_op_copy_make_border, vs_op_fade_blend, vs_op_fade_update, vs_op_canvas_*) and, for the fade stream, through the stream:
make_border_kernel, fade_blend_kernel, fade_update_kernel (k_traj.hip); canvas_bits_kernel, canvas_fill_kernel, canvas_motion_kernel
and the host decisions of canvas_apply (k_canvas.hip).  Cases and the conditions that keep them from passing trivially are those of
tests/test_compref_oracle.py (tests/compref_cases.py); every comparison is array_equal."""
import ctypes as C

import numpy as np
import pytest

import compref
import compref_cases as cc
import ref64_checks as rc
import ref64_inputs
from vsamd import capi

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED = 1, 4


# ---- border pad ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.BORDER_MODES)
def test_copy_make_border(gpu, mode):
    cc.check_border_cases_fold()
    for w, h, cn, b, pitch in cc.BORDER_SHAPES:
        img = cc.border_image(w, h, cn)
        assert np.array_equal(gpu.copy_make_border(img, b, mode, pitch), compref.copy_make_border(img, b, mode)), (w, h, cn, b, pitch)


# ---- fade ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", cc.fade_alphas(), ids=lambda a: "%.6g" % a)
def test_fade_blend_on_every_pair(gpu, alpha):
    a, b = cc.pair_planes()
    if alpha in cc.TIE_ALPHAS:
        assert cc.fade_ties(alpha) >= 100
    beta = F(1) - alpha
    # 65 536 + 4 bytes (a last word in a block of its own), 4 bytes (one word), 7 and 1 bytes (the rounded count)
    for n in (65536 + 4, 4, 7, 1):
        x, y = np.resize(a, n), np.resize(b, n)
        if n < 8:
            x, y = np.roll(a, -7000)[:n], np.roll(b, -7000)[:n]
        got = gpu.fade_blend(x, y, alpha, beta)
        assert np.array_equal(got, compref.fade_blend(x, y, alpha, beta)), n
        # two float roundings below 256 cost at most 2^-17 each, whatever is fused
        assert np.abs(got.astype(np.float64) - np.clip(compref.fade_real(x, y, alpha, beta), 0, 255)).max() <= 0.5 + 2.0 ** -16, n


def test_fade_update_on_every_pair_and_ragged_rows(gpu):
    a, b = cc.pair_planes()
    assert np.array_equal(gpu.fade_update(a, b.reshape(256, 256), 256, 256), compref.fade_update(a, b))
    guard = np.full(16, 0xA5, np.uint8)
    for row_bytes, rows, pitch in cc.FADE_UPDATE_GEOMETRY:
        hist = ref64_inputs.noise(rows, row_bytes, seed=row_bytes)
        stab = ref64_inputs.noise(rows, pitch, seed=pitch + 1)
        got = gpu.fade_update(np.concatenate([hist.reshape(-1), guard]), stab, row_bytes, rows)
        assert np.array_equal(got[:rows * row_bytes].reshape(rows, row_bytes), compref.fade_update(hist, stab[:, :row_bytes])), (row_bytes, rows, pitch)
        assert np.array_equal(got[rows * row_bytes:], guard), (row_bytes, rows, pitch)        # the history is packed: nothing behind it is touched


# ---- canvas ------------------------------------------------------------------------------------------------------------------------------
class _Pitched:
    """A canvas operator whose device frames have a row pitch of their own"""

    def __init__(self, vs):
        self.op = vs.canvas_op()

    def apply(self, params, frame, t, transforms=None):
        return self.op.apply(params, frame, t, transforms, pitch=frame.shape[1] * 3 + 5)

    def close(self):
        self.op.close()


@pytest.fixture(scope="module")
def canvas_runs(gpu):
    """{case: its model counters, or the assertion that failed}: every case runs once, through vs_op_canvas_apply"""
    out = {}
    for name, steps in cc.canvas_cases().items():
        make = (lambda: _Pitched(gpu)) if name[0] in "af" else gpu.canvas_op
        try:
            out[name] = cc.Runner(gpu.params, make).run(steps, name).stats
        except AssertionError as e:
            out[name] = e
    return out


@pytest.mark.parametrize("name", sorted(cc.canvas_cases()))
def test_canvas_case(canvas_runs, name):
    if isinstance(canvas_runs[name], AssertionError):
        raise canvas_runs[name]


def test_canvas_cases_are_not_trivial(canvas_runs):
    cc.check_canvas_stats({k: v for k, v in canvas_runs.items() if not isinstance(v, AssertionError)})


def test_canvas_adaptive_scale(gpu):
    """canvas_motion_kernel on rings of 0 .. 300 transforms: the window of 30 starts at n - 30, also after the ring has wrapped"""
    r = cc.Runner(gpu.params, gpu.canvas_op)
    scales = {}
    frame = cc.content(96, 64, 3)
    for name, params, tr in cc.adaptive_cases():
        st = r.run([cc._step(params, frame, [1.5, -2.0, 0.0], tr), cc._step(params, cc.content(96, 64, 4), [3.0, -1.0, 0.0], tr[:0])], name)
        scales[name] = float(st.scale)
    assert scales["n31_at1"] > scales["n31_at0"] == float(F(1.3)) and scales["n300_at270"] > scales["n300_at269"] == float(F(1.3))
    assert scales["max_clamp"] == 2.0 and scales["min_clamp"] == float(F(1.2))


# ---- fade stream -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,duration", cc.FADE_STREAMS)
def test_fade_stream(gpu, alpha, duration):
    stab = gpu.stabilizer(gpu.params(smoothing_radius=5, border_size=cc.FADE_BORDER, border_type=capi.BORDER_FADE, fade_alpha=alpha,
                                     fade_duration=duration))
    used = cc.run_fade_stream(stab, alpha, duration, rc.check_warp)
    stab.close()
    assert len(used) == 22 and len(set(used)) == (duration + 1 if duration < 22 else 22)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gpu):
    L = gpu.lib
    d = capi.DevBuf(gpu, 1 << 17)            # (large enough for every call below, were one of them not refused)
    p = d.ptr
    ok = (p, 24, 8, 4, 3, p + 65536, 36, 2, compref.REFLECT, None)        # src, pitch, w, h, cn, dst, pitch, b, mode, stream

    def border(**kw):
        names = ["src", "sp", "w", "h", "cn", "dst", "dp", "b", "mode", "st"]
        return L.vs_op_copy_make_border(*[kw.get(n, v) for n, v in zip(names, ok)])

    assert border() == 0
    for kw in (dict(src=None), dict(dst=None), dict(cn=2), dict(cn=0), dict(b=-1), dict(mode=capi.BORDER_FADE), dict(mode=-1), dict(w=0), dict(sp=23),
               dict(dp=35)):
        assert border(**kw) == INVALID, kw
    assert L.vs_op_fade_blend(None, p, 16, 0.5, 0.5, None) == INVALID and L.vs_op_fade_blend(p, None, 16, 0.5, 0.5, None) == INVALID
    assert L.vs_op_fade_blend(p, p + 65536, 0, 0.5, 0.5, None) == INVALID and L.vs_op_fade_blend(p + 1, p + 65536, 16, 0.5, 0.5, None) == INVALID
    assert L.vs_op_fade_blend(p, p + 65536, 16, 1.5, 0.5, None) == INVALID
    assert L.vs_op_fade_update(None, p, 16, 16, 1, None) == INVALID and L.vs_op_fade_update(p, None, 16, 16, 1, None) == INVALID
    assert L.vs_op_fade_update(p, p + 65536, 15, 16, 1, None) == INVALID and L.vs_op_fade_update(p, p + 65536, 16, 0, 1, None) == INVALID
    gpu.sync()
    op = gpu.canvas_op()
    t = np.zeros(3, np.float32)
    tp = t.ctypes.data_as(capi.f32p)
    info = np.full(8, -7, np.int32)
    ip = info.ctypes.data_as(capi.i32p)

    def apply(params, frame=p, w=8, h=4, pitch=24, t=tp, n=0, out=p + 65536, op_=op.h):
        return L.vs_op_canvas_apply(op_, C.byref(params) if params is not None else None, frame, pitch, w, h, t, None, n, out, max(pitch, 24), ip)

    good = gpu.params(**cc.BASE)
    for kw in (dict(frame=None), dict(out=None), dict(t=None), dict(op_=None), dict(w=0), dict(pitch=23), dict(n=3)):
        assert apply(good, **kw) == INVALID, kw
    assert apply(None) == INVALID
    assert apply(gpu.params(**dict(cc.BASE, temporal_buffer_size=-1))) == INVALID
    assert apply(gpu.params(**dict(cc.BASE, canvas_blend_weight=1.5))) == UNSUPPORTED
    assert apply(gpu.params(**dict(cc.BASE, canvas_scale_factor=0.1))) == UNSUPPORTED                 # 8 x 4 at 0.1: no canvas
    assert apply(gpu.params(**dict(cc.BASE, canvas_scale_factor=16.0)), w=5000, pitch=15000) == UNSUPPORTED    # 80 000 wide
    assert apply(gpu.params(**dict(cc.BASE, adaptive_canvas_size=1, max_canvas_scale=16.0)), w=5000, pitch=15000) == UNSUPPORTED
    assert info.tolist() == [-7] * 8                                      # no refused call wrote its info
    assert L.vs_op_canvas_info(op.h, ip) == 0 and info.tolist() == [0] * 8           # ... or reached the canvas
    assert L.vs_op_canvas_info(None, ip) == INVALID and L.vs_op_canvas_create(None) == INVALID
    op.close()
    d.free()
