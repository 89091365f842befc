"""The CPU oracle held to the numpy statements of tests/compref.py: border pad, fade blend and history, 8-bit linear upscale,
reflect warp, the virtual canvas and the fade stream.  The same cases run on the kernels in tests/test_gpu_compref.py; the
conditions that keep a case from passing trivially are asserted here on the model alone."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import compref
import compref_cases as cc
import ref64_checks as rc
import ref64_inputs

F = np.float32


# ---- border pad ------------------------------------------------------------------------------------------------------------------------
def test_border_cases_need_more_than_one_fold():
    cc.check_border_cases_fold()


@pytest.mark.parametrize("mode", cc.BORDER_MODES)
def test_copy_make_border_statement_oracle_and_numpy_agree(oracle, mode):
    for w, h, cn, b, _ in cc.BORDER_SHAPES:
        img = cc.border_image(w, h, cn)
        want = compref.copy_make_border(img, b, mode)
        assert np.array_equal(oracle.copy_make_border(img, b, mode), want), (w, h, cn, b)
        kw = dict(constant_values=0) if mode == compref.BLACK else {}
        assert np.array_equal(np.pad(img, ((b, b), (b, b)) + (((0, 0),) if cn > 1 else ()), mode=compref.NP_PAD[mode], **kw), want), (w, h, cn, b)


def test_border_index_by_hand():
    p = np.arange(-7, 10)
    assert compref.border_index(p, 3, compref.REFLECT).tolist() == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2]
    assert compref.border_index(p, 3, compref.REFLECT_101).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert compref.border_index(p, 3, compref.WRAP).tolist() == [2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    assert compref.border_index(p, 3, compref.REPLICATE).tolist() == [0] * 7 + [0, 1, 2] + [2] * 7
    assert compref.border_index(p, 1, compref.REFLECT_101).tolist() == [0] * 17 and compref.border_index(p, 1, compref.REFLECT).tolist() == [0] * 17


# ---- fade ------------------------------------------------------------------------------------------------------------------------------
def test_fade_planes_hold_ties():
    for alpha in cc.TIE_ALPHAS:
        assert alpha in cc.fade_alphas() and cc.fade_ties(alpha) >= 100, alpha


@pytest.mark.parametrize("alpha", cc.fade_alphas(), ids=lambda a: "%.6g" % a)
def test_fade_blend_statement_and_oracle_agree_on_every_pair(oracle, alpha):
    a, b = cc.pair_planes()
    beta = F(1) - alpha
    want = compref.fade_blend(a, b, alpha, beta)
    assert np.array_equal(oracle.add_weighted(a, float(alpha), b, float(beta)), want)
    # two float roundings below 256 cost at most 2^-17 each, whatever is fused
    assert np.abs(want.astype(np.float64) - np.clip(compref.fade_real(a, b, alpha, beta), 0, 255)).max() <= 0.5 + 2.0 ** -16


def test_fade_update_by_hand():
    # 0.9f = 1 - 0.1f = 0.89999998...: 10 * 0.9f + 10 * 0.1f is 10 in float32 after its roundings, 255 stays 255
    assert compref.fade_update([10, 255, 0, 0, 100], [10, 255, 0, 9, 109]).tolist() == [10, 255, 0, 0, 100]
    assert compref.fade_update([0, 200], [10, 100]).tolist() == [1, 190]


# ---- resize and reflect warp -----------------------------------------------------------------------------------------------------------
def test_resize_statement_and_oracle_agree(oracle):
    n = 0
    for (sh, sw), sizes in cc.RESIZE_CASES:
        for cn in (1, 3):
            img = ref64_inputs.noise(sh, sw, cn, seed=sh)
            for dw, dh in sizes:
                assert sw <= dw <= 3 * sw and sh <= dh <= 3 * sh and (sw == 1 or dw == sw or dw % sw) and (sh == 1 or dh == sh or dh % sh)     # no integer ratio but 1, where the axis allows one
                assert np.array_equal(oracle.resize(img, dw, dh), compref.resize_linear_u8(img, dw, dh)), (sh, sw, dw, dh, cn)
                n += 1
    assert n >= 20


def test_reflect_warp_statement_and_oracle_agree(oracle):
    twice = 0
    for h, w in cc.WARP_SHAPES:
        img = ref64_inputs.noise(h, w, 3, seed=h + w)
        for M in cc.warp_matrices():
            assert np.array_equal(oracle.warp_affine_d(img, M, compref.REFLECT), compref.warp_reflect(img, M)), (h, w, M)
            twice += compref.reflect_tap_passes(img.shape, M, 0, 0, w, h)[2]
    assert twice > 0


# ---- cosf / sinf -------------------------------------------------------------------------------------------------------------------------
def test_identity_rotation_is_exact():
    c, s = compref.cos_sin32(F(0))
    assert c == 1 and s == 0 and not np.signbit(s) and np.signbit(-s)          # [cos -sin; sin cos] = [1 -0.0; 0 1]


def _host_libm():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (m.cosf, m.sinf):
        f.restype, f.argtypes = C.c_float, [C.c_float]
    return m


# ---- canvas ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def canvas_stats(oracle):
    r = cc.Runner(oracle.params, oracle.canvas)
    return {name: r.run(steps, name).stats for name, steps in cc.canvas_cases().items()}


def test_canvas_statement_and_oracle_agree_and_no_case_is_trivial(canvas_stats):
    cc.check_canvas_stats(canvas_stats)


def test_canvas_angles_round_the_same_in_the_host_libm(canvas_stats):
    """Every angle the model used: the margin was asserted when it was used; here the host's own cosf / sinf give the same floats"""
    m = _host_libm()
    assert len(compref.ANGLES_USED) >= 8
    for x in compref.ANGLES_USED:
        c, s = compref.cos_sin32(F(x))
        assert (F(m.cosf(x)), F(m.sinf(x))) == (c, s), x


def test_canvas_overlapping_fills_depend_on_their_order(oracle):
    steps = cc.canvas_cases()["b_blobs"]
    p = oracle.params(**steps[0]["params"])
    a, b = compref.CanvasState(), compref.CanvasState()
    differ = 0
    for s in steps:
        x, _ = compref.canvas(a, p, s["frame"], s["t"])
        y, _ = compref.canvas(b, p, s["frame"], s["t"], fill_order=lambda n: range(n - 1, -1, -1))
        differ += int(not np.array_equal(x, y))
    boxes = [r for r, _ in a.fill_log[-1]]
    overlap = [(q, r) for i, q in enumerate(boxes) for r in boxes[i + 1:] if compref._inter(q, r)[2] > 0]
    assert len(overlap) == 1 and differ > 0          # one pair of boxes overlaps: only its order can matter
    # regions of the last call: interior (gray 1), left border, ring, L, the blob in the L's box - not the 30 pixels, not the
    # blob inside the ring's island, not the rectangle of gray 2
    assert sorted(boxes) == sorted([(34, 28, 15, 14), (0, 44, 9, 16), (2, 2, 28, 24), (60, 30, 36, 31), (72, 34, 17, 15)])


def test_canvas_adaptive_scale(oracle):
    r = cc.Runner(oracle.params, oracle.canvas)
    scales = {}
    frame = cc.content(96, 64, 3)
    for name, params, tr in cc.adaptive_cases():
        st = r.run([cc._step(params, frame, [1.5, -2.0, 0.0], tr), cc._step(params, cc.content(96, 64, 4), [3.0, -1.0, 0.0], tr[:0])], name)
        assert st.stats["reinit"] == 1
        scales[name] = float(st.scale)
    assert scales["n0_at-30"] == scales["n5_at-25"] == scales["n5_at-26"] == float(F(1.3)) or scales["n5_at-25"] > 1.3
    assert scales["n31_at1"] > scales["n31_at0"] == float(F(1.3))          # index n - 30 is read, n - 31 is not
    assert scales["n300_at270"] > scales["n300_at269"] == float(F(1.3))    # ... in a ring that has wrapped
    assert scales["n30_at0"] == scales["n30_at-1"] > 1.3
    assert scales["max_clamp"] == 2.0 and scales["min_clamp"] == float(F(1.2))


# ---- fade stream -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,duration", cc.FADE_STREAMS)
def test_fade_stream_statement_and_oracle_agree(oracle, alpha, duration):
    stab = oracle.stabilizer(oracle.params(smoothing_radius=5, border_size=cc.FADE_BORDER, border_type=5, fade_alpha=alpha, fade_duration=duration))
    used = cc.run_fade_stream(stab, alpha, duration, rc.check_warp)
    stab.close()
    # 22 blended outputs in two passes; the fade-in runs once (clean() does not restart it) and ends at alpha if it ends at all
    assert len(used) == 22 and used[0] == (0.0 if duration else float(F(alpha))) and (used[-1] == float(F(alpha))) == (duration < 22)
    assert len(set(used)) == (duration + 1 if duration < 22 else 22)
