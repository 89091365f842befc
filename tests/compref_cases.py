"""The cases of tests/test_compref_oracle.py (the CPU oracle) and tests/test_gpu_compref.py (the kernels): both run the same inputs
against tests/compref.py, and every case states on the MODEL ALONE what has to happen in it, so that none passes trivially."""
import numpy as np

import compref
import ref64_inputs

F = np.float32

# ---- border pad: (w, h, cn, b, source pitch or None) ---------------------------------------------------------------------------------
BORDER_SHAPES = [(1, 1, 3, 5, None), (2, 3, 1, 7, None), (5, 4, 3, 11, None), (7, 13, 4, 16, None), (300, 2, 3, 1, None),
                 (64, 36, 3, 16, 64 * 3 + 5), (257, 3, 1, 2, None), (5, 4, 3, 0, None)]
BORDER_MODES = [compref.BLACK, compref.REFLECT, compref.REFLECT_101, compref.REPLICATE, compref.WRAP]


def border_image(w, h, cn):
    img = ref64_inputs.noise(h, w, cn, seed=w + 7 * h)
    return img if cn > 1 else img.reshape(h, w)


def check_border_cases_fold():
    """At least one (mode, shape) per looping mode needs more than one pass of borderInterpolate, and one has a single sample"""
    for mode in (compref.REFLECT, compref.REFLECT_101, compref.WRAP):
        deepest = max(int(compref.border_passes(np.arange(-b, n + b), n, mode).max()) for w, h, _, b, _ in BORDER_SHAPES for n in (w, h))
        assert deepest >= 2, mode
    assert any(w == 1 and b > 0 for w, _, _, b, _ in BORDER_SHAPES)


# ---- fade ----------------------------------------------------------------------------------------------------------------------------
def fade_alphas():
    """The weights of the fade planes as float32: fixed values, fade-in values alpha * (k / duration) as the stream forms them"""
    out = [F(0), F(2.0 ** -20), F(0.1), F(0.35), F(0.5), F(0.9), F(1)]
    out += [F(0.1) * (F(k) / F(30)) for k in (1, 7, 29)]
    out += [F(0.35) * (F(k) / F(4)) for k in (1, 3)]
    out += [F(0.5) * (F(1) / F(2))]             # 0.25: a fade-in value that is a dyadic fraction (see TIE_ALPHAS)
    return out


# Half-to-even is exercised where the real value a alpha + b beta ends in exactly .5.  The weights with many such pairs are the
# short dyadic ones: 0.5 has 32 768 and 0.25 has 16 384.  0.35f * (1 / 4) is a 24-bit fraction and (counted with fade_real) ONE of
# its 65 536 pairs is a tie, 0.1f has 8: those planes are compared all the same, but they cannot carry this condition.
TIE_ALPHAS = [F(0.5), F(0.25)]


def pair_planes():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b.reshape(-1))


def fade_ties(alpha):
    a, b = pair_planes()
    real = compref.fade_real(a, b, alpha, F(1) - F(alpha))
    return int((real - np.floor(real) == 0.5).sum())


FADE_UPDATE_GEOMETRY = [(1, 1, 1), (3, 2, 8), (4, 1, 4), (5, 3, 9), (1027, 2, 1031)]          # (row_bytes, rows, pitch of the output)
FADE_STREAMS = [(0.35, 4), (0.9, 0), (0.1, 30)]                                              # (fade_alpha, fade_duration)

# ---- resize and reflect warp ---------------------------------------------------------------------------------------------------------
RESIZE_CASES = [((1, 1), [(1, 1), (2, 3), (3, 2)]), ((1, 7), [(10, 2), (20, 1), (8, 3)]), ((5, 3), [(5, 14), (8, 6), (4, 13)]),
                ((37, 23), [(32, 97), (68, 38), (24, 110), (23, 37)])]        # (source (h, w), [(dw, dh)]): between 1x and 3x, no integer ratio but 1


def warp_matrices():
    c, s = np.cos(0.5), np.sin(0.5)
    return [[1, 0, 0, 0, 1, 0], [1, 0, 40.3, 0, 1, -77.7], [c, -s, 13.2, s, c, -60.1], [np.cos(-0.15), -np.sin(-0.15), -144.0, np.sin(-0.15), np.cos(-0.15), 96.0]]


WARP_SHAPES = [(1, 1), (2, 7), (31, 17)]


# ---- canvas --------------------------------------------------------------------------------------------------------------------------
def content(w, h, seed, blobs=()):
    """ref64_inputs.smooth (38 .. 218: nothing dark) with rectangles (x0, y0, x1, y1[, value]), ends exclusive: black, or of the
    given value (a level or a BGR triple)"""
    img = ref64_inputs.smooth(h, w, 3, seed=seed).copy()
    assert compref.empty_mask(img).sum() == 0
    for x0, y0, x1, y1, *v in blobs:
        img[y0:y1, x0:x1] = v[0] if v else 0
    return img


def grid_angle(target, multiples=(1, 2, 3, 4, 5)):
    """The multiple of 2^-12 nearest to `target` whose small multiples all pass compref.cos_sin32's margin: corrections that move by
    it per call have exact float32 differences, so those multiples are all the angles a case uses."""
    m0 = int(round(target * 4096))
    for m in sorted(range(m0 - 40, m0 + 41), key=lambda m: abs(m - m0)):
        try:
            for j in multiples:
                compref.cos_sin32(F(j * m / 4096.0))
        except AssertionError:
            continue
        return m / 4096.0
    raise AssertionError("no angle near %r" % target)


BASE = dict(enable_virtual_canvas=1, adaptive_canvas_size=0, canvas_scale_factor=1.2, temporal_buffer_size=4, canvas_blend_weight=0.7,
            edge_blend_radius=6, min_canvas_scale=1.2, max_canvas_scale=2.0)

# case (b): an interior blob of gray 1 - (8, 0, 0): (8 * 3735 + 2^14) >> 15 = 1, still "empty" -; one touching the left border; one
# of 30 pixels; a rectangle of gray 2 - (0, 3, 0): (3 * 19235 + 2^14) >> 15 = 2, the darkest content -; a dark ring around a bright
# island that holds a dark blob; an L whose bounding box holds another blob (the L reaches the right border, so its fill is
# stretched and the other's is not)
BLOBS_B = [(34, 28, 49, 42, (8, 0, 0)), (0, 44, 9, 60), (40, 4, 46, 9), (50, 4, 64, 14, (0, 3, 0)),
           (2, 2, 30, 26), (5, 5, 27, 23, 200), (11, 10, 21, 18),
           (60, 30, 65, 61), (60, 56, 96, 61), (72, 34, 89, 49)]


def _step(params, frame, t, transforms=None):
    return dict(params=params, frame=frame, t=np.array(t, np.float32), transforms=transforms)


def _drift(n, w, h, params, per_call, blobs=(), seed0=0):
    return [_step(params, content(w, h, seed0 + k, blobs), [F(k) * F(v) for v in per_call]) for k in range(n)]


def canvas_cases():
    cases = {}
    a01, a004, a002 = grid_angle(0.01), grid_angle(0.004), grid_angle(0.002)
    cases["a_ringed_stretch"] = _drift(6, 96, 64, dict(BASE), (3.4, -2.7, a01))
    pb = dict(BASE, canvas_scale_factor=1.0, min_canvas_scale=1.0)
    cases["b_blobs"] = _drift(5, 96, 64, pb, (1.3, -0.8, a004), BLOBS_B, seed0=10)
    blob_c = [(58, 38, 94, 62)]
    ts = [(0, 0), (0, 0), (40, 25), (46, 29), (0, 0), (-40, -25), (0, 0), (40, -25)]
    cases["c_clipped_two_sides"] = [_step(pb, content(96, 64, 20 + k, blob_c), [tx, ty, 0]) for k, (tx, ty) in enumerate(ts)]
    pd_ = dict(pb, temporal_buffer_size=3)
    a15 = grid_angle(0.15, (1, 2, 3))
    td = [(0, 0, 0), (144, 96, a15), (72, 40, 2 * a15), (60, 30, a15), (-10, 70, 2 * a15), (20, 30, 3 * a15), (90, 60, 2 * a15)]
    blob_d = [(4, 6, 30, 22)]
    cases["d_reflect_twice"] = [_step(pd_, content(96, 64, 30 + k, blob_d), t) for k, t in enumerate(td)]
    for name, kw in [("e_radius0", dict(edge_blend_radius=0)), ("e_radius400", dict(edge_blend_radius=400)), ("e_weight0", dict(canvas_blend_weight=0.0)),
                     ("e_buffer0", dict(temporal_buffer_size=0)), ("e_buffer1", dict(temporal_buffer_size=1)), ("e_buffer2", dict(temporal_buffer_size=2))]:
        cases[name] = _drift(3, 96, 64, dict(BASE, **kw), (3.4, -2.7, a01), seed0=40)
    pf = dict(BASE, canvas_scale_factor=0.8, min_canvas_scale=0.5)
    cases["f_scale_below_one"] = _drift(3, 96, 64, pf, (1.3, -0.8, a004), [(34, 22, 52, 38)], seed0=50)
    pg = dict(BASE, canvas_scale_factor=1.5)
    cases["g_window_clamped"] = [_step(pg, content(96, 64, 60 + k), [tx, ty, 0.0]) for k, (tx, ty) in enumerate([(200, 200), (-200, 200), (200, -200), (-200, -200), (3, 2)])]
    cases["h_size_change"] = (_drift(3, 96, 64, dict(BASE), (3.4, -2.7, a01), seed0=70) +
                              [_step(dict(BASE), content(80, 48, 73 + k), [F(3 + k) * F(3.4), F(3 + k) * F(-2.7), F(3 + k) * F(a01)]) for k in range(3)])
    cases["j_wide_region"] = _drift(3, 300, 40, dict(BASE), (3.4, -1.2, a002), seed0=80)
    pk = dict(pb, temporal_buffer_size=2)
    blobs_k = [(100, 1, 160, 5), (16440, 1, 16500, 5)]
    cases["k_wide_bit_plane"] = [_step(pk, content(16500, 6, 90 + k, blobs_k), [F(40 * k), 0, 0]) for k in range(2)]
    for w in (63, 64, 65, 129):
        cases["l_width_%d" % w] = _drift(3, w, 20, pb, (-1.3, 0.4, 0.0), [(w - 12, 4, w, 16), (w - 30, 3, w - 17, 15)], seed0=100 + w)
    return cases


def adaptive_cases():
    """Case (i): (params, transforms) of single calls on new objects, in pairs that differ only in where the largest motion sits:
    at index n - 30 (the oldest transform the window of 30 reads) or at n - 31 (just outside it)."""
    out = []
    pa = dict(BASE, adaptive_canvas_size=1, canvas_scale_factor=1.3, min_canvas_scale=1.2, max_canvas_scale=2.0)
    for n in (0, 5, 30, 31, 300):
        for at in (n - 30, n - 31):
            tr = np.zeros((n, 3), np.float32)
            if n:
                r = np.random.default_rng(n)
                tr[:, :2] = r.uniform(-9, 9, (n, 2))
                tr[max(at, 0) if n < 31 else at, :2] = (52.5, -41.25)
            out.append(("n%d_at%d" % (n, at), pa, tr))
    big = np.zeros((40, 3), np.float32); big[35, :2] = (400, 300)
    out.append(("max_clamp", pa, big))
    out.append(("min_clamp", dict(pa, canvas_scale_factor=1.0), np.ones((7, 3), np.float32)))
    return out


class Runner:
    """Runs a case's steps through the model and through `make()` -> an object with apply(params, frame, t, transforms) ->
    (output, info8), comparing every call.  params_of(**kw) builds the parameter struct both sides read."""

    def __init__(self, params_of, make):
        self.params_of, self.make = params_of, make

    def run(self, steps, what=""):
        st, obj = compref.CanvasState(), self.make()
        for k, s in enumerate(steps):
            p = self.params_of(**s["params"])
            want, winfo = compref.canvas(st, p, s["frame"], s["t"], s["transforms"])
            got, ginfo = obj.apply(p, s["frame"], s["t"], s["transforms"])
            assert ginfo.tolist() == winfo.tolist(), "%s call %d: info %s, model %s" % (what, k, ginfo.tolist(), winfo.tolist())
            assert np.array_equal(got, want), "%s call %d: %d bytes differ" % (what, k, int((got != want).sum()))
        if hasattr(obj, "close"):
            obj.close()
        return st


def check_canvas_stats(stats):
    """Section 5 of the issue, on the model's counters: stats = {case name: CanvasState.stats}"""
    for name, s in stats.items():
        if name[0] in "abcdjk":
            assert s["fills"] > 0, name
    total = {k: sum(s[k] for s in stats.values()) for k in ("stretch", "no_stretch", "mask_3_regions", "ringed", "older_chosen", "no_fit")}
    assert all(v > 0 for v in total.values()), total
    a, b, c, d = stats["a_ringed_stretch"], stats["b_blobs"], stats["c_clipped_two_sides"], stats["d_reflect_twice"]
    assert a["ringed"] > 0 and a["stretch"] > 0
    assert b["no_stretch"] > 0 and b["stretch"] > 0 and b["mask_3_regions"] > 0 and b["regions_small"] > 0
    assert c["stretch_two_sides"] > 0 and c["newest_refused"] > 0 and c["older_chosen"] > 0 and c["none_available"] > 0
    assert d["taps_fold"] * 100 >= d["taps"] > 0 and d["taps_fold_twice"] > 0, d
    f, g, h = stats["f_scale_below_one"], stats["g_window_clamped"], stats["h_size_change"]
    assert f["no_fit"] == f["calls"] and f["fills"] > 0
    assert g["clamped"] == {"left", "right", "top", "bottom"}
    assert h["reinit"] == 2 and h["other_size"] > 0
    assert stats["e_weight0"]["fills"] == 0 and stats["e_buffer0"]["fills"] == 0 and stats["e_buffer1"]["fills"] == 0
    assert stats["e_radius0"]["fills"] > 0 and stats["e_radius400"]["fills"] > 0 and stats["e_buffer2"]["fills"] > 0
    assert stats["k_wide_bit_plane"]["fills"] == 1 and stats["k_wide_bit_plane"]["none_available"] == 1
    for w in (63, 64, 65, 129):
        assert stats["l_width_%d" % w]["fills"] > 0


# ---- the fade stream -------------------------------------------------------------------------------------------------------------------
FADE_BORDER = 6


def fade_clip(n=12, w=96, h=64):
    """Windows of one smooth picture that drift by a few pixels per frame"""
    world = ref64_inputs.smooth(h + 40, w + 40 + 2 * n, 3, seed=7)
    clip = [np.ascontiguousarray(world[20 + (3 * k) % 7:20 + (3 * k) % 7 + h, 20 + 2 * k:20 + 2 * k + w]) for k in range(n)]
    assert all(f.shape == (h, w, 3) for f in clip)
    return clip


def run_fade_stream(stab, alpha, duration, check_warp, passes=2):
    """A stabilizer with borderType fade (object with push / flush / debug / clean) held to compref's statement of the stream's host
    logic, output by output, push and flush alike:
      * output k is frame k; while k has a transform it is the warp, by the matrix the stabilizer reports, of
        blended_k = fade_blend(history, pad(frame_k)) - within check_warp's bound, the warp being held exactly elsewhere - and the
        history becomes fade_update(history, output_k), the output as returned;
      * the last frame of a pass has no transform (Stabilizer.cpp:774-780): it comes back as it came, in the top left corner of a
        black output, and the history stays;
      * clean() keeps the history and the fade-in count (Stabilizer.cpp:221-256).
    The history steps are exact, and seen: every later blended_k is built from them.  -> the alphas used."""
    clip = fade_clip()
    b = FADE_BORDER
    h, w = clip[0].shape[:2]
    hist, count, used = None, 0, []
    for rep in range(passes):
        k = 0
        for pushing in (True, False):
            for f in (clip if pushing else [clip[0]] * (len(clip) + 1)):
                out = stab.push(f) if pushing else stab.flush(f)
                if out is None:
                    if pushing:
                        continue
                    break
                assert out.shape == (h + 2 * b, w + 2 * b, 3), out.shape
                if k >= len(clip) - 1:
                    want = np.zeros_like(out)
                    want[:h, :w] = clip[k]
                    assert np.array_equal(out, want), (rep, k)
                else:
                    d = stab.debug()
                    if pushing:
                        assert d.out_index == k, (rep, k, d.out_index)
                    blended, hist, count, a = compref.fade_stream_step(hist, count, clip[k], b, alpha, duration)
                    used.append(float(a))
                    check_warp(out, blended, np.array(d.warp_matrix, np.float32), what="pass %d output %d" % (rep, k))
                    hist = compref.fade_update(hist, out)
                k += 1
        assert k == len(clip), k
        stab.clean()
    return used
