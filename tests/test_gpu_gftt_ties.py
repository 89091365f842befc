"""The corner detector (k_gftt.hip: min-eigenvalue map, nms_row, select_corners) on pictures whose local maxima TIE
(tests/gftt_tie_inputs.py), on a real MI355X.  No tolerance anywhere.

What natural pictures never reach and these do:
  * a candidate list longer than w * h / 4: on a plateau every pixel equals its 3 x 3 maximum (plateau3, plateau3_two, plateau5,
    and the stream's clip).  The list is sized by the interior (gftt_cand_cap); with the old size the pictures overflowed it and
    the corners were whichever candidates the waves' atomicAdd put below the cap;
  * the radix search of select_corners descending into the index bytes of the keys, and a chunk that ends inside a group
    of equal values (s_upper = last_key): more than SORT_CAP keys share their upper 32 bits on the plateaus;
  * the order among equal values (higher address first) as the whole output: minDistance 0;
  * 64-candidate steps of the greedy pass in which many lanes hold one value and conflict with each other, on the grid path
    (cells of 1 and 4 pixels) and on the brute-force path (cell 2: 80 x 60 cells at 160 x 120, more than the grid holds).

Each case asserts: the device's map equals the oracle's as bits (so the plateau is a plateau on the device); the points equal
tests/gfttref.py's selection from the DEVICE's map and the oracle's list; a second call returns the same points."""
import numpy as np
import pytest

import gfttref
import gftt_tie_inputs as ties
from vsamd import capi

pytestmark = pytest.mark.gpu

_ref = {}


def reference(oracle, name, bs):
    """(oracle map, {args: (oracle points, candidates)}), computed once and left unchanged"""
    if (name, bs) not in _ref:
        g = ties.picture(name)
        eig = oracle.min_eigen(g, bs)
        eig.setflags(write=False)
        sel = {}
        for args in ties.PARAMS:
            pts, nc = oracle.gftt(g, *args, bs)
            pts.setflags(write=False)
            sel[args] = (pts, nc)
        _ref[(name, bs)] = (eig, sel)
    return _ref[(name, bs)]


@pytest.mark.parametrize("args", ties.PARAMS, ids=lambda a: "%d-%g-%g" % a)
@pytest.mark.parametrize("name,bs", ties.CASES)
def test_corners_on_tied_maxima(gpu, oracle, name, bs, args):
    g = ties.picture(name)
    eig_o, sel = reference(oracle, name, bs)
    pts_o, nc = sel[args]
    pts_g, eig_g = gpu.gftt(g, *args, bs, want_eig=True)
    assert np.array_equal(eig_g.view(np.uint32), eig_o.view(np.uint32)), "map"
    pts_r, nc_r = gfttref.select(eig_g, *args)
    assert nc_r == nc
    assert pts_g.shape == pts_r.shape, (len(pts_g), len(pts_r), nc)
    assert np.array_equal(pts_g, pts_r), "first difference at %d of %d" % (int(np.flatnonzero((pts_g != pts_r).any(axis=1))[0]), len(pts_r))
    assert pts_g.shape == pts_o.shape and np.array_equal(pts_g, pts_o)
    again = gpu.gftt(g, *args, bs)
    assert again.shape == pts_g.shape and np.array_equal(again, pts_g), "second call"


# ---- through the stream: the work buffers of stabilizer.cpp, nms_batch_kernel and select_batch_kernel ---------------------------
PARAMS = dict(smoothing_radius=3)


def _same_model(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def _oracle_run(oracle):
    """The oracle over the clip, once: per push (output or None, detected points, points handed to LK, model), then the flushed frames."""
    if "stream" not in _ref:
        clip = ties.plateau_clip()
        so = oracle.stabilizer(oracle.params(**PARAMS))
        pushes = []
        for f in clip:
            out = so.push(f)
            d, a = so.debug(), so.debug_arrays()
            pushes.append((out, a["detected"].copy(), a["prev"].copy(), a["curr"].copy(), a["status"].copy(), np.array(d.model), int(d.detected)))
        tail = []
        while True:
            out = so.flush(clip[0])
            if out is None:
                break
            tail.append(out)
        so.close()
        _ref["stream"] = (pushes, tail)
    return _ref["stream"]


def test_stream_per_frame_on_a_plateau_clip(gpu, oracle):
    """Every detection of the stream sees about 511 000 candidates where the old list held 129 664: features, tracks, models
    and frames equal the oracle's, and no frame reports a truncated list."""
    clip = ties.plateau_clip()
    w, h = ties.CLIP_SIZE
    pushes, tail = _oracle_run(oracle)
    sg = gpu.stabilizer(gpu.params(**PARAMS))
    n_out = n_det = 0
    for k, f in enumerate(clip):
        out = sg.push(f)
        ref_out, det, prev, curr, status, model, detected = pushes[k]
        d, a = sg.debug(), sg.debug_arrays()
        c = sg.counters()
        assert c.gftt_overflow == 0, (k, c.last_candidates)
        # (the detections of frames 0 and 1 run on the 480 x 270 image of the first frame: a plateau too, 476 x 264 candidates)
        assert c.last_candidates > (ties.old_cap(w, h) if k >= 2 else ties.old_cap(480, 270)), (k, c.last_candidates)
        assert d.detected == detected, k
        assert np.array_equal(a["detected"], det), k
        assert np.array_equal(a["prev"], prev) and np.array_equal(a["status"], status), k
        assert np.array_equal(a["curr"].view(np.uint32), curr.view(np.uint32)), k
        if k > 0:
            assert _same_model(np.array(d.model), model), k
        n_det += detected
        assert (out is None) == (ref_out is None), k
        if out is not None:
            assert np.array_equal(out, ref_out), k
            n_out += 1
    for ref_out in tail:
        out = sg.flush(clip[0])
        assert out is not None and np.array_equal(out, ref_out)
        n_out += 1
    assert sg.flush(clip[0]) is None
    sg.close()
    assert n_out == len(clip) and n_det >= 4, (n_out, n_det)


def test_stream_in_batch_mode_on_a_plateau_clip(gpu, oracle):
    """The same clip with 8 frames a step: the detections of a step share one launch per stage (nms_batch_kernel,
    select_batch_kernel), each with a work buffer of its own.  The counters name the step's last detection."""
    clip = ties.plateau_clip()
    w, h = ties.CLIP_SIZE
    pushes, tail = _oracle_run(oracle)
    ref = [p[0] for p in pushes if p[0] is not None] + tail
    sg = gpu.stabilizer(gpu.params(**PARAMS))
    sg.set_batch(8)
    fb = clip[0].nbytes
    d_in, d_out = capi.DevBuf(gpu, fb * len(clip)), capi.DevBuf(gpu, fb * (len(clip) + 1))
    k = 0
    for i, f in enumerate(clip):
        d_in.upload(f, i * fb)
        k += sg.push_dev(d_in.ptr + i * fb, w, h, w * 3, capi.FMT_BGR8, d_out.ptr + k * fb, w * 3)
        if i == 8:                          # the step of frames 1 .. 8 has just been issued; (reading the counters synchronises, which
            c = sg.counters()               # closes the step being collected: asked after every push it would make every step one frame)
            assert c.gftt_overflow == 0 and c.last_candidates > ties.old_cap(w, h), (c.gftt_overflow, c.last_candidates)
            a, d = sg.debug_arrays(), sg.debug()
            assert np.array_equal(a["prev"], pushes[8][2]) and np.array_equal(a["curr"].view(np.uint32), pushes[8][3].view(np.uint32))
            assert _same_model(np.array(d.model), pushes[8][5])
    while sg.flush_dev(d_out.ptr + k * fb, w * 3):
        k += 1
    sg.sync()
    assert sg.counters().gftt_overflow == 0
    assert k == len(ref) == len(clip)
    got = d_out.download((k, h, w, 3), np.uint8)
    for j in range(k):
        assert np.array_equal(got[j], ref[j]), j
    sg.close()
    d_in.free()
    d_out.free()
