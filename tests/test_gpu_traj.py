"""The trajectory kernels against the float64 model (traj_ref.py), driven with the designed streams of traj_inputs.py through
vs_op_trajectory: the one-lane append + traj_emit_kernel (per-frame form), ransac_tail_batch_kernel and
ransac_release_batch_kernel (batch form, steps of 1, of 64 and ragged), several streams in one launch; and the append inside
ransac_select_kernel through the per-frame pipeline on three rendered clips."""
import numpy as np
import pytest

import traj_checks as K
import traj_inputs as I
import traj_ref as R
from test_traj_model_cpu import CLIPS, check_stabilizer, clip_coverage, clip_frames
from vsamd import capi

pytestmark = pytest.mark.gpu

METHOD = {"box": capi.SMOOTH_BOX, "gaussian": capi.SMOOTH_GAUSSIAN, "kalman": capi.SMOOTH_KALMAN}
KIND = {None: 1, R.FAIL: 0, R.SKIP: -1}
RAGGED = [1, 7, 64, 3, 33, 2, 50, 5]
CASES = [(n, m, tuple(sorted(kw.items()))) for n in I.SEQUENCES for m, kw in I.SMOOTHERS]


def c_params(gpu, mp):
    """vs_params_c of a traj_ref.Params"""
    return gpu.params(smoothing_radius=mp.smoothing_radius, smoothing_method=METHOD[mp.method], gaussian_sigma=mp.gaussian_sigma,
                      horizon_lock=int(mp.horizon_lock), drone_high_freq_mode=int(mp.drone), adaptive_smoothing=int(mp.adaptive),
                      min_smoothing_radius=mp.min_radius, max_smoothing_radius=mp.max_radius, hf_shake_px=mp.hf_shake_px,
                      hf_rot_lp_alpha=mp.hf_rot_lp_alpha, hf_dead_zone_threshold=mp.hf_dead_zone, hf_freeze_duration=mp.hf_freeze_duration,
                      hf_motion_accumulator_decay=mp.hf_decay)


def arrays(stream):
    return (np.array([m for m, _ in stream], np.float64).reshape(-1, 6), np.array([KIND[k] for _, k in stream], np.int32))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def per_frame_checked(gpu, mp, stream, what):
    """The per-frame form, every push and every release held to the model.  -> (records, releases, model releases)"""
    rec, rel = gpu.trajectory(c_params(gpu, mp), [arrays(stream)])[0]
    n = len(stream)
    assert len(rec) == n + (len(rel) - sum(1 for r in rel if r.push >= 0)) and len(rel) == n + 1, (len(rec), len(rel))
    ck = K.Checker(mp, what)
    by_push = {r.push: r for r in rel if r.push >= 0}
    flushed = [r for r in rel if r.push < 0]
    out = []

    def hold(r, d, tag):
        assert d.out_index == r.idx, (tag, d.out_index, r.idx)
        assert r.has_M and bits(d.warp_matrix) == bits(r.M[:6]), tag
        m = ck.release(r.idx, r.n_seen, d.box_radius, d.intent, list(d.smoothed), list(r.M[:6]), list(r.M[6:]), tag=tag)
        if m.decided:
            # the inverse maps the warp consumes, inverted back in float64
            for got, (ref, E) in ((K.invert_map(r.Minv[:6]), m.matrix()), (K.invert_map(r.Minv[6:]), m.chroma_matrix())):
                B = E + 1e-9 + np.array([[0, 0, 1], [0, 0, 1]]) * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                assert (np.abs(got - ref) <= B).all(), (what, tag, got, ref)
        out.append(m)

    for i, (mod, kind) in enumerate(stream):
        d = rec[i]
        ck.push(mod, kind, list(d.transform), "push %d" % i)
        if i in by_push:
            assert by_push[i].n_seen == i + 1
            hold(by_push[i], d, "push %d" % i)
    for j, r in enumerate(flushed):
        assert r.n_seen == n
        hold(r, rec[n + j], "flush %d" % j)
    # the schedule the library ran is the one the model's own queue gives
    want = [(p if p is not None else -1, m.idx) for p, m in R.schedule(stream, mp)[1]] if not mp.adaptive else None
    if want is not None:
        assert [(r.push, r.idx) for r in rel] == want
    last = out[-1]
    assert last.identity and flushed[-1].idx == n and bits(flushed[-1].M) == bits([1, 0, 0, 0, 1, 0] * 2), "flush of idx >= n"
    share = ck.finish()
    print("%s: %d releases, %d undecided (%.2f%%), worst error / bound %s" % (what, ck.n_rel, ck.skipped, 100 * share, ck.worst))
    return rec, rel, out


def hold_batch(gpu, mp, streams, steps, ref, what):
    """The batch form of `streams` against their per-frame runs `ref` [(records, releases, model releases)]: every release's
    inverse maps bit-equal (and, inverted, within the model's matrix bound), every step's record and matrix equal to the
    per-frame record of the step's last push."""
    res = gpu.trajectory(c_params(gpu, mp), [arrays(s) for s in streams], steps=steps)
    for si, ((rec, rel), (prec, prel, mrel)) in enumerate(zip(res, ref)):
        t = "%s stream %d steps %s" % (what, si, steps[:4])
        n = len(streams[si])
        assert [(r.push, r.idx, r.n_seen) for r in rel] == [(r.push, r.idx, r.n_seen) for r in prel], t
        for r, pr, m in zip(rel, prel, mrel):
            assert list(r.Minv) == list(pr.Minv), (t, r.push, r.idx, list(r.Minv), list(pr.Minv))
            if r.has_M:
                assert bits(r.M) == bits(pr.M), (t, r.push)
            if m.decided:
                ref_M, E = m.matrix()
                assert (np.abs(K.invert_map(r.Minv[:6]) - ref_M) <= E + 1e-9 + np.spacing(np.abs(ref_M).astype(np.float32))).all(), (t, r.idx)
        # the steps this stream took part in: their last pushes
        ends, pos, k = [], 0, 0
        while pos < n:
            pos = min(n, pos + steps[k % len(steps)])
            ends.append(pos - 1)
            k += 1
        assert len(rec) == len(ends) + sum(1 for r in rel if r.push < 0), (t, len(rec), len(ends))
        seen_last = None
        for d, e in zip(rec, ends):
            p = prec[e]
            assert bits(d.transform) == bits(p.transform), (t, e)
            due = [r for r in rel if 0 <= r.push <= e]
            if due:                                  # the record keeps the step's (or an earlier step's) last release
                lastr = due[-1]
                q = prec[lastr.push]
                assert (d.out_index, d.box_radius, d.intent) == (q.out_index, q.box_radius, q.intent), (t, e)
                assert bits(d.smoothed) == bits(q.smoothed) and bits(d.warp_matrix) == bits(q.warp_matrix), (t, e)
                seen_last = lastr
        for d, p in zip(rec[len(ends):], prec[n:]):  # the flush
            assert bits(d.warp_matrix) == bits(p.warp_matrix) and d.out_index == p.out_index, t


_pf = {}


def pf(gpu, name, method, kw):
    key = (name, method, kw)
    if key not in _pf:
        mp = R.Params(**dict(I.SEQUENCES[name][1], method=method, **dict(kw)))
        _pf[key] = (mp,) + per_frame_checked(gpu, mp, I.stream(name), "%s %s %s" % (name, method, dict(kw)))
    return _pf[key]


@pytest.mark.parametrize("name,method,kw", CASES)
def test_per_frame_form(gpu, name, method, kw):
    pf(gpu, name, method, kw)


@pytest.mark.parametrize("steps", [[1], [64], RAGGED], ids=["step1", "step64", "ragged"])
@pytest.mark.parametrize("name,method,kw", [c for c in CASES if I.SEQUENCES[c[0]][2]])
def test_batch_form(gpu, name, method, kw, steps):
    """Kalman: releases in order on wave 0 of the tail; box and Gaussian: releases apart, one workgroup each; drone streams
    take the full append for every frame, the others the register fast path for all but a step's last."""
    mp, rec, rel, mrel = pf(gpu, name, method, kw)
    hold_batch(gpu, mp, [I.stream(name)], steps, [(rec, rel, mrel)], "%s %s" % (name, method))


@pytest.mark.parametrize("method,kw", [("box", ()), ("gaussian", (("gaussian_sigma", 2.0),)), ("kalman", ())])
def test_three_streams_one_launch(gpu, method, kw):
    """Three streams of different lengths, one tail workgroup each: every stream equals its own per-frame run."""
    streams = [I.stream("steady_pan")[:300], I.stream("reversals"), I.stream("with_failures")[:77]]
    mp = R.Params(smoothing_radius=6, method=method, **dict(kw))
    ref = [per_frame_checked(gpu, mp, s, "three streams %s #%d" % (method, i)) for i, s in enumerate(streams)]
    for steps in ([64], RAGGED):
        hold_batch(gpu, mp, streams, steps, ref, "three streams " + method)


@pytest.mark.parametrize("name", list(CLIPS))
def test_pipeline_on_clips(gpu, name):
    """The per-frame pipeline on the rendered clips: the record of every push (the append fused into the RANSAC selection) and
    of every release against the model."""
    p = gpu.params(**CLIPS[name][1])
    ck, intents = check_stabilizer(gpu.stabilizer(p), p, clip_frames(name), "device " + name)
    print(name, "releases", ck.n_rel, "skipped", ck.skipped, "intents", sorted(intents), "worst", ck.worst)
    assert ck.n_rel >= 30
    clip_coverage(name, ck, intents)
