"""The float64 trajectory model (traj_ref.py) against the CPU oracle, on the designed streams of traj_inputs.py and
on three rendered clips; and the coverage each stream claims, counted from the model.  No GPU."""
import math

import numpy as np
import pytest

import traj_checks as K
import traj_inputs as I
import traj_ref as R
from vsamd import synth

U = R.U


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib
    return oracle_lib.load()


_runs = {}


def model_run(name, method="box", **kw):
    key = (name, method, tuple(sorted(kw.items())))
    if key not in _runs:
        p = dict(I.SEQUENCES[name][1], method=method, **kw)
        _runs[key] = R.schedule(I.stream(name), R.Params(**p))
    return _runs[key]


# ---- the model alone: stateful decisions are never undecided, and every stream reaches what it was built for -----------
@pytest.mark.parametrize("name", list(I.SEQUENCES))
def test_stateful_decisions_decided(name):
    m, rel = model_run(name)
    c = K.coverage(m, rel)
    assert 300 <= len(m.pushes) <= 600
    assert c["stateful_undecided"] == [], c["stateful_undecided"]
    share = c["undecided"] / len(rel)
    print("%s: %d pushes, %d releases, %d undecided (%.2f%%)" % (name, len(m.pushes), len(rel), c["undecided"], 100 * share))
    assert share <= K.MAX_SKIPPED, "%s: %d of %d releases undecided" % (name, c["undecided"], len(rel))
    # the ring wraps, the flush ends on a frame without a transform, and a short queue releases before 15 transforms exist
    assert c["wrapped"] > 0 and c["identity"] == 1, c
    assert c["short"] > 0 or I.SEQUENCES[name][1]["smoothing_radius"] >= 15, c


def test_coverage_claims():
    c = {n: K.coverage(*model_run(n)) for n in I.SEQUENCES}
    for n, v in c.items():
        print(n, {k: (dict(x) if hasattr(x, "items") else x) for k, x in v.items()})
    assert c["steady_pan"]["intents"][1] >= 250, c["steady_pan"]["intents"]
    assert c["still_rotation_jitter"]["intents"][2] >= 250, c["still_rotation_jitter"]["intents"]
    assert c["reversals"]["intents"][3] >= 150 and c["reversals"]["intents"][0] >= 50, c["reversals"]["intents"]
    d = c["drone_dead_zone"]
    assert set(d["exits"]) == {"duration", "motion", "accum"} and min(d["exits"].values()) >= 5, d["exits"]
    assert d["frozen"] >= 50 and d["entered"] >= 20, d
    assert set(d["bands"]) == {0, 1, 2} and min(d["bands"].values()) >= 20, d["bands"]
    assert max(d["box_radii"]) == 25 and min(d["box_radii"]) == 10 and len(d["box_radii"]) >= 10, d["box_radii"]   # > 17 samples: the long-window path
    h = c["drone_horizon"]
    assert h["frozen"] >= 20 and set(h["bands"]) == {0, 1, 2}, h
    s = c["drone_short_history"]
    assert s["median_n"][0] >= 8 and all(s["median_n"][k] >= 1 for k in (5, 6, 7, 8, 9)) and s["median_n"][10] >= 200, s["median_n"]
    b = c["radius_bands"]
    assert b["q_low"] >= 80 and b["q_high"] >= 80 and b["q_mid"] >= 40, b
    assert set(b["box_radii"]) == {5, 6, 7, 8}, b["box_radii"]
    a = c["adaptive_sweep"]
    assert set(a["radii"]) >= set(range(5, 51)), sorted(a["radii"])
    f = c["with_failures"]
    assert len(f["intents"]) >= 2, f["intents"]
    kinds = [k for _, k in I.stream("with_failures")]
    assert kinds.count(R.FAIL) >= 30 and kinds.count(R.SKIP) >= 20


def test_adaptive_radius_moves_the_queue():
    """With adaptive smoothing the release threshold clamp(radius, 5, 35) moves mid-stream: pushes that release nothing
    after the first release, and releases at the shortest and at the longest queue."""
    m, rel = model_run("adaptive_sweep")
    lags = {r.n_seen - r.idx for p, r in rel if p is not None}
    assert lags == {4, 34}, lags                                  # released at 5 queued frames, later at the cap of 35
    first = min(p for p, _ in rel if p is not None)
    silent = len(m.pushes) - first - sum(1 for p, _ in rel if p is not None)
    assert silent >= 20, silent                                   # pushes after the first release that released nothing
    assert sum(1 for p, _ in rel if p is None) == 34              # the flush empties the queue the cap left


# ---- the oracle's pure functions --------------------------------------------------------------------------------------
def _paths(name):
    m, _ = model_run(name)
    return np.asarray(m.path, np.float32), np.asarray(m.tr, np.float32)


LENGTHS = (1, 2, 5, 9, 10, 14, 15, 21, 31, 32, 40, 64, 150)


@pytest.mark.parametrize("name", list(I.SEQUENCES))
def test_box_filter_and_adaptive_radius(oracle, name):
    path, _ = _paths(name)
    drone = bool(I.SEQUENCES[name][1].get("drone"))
    worst = 0.0
    for n in LENGTHS + (len(path),):
        p = path[len(path) - n:] if n < len(path) else path
        m = R.Model(R.Params(method="box", drone=drone, smoothing_radius=7))
        m.path = [list(map(float, v)) for v in p]
        p64 = p.astype(np.float64)
        rel = R.Release()
        m.box(p64, 0, rel)
        if rel.box_radius_decided:
            want = oracle.adaptive_radius(p[:, 0], p[:, 1], p[:, 2], 7)
            ar = int(max(5.0, min(25.0, rel.adaptive_q))) if rel.adaptive_q is not None else 7
            assert want == ar, (name, n, want, ar, rel.adaptive_q)
        for radius_param in (1, 5, 8, 13, 25, 60):
            got = [oracle.box_filter(p[:, c], radius_param, drone) for c in range(3)]
            for idx in sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n))):
                sm, err = _box_fixed(p64, idx, radius_param, drone)
                for c in range(3):
                    e = abs(float(got[c][idx]) - sm[c])
                    b = err[c] + (K.ulp32(sm[c]) if err[c] > 0 else 0)
                    assert e <= b, (name, n, radius_param, idx, c, got[c][idx], sm[c], e, b)
                    if b > 0:
                        worst = max(worst, e / b)
    print("box worst error / bound %.3f" % worst)


def _box_fixed(p64, idx, radius_param, drone):
    """The model's box mean for a given radius parameter, the adaptive radius set aside."""
    return R.Model(R.Params(method="box", drone=drone)).box(p64, idx, R.Release(), radius=radius_param)


@pytest.mark.parametrize("sigma,taps", [(0.5, 3), (2.0, 13), (10.4, 63)])
def test_gaussian_filter(oracle, sigma, taps):
    k, _ = R.gaussian_taps(sigma)
    assert len(k) == taps and abs(k.sum() - 1) < 1e-15
    worst = 0.0
    for name in I.SEQUENCES:
        path, _ = _paths(name)
        for n in LENGTHS + (len(path),):                      # 1 .. 31 are shorter than the half-width of 63 taps
            p = path[:n]
            m = R.Model(R.Params(method="gaussian", gaussian_sigma=sigma))
            got = [oracle.gaussian_filter(p[:, c], sigma) for c in range(3)]
            for idx in range(n) if n <= 64 else list(range(40)) + list(range(n - 40, n)):
                sm, err = m.gaussian(p.astype(np.float64), idx)
                for c in range(3):
                    e = abs(float(got[c][idx]) - sm[c])
                    b = err[c] + K.ulp32(sm[c])
                    assert e <= b, (name, n, idx, c, got[c][idx], sm[c], e, b)
                    worst = max(worst, e / b if b else 0)
    print("gaussian sigma %g worst error / bound %.3f" % (sigma, worst))


def test_kalman_filter_and_its_constant(oracle):
    """Measures what KALMAN_MEASURED records and holds the oracle to KALMAN_TOL."""
    worst = 0.0
    for name in I.SEQUENCES:
        path, _ = _paths(name)
        for c in range(3):
            got = oracle.kalman_filter(path[:, c]).astype(np.float64)
            ref = R.kalman64(path[:, c].astype(np.float64))
            scale = float(np.max(np.abs(path[:, c])))
            if scale > 0:
                worst = max(worst, float(np.max(np.abs(got - ref))) / scale)
    print("kalman: worst |oracle - float64| / max|path| = %.4g (recorded %.4g, factor %g, tolerance %.4g)" % (
        worst, K.KALMAN_MEASURED, K.KALMAN_FACTOR, K.KALMAN_TOL))
    assert worst <= K.KALMAN_MEASURED, "measured %.4g exceeds the recorded basis %.4g of KALMAN_TOL" % (worst, K.KALMAN_MEASURED)
    assert K.KALMAN_MEASURED <= 2 * worst + 1e-12, "recorded basis %.4g is stale (measured %.4g)" % (K.KALMAN_MEASURED, worst)
    assert K.KALMAN_TOL == K.KALMAN_FACTOR * K.KALMAN_MEASURED


@pytest.mark.parametrize("name", list(I.SEQUENCES))
def test_motion_intent(oracle, name):
    _, tr = _paths(name)
    m = R.Model(R.Params())
    m.tr = [list(map(float, v)) for v in tr]
    skipped = total = 0
    seen = set()
    for n in (14, 15, 16, 40, len(tr)):
        for idx in range(1, n + 3) if n <= 40 else range(1, n, 3):
            total += 1
            if idx < n:
                it, ok = m.intent(np.asarray(m.tr[idx]), idx, n)
                got = oracle.motion_intent(tr[:n], idx)
            else:
                # the window [idx - 15, min(idx, n)) with a zero motion, as the oracle's entry point defines idx >= n
                mm = R.Model(R.Params()); mm.tr = m.tr[:n] + [[0.0, 0.0, 0.0]] * (idx - n + 1)
                it, ok = mm.intent(np.zeros(3), idx, n)
                got = oracle.motion_intent(tr[:n], idx)
            if not ok:
                skipped += 1
                continue
            seen.add(it)
            assert got == it, (name, n, idx, got, it)
    print("%s: intents %s, %d of %d undecided" % (name, sorted(seen), skipped, total))
    assert skipped <= K.MAX_SKIPPED * total, (skipped, total)


# ---- the oracle stabilizer on rendered clips ---------------------------------------------------------------------------
CLIPS = {
    "intent": (None, dict(smoothing_radius=6)),                # traj_inputs.intent_clip: all four intents
    "drone": (dict(seed=synth.SEED_CONFIG1 + 6, n=48), dict(smoothing_radius=10, drone_high_freq_mode=1, hf_dead_zone_threshold=2.0,
                                                            hf_freeze_duration=4, hf_shake_px=1.5)),
    "adaptive": (dict(seed=synth.SEED_CONFIG1 + 7, n=48), dict(smoothing_radius=8, adaptive_smoothing=1, min_smoothing_radius=5,
                                                               max_smoothing_radius=12)),
}
CLIP_SMOOTHERS = [dict(), dict(smoothing_method=1, gaussian_sigma=0.5), dict(smoothing_method=1, gaussian_sigma=2.0),
                  dict(smoothing_method=1, gaussian_sigma=10.4), dict(smoothing_method=2)]
_clips = {}


def clip_frames(name):
    if name not in _clips:
        c = CLIPS[name][0]
        _clips[name] = I.intent_clip() if c is None else synth.make_clip(c["seed"], 320, 240, c["n"])
    return _clips[name]


def model_params(p):
    """traj_ref.Params of a vs_params_c."""
    return R.Params(smoothing_radius=p.smoothing_radius, method=("box", "gaussian", "kalman")[p.smoothing_method],
                    gaussian_sigma=p.gaussian_sigma, horizon_lock=p.horizon_lock, drone=p.drone_high_freq_mode,
                    adaptive=p.adaptive_smoothing, min_radius=p.min_smoothing_radius, max_radius=p.max_smoothing_radius,
                    hf_shake_px=p.hf_shake_px, hf_rot_lp_alpha=p.hf_rot_lp_alpha, hf_dead_zone=p.hf_dead_zone_threshold,
                    hf_freeze_duration=p.hf_freeze_duration, hf_decay=p.hf_motion_accumulator_decay)


def check_stabilizer(stab, params, frames, what):
    """Pushes frames through a stabilizer (oracle or device: push() / debug()) and holds every debug record to the model."""
    ck = K.Checker(model_params(params), what)
    n_tr = 0
    intents = set()
    for k, f in enumerate(frames):
        out = stab.push(f)
        if k == 0:
            assert out is None
            continue
        d = stab.debug()
        model = [d.model[i] for i in range(6)]
        kind = R.SKIP if d.n_prev == 0 else (R.FAIL if math.isnan(model[0]) else None)
        ck.push(model, kind, [d.transform[i] for i in range(3)], "push %d" % k)
        n_tr += 1
        if out is not None:
            r = ck.release(d.out_index, n_tr, d.box_radius, d.intent, list(d.smoothed), list(d.warp_matrix), tag="push %d" % k)
            if r.decided:
                intents.add(r.intent)
    ck.finish()
    return ck, intents


def clip_coverage(name, ck, intents):
    """What each clip is there for, counted from the model that was fed the run."""
    P = ck.m.pushes
    if name == "intent":
        assert intents == {0, 1, 2, 3}, intents
    if name == "drone":
        assert sum(p.frozen for p in P) >= 3 and sum(p.entered for p in P) >= 1, "no frozen frame"
        assert len({p.shake_band for p in P if p.shake_band is not None}) >= 2, "one shake band only"
        assert any(p.exit for p in P), "no dead-zone exit"
    if name == "adaptive":
        assert len({p.radius for p in P}) >= 3, sorted({p.radius for p in P})


@pytest.mark.parametrize("smoother", range(len(CLIP_SMOOTHERS)), ids=["box", "gauss3", "gauss13", "gauss63", "kalman"])
@pytest.mark.parametrize("name", list(CLIPS))
def test_oracle_stabilizer_on_clips(oracle, name, smoother):
    """Every clip with every smoother: the whole release path (smoothing, gain blend, matrix) of the oracle against the model."""
    p = oracle.params(**dict(CLIPS[name][1], **CLIP_SMOOTHERS[smoother]))
    ck, intents = check_stabilizer(oracle.stabilizer(p), p, clip_frames(name), "oracle %s %s" % (name, CLIP_SMOOTHERS[smoother]))
    print(name, "releases", ck.n_rel, "skipped", ck.skipped, "intents", sorted(intents), "worst", ck.worst)
    assert ck.n_rel >= 30
    clip_coverage(name, ck, intents)


def test_gaussian_short_streams_follow_the_projects_definition(oracle):
    """Streams no longer than the half-width: the reference indexes past the ends of its vector there (undefined), so these
    cases hold the oracle to the project's own definition - the nearest valid sample - and to nothing the reference states."""
    path, _ = _paths("reversals")
    m = R.Model(R.Params(method="gaussian", gaussian_sigma=10.4))
    for n in (1, 2, 5, 31):
        got = oracle.gaussian_filter(path[:n, 0], 10.4)
        for idx in range(n):
            sm, err = m.gaussian(path[:n].astype(np.float64), idx)
            assert abs(float(got[idx]) - sm[0]) <= err[0] + K.ulp32(sm[0]), (n, idx)
