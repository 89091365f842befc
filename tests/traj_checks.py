"""Bounds that hold a float32 trajectory stage (the CPU oracle or the HIP kernels) against the float64 model of
traj_ref.py.  The same checks run on both, so neither is judged by the other.  u = 2^-24, the unit roundoff of float32.

MEAN.  A sequential float32 sum of n samples is off by at most (n - 1) u sum|x_i| (first order), the division by n adds
u |mean|, and sum|x_i| / n <= max|x_i| = M: |mean32 - mean64| <= n u M.  traj_ref.mean_err uses (n + 2) u M; the two
extra terms cover the second-order remainder ((n u)^2 M < u M for n <= 101) and the float64 evaluation.  This is the
box-filter bound (`(terms + 2) 2^-24 max|sample in window|`).

VARIANCE.  A deviation d_i = x_i - mean carries e_d = e_mean + u |d_i|; its square 2 |d_i| e_d + u d_i^2; the n squares
are summed sequentially ((n - 1) u sum d_i^2) and divided (u var); with D = max|d_i| + e_mean:
|var32 - var64| <= 2 D e_d + (n + 3) u D^2  (traj_ref.mean_var).  The adaptive radius takes sqrt(vx + vy + 1000 va)
(three more roundings, then e / (2 total) + u total through the root) and doubles it; the consistency 1 / (1 + var / mean^2)
propagates e_var and e_mean through the quotient (traj_ref.Model.intent).

GAUSSIAN.  A float32 tap exp(-x^2 / (2 s^2)) / sum: the argument a = x^2 / (2 s^2) carries three roundings (3 a u on
the exponential), expf one ulp, the normalising sum of ks taps (ks - 1) u and the division u: relative (ks + 5 + 3 a_max) u
per tap (traj_ref.gaussian_taps).  The taps sum to 1, so sum |p_j| k_j <= M; each product rounds once and the ks products
are summed sequentially: |g32 - g64| <= (tap bound + (ks + 1) u) M.

BLEND.  out = raw + g (smoothed - path): the difference, the product and the sum round once each, on top of g times the
bound of `smoothed`: g e_sm + 3 u (|diff| + |out| + |raw|).

MATRIX.  cos(da) and sin(da): the float64 value within one float32 ulp of it, plus the slope (|sin|, |cos| <= 1) times the
bound of da.  The inverse maps are double inversions of that float matrix; inverting them back in float64 returns the
matrix to ~1e-15, so they are held to the matrix bound plus INV_EPS.

DRONE FILTERS (traj_ref.Model._drone).  magnitude = sqrt(dx^2 + dy^2 + 100 da^2): three squares, the product by 100, two
sums and the root round once each, every one relative to a quantity <= magnitude^2 (or magnitude): <= 6 u magnitude; da's
own ulp e_a enters as 100 |da| e_a / magnitude <= 10 e_a.  e_mag = 6 u mag + 10 e_a.  The accumulator max(acc * decay, mag) is
either mag (error e_mag) or a product that rounds once per push it keeps decaying: after k pushes of decay since it last was
a magnitude, (k + 1) u acc + e_mag; the clamps min / max are exact.  The deviation from the median: two differences, two
squares, a sum and a root, each relative to at most max(|tr|, |median|, dm): 6 u of that.  The shake blend
median + d * g: the difference d, the product and the sum round once each, plus the even median's own rounding: 4 u of the
largest of |median|, |d|, |out|; the rotation low-pass (1 - a) lp + a da: two products, the sum and 1 - a: 4 u of
max(|lp|, |da|) plus a times da's ulp.  The adaptive radius (1 - min(1, mag / 50)) span: root of two squares and a sum (3), the
division, the subtraction (absolute u), the product: 6 u span.

KALMAN.  No bound derived.  Measured on this project's CPU oracle (vso_kalman_filter, float32, one sequential
recursion) against traj_ref.kalman64 over the x, y and angle paths of every stream of traj_inputs.py (9 streams, 27
tracks): the worst |oracle - float64| / max|path| is KALMAN_MEASURED.  The tolerance is KALMAN_FACTOR times that, for an
implementation that rounds the same recursion in another (still sequential) pattern.  test_traj_model_cpu.py
re-measures the figure and fails if the oracle exceeds the recorded one; it was not tuned against the GPU.
"""
import numpy as np

import traj_ref as R

U = R.U
KALMAN_MEASURED, KALMAN_FACTOR, KALMAN_TOL = R.KALMAN_MEASURED, R.KALMAN_FACTOR, R.KALMAN_TOL   # the constants live in traj_ref.py
INV_EPS = 1e-12
MAX_SKIPPED = 0.02        # share of a run's releases that may be undecided


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


class Checker:
    """Holds one recorded run to the model: push() every append with the transform the implementation reported,
    release() every output with what it reported; the model continues from the reported float32 transforms."""

    def __init__(self, params, what=""):
        self.m = R.Model(params)
        self.what = what
        self.n_rel = 0
        self.skipped = 0
        self.worst = {"transform": 0.0, "smoothed": 0.0, "matrix": 0.0}

    def _ratio(self, key, err, bound):
        if bound > 0:
            self.worst[key] = max(self.worst[key], err / bound)

    def push(self, model, kind, observed, tag=""):
        r = self.m.push(model, kind, observed=observed)
        assert not r.undecided, "%s %s: stateful decision too close to call in the model: %s" % (self.what, tag, r.undecided)
        for c in range(3):
            e = abs(float(observed[c]) - r.tr[c])
            # one more float32 rounding of the value itself on top of the bound of the float64 quantity
            b = r.tr_err[c] + (ulp32(r.tr[c]) if r.tr_err[c] > 0 else 0.0)
            assert e <= b, "%s %s: transform[%d] %r, model %r, |diff| %.3g > bound %.3g" % (self.what, tag, c, observed[c], r.tr[c], e, b)
            self._ratio("transform", e, b)
        return r

    def release(self, idx, n_seen, box_radius=None, intent=None, smoothed=None, M=None, Mc=None, tag=""):
        """-> the model's Release; counted as skipped (and not compared) when one of its own decisions is undecided."""
        r = self.m.release(idx, n_seen)
        self.n_rel += 1
        if not r.decided:
            self.skipped += 1
            return r
        t = "%s %s (idx %d, n_seen %d)" % (self.what, tag, idx, n_seen)
        if box_radius is not None:
            want = r.box_radius if self.m.p.method == "box" else 0
            assert box_radius == want, "%s: box_radius %d, model %d" % (t, box_radius, want)
        if intent is not None:
            assert intent == r.intent, "%s: intent %d, model %d" % (t, intent, r.intent)
        if smoothed is not None:
            for c in range(3):
                e = abs(float(smoothed[c]) - r.smoothed[c])
                b = r.smoothed_err[c] + (ulp32(r.smoothed[c]) if r.smoothed_err[c] > 0 else 0.0)
                assert e <= b, "%s: smoothed[%d] %r, model %r, |diff| %.3g > bound %.3g" % (t, c, smoothed[c], r.smoothed[c], e, b)
                self._ratio("smoothed", e, b)
        for got, (ref, E), name in ((M, r.matrix(), "matrix"), (Mc, r.chroma_matrix(), "chroma matrix")):
            if got is None:
                continue
            got = np.asarray(got, np.float64).reshape(2, 3)
            err = np.abs(got - ref)
            # the translation is rounded to float32 once more
            B = E + INV_EPS + np.array([[0, 0, 1], [0, 0, 1]]) * np.where(E > 0, np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), 0)
            bad = err > B
            assert not bad.any(), "%s: %s\n%s\nmodel\n%s\n|diff|\n%s\nbound\n%s" % (t, name, got, ref, err, B)
            self._ratio("matrix", float((err / np.maximum(B, 1e-300)).max()), 1.0)
        return r

    def finish(self):
        share = self.skipped / max(self.n_rel, 1)
        assert share <= MAX_SKIPPED, "%s: %d of %d releases undecided (%.1f%% > %.0f%%)" % (
            self.what, self.skipped, self.n_rel, 100 * share, 100 * MAX_SKIPPED)
        return share


def invert_map(minv6):
    """The forward 2x3 matrix whose inverse map is minv6 (float64)."""
    A = np.asarray(minv6, np.float64).reshape(2, 3)
    L = np.linalg.inv(A[:, :2])
    return np.hstack([L, (-L @ A[:, 2])[:, None]])


def coverage(model, releases):
    """Counts the assertions of the tests are made of: from the model's own records."""
    from collections import Counter
    P = model.pushes
    return dict(
        intents=Counter(r.intent for _, r in releases if r.decided and not r.identity),
        box_radii=Counter(r.box_radius for _, r in releases if r.decided and not r.identity),
        q_low=sum(1 for _, r in releases if r.adaptive_q is not None and r.adaptive_q < 5),
        q_high=sum(1 for _, r in releases if r.adaptive_q is not None and r.adaptive_q > 25),
        q_mid=sum(1 for _, r in releases if r.adaptive_q is not None and 5 < r.adaptive_q < 25),
        frozen=sum(p.frozen for p in P),
        entered=sum(p.entered for p in P),
        exits=Counter(p.exit for p in P if p.exit),
        bands=Counter(p.shake_band for p in P if p.shake_band is not None),
        median_n=Counter(p.median_n for p in P),
        radii=Counter(p.radius for p in P),
        identity=sum(r.identity for _, r in releases),
        short=sum(1 for _, r in releases if r.n_seen < 15 and not r.identity),
        wrapped=sum(1 for _, r in releases if r.n_seen > 256),
        undecided=sum(not r.decided for _, r in releases),
        stateful_undecided=[u for p in P for u in p.undecided],
    )
