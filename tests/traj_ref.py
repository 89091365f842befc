"""Float64 model of the trajectory stage: what one push appends and what one release hands to the warp.

Written from the behaviour of the reference stabilizer (append of the measured transform with the drone filters, path
accumulation, adaptive smoothing radius, the three smoothers, motion intent, gain blend, 2x3 matrix); it shares no code
with the CPU oracle or the device headers.  numpy only.

Precision model
 - a transform and a path sample are float32 values.  The path is one rounded float32 addition per push and has one
   possible value: it is carried in float32.  dx = float(model[2]) and dy = float(model[5]) are exact too.
 - everything that is a sum over a window (box mean, Gaussian taps, variances, means) is evaluated in float64 over
   those float32 samples and comes with a bound `err` on what a float32 evaluation in any sequential order may differ
   by (traj_checks.py has the derivations).
 - every decision (a comparison with a threshold, a truncation to int) is reported as undecided when the float64
   quantity is closer to the threshold than its bound.
 - the model can be "fed back": push(..., observed=(dx, dy, da)) continues from the float32 transform that the
   implementation under test reported, after the caller has held that transform to the model's own prediction
   (Push.tr, Push.tr_err).  Later windows are then evaluated over the very samples the implementation used, so one
   float32 ulp in an arctangent does not grow into a path difference.
"""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
# Kalman tolerance relative to max|path| (traj_checks.py, KALMAN, says where the figures come from)
KALMAN_MEASURED = 1.0e-7  # measured 9.321e-08 (CPU oracle, 27 tracks), rounded up
KALMAN_FACTOR = 4.0
KALMAN_TOL = KALMAN_FACTOR * KALMAN_MEASURED
F32 = np.float32

FAIL = "fail"           # estimation failed: the identity goes through the drone filters
SKIP = "skip"           # no previous gray image / no keypoints: (0, 0, 0) is appended as it is


def f32(x):
    return float(F32(x))


class Params:
    def __init__(self, smoothing_radius=30, method="box", gaussian_sigma=2.0, horizon_lock=False, drone=False,
                 adaptive=False, min_radius=5, max_radius=50, hf_shake_px=1.5, hf_rot_lp_alpha=0.2, hf_dead_zone=2.0,
                 hf_freeze_duration=10, hf_decay=0.9):
        self.smoothing_radius = int(smoothing_radius)
        self.method = method
        self.gaussian_sigma = f32(gaussian_sigma)
        self.horizon_lock = bool(horizon_lock)
        self.drone = bool(drone)
        self.adaptive = bool(adaptive)
        self.min_radius, self.max_radius = int(min_radius), int(max_radius)
        self.hf_shake_px, self.hf_rot_lp_alpha = f32(hf_shake_px), f32(hf_rot_lp_alpha)
        self.hf_dead_zone, self.hf_decay = f32(hf_dead_zone), f32(hf_decay)
        self.hf_freeze_duration = int(hf_freeze_duration)


# ---- three-valued comparisons ---------------------------------------------------------------------------------------
def lt(a, b, err):
    """a < b, or None when |a - b| <= err."""
    if abs(a - b) <= err:
        return None
    return bool(a < b)


def gt(a, b, err):
    return lt(b, a, err)


def and3(*v):
    if any(x is False for x in v):
        return False
    if any(x is None for x in v):
        return None
    return True


def or3(*v):
    if any(x is True for x in v):
        return True
    if any(x is None for x in v):
        return None
    return False


# ---- window statistics with bounds ----------------------------------------------------------------------------------
def mean_err(x, sample_err=0.0):
    """Bound on a float32 sequential mean of the float32 samples x (traj_checks.MEAN)."""
    n = len(x)
    return (n + 2) * U * float(np.max(np.abs(x))) + sample_err if n else 0.0


def mean_var(x, sample_err=0.0):
    """(mean, mean_err, variance, variance_err) of samples x in float64; sample_err: absolute error each sample may carry."""
    x = np.asarray(x, np.float64)
    n = len(x)
    m = float(x.sum() / n)
    em = mean_err(x, sample_err)
    d = x - m
    D = float(np.max(np.abs(d))) + em + sample_err
    ed = em + sample_err + U * D                       # error of one deviation
    v = float((d * d).sum() / n)
    ev = 2 * D * ed + (n + 3) * U * D * D                # squares, their sequential sum, the division
    return m, em, v, ev


class Push:
    """What one push appended."""
    def __init__(self):
        self.tr = None          # float64 prediction of (dx, dy, da) after the drone filters
        self.tr_err = None      # bound per component (0: the value is exact)
        self.used = None        # float32 transform the model continued from
        self.path = None        # float32 path sample
        self.frozen = False
        self.shake_band = None  # drone: 0 (<shake), 1 (<2 shake), 2 (pass-through)
        self.median_n = 0       # history length the median was taken over (0: none taken)
        self.exit = None        # dead zone left by: "duration" | "motion" | "accum"
        self.entered = False
        self.radius = None      # smoothing_radius after the push
        self.undecided = []     # names of stateful decisions that were too close to call


class Release:
    def __init__(self):
        self.idx = self.n_seen = 0
        self.identity = False
        self.box_radius = 0
        self.box_radius_decided = True
        self.adaptive_q = None          # total * 2 before the clamp (box, n_seen >= 10)
        self.intent = 0
        self.intent_decided = True
        self.smoothed = None            # float64[3]
        self.smoothed_err = None
        self.out = None                 # float64 (dx, dy, da)
        self.out_err = None
        self.gain = None

    @property
    def decided(self):
        return self.box_radius_decided and self.intent_decided

    def matrix(self):
        """(M 2x3 float64, bound 2x3): [cos -sin dx; sin cos dy]; cos / sin within one float32 ulp plus the slope times
        the bound of da."""
        if self.identity:
            return np.array([[1., 0., 0.], [0., 1., 0.]]), np.zeros((2, 3))
        dx, dy, da = self.out
        c, s = math.cos(da), math.sin(da)
        ec = float(np.spacing(F32(abs(c)))) + abs(s) * self.out_err[2] + self.out_err[2] ** 2
        es = float(np.spacing(F32(abs(s)))) + abs(c) * self.out_err[2] + self.out_err[2] ** 2
        M = np.array([[c, -s, dx], [s, c, dy]])
        E = np.array([[ec, es, self.out_err[0]], [es, ec, self.out_err[1]]])
        return M, E

    def chroma_matrix(self):
        M, E = self.matrix()
        M = M.copy(); E = E.copy()
        M[:, 2] *= 0.5; E[:, 2] *= 0.5
        return M, E


def gaussian_taps(sigma):
    """(taps float64, relative bound of one float32 tap)."""
    sigma = f32(sigma)
    ks = max(3, int(math.ceil(6 * sigma)))
    if ks % 2 == 0:
        ks += 1
    c = ks // 2
    x = np.arange(ks, dtype=np.float64) - c
    a = (x * x) / (2.0 * sigma * sigma)
    k = np.exp(-a)
    k /= k.sum()
    return k, (ks + 5 + 3 * float(a.max())) * U


class Model:
    def __init__(self, params):
        self.p = params
        self.tr = []            # float32 transforms, as float64 numbers
        self.path = []          # float32 path samples
        self.radius = params.smoothing_radius
        # drone state
        self.hist = []
        self.median = [0.0, 0.0]
        self.rot_lp = 0.0
        self.in_dz = False
        self.freeze = 0
        self.accum = 0.0
        self.accum_ulps = 0
        # kalman
        self._kal_out = []
        self.pushes = []

    # -- append -----------------------------------------------------------------------------------------------------
    def push(self, model, kind=None, observed=None):
        p = self.p
        r = Push()
        tr = [0.0, 0.0, 0.0]
        err = [0.0, 0.0, 0.0]
        if kind != SKIP:
            T = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] if (kind == FAIL or model is None) else [f32(v) for v in model]
            tr = [T[2], T[5], math.atan2(T[3], T[0])]
            err = [0.0, 0.0, float(np.spacing(F32(abs(tr[2]))))]
            if tr[2] == 0.0:
                err[2] = 0.0
            if p.drone:
                tr, err = self._drone(tr, err, r)
        r.tr, r.tr_err = tr, err
        used = [f32(v) for v in tr] if observed is None else [float(F32(v)) for v in observed]
        r.used = used
        if p.drone and kind != SKIP:
            if p.horizon_lock:
                self.rot_lp = used[2]
            self.hist.append((used[0], used[1]))
            if len(self.hist) > 10:
                self.hist.pop(0)
        self.tr.append(used)
        if not self.path:
            self.path.append(list(used))
        else:
            last = self.path[-1]
            self.path.append([float(F32(last[c]) + F32(used[c])) for c in range(3)])
        r.path = self.path[-1]
        if p.adaptive and len(self.tr) >= 3:
            mag = math.hypot(used[0], used[1])
            ms = 1.0 - max(0.0, min(1.0, mag / 50.0))
            span = p.max_radius - p.min_radius
            v = ms * span
            # float32: sqrt of two squares and a sum (3 roundings), the division, the subtraction from 1 (absolute U),
            # the product: within 6 U of span
            e = 6 * U * max(abs(span), 1)
            exact = mag == 0.0 or mag / 50.0 >= 1.0 + 4 * U        # motionScale is exactly 1 or exactly 0
            if abs(v - round(v)) <= e and not exact:
                r.undecided.append("adaptive_radius")
            self.radius = p.min_radius + int(v)
        r.radius = self.radius
        self.pushes.append(r)
        return r

    def _drone(self, tr, err, r):
        p = self.p
        dz = p.hf_dead_zone
        mag = math.sqrt(tr[0] ** 2 + tr[1] ** 2 + tr[2] ** 2 * 100.0)
        emag = 6 * U * mag + 10 * err[2]
        dec = self.accum * p.hf_decay
        if dec >= mag:
            self.accum_ulps += 1
        else:
            self.accum_ulps = 0
        acc = max(dec, mag)
        eacc = (self.accum_ulps + 1) * U * acc + emag
        acc = min(acc, f32(dz * 5.0))
        acc = max(0.0, min(acc, 100.0))
        self.accum = acc
        frozen = False
        if not self.in_dz:
            enter = lt(mag, dz, emag)
            if enter is None:
                r.undecided.append("dead_zone_enter")
            if enter:
                self.in_dz = True
                self.freeze = p.hf_freeze_duration
                r.entered = True
        if self.in_dz:
            self.freeze -= 1
            expired = self.freeze <= 0
            motion = gt(mag, f32(dz * 1.5), emag)
            accum = gt(acc, f32(dz * 1.2), eacc)
            leave = or3(expired, motion, accum)
            if leave is None:
                r.undecided.append("dead_zone_exit")
            if leave:
                # the order of the tests does not change the outcome; it names the exit for the coverage counts
                r.exit = "duration" if expired else ("motion" if motion else "accum")
                self.in_dz = False
                self.freeze = 0
                self.accum = 0.0
                self.accum_ulps = 0
            else:
                frozen = True
        r.frozen = frozen
        if frozen:
            tr, err = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        # micro-shake suppression around the median of the last <= 10 appended translations (taken from 5 on)
        n = len(self.hist)
        if n >= 5:
            r.median_n = n
            for c in range(2):
                v = sorted(h[c] for h in self.hist)
                self.median[c] = f32((F32(v[n // 2 - 1]) + F32(v[n // 2])) / F32(2.0)) if n % 2 == 0 else v[n // 2]
        d = [tr[0] - self.median[0], tr[1] - self.median[1]]
        dm = math.hypot(d[0], d[1])
        edm = 6 * U * max(dm, abs(tr[0]), abs(tr[1]), abs(self.median[0]), abs(self.median[1]))
        b0 = lt(dm, p.hf_shake_px, edm)
        b1 = lt(dm, f32(p.hf_shake_px * 2.0), edm)
        if b0 is None or (b0 is False and b1 is None):
            r.undecided.append("shake_band")
        out = list(tr)
        oerr = list(err)
        if b0:
            r.shake_band = 0
            g = f32(0.01)
        elif b1:
            r.shake_band = 1
            g = f32(0.05)
        else:
            r.shake_band = 2
            g = None
        if g is not None:
            for c in range(2):
                out[c] = self.median[c] + d[c] * g
                oerr[c] = 4 * U * max(abs(self.median[c]), abs(d[c]), abs(out[c]))
        if p.horizon_lock:
            a = p.hf_rot_lp_alpha
            out[2] = f32(1.0 - a) * self.rot_lp + a * tr[2]
            oerr[2] = 4 * U * max(abs(self.rot_lp), abs(tr[2])) + a * err[2]
        return out, oerr

    # -- release ----------------------------------------------------------------------------------------------------
    def release(self, idx, n_seen=None):
        p = self.p
        n = len(self.tr) if n_seen is None else n_seen
        r = Release()
        r.idx, r.n_seen = idx, n
        if idx >= n:
            r.identity = True
            r.smoothed = np.zeros(3); r.smoothed_err = np.zeros(3)
            r.out = np.zeros(3); r.out_err = np.zeros(3)
            return r
        path = np.asarray(self.path[:n], np.float64)
        if p.method == "gaussian":
            sm, esm = self.gaussian(path, idx)
        elif p.method == "kalman":
            sm, esm = self.kalman(path, idx)
        else:
            sm, esm = self.box(path, idx, r)
        r.smoothed, r.smoothed_err = sm, esm
        raw = np.asarray(self.tr[idx], np.float64)
        d = sm - path[idx]
        g = 1.0
        if idx > 0:
            r.intent, r.intent_decided = self.intent(raw, idx, n)
            g = {0: f32(0.7), 1: 0.5, 2: 1.0, 3: f32(0.8)}[r.intent]
        r.gain = g
        out = raw + g * d
        oerr = g * esm + 3 * U * (np.abs(d) + np.abs(out) + np.abs(raw))
        if p.horizon_lock:
            out[2] = 0.0; oerr[2] = 0.0
        r.out, r.out_err = out, oerr
        return r

    def box(self, path, idx, r, radius=None):
        """radius: the radius parameter to smooth with, the adaptive radius set aside (the oracle's vso_box_filter)."""
        p = self.p
        n = len(path)
        ar = self.radius
        if radius is not None:
            ar = radius
        adapt = radius is None and n >= 10
        if adapt:
            w = path[max(0, n - 20):]
            tot2, etot2 = 0.0, 0.0
            for c, k in ((0, 1.0), (1, 1.0), (2, 1000.0)):
                _, _, v, ev = mean_var(w[:, c])
                tot2 += k * v; etot2 += k * ev
            etot2 += 4 * U * tot2
            total = math.sqrt(tot2)
            etotal = (etot2 / (2 * total) + U * total) if total > 0 else math.sqrt(etot2)
            q, eq = 2 * total, 2 * etotal
            r.adaptive_q = q
            lo, hi = q - eq, q + eq
            # (int)max(5, min(25, q)): changes value at the integers 6..25
            if hi >= 6 and lo <= 25 and math.floor(min(hi, 25.0)) != math.floor(max(lo, 5.0)):
                r.box_radius_decided = False
            ar = int(max(5.0, min(25.0, q)))
        rad = max(10, min(ar, 50)) if p.drone else max(2, min(ar, 8))
        if p.drone and adapt and not r.box_radius_decided:
            # the drone clamp [10, 50] hides boundaries below 10
            lo_r = int(max(5.0, min(25.0, q - eq))); hi_r = int(max(5.0, min(25.0, q + eq)))
            r.box_radius_decided = max(10, lo_r) == max(10, hi_r)
        if not p.drone and adapt and not r.box_radius_decided:
            lo_r = int(max(5.0, min(25.0, q - eq))); hi_r = int(max(5.0, min(25.0, q + eq)))
            r.box_radius_decided = min(8, lo_r) == min(8, hi_r)
        r.box_radius = rad
        if n <= rad:
            return path[idx].copy(), np.zeros(3)
        w = path[max(0, idx - rad):min(n - 1, idx + rad) + 1]
        sm = w.sum(axis=0) / len(w)
        return sm, np.array([mean_err(w[:, c]) for c in range(3)])

    def gaussian(self, path, idx):
        k, erel = gaussian_taps(self.p.gaussian_sigma)
        ks, c, n = len(k), len(k) // 2, len(path)
        src = []
        for j in range(ks):
            q = idx + j                         # index into the padded sequence
            if q < c:
                s = c - q                       # mirrored head: padded[i] = path[c - i]
            elif q < c + n:
                s = q - c
            else:
                s = n - 1 - (q - c - n)         # mirrored tail: padded[c + n + i] = path[n - 1 - i]
            # a stream no longer than the half-width indexes past its ends in the reference: path[c - i] with c - i >= n reads
            # beyond a std::vector, which is undefined there, so the reference gives no behaviour to model.  The nearest valid
            # sample is this project's definition, adopted here and NOT independently derived; the tests hold
            # these short streams apart (test_gaussian_short_streams_follow_the_projects_definition)
            src.append(min(max(s, 0), n - 1))
        w = path[src]
        sm = (w * k[:, None]).sum(axis=0)
        err = (erel + (ks + 1) * U) * np.max(np.abs(w), axis=0)
        return sm, err

    def kalman(self, path, idx):
        """cv::KalmanFilter(2, 1): A = [1 1; 0 1], H = [1 0], Q = 0.01 I, R = 0.1, x0 = (path[0], 0), P0 = 0; the filtered
        position after correcting with sample idx.  Float64, with the constants as float32 values.  The filter only
        looks back, so its outputs are kept and extended as the path grows."""
        while len(self._kal_out) <= idx:
            i = len(self._kal_out)
            if i == 0:
                self._kal_f = [Kalman64(self.path[0][c]) for c in range(3)]
                self._kal_out.append(list(self.path[0]))
            else:
                self._kal_out.append([self._kal_f[c].step(self.path[i][c]) for c in range(3)])
        out = np.array(self._kal_out[idx])
        return out, KALMAN_TOL * np.max(np.abs(path[:idx + 1]), axis=0)

    def intent(self, raw, idx, n):
        """-> (intent, decided)"""
        mag = math.hypot(raw[0], raw[1])
        emag = 4 * U * mag
        ang = abs(raw[2]) * 180.0 / math.pi * 30.0
        eang = 6 * U * ang
        if n < 15:
            return 0, True
        lo = max(0, idx - 15)
        hi = min(idx, n)
        if hi <= lo:
            return 0, True
        t = np.asarray(self.tr[lo:hi], np.float64)
        mags = np.hypot(t[:, 0], t[:, 1])
        dirs = np.arctan2(t[:, 1], t[:, 0])
        _, _, dv, edv = mean_var(dirs, 2 * U * math.pi)
        if len(mags) < 2:
            mc, emc, zero = 0.0, 0.0, True
        else:
            se = 3 * U * float(mags.max())
            m, em, v, ev = mean_var(mags, se)
            zero = None if (m != 0.0 and abs(m) <= em) else (m == 0.0)
            if zero is not False:
                mc, emc = 0.0, 0.0
            else:
                ratio = v / (m * m)
                er = ev / (m * m) + 2 * v * em / abs(m) ** 3 + 4 * U * ratio
                mc = 1.0 / (1.0 + ratio)
                emc = er / (1.0 + ratio) ** 2 + 3 * U * mc
        if zero is None:
            return 0, False
        h = f32(0.5)
        c1 = and3(lt(dv, h, edv), gt(mc, f32(0.7), emc), gt(mag, 5.0, emag))
        if c1 is None:
            return 0, False
        if c1:
            return 1, True
        c2 = and3(lt(mag, 3.0, emag), lt(mc, f32(0.3), emc), gt(ang, 10.0, eang))
        if c2 is None:
            return 0, False
        if c2:
            return 2, True
        c3 = and3(gt(mag, 3.0, emag), lt(mag, 15.0, emag), gt(dv, h, edv))
        if c3 is None:
            return 0, False
        return (3 if c3 else 0), True


class Kalman64:
    """cv::KalmanFilter(2, 1) on a scalar track in float64: predict with A = [1 1; 0 1], correct with H = [1 0]."""
    def __init__(self, first):
        self.x0, self.x1 = float(first), 0.0
        self.P = [0.0, 0.0, 0.0, 0.0]
        self.q, self.r = f32(0.01), f32(0.1)

    def step(self, z):
        P00, P01, P10, P11 = self.P
        # x' = A x, P' = A P A^T + Q
        x0, x1 = self.x0 + self.x1, self.x1
        a00, a01, a10, a11 = P00 + P10, P01 + P11, P10, P11
        P00, P01, P10, P11 = a00 + a01 + self.q, a01, a10 + a11, a11 + self.q
        # K = P' H^T / (H P' H^T + R); x = x' + K (z - H x'); P = P' - K H P'
        S = P00 + self.r
        K0, K1 = P00 / S, P10 / S
        y = z - x0
        self.x0, self.x1 = x0 + K0 * y, x1 + K1 * y
        self.P = [P00 - K0 * P00, P01 - K0 * P01, P10 - K1 * P00, P11 - K1 * P01]
        return self.x0


def kalman64(path):
    """Filtered positions of every sample of path (n,) or (n, k) in float64."""
    path = np.asarray(path, np.float64)
    if path.ndim == 1:
        return kalman64(path[:, None])[:, 0]
    out = np.empty_like(path)
    for c in range(path.shape[1]):
        f = Kalman64(path[0, c])
        out[0, c] = path[0, c]
        for i in range(1, len(path)):
            out[i, c] = f.step(path[i, c])
    return out


# ---- the queue: which push lets which frame go ----------------------------------------------------------------------
def schedule(model_stream, params):
    """Runs a stream [(model, kind), ...] through a fresh Model the way stabilize() does: frame 0 only enters the queue,
    every later frame appends a transform, and a push releases the oldest queued frame once the queue holds
    clamp(smoothing_radius, 5, 35) frames; a flush then releases the rest, the last of them with no transform of its own.
    -> (model, [(push index or None for the flush, Release)])"""
    m = Model(params)
    queue = [0]
    rel = []
    for i, (mod, kind) in enumerate(model_stream):
        queue.append(i + 1)
        m.push(mod, kind)
        if len(queue) >= max(5, min(m.radius, 35)):
            rel.append((i, m.release(queue.pop(0))))
    while queue:
        rel.append((None, m.release(queue.pop(0))))
    return m, rel
