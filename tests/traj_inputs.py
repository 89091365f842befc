"""Designed (model, kind) streams for the trajectory stage.  Each is built to reach named branches; the tests assert the
coverage from the float64 model (traj_ref.py), and the model is confirmed by the oracle and by the device.

A stream is a list of (model, kind): model = the refined 2x3 similarity as six doubles, kind = None | traj_ref.FAIL |
traj_ref.SKIP.  300 to 600 pushes each, so the 256-entry history ring wraps.
"""
import math

import numpy as np

from traj_ref import FAIL, SKIP


def mk(dx, dy, da, scale=1.0):
    c, s = math.cos(da) * scale, math.sin(da) * scale
    return [c, -s, float(dx), s, c, float(dy)]


def _stream(rows):
    return [(mk(*r), None) for r in rows]


def steady_pan(seed=11, n=320):
    """8 px per frame to the right with a little noise: direction variance ~0, consistent magnitude above 5 -> intent 1."""
    g = np.random.default_rng(seed)
    return _stream([(8.0 + g.uniform(-0.3, 0.3), 1.0 + g.uniform(-0.2, 0.2), g.uniform(-2e-4, 2e-4)) for _ in range(n)])


def still_rotation_jitter(seed=12, n=320):
    """Translations of a hundredth of a pixel with a 1.5 px kick every eighth frame (magnitude consistency ~0.13 < 0.3)
    and +-0.01..0.02 rad per frame (17..34 deg/s at 30 fps > 10) -> intent 2 on the quiet frames."""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        a = g.uniform(0, 2 * math.pi)
        m = 1.5 if i % 8 == 3 else g.uniform(0.005, 0.02)
        rows.append((m * math.cos(a), m * math.sin(a), g.choice([-1, 1]) * g.uniform(0.01, 0.02)))
    return _stream(rows)


def reversals(seed=13, n=360):
    """Blocks of 2..5 frames at 3.5..14 px that flip between right and left (direction variance ~2.4 > 0.5) -> intent 3;
    every fourth block moves 0.5..2.5 px or 16..20 px, which is neither follow-action nor pan -> intent 0."""
    g = np.random.default_rng(seed)
    rows, sign, k = [], 1.0, 0
    while len(rows) < n:
        k += 1
        sign = -sign
        lo, hi = (3.5, 14.0) if k % 4 else ((0.5, 2.5) if k % 8 else (16.0, 20.0))
        for _ in range(int(g.integers(2, 6))):
            rows.append((sign * g.uniform(lo, hi), g.uniform(-0.4, 0.4), g.uniform(-1e-3, 1e-3)))
    return _stream(rows[:n])


def drone_dead_zone(seed=14, n=330):
    """Drone mode (dead zone 2.0, freeze 10, decay 0.9, shake 1.5 px).  A cycle of 33 pushes:
      6 x 6 px           pass-through band (deviation from the median > 3 px once the median lags), accumulator at 6
      1 x 1 px           enters the dead zone and leaves it on the same push: accumulator 5.4 > 2.4         (exit: accum)
      12 x 0.2..0.9 px   enters (the exit reset the accumulator), frozen 9 pushes, the counter runs out      (exit: duration)
                          then re-enters and stays frozen
      1 x 3.6 px         > 1.5 * 2.0 while frozen                                                            (exit: motion)
      7 x 2.2..2.9 px    outside the dead zone; deviation from the median inside the two shake bands
      6 x 0.2 px steps around 2.5 px  first band (< 1.5 px)
    """
    g = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        rows += [(6.0 + g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2), g.uniform(-1e-3, 1e-3)) for _ in range(6)]
        rows += [(1.0, 0.1, 0.0)]
        rows += [(g.uniform(0.2, 0.9), g.uniform(-0.3, 0.3), g.uniform(-1e-3, 1e-3)) for _ in range(12)]
        rows += [(3.6, 0.3, 1e-3)]
        rows += [(g.uniform(2.2, 2.9), g.uniform(-0.3, 0.3) + (2.0 if j % 3 == 1 else 0.0), g.uniform(-1e-3, 1e-3)) for j in range(7)]
        rows += [(2.5 + g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2), g.uniform(-1e-3, 1e-3)) for _ in range(6)]
    return _stream(rows[:n])


def drone_horizon(seed=15, n=300):
    """Drone mode with horizon_lock: rotations of up to 0.03 rad through the exponential low-pass (alpha 0.2), the
    translations large enough (3..5 px) to stay out of the dead zone most of the time, with quiet stretches that freeze."""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        quiet = (i // 25) % 3 == 2
        m = g.uniform(0.1, 0.8) if quiet else g.uniform(3.0, 5.0)
        rows.append((m, g.uniform(-0.5, 0.5), g.uniform(-0.03, 0.03) * (0.1 if quiet else 1.0)))
    return _stream(rows)


def drone_short_history(seed=16, n=300):
    """Drone mode whose first pushes alternate with skipped ones (no keypoints), so the translation history stays below
    5 entries for 8 pushes, holds 5..9 for the next 10 and 10 from then on: no median, odd and even medians."""
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        r = (2.6 + g.uniform(-1.5, 1.5), g.uniform(-1.5, 1.5), g.uniform(-2e-3, 2e-3))
        out.append((mk(*r), SKIP if (i < 20 and i % 2 == 1) else None))
    return out


def radius_bands(seed=17, n=420):
    """Box smoother: 140 pushes of +-0.05 px jitter (path spread * 2 < 5: radius pinned at 5), 140 of a 9 px pan (> 25:
    pinned at 25), 140 of +-2.2 px jitter, whose 20-sample path spread * 2 wanders between 5 and 25
    (radii 5 to 8 after the clamp of the normal mode)."""
    g = np.random.default_rng(seed)
    rows = [(g.uniform(-0.05, 0.05), g.uniform(-0.05, 0.05), g.uniform(-1e-5, 1e-5)) for _ in range(140)]
    rows += [(9.0 + g.uniform(-0.5, 0.5), g.uniform(-0.5, 0.5), g.uniform(-1e-4, 1e-4)) for _ in range(140)]
    rows += [(g.uniform(-2.2, 2.2), g.uniform(-2.2, 2.2), g.uniform(-3e-4, 3e-4)) for _ in range(140)]
    return _stream(rows[:n])


def adaptive_sweep(seed=18, n=330, min_radius=5, max_radius=50):
    """Adaptive smoothing: the magnitude of push i is 50 (1 - (k + 1/2) / span) for k walking over 0 .. span - 1 and back, so
    that motionScale * span sits half way between two integers and newRadius takes every value of [min, max); then
    a still stretch (radius max) and one far above 50 px (radius min).  It opens with the latter, so that the queue first
    releases at 5 frames and then grows with the radius (pushes that release nothing) up to its cap of 35."""
    g = np.random.default_rng(seed)
    span = max_radius - min_radius
    ks = list(range(span)) + list(range(span - 1, -1, -1))
    rows = [(70.0, 10.0, 0.0)] * 12         # radius min from the third push on: the queue releases at 5 frames
    i = 0
    while len(rows) < n:
        for k in ks:
            m = 50.0 * (1.0 - (k + 0.5) / span)
            a = g.uniform(0, 2 * math.pi)
            rows.append((m * math.cos(a), m * math.sin(a), g.uniform(-1e-3, 1e-3)))
        rows += [(0.0, 0.0, 0.0)] * 40 + [(70.0, 10.0, 0.0)] * 12
        i += 1
    return _stream(rows[:n])


def with_failures(seed=19, n=340):
    """A 6 px pan with jitter in which one push in seven failed to estimate and one in eleven had nothing to track."""
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        r = (6.0 + g.uniform(-2, 2), g.uniform(-2, 2), g.uniform(-5e-3, 5e-3))
        kind = FAIL if i % 7 == 5 else (SKIP if i % 11 == 9 else None)
        out.append((mk(*r), kind))
    return out


DRONE = dict(drone=True, hf_shake_px=1.5, hf_dead_zone=2.0, hf_freeze_duration=10, hf_decay=0.9, hf_rot_lp_alpha=0.2)

# name -> (stream builder, model parameters without the smoother, runs in batch mode)
SEQUENCES = {
    "steady_pan": (steady_pan, dict(smoothing_radius=6), True),
    "still_rotation_jitter": (still_rotation_jitter, dict(smoothing_radius=6), True),
    "reversals": (reversals, dict(smoothing_radius=7), True),
    "drone_dead_zone": (drone_dead_zone, dict(smoothing_radius=12, **DRONE), True),
    "drone_horizon": (drone_horizon, dict(smoothing_radius=30, horizon_lock=True, **DRONE), True),
    "drone_short_history": (drone_short_history, dict(smoothing_radius=9, **DRONE), True),
    "radius_bands": (radius_bands, dict(smoothing_radius=5), True),
    "adaptive_sweep": (adaptive_sweep, dict(smoothing_radius=20, adaptive=True, min_radius=5, max_radius=50), False),
    "with_failures": (with_failures, dict(smoothing_radius=8), True),
}

# sigmas whose kernels have 3, 13 and 63 taps
SMOOTHERS = [("box", {}), ("gaussian", dict(gaussian_sigma=0.5)), ("gaussian", dict(gaussian_sigma=2.0)),
             ("gaussian", dict(gaussian_sigma=10.4)), ("kalman", {})]

_cache = {}


def stream(name):
    if name not in _cache:
        _cache[name] = SEQUENCES[name][0]()
    return _cache[name]


# ---- a rendered clip that reaches all four intents ---------------------------------------------------------------------
def intent_clip_poses(n=72, width=320, height=240, seed=5):
    """Camera poses (ox_q8, oy_q8, sin_q16) for vsamd.synth.render_frame:
      frames 0..13   2 px pan with 1.5 px jitter: intents 0 and 3 (what the old intent clip gave throughout);
      frames 14..33  the picture moves 8.6 px per frame towards +x (camera towards -x), where the direction atan2 stays
                     near 0 and does not flip between +pi and -pi: intent 1;
      frames 34..    the camera rolls by +-0.004 rad about the picture's corner (0, 0) - the origin of the measured model, so
                     the rotation brings no translation - with a 12 px step every eighth frame, which makes the magnitudes
                     inconsistent: 14 deg/s, under 3 px: intent 2."""
    g = np.random.default_rng(seed)
    px, py = 256 * 256, 256 * 256
    cx, cy = width // 2, height // 2
    poses = []
    for k in range(n):
        if k < 14:
            if k:
                px += 512
            poses.append((px + int(g.normal(0, 384)), py + int(g.normal(0, 384)), int(g.normal(0, 130))))
        elif k < 34:
            px -= 2200
            poses.append((px + int(g.normal(0, 60)), py + int(g.normal(0, 60)), 0))
        else:
            if k % 8 == 5:
                px += 3072
            s16 = 262 if k % 2 else -262                       # sin(0.004) * 65536
            c16 = 65536 - ((s16 * s16) >> 17)
            # world = o + c + R (x - c) = R x + (o + c - R c): o = base + R c - c keeps the corner fixed
            ox = px + (((c16 * cx - s16 * cy) >> 8) - cx * 256)
            oy = py + (((s16 * cx + c16 * cy) >> 8) - cy * 256)
            poses.append((ox, oy, s16))
    return poses


def intent_clip(n=72, width=320, height=240):
    from vsamd import synth
    world = synth.make_world(synth.SEED_CONFIG1 + 1, width, height)
    return [synth.render_frame(world, width, height, p) for p in intent_clip_poses(n, width, height)]
