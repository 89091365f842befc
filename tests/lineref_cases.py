"""Inputs shared by tests/test_lineref_oracle.py (CPU: the statements of lineref.py against the oracle) and tests/test_gpu_lineref.py
(GPU: the kernels against the statements).  Everything is built once per session and handed out as is: callers must not write into it."""
import functools
import math

import numpy as np

import lineref
import roll_scene
from vsamd import synth

THETA = np.float32(math.pi / 180.0)

# one word, a ragged last word, two hysteresis bands (63 and 62 rows + 1), 17 words (two workgroups side by side), tiny pictures
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (8, 8), (63, 64), (62, 65), (135, 240), (70, 1030)]
TINY = [s for s in SHAPES if s[0] * s[1] < 64]
THRESHOLDS = [(50, 150), (10, 30), (150, 50), (0, 0), (10.9, 30.2)]
KINDS = ["noisy", "binary"]


@functools.lru_cache(maxsize=None)
def gray(kind, shape):
    h, w = shape
    if kind == "noisy":
        return roll_scene.noisy_gray(w, h, 3 + h)
    assert kind == "binary"          # the largest gradients an 8-bit picture has
    return (np.random.default_rng(w * 1000 + h).integers(0, 2, shape) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def serpentine(strong=True):
    """The picture of test_roll.py's hysteresis tests: one strong spot at the head of a weak serpentine bar, 400 x 300."""
    h, w = 400, 300
    g = np.full((h, w), 100, np.uint8)
    xs = list(range(10, w - 20, 24))
    for i, x in enumerate(xs):
        g[20:h - 20, x:x + 6] = 112
        if i + 1 < len(xs):
            y = h - 26 if i % 2 == 0 else 20
            g[y:y + 6, x:x + 30] = 112
    g[20:26, 10:16] = 230 if strong else 112
    return g


SERPENTINE_THRESHOLDS = (20, 100)
SERPENTINE_FAR_END = (200, range(273, 276))          # row, columns: the last bar's left edge


@functools.lru_cache(maxsize=None)
def rendered_grays():
    return [lineref.bgr2gray(f) for f in synth.make_clip(synth.SEED_CONFIG1, 320, 240, 3)]


# ---- Hough -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_map(shape):
    return lineref.canny(gray("noisy", shape), 10, 30)


# (rho, theta) and, per shape, a threshold that leaves a list that is neither empty nor near the library's cap of 8192
RESOLUTIONS = [(1.0, THETA), (2.0, THETA), (1.0, np.float32(math.pi / 90)), (0.5, np.float32(math.pi / 360))]
HOUGH_SHAPES = {(63, 64): (16, 40, 16, 12), (62, 65): (22, 40, 22, 12), (135, 240): (60, 60, 60, 40), (70, 1030): (60, 60, 60, 60)}


def hough_cases():
    """(edge map shape, rho, theta, threshold): the four resolutions on the larger shapes (widths that are and are not multiples of
    8), threshold 0 on the tiny ones."""
    out = [(s, rho, th, HOUGH_SHAPES[s][i]) for s in HOUGH_SHAPES for i, (rho, th) in enumerate(RESOLUTIONS)]
    return out + [(s, 1.0, THETA, 0) for s in TINY]


def tiny_edges(shape, full):
    """Tiny edge maps: every pixel set, or Canny(0, 0) of the random {0, 255} picture (empty for 1 x 1)."""
    return np.full(shape, 255, np.uint8) if full else lineref.canny(gray("binary", shape), 0, 0)


# lines at threshold 0 on the tiny maps, as the statement counts them (full map, Canny map)
TINY_COUNTS = {(1, 1): (1, 0), (1, 9): (45, 9), (9, 1): (40, 21), (2, 2): (6, 3), (3, 3): (21, 12)}


@functools.lru_cache(maxsize=None)
def fine_rho_edges():
    """520 x 260, a few drawn lines: at rho = 0.1 the accumulator rows have 15610 cells and do not fit LDS."""
    h, w = 260, 520
    e = np.zeros((h, w), np.uint8)
    e[40, 30:500] = 255
    e[200, 100:480] = 255
    e[20:250, 77] = 255
    e[10:255, 400] = 255
    i = np.arange(220)
    e[10 + i, 60 + 2 * i] = 255           # slope 1/2
    e[250 - i, 120 + i] = 255             # 45 degrees upward
    e[5 + i, 300 + i // 3] = 255          # steep
    return e


FINE_RHO = (0.1, THETA, 60)
FINE_RHO_NUMRHO = 15610


# ---- the peak cap ------------------------------------------------------------------------------------------------------
OVER_CAP_THRESHOLD = 15
OVER_CAP_CANNY = (10, 30)


@functools.lru_cache(maxsize=None)
def over_cap_gray():
    """330 x 200 noise whose edge map has well over 8192 Hough peaks at threshold 15, plus three long steep bright lines whose peaks
    are the strongest and lie at theta >= 150 degrees: late in any scan of the accumulator by angle."""
    h, w = 200, 330
    g = roll_scene.noisy_gray(w, h, 5).copy()
    y = np.arange(4, h - 4)
    for x0, deg in ((40, 160), (150, 165), (235, 170)):            # the pixels nearest to x cos(theta) + y sin(theta) = x0 cos(theta)
        x = np.rint(x0 - y * math.tan(math.radians(deg))).astype(int)
        for d in range(3):
            g[y, x + d] = 255
    return g


def over_cap_params(**kw):
    return dict(scale_factor=1.0, canny_threshold_low=OVER_CAP_CANNY[0], canny_threshold_high=OVER_CAP_CANNY[1],
                hough_threshold=OVER_CAP_THRESHOLD, angle_filter_min=-100.0, angle_filter_max=100.0, **kw)


# ---- roll sequences ----------------------------------------------------------------------------------------------------
ROLL_SIZE = (640, 360)


@functools.lru_cache(maxsize=None)
def roll_frames(n=11):
    """BGR frames: tilted horizons with texture, a flat frame (decay: no lines) at index 3 and at index 6 a bare 45 degree horizon,
    whose only lines fall outside the default angle filter."""
    w, h = ROLL_SIZE
    frames = [roll_scene.horizon_frame(w, h, 40 + 3 * i, seed=i, offset=i - 3) for i in range(n)]
    frames[3] = np.full((h, w, 3), 77, np.uint8)
    frames[6] = roll_scene.horizon_frame(w, h, 1024, texture=False)
    return frames


@functools.lru_cache(maxsize=None)
def roll_surfaces(n=11):
    return [synth.bgr_to_nv12(f) for f in roll_frames(n)]


def roll_threshold(scale):
    return {0.25: 40, 0.5: 60, 1.0: 100}[scale]


OTHER_PARAMS = dict(angle_smoothing_alpha=0.35, angle_decay=0.9, angle_filter_min=-0.5, angle_filter_max=3.5, max_angle_change_deg=0.0)


@functools.lru_cache(maxsize=None)
def serpentine_states(n):
    """The states of n serpentine frames at scale 1 with every line counted (the roll tests of test_roll.py use these settings)."""
    p = lineref.roll_params(**SERPENTINE_ROLL)
    return lineref.roll_run([serpentine()] * n, p)


SERPENTINE_ROLL = dict(scale_factor=1.0, canny_threshold_low=20, canny_threshold_high=100, hough_threshold=60,
                       angle_filter_min=-100.0, angle_filter_max=100.0)


# ---- content mask ------------------------------------------------------------------------------------------------------
MASK_SHAPES = [(270, 480), (101, 67), (64, 64), (5, 7), (1080, 1920), (33, 70), (40, 1030), (9, 1025), (120, 129), (57, 64),
               (1, 1), (1, 7), (7, 1), (3, 3), (4, 5), (5, 5)]


@functools.lru_cache(maxsize=None)
def mask_picture(shape, cn):
    """Mostly dark values around the threshold (a busy mask) plus a bright patch, as test_azc.py::test_content_mask_bit_exact."""
    h, w = shape
    rng = np.random.default_rng(h * 7 + w * 3 + cn)
    img = rng.integers(0, 4, (h, w, 3), dtype=np.uint8)
    img[rng.random((h, w)) < 0.6] = 0
    img[h // 4:h // 2, w // 4:w // 2] = 180
    return np.ascontiguousarray(img[..., 1]) if cn == 1 else img


# ---- the roll stage at a fine rho (accumulator rows past LDS) and on 16-bit surfaces -----------------------------------------------
FINE_RHO_SIZE = (520, 260)
FINE_RHO_ROLL = dict(scale_factor=1.0, hough_rho=0.1, hough_threshold=30, angle_filter_min=-100.0, angle_filter_max=100.0)


@functools.lru_cache(maxsize=None)
def fine_rho_surfaces(n=5):
    """NV12 surfaces, 520 x 260: level horizons (a tilted one spreads over the 0.1-pixel bins) at different rows, with texture."""
    w, h = FINE_RHO_SIZE
    return [synth.bgr_to_nv12(roll_scene.horizon_frame(w, h, 0, seed=20 + i, offset=7 * i - 11)) for i in range(n)]


def gray_surface(g):
    """The NV12 surface of a gray picture (even sides): the picture as luma, a flat chroma plane."""
    h, w = g.shape
    return np.concatenate([g, np.full((h // 2, w), 128, np.uint8)])
