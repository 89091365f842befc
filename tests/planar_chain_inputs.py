"""Inputs shared by tests/test_planar_chain_cpu.py and tests/test_gpu_planar_chain.py: tilted horizons, rotated content in black
corners and the chain clip as three-plane surfaces of any subsampling, with real chroma (synth.bgr_to_yuv_planes) and, in the 10- and
12-bit forms, live low bits (synth.yuv_to_depth).  The analysis plane of Y - the bytes of bgr_to_nv12's luma - is the same for every
format of a scene, so one oracle run per scene serves all formats.  Everything is built once per session: callers must not write into
what they get.

The geometries are those at which the kernels can go wrong, not a workload's: 130 x 96 (4:2:2 chroma planes of 65 columns, one tile
row), 322 x 200 (three tile columns of luma, a ragged last one in either plane size) and 704 x 400 (where 640 x 360 is a zoom-in of
some crops and a downscale of others)."""
import functools

import numpy as np

import planar_chain_ref as ref
import roll_scene
from vsamd import synth

SIZES = [(130, 96), (322, 200), (704, 400)]
FORMATS = ["I422", "I444", "I210", "I212", "I410", "I412"]

# ---- roll: the smoothed angle follows the detected one at once (alpha 1, no step limit), so a tilt is an angle -----------------------
# Small pictures are analysed at a larger scale and with a lower Hough threshold, or they hold no line.
ROLL_PARAMS = {(130, 96): dict(scale_factor=1.0, hough_threshold=30), (322, 200): dict(scale_factor=0.5, hough_threshold=40),
               (704, 400): dict(scale_factor=0.25, hough_threshold=40)}
FOLLOW = dict(angle_smoothing_alpha=1.0, max_angle_change_deg=0.0)
# tilt -> (target angle in degrees, slope of the horizon in 1/1024); HoughLines resolves whole degrees, the mean of the lines lands near
TILTS = {"1deg": (1.0, 18), "3deg": (3.0, 54), "8deg": (8.0, 144)}
# per (size, tilt): the seeds of roll_scene.horizon_frame whose scenes the oracle sees within 0.75 degrees of the target and not at 0
# (found by a search over the seeds from 0 up; tests/test_planar_chain_cpu.py asserts it)
ROLL_SEEDS = {
    ((130, 96), "1deg"): [0, 1, 2, 3, 7, 8, 9, 11, 12, 13, 14],
    ((130, 96), "3deg"): [1, 2, 5, 6, 8, 9, 10, 11, 13, 14, 15],
    ((130, 96), "8deg"): [1, 3, 6, 7, 8, 10, 13, 14, 16, 17, 19],
    ((322, 200), "1deg"): [0, 1, 2, 3, 4, 6, 7, 9, 10, 11, 12],
    ((322, 200), "3deg"): [0, 1, 2, 3, 4, 7, 9, 10, 11, 12, 13],
    ((322, 200), "8deg"): [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 13],
    ((704, 400), "1deg"): [0, 1, 3, 4, 6, 7, 8, 9, 12, 13, 15],
    ((704, 400), "3deg"): [0, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13],
    ((704, 400), "8deg"): [0, 1, 3, 4, 6, 7, 10, 11, 12, 13, 17],
}
N_ROLL = 11          # a batch of eight and three more that vs_roll_sync closes


def roll_params(oracle_or_gpu, size, **more):
    return oracle_or_gpu.roll_params(**dict(ROLL_PARAMS[size], **more))


def to_format(frame, fmt, seed):
    """(Y, U, V) of a BGR frame in format `fmt`; black pixels (0, 0, 0) become luma sample 0, as a warp's constant border leaves them."""
    sx, sy = ref.shifts(fmt)
    planes = synth.bgr_to_yuv_planes(frame, sx, sy)
    if ref.bits(fmt) != 8:
        planes = synth.yuv_to_depth(planes, ref.bits(fmt), seed)
    planes = [np.ascontiguousarray(p) for p in planes]
    planes[0][(frame == 0).all(axis=2)] = 0
    return planes


@functools.lru_cache(maxsize=None)
def roll_frames(size, tilt):
    w, h = size
    _, slope = TILTS[tilt]
    return [roll_scene.horizon_frame(w, h, slope, seed=s) for s in ROLL_SEEDS[(size, tilt)]]


@functools.lru_cache(maxsize=None)
def roll_planes(fmt, size, tilt):
    """N_ROLL surfaces (Y, U, V) of one tilt."""
    return [to_format(f, fmt, 4000 + 16 * i + ref.bits(fmt)) for i, f in enumerate(roll_frames(size, tilt))]


_roll_orc = {}


def roll_oracle(oracle, size, tilt):
    """The oracle's roll object over the analysis surfaces of (size, tilt): its state after each of the N_ROLL surfaces."""
    key = (size, tilt)
    if key not in _roll_orc:
        w, h = size
        ro = oracle.roll_correction(roll_params(oracle, size, **FOLLOW))
        states = []
        for p in roll_planes("I444", size, tilt):
            ro.correct_nv12(ref.analysis_nv12(p, "I444"), w, h)
            states.append(ro.state())
        ro.close()
        _roll_orc[key] = states
    return _roll_orc[key]


# ---- zoom: rotated content in black corners ----------------------------------------------------------------------------------------------
ZOOM_DEGS = [4.0, -2.5, 7.5]
ZOOM_OUT = [(640, 360), (0, 0), (416, 232)]          # the default, the surface's own size, an explicit one


_zoom_frames = {}


def zoom_frames(oracle, size):
    if size not in _zoom_frames:
        from test_azc import rotated_frame
        _zoom_frames[size] = [rotated_frame(oracle, size[0], size[1], deg, seed=10 + i) for i, deg in enumerate(ZOOM_DEGS)]
    return _zoom_frames[size]


_zoom_planes = {}


def zoom_planes(oracle, fmt, size):
    if (fmt, size) not in _zoom_planes:
        _zoom_planes[(fmt, size)] = [to_format(f, fmt, 5000 + 16 * i + ref.bits(fmt)) for i, f in enumerate(zoom_frames(oracle, size))]
    return _zoom_planes[(fmt, size)]


_zoom_info = {}


def zoom_info(oracle, size):
    """info8 of the oracle's NV12 auto zoom/crop per surface of zoom_planes (the same for every format)."""
    if size not in _zoom_info:
        _zoom_info[size] = [oracle.auto_zoom_crop_nv12(ref.analysis_nv12(p, "I444"), size[0], size[1])[1] for p in zoom_planes(oracle, "I444", size)]
    return _zoom_info[size]


# ---- chain: the configs[2] clip at 704 x 400 with a tilted horizon in its lower two thirds ------------------------------------------------
CHAIN_SIZE = (704, 400)
CHAIN_N = 8


@functools.lru_cache(maxsize=None)
def chain_frames():
    w, h = CHAIN_SIZE
    base = synth.make_clip(synth.SEED_CONFIG3, w, h, 7)
    tilt = roll_scene.horizon_frame(w, h, 45, seed=7)
    out = []
    for f in base:
        f = np.array(f)
        f[h // 3:] = tilt[h // 3:]
        out.append(f)
    return [out[i % 7] for i in range(CHAIN_N)]


@functools.lru_cache(maxsize=None)
def chain_planes(fmt):
    return [to_format(f, fmt, 6000 + i % 7) for i, f in enumerate(chain_frames())]
