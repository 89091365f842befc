"""Inputs shared by tests/test_p010_geom_cpu.py and tests/test_gpu_p010_chain.py: the NV12 scenes of the 8-bit roll, zoom and chain
tests turned into P010 surfaces, sample = byte << 8 | low with a seeded pseudo-random `low` over all eight bits (nothing assumes
that the low six bits are zero), and the cases of the 16-bit plane warp.  The CPU tests assert that these inputs hold rounding ties
(half-even and half-up differ on every blended plane) and that the zoom scenes take both branches; the GPU tests compare the
device with tests/ref16_geom.py on them.  Everything is built once per session: callers must not write into what they get."""
import functools
import math

import numpy as np

import roll_scene
from vsamd import synth

# roll: the cases of test_roll.py::test_roll_correct_nv12_async_matches_oracle without 1280 x 720 - (size, slope, padded)
ROLL_CASES = [((640, 360), 51, False), ((322, 242), 20, True)]
# zoom: the wide-load mask kernel (rows of 8-sample groups, 16-byte aligned: 800 and - unlike 8 bits, whose groups are 16 wide - 808) and
# the general one (804: a width that is no multiple of 8)
ZOOM_SIZES = [(800, 450), (808, 454), (804, 452)]
ZOOM_DEGS = [4.0, -2.5, 1.0, 7.5, -6.0, 0.5, 3.0, -1.0, 2.0, -4.5]
CHAIN_SIZE = (704, 400)


def to_p010(nv12, seed):
    """(byte << 8) | low, low = seeded random 0 .. 255."""
    nv12 = np.asarray(nv12, np.uint8)
    low = np.random.default_rng(seed).integers(0, 256, nv12.shape, np.uint16)
    return (nv12.astype(np.uint16) << 8) | low


def roll_hough_threshold(w):
    return 100 if w >= 640 else 40


@functools.lru_cache(maxsize=None)
def roll_surfaces(size, slope):
    """Eleven P010 surfaces (h * 3 / 2, w): ten tilted horizons and, in the middle, a flat frame (the decay branch)."""
    w, h = size
    frames = [roll_scene.horizon_frame(w, h, slope + i, seed=i, offset=i - 3) for i in range(10)]
    frames.insert(5, np.full((h, w, 3), 77, np.uint8))
    return [to_p010(synth.bgr_to_nv12(f), 1000 + i) for i, f in enumerate(frames)]


_zoom_cache = {}


def zoom_surfaces(oracle, size):
    """The twelve surfaces of test_azc.py::test_auto_zoom_crop_nv12_async_matches_oracle as P010: rotated content in black corners,
    an all-black one, an all-content one.  Black is sample 0 (high and low byte)."""
    if size not in _zoom_cache:
        from test_azc import rotated_frame
        w, h = size
        frames = [rotated_frame(oracle, w, h, deg, seed=i) for i, deg in enumerate(ZOOM_DEGS)]
        frames.insert(3, np.zeros((h, w, 3), np.uint8))
        frames.insert(8, np.full((h, w, 3), 200, np.uint8))
        out = []
        for i, f in enumerate(frames):
            s = to_p010(synth.bgr_to_nv12(f), 2000 + i)
            s[:h][(f == 0).all(axis=2)] = 0          # (BT.601 black is 16; the warp's black border in a P010 stream is sample 0)
            out.append(s)
        _zoom_cache[size] = out
    return _zoom_cache[size]


@functools.lru_cache(maxsize=None)
def chain_surfaces(n):
    w, h = CHAIN_SIZE
    return [to_p010(s, 3000 + i % 7) for i, s in enumerate(roll_scene.chain_surfaces(w, h, n))]


# ---- the 16-bit plane warp: 130 x 66 into 200 x 90 and into 64 x 40 -----------------------------------------------------------------
WARP16_SRC = (130, 66)
WARP16_DSTS = [(200, 90), (64, 40)]


def _rot(deg, sx, sy, tx, ty):
    a = math.radians(deg)
    return [sx * math.cos(a), sx * math.sin(a), tx, -sy * math.sin(a), sy * math.cos(a), ty]


def warp16_matrices(dsize):
    """Forward matrices (double) into a dw x dh destination: the scale that fills it, a small rotation with a fractional shift, and a
    rotation large enough that whole 128 x 16 tiles of the destination fall outside the source."""
    (sw, sh), (dw, dh) = WARP16_SRC, dsize
    return {"fill": [dw / sw, 0.0, 0.0, 0.0, dh / sh, 0.0],
            "small_rot": _rot(2.5, dw / sw, dh / sh, 3.3, -2.7),
            "tiles_outside": _rot(38.0, 1.7, 1.7, dw * 0.55, -dh * 0.3)}      # (200 x 90: the source lands right of x = 130)


def warp16_plane(cn, seed=7):
    sw, sh = WARP16_SRC
    shape = (sh, sw) if cn == 1 else (sh, sw, cn)
    return np.random.default_rng(seed + cn).integers(0, 65536, shape, np.uint16)
