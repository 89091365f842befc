"""Inputs and the reference shared by tests/test_rgb_chain_cpu.py and tests/test_gpu_rgb_chain.py: roll correction and auto zoom/crop
on interleaved colour frames (BGR8, RGB8, BGRA8, RGBA8).

A frame of format fmt is pack(bgr, alpha, fmt): B, G, R at the format's positions and, for the four-channel formats, a fourth channel
of seeded random bytes over all 256 values, independent of the colour.  The reference needs no arithmetic of its own:
    analysis   angle, state and info8 come from the ORACLE's BGR operators on the frame's BGR permutation (unpack) - that is the
               definition: the fourth channel never enters;
    pixels     every channel, the fourth included, through ref16_geom.warp(frame, M, dsize, border, HALF_UP) - cv::warpAffine's 8-bit
               arithmetic on (h, w, cn) arrays - with ref16_geom.roll_matrices (BORDER_REPLICATE) and azc_size_inputs.reference (the
               CV_32F scale matrix, BORDER_CONSTANT 0 on the crop).
tests/test_rgb_chain_cpu.py pins this construction to the oracle (BGR8: the oracle's own results; the others: the BGR8 reference
permuted, and the oracle's one-channel warp of the fourth plane) and asserts that the scenes take every branch.
Everything is built once per session: callers must not write into what they get."""
import functools

import numpy as np

import azc_size_inputs
import ref16_geom as geom
import roll_scene
from p010_chain_inputs import CHAIN_SIZE, ROLL_CASES, ZOOM_DEGS, roll_hough_threshold      # noqa: F401  (the geometry of the 16-bit chain tests)
from vsamd import capi, synth

BGR8, RGB8, BGRA8, RGBA8 = capi.FMT_BGR8, capi.FMT_RGB8, capi.FMT_BGRA8, capi.FMT_RGBA8
FORMATS = [BGR8, RGB8, BGRA8, RGBA8]
FMT_NAMES = {BGR8: "BGR8", RGB8: "RGB8", BGRA8: "BGRA8", RGBA8: "RGBA8"}
CN = {BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
# zoom: the two sizes of the 8-bit stage tests (804: rows that are no multiple of 16 bytes for three-byte pixels) and one below the
# reference's 640 x 360 both ways
ZOOM_SIZES = [(800, 450), (804, 452), (130, 96)]
OUT_SIZES = [(640, 360), (0, 0), (322, 182)]


def alpha_plane(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), np.uint8)


def pack(bgr, alpha, fmt):
    """The frame of format fmt with bgr's B, G, R and, where the format has a fourth channel, alpha."""
    c = bgr if fmt in (BGR8, BGRA8) else bgr[..., ::-1]
    return np.ascontiguousarray(c if CN[fmt] == 3 else np.dstack([c, alpha]))


def unpack(frame, fmt):
    """(bgr, alpha or None) of a frame of format fmt."""
    c = frame[..., :3] if fmt in (BGR8, BGRA8) else frame[..., 2::-1]
    return np.ascontiguousarray(c), (np.ascontiguousarray(frame[..., 3]) if CN[fmt] == 4 else None)


def pack_all(bgrs, fmt, seed):
    return [pack(f, alpha_plane(f.shape[0], f.shape[1], seed + i), fmt) for i, f in enumerate(bgrs)]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def roll_ref(frames, fmt, oracle_roll):
    """frames of format fmt through the roll stage -> ([result], [state after each frame]).  oracle_roll: the oracle's roll object; it
    carries the smoothed angle and is advanced by its BGR call on each frame's BGR permutation."""
    outs, states = [], []
    for f in frames:
        h, w = f.shape[:2]
        oracle_roll.correct(unpack(f, fmt)[0])
        states.append(oracle_roll.state())
        outs.append(geom.warp(f, geom.roll_matrices(w, h, states[-1][0])[0], None, geom.REPLICATE, geom.HALF_UP))
    return outs, states


def azc_ref(frame, fmt, oracle, out_size=(640, 360)):
    """One frame through the zoom stage at the object's output size (0, 0 = the frame's own) -> (result, info8)."""
    h, w = frame.shape[:2]
    _, info = oracle.auto_zoom_crop(unpack(frame, fmt)[0])
    if not info[7]:
        return frame.copy(), info
    cx, cy, cw, ch = (int(v) for v in info[2:6])
    return azc_size_inputs.reference(frame[cy:cy + ch, cx:cx + cw], azc_size_inputs.resolved(tuple(out_size), w, h)), info


# ---- scenes (BGR) ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def roll_bgr(size, slope):
    """Eleven BGR frames: ten tilted horizons and, in the middle, a flat frame (the decay branch) - two batches, 8 + 3."""
    w, h = size
    frames = [roll_scene.horizon_frame(w, h, slope + i, seed=i, offset=i - 3) for i in range(10)]
    frames.insert(5, np.full((h, w, 3), 77, np.uint8))
    return frames


_zoom_cache = {}


def zoom_bgr(oracle, size):
    """Thirteen BGR frames: rotated content in black corners, an all-black one (fall-back: no contour), an all-content one and, last,
    a black one with content on half of one row (fall-back: its contour has no height, the crop is empty)."""
    if size not in _zoom_cache:
        from test_azc import rotated_frame
        w, h = size
        frames = [rotated_frame(oracle, w, h, deg, seed=i) for i, deg in enumerate(ZOOM_DEGS)]
        frames.insert(3, np.zeros((h, w, 3), np.uint8))
        frames.insert(8, np.full((h, w, 3), 200, np.uint8))
        line = np.zeros((h, w, 3), np.uint8)
        line[h // 2, w // 4:3 * w // 4] = 200
        frames.append(line)
        _zoom_cache[size] = frames
    return _zoom_cache[size]


@functools.lru_cache(maxsize=None)
def chain_bgr(n):
    """roll_scene's chain clip as BGR frames: the seven frames of the SEED_CONFIG3 clip, each with the band of a tilted horizon from
    h / 3 down, repeated."""
    w, h = CHAIN_SIZE
    base = [f.copy() for f in synth.make_clip(synth.SEED_CONFIG3, w, h, 7)]
    tilt = roll_scene.horizon_frame(w, h, 45, seed=7)
    for f in base:
        f[h // 3:h // 3 + 400] = tilt[h // 3:h // 3 + 400]
    return [base[i % 7] for i in range(n)]


def roll_frames(size, slope, fmt):
    return _cached(("roll", size, slope, fmt), lambda: pack_all(roll_bgr(size, slope), fmt, 1000))


def zoom_frames(oracle, size, fmt):
    return _cached(("zoom", size, fmt), lambda: pack_all(zoom_bgr(oracle, size), fmt, 2000))


def chain_frames(n, fmt):
    return _cached(("chain", n, fmt), lambda: pack_all(chain_bgr(n), fmt, 3000))


def _cached(key, make):
    c = azc_size_inputs.cache("rgb_chain")
    if key not in c:
        c[key] = make()
    return c[key]


def roll_refs(oracle, size, slope, fmt):
    """(results, states) of the case's frames through a fresh oracle roll object, once per session."""
    def make():
        ro = oracle.roll_correction(oracle.roll_params(hough_threshold=roll_hough_threshold(size[0])))
        try:
            return roll_ref(roll_frames(size, slope, fmt), fmt, ro)
        finally:
            ro.close()
    return _cached(("roll_ref", size, slope, fmt), make)


def zoom_refs(oracle, size, fmt, out_size):
    return _cached(("zoom_ref", size, fmt, tuple(out_size)), lambda: [azc_ref(f, fmt, oracle, out_size) for f in zoom_frames(oracle, size, fmt)])
