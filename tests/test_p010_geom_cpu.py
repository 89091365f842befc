"""tests/ref16_geom.py pinned before any kernel is compared with it (no GPU):

1. on surfaces whose samples are all <= 255, with half-up rounding, its rotation and its crop-and-scale equal the oracle's NV12 roll
   correction and auto zoom/crop byte for byte - coordinates, replicate handling, rectangle halving and the scale matrix;
2. with a constant border, one size and a float matrix it is ref16.warp_affine;
3. its replicate border is the constant border on the plane edge-padded by 64 samples;
4. the inputs of tests/test_gpu_p010_chain.py hold rounding ties on every blended plane (a kernel that rounds half up must fail
   there), and the zoom scenes take both branches."""
import numpy as np
import pytest

import p010_chain_inputs as inputs
import ref16
import ref16_geom as geom
from p010_inputs import MATS, random_plane
from ref16 import HALF_EVEN, HALF_UP


def _roll_angles(oracle, size, slope):
    """The oracle's NV12 roll object over the high bytes of the case's surfaces: (its outputs, the smoothed angle after each frame)."""
    w, h = size
    ro = oracle.roll_correction(oracle.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
    outs, angles = [], []
    for s in inputs.roll_surfaces(size, slope):
        outs.append(ro.correct_nv12(geom.high_bytes(s), w, h))
        angles.append(ro.state()[0])
    ro.close()
    return outs, angles


@pytest.fixture(scope="module")
def roll_runs(oracle):
    return {(size, slope): _roll_angles(oracle, size, slope) for size, slope, _ in inputs.ROLL_CASES}


@pytest.fixture(scope="module")
def zoom_runs(oracle):
    return {size: [oracle.auto_zoom_crop_nv12(geom.high_bytes(s), *size) for s in inputs.zoom_surfaces(oracle, size)] for size in inputs.ZOOM_SIZES}


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,slope,padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_half_up_rotation_of_8_bit_surfaces_is_the_oracles_roll_correction(roll_runs, size, slope, padded):
    w, h = size
    outs, angles = roll_runs[(size, slope)]
    assert angles[-1] != 0.0
    for i, s in enumerate(inputs.roll_surfaces(size, slope)):
        nv12 = geom.high_bytes(s)
        assert np.array_equal(geom.rotate_surface(nv12, w, h, angles[i], HALF_UP), outs[i]), i
        assert np.array_equal(geom.rotate_surface(nv12.astype(np.uint16), w, h, angles[i], HALF_UP), outs[i]), i      # (samples <= 255 in 16 bits)


def test_half_up_crop_and_scale_of_8_bit_surfaces_is_the_oracles_auto_zoom_crop(oracle, zoom_runs):
    size = (808, 454)
    w, h = size
    for i, (s, (want, info)) in enumerate(zip(inputs.zoom_surfaces(oracle, size), zoom_runs[size])):
        nv12 = geom.high_bytes(s)
        got = geom.crop_scale_surface(nv12.astype(np.uint16), w, h, info, HALF_UP)
        assert got.shape == want.shape and np.array_equal(got, want), i


@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_zoom_scenes_take_both_branches(zoom_runs, size):
    """Between 9 and 11 of the 12 surfaces are cropped, as in the NV12 test: the oracle alone says so."""
    assert 9 <= sum(int(info[7]) for _, info in zoom_runs[size]) <= 11


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 2])
def test_constant_border_same_size_float_matrix_is_ref16(cn):
    img = random_plane(5 + cn, 66, 130, cn, ten_bit=False)
    for name, M in MATS.items():
        M64 = np.asarray(M, np.float32).astype(np.float64)
        for rounding in (HALF_EVEN, HALF_UP):
            assert np.array_equal(geom.warp(img, M64, None, geom.CONSTANT, rounding), ref16.warp_affine(img, M, rounding)), (name, rounding)


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,slope,padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_replicate_border_is_the_constant_border_on_the_edge_padded_plane(roll_runs, size, slope, padded):
    """The matrices of the roll test's angles; the padded plane's matrix maps the padded source (p + 64) to the same destination."""
    w, h = size
    P = 64
    _, angles = roll_runs[(size, slope)]
    surfs = inputs.roll_surfaces(size, slope)
    for i, a in enumerate(angles):
        y, uv = geom.planes(surfs[i], w, h)
        for plane, M in zip((y, uv), geom.roll_matrices(w, h, a)):
            ph, pw = plane.shape[:2]
            pad = np.pad(plane, ((P, P), (P, P)) + ((0, 0),) * (plane.ndim - 2), mode="edge")
            Mp = [M[0], M[1], M[2] - (M[0] + M[1]) * P, M[3], M[4], M[5] - (M[3] + M[4]) * P]
            want = geom.warp(pad, Mp, (pw, ph), geom.CONSTANT)
            assert np.array_equal(geom.warp(plane, M, None, geom.REPLICATE), want), (i, plane.ndim)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return bool((np.asarray(a) != np.asarray(b)).any())


@pytest.mark.parametrize("size,slope,padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_roll_inputs_hold_ties_on_both_planes_of_every_rotated_frame(roll_runs, size, slope, padded):
    w, h = size
    _, angles = roll_runs[(size, slope)]
    # (while the smoothed angle is still exactly 0 - no line found yet - the rotation is the identity: S = 1024 v, nothing is blended
    # and no rounding can show; every other frame must tell the two roundings apart on both planes)
    assert sum(a != 0.0 for a in angles) >= 8
    for i, s in enumerate(inputs.roll_surfaces(size, slope)):
        even, up = geom.rotate_surface(s, w, h, angles[i], HALF_EVEN), geom.rotate_surface(s, w, h, angles[i], HALF_UP)
        if angles[i] == 0.0:
            assert np.array_equal(even, s) and np.array_equal(up, s), i
            continue
        assert _differs(even[:h], up[:h]) and _differs(even[h:], up[h:]), i
        y, uv = geom.planes(s, w, h)
        M, Mc = geom.roll_matrices(w, h, angles[i])
        assert geom.tie_mask(y, M, None, geom.REPLICATE).any() and geom.tie_mask(uv, Mc, None, geom.REPLICATE).any(), i


@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_zoom_inputs_hold_ties_on_both_planes_of_every_cropped_surface(oracle, zoom_runs, size):
    w, h = size
    for i, (s, (_, info)) in enumerate(zip(inputs.zoom_surfaces(oracle, size), zoom_runs[size])):
        even, up = geom.crop_scale_surface(s, w, h, info, HALF_EVEN), geom.crop_scale_surface(s, w, h, info, HALF_UP)
        if info[7]:
            assert _differs(even[:360], up[:360]) and _differs(even[360:], up[360:]), i
        else:
            assert np.array_equal(even, s) and np.array_equal(up, s), i          # (unchanged, all 16 bits)


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("dsize", inputs.WARP16_DSTS, ids=lambda s: "%dx%d" % s)
def test_plane_warp_inputs_hold_ties_in_every_case(cn, dsize):
    img = inputs.warp16_plane(cn)
    for name, M in inputs.warp16_matrices(dsize).items():
        for border in (geom.CONSTANT, geom.REPLICATE):
            assert geom.tie_mask(img, M, dsize, border).any(), (name, border)
            assert _differs(geom.warp(img, M, dsize, border, HALF_EVEN), geom.warp(img, M, dsize, border, HALF_UP)), (name, border)
