"""Pins tests/planar_chain_ref.py - the reference of roll correction and auto zoom/crop on three-plane surfaces of any subsampling -
and the inputs of tests/test_gpu_planar_chain.py, without a device:

1. 8-bit planes: rotate_planar equals the oracle's cv::warpAffine (warp_affine_d, double matrix, BORDER_REPLICATE) plane by plane,
   the sheared chroma matrix of 4:2:2 included;
2. with (sx, sy) = (1, 1) both helper functions are ref16_geom.rotate_surface / crop_scale_surface de-interleaved, 8- and 16-bit;
3. the inputs: every roll scene is seen by the oracle near its target angle and never at 0; every zoom scene is cropped; the first
   surface of every 16-bit case holds a chroma sample on which half-even and half-up differ (ref16_geom.tie_mask), so the rounding
   rule is exercised on the device;
4. the layout rules of the two stages (csrc/planar_layout.h through tests/cpp/planar_layout_check.cpp): the 4:2:0 texts byte for byte
   what they were, the new formats' rules with the shifts."""
import numpy as np
import pytest

import planar_chain_inputs as inp
import planar_chain_ref as ref
import planar_layout_prog
import ref16_geom as geom
from ref16 import HALF_EVEN, HALF_UP
from vsamd import capi


# ---- 1. against the oracle, 8 bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [1.5, 3.0, 8.0])
@pytest.mark.parametrize("size", [(130, 96), (322, 200)], ids=["130x96", "322x200"])
@pytest.mark.parametrize("fmt", ["I422", "I444"])
def test_rotate_planar_is_the_oracles_warp_per_plane(oracle, fmt, size, angle):
    w, h = size
    rng = np.random.default_rng(w + int(angle * 10))
    planes = [rng.integers(0, 256, s, np.uint8) for s in ref.plane_shapes(fmt, w, h)]
    M, Mc = ref.roll_matrices(fmt, w, h, angle)
    sx, sy = ref.shifts(fmt)
    if (sx, sy) == (1, 0):          # the shear: m1 halved, m3 doubled, only the x translation halved
        assert Mc == [M[0], M[1] * 0.5, M[2] * 0.5, M[3] * 2.0, M[4], M[5]]
    else:
        assert Mc == M
    got = ref.rotate_planar(planes, fmt, angle)
    for name, g, p, m in zip("YUV", got, planes, (M, Mc, Mc)):
        assert g.dtype == np.uint8 and np.array_equal(g, oracle.warp_affine_d(p, m, geom.REPLICATE)), name


@pytest.mark.parametrize("fmt", ["I422", "I444"])
def test_crop_scale_planar_is_the_oracles_warp_per_plane(oracle, fmt):
    """The scale half against cv::warpAffine with the CV_32F scale matrix on the cropped plane (BORDER_CONSTANT 0), a zoom-in and a
    downscale."""
    w, h = 322, 200
    sx, sy = ref.shifts(fmt)
    rng = np.random.default_rng(5)
    planes = [rng.integers(1, 256, s, np.uint8) for s in ref.plane_shapes(fmt, w, h)]
    info = np.array([1, 0, 17, 11, 289, 180, 0, 1], np.int32)
    for ow, oh in ((640, 360), (200, 120)):
        got = ref.crop_scale_planar(planes, fmt, info, ow, oh)
        jobs = ref.zoom_jobs(info, sx, sy, ow, oh)
        for name, g, p, (x, y, cw, ch, dw, dh, M) in zip("YUV", got, planes, (jobs[0], jobs[1], jobs[1])):
            assert g.shape == (dh, dw)
            roi = np.ascontiguousarray(p[y:y + ch, x:x + cw])
            # the oracle's call keeps the size: the crop in the corner of a plane of zeros that holds the destination too - what lies
            # beyond the crop is 0 either way
            big = np.zeros((max(ch, dh), max(cw, dw)), np.uint8)
            big[:ch, :cw] = roi
            assert np.array_equal(g, oracle.warp_affine_d(big, M, geom.CONSTANT)[:dh, :dw]), (name, ow, oh)
    assert jobs[1][:6] == (17 >> sx, 11 >> sy, 289 >> sx, 180 >> sy, 200 >> sx, 120 >> sy)


# ---- 2. (1, 1) is the 4:2:0 reference ----------------------------------------------------------------------------------------------------
def _interleave(y, u, v):
    h, w = y.shape
    out = np.empty((h * 3 // 2, w), y.dtype)
    out[:h] = y
    out[h:, 0::2] = u
    out[h:, 1::2] = v
    return out


@pytest.mark.parametrize("fmt,rounding", [("I420", HALF_UP), ("I010", HALF_EVEN)])
def test_shifts_one_one_are_the_420_references(fmt, rounding):
    w, h = 130, 96
    rng = np.random.default_rng(ref.bits(fmt))
    hi = 256 if ref.bits(fmt) == 8 else 65536
    dt = np.uint8 if ref.bits(fmt) == 8 else np.uint16
    planes = [rng.integers(1, hi, s, dt) for s in ref.plane_shapes(fmt, w, h)]
    surf = _interleave(*planes)
    for angle in (1.5, -8.0):
        want = geom.rotate_surface(surf, w, h, angle, rounding)
        got = ref.rotate_planar(planes, fmt, angle)
        assert np.array_equal(_interleave(*got), want), angle
    info = np.array([1, 0, 9, 6, 111, 82, 0, 1], np.int32)
    want = geom.crop_scale_surface(surf, w, h, info, rounding)
    got = ref.crop_scale_planar(planes, fmt, info, 640, 360)
    assert np.array_equal(_interleave(*got), want)
    info[7] = 0
    assert all(np.array_equal(a, b) for a, b in zip(ref.crop_scale_planar(planes, fmt, info, 640, 360), planes))


# ---- 3. the inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilt", list(inp.TILTS))
@pytest.mark.parametrize("size", inp.SIZES, ids=lambda s: "%dx%d" % s)
def test_roll_scenes_are_seen_near_their_target_angle(oracle, size, tilt):
    target = inp.TILTS[tilt][0]
    states = inp.roll_oracle(oracle, size, tilt)
    assert len(states) == inp.N_ROLL
    for i, st in enumerate(states):
        assert st[0] != 0.0 and abs(st[0] - target) <= 0.75 and st[3] > 0, (i, st)
    # the analysis plane is the same for every format of a scene
    for fmt in inp.FORMATS:
        a = ref.analysis_nv12(inp.roll_planes(fmt, size, tilt)[0], fmt)
        assert np.array_equal(a, ref.analysis_nv12(inp.roll_planes("I444", size, tilt)[0], "I444")), fmt


@pytest.mark.parametrize("size", inp.SIZES, ids=lambda s: "%dx%d" % s)
def test_zoom_scenes_are_cropped(oracle, size):
    infos = inp.zoom_info(oracle, size)
    assert len(infos) == len(inp.ZOOM_DEGS) and all(int(i[7]) == 1 for i in infos)
    w, h = size
    if size == (704, 400):           # 640 x 360 is a zoom-in of one crop and a downscale of another
        assert any(i[4] < 640 for i in infos) and any(i[4] > 640 for i in infos)
    for fmt in inp.FORMATS:
        a = ref.analysis_nv12(inp.zoom_planes(oracle, fmt, size)[0], fmt)
        assert np.array_equal(a, ref.analysis_nv12(inp.zoom_planes(oracle, "I444", size)[0], "I444")), fmt


SIXTEEN = [f for f in inp.FORMATS if ref.bits(f) != 8]


@pytest.mark.parametrize("tilt", list(inp.TILTS))
@pytest.mark.parametrize("size", inp.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", SIXTEEN)
def test_16_bit_roll_inputs_hold_rounding_ties_in_chroma(oracle, fmt, size, tilt):
    w, h = size
    planes = inp.roll_planes(fmt, size, tilt)[0]
    _, Mc = ref.roll_matrices(fmt, w, h, inp.roll_oracle(oracle, size, tilt)[0][0])
    ties = sum(int(geom.tie_mask(p, Mc, None, geom.REPLICATE).sum()) for p in planes[1:])
    assert ties > 0


@pytest.mark.parametrize("out", inp.ZOOM_OUT, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", inp.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", SIXTEEN)
def test_16_bit_zoom_inputs_hold_rounding_ties_in_chroma(oracle, fmt, size, out):
    w, h = size
    ow, oh = out[0] or w, out[1] or h
    planes = inp.zoom_planes(oracle, fmt, size)[0]
    _, (x, y, cw, ch, dw, dh, Mu) = ref.zoom_jobs(inp.zoom_info(oracle, size)[0], *ref.shifts(fmt), ow, oh)
    ties = sum(int(geom.tie_mask(p[y:y + ch, x:x + cw], Mu, (dw, dh), geom.CONSTANT).sum()) for p in planes[1:])
    assert ties > 0


# ---- 4. the layout rules -------------------------------------------------------------------------------------------------------------------
F = {n: capi.PIXFMT_BY_NAME[n].fmt for n in ("I420", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412")}


def _case(name, ptr=0, w=64, h=48, pitch=None, c_pitch=0, u_off=0, v_off=0, need=None):
    sb = capi.PIXFMT_BY_NAME[name].sample_bytes
    nw, nh = need or (w, h)
    return (F[name], ptr, w, h, nw * sb if pitch is None else pitch, c_pitch, u_off, v_off, nw, nh)


def test_layout_defaults_follow_the_shifts():
    names = ["I420", "I010", "I422", "I210", "I444", "I412"]
    got = planar_layout_prog.check([_case(n) for n in names] + [_case("I422", need=(640, 360)), _case("I444", pitch=65)])
    want = ["64 32 3072 3840", "128 64 6144 7680", "64 32 3072 4608", "128 64 6144 9216", "64 64 3072 6144", "128 128 6144 12288",
            "640 320 230400 345600", "65 65 3120 6240"]          # (4:4:4: any pitch of whole samples has a default chroma pitch)
    assert got == [(0, w) for w in want]


def test_layout_texts_of_the_420_formats_are_unchanged():
    cases = [(_case("I420", w=63), "w and h must be even"), (_case("I010", h=47), "w and h must be even"),
             (_case("I420", pitch=62), "the pitch must hold a row of the picture"),
             (_case("I010", pitch=129), "pointers, pitches and plane offsets must be even (16-bit samples)"),
             (_case("I012", ptr=1), "pointers, pitches and plane offsets must be even (16-bit samples)"),
             (_case("I420", pitch=65), "the default chroma pitch needs an even pitch"),
             (_case("I010", pitch=130), "the default chroma pitch needs a pitch that is a multiple of 4"),
             (_case("I420", c_pitch=30), "the chroma pitch must be at least w / 2"),
             (_case("I010", c_pitch=62), "the chroma pitch must be at least w bytes"),
             (_case("I420", u_off=64 * 48 - 2), "the chroma planes must start behind the luma rows"),
             (_case("I420", u_off=64 * 48, v_off=64 * 48 + 32 * 23), "the U and V planes overlap"),
             (_case("I420", need=(640, 360), pitch=640, u_off=640 * 360, v_off=640 * 360 + 320 * 179), "the U and V planes overlap")]
    got = planar_layout_prog.check([c for c, _ in cases])
    for (c, text), (rc, msg) in zip(cases, got):
        name = [n for n, v in F.items() if v == c[0]][0]
        assert (rc, msg) == (1, "stage: %s: %s" % (name, text)), c


def test_layout_rules_of_the_new_formats():
    """One refusal per rule that the shifts change, naming the format, and the accepted case right beside it."""
    cases = [
        # w and h stay even for every format of the two stages
        (_case("I422", h=47), "I422: w and h must be even"), (_case("I444", w=63), "I444: w and h must be even"),
        # the default chroma pitch: pitch >> sx - 4:2:2 keeps the evenness rule, 4:4:4 needs none beyond whole samples
        (_case("I422", pitch=65), "I422: the default chroma pitch needs an even pitch"),
        (_case("I210", pitch=130), "I210: the default chroma pitch needs a pitch that is a multiple of 4"),
        (_case("I444", pitch=65), None), (_case("I410", pitch=130), None),
        (_case("I410", pitch=131), "I410: pointers, pitches and plane offsets must be even (16-bit samples)"),
        # a chroma pitch holds (need_w >> sx) samples
        (_case("I422", c_pitch=31), "I422: the chroma pitch must hold a chroma row (32 bytes)"), (_case("I422", c_pitch=32), None),
        (_case("I444", c_pitch=63), "I444: the chroma pitch must hold a chroma row (64 bytes)"), (_case("I444", c_pitch=64), None),
        (_case("I212", c_pitch=62), "I212: the chroma pitch must hold a chroma row (64 bytes)"),
        (_case("I412", c_pitch=126), "I412: the chroma pitch must hold a chroma row (128 bytes)"),
        (_case("I422", need=(640, 360), pitch=640, c_pitch=318), "I422: the chroma pitch must hold a chroma row (320 bytes)"),
        # the chroma planes hold need_h >> sy rows: 48 rows of chroma for 4:2:2 and 4:4:4 where 4:2:0 has 24
        (_case("I422", u_off=64 * 48, v_off=64 * 48 + 32 * 47), "I422: the U and V planes overlap"), (_case("I422", u_off=64 * 48, v_off=64 * 48 + 32 * 48), None),
        (_case("I444", u_off=64 * 48, v_off=64 * 48 + 64 * 47), "I444: the U and V planes overlap"),
        (_case("I210", u_off=128 * 48 + 64 * 48, v_off=128 * 48 + 64 * 2), "I210: the U and V planes overlap"),       # V before U, too close
        (_case("I210", u_off=128 * 48 + 64 * 48, v_off=128 * 48), None),                                             # V before U
        (_case("I444", u_off=64 * 48 - 1), "I444: the chroma planes must start behind the luma rows"),
        (_case("I422", need=(640, 360), pitch=640, u_off=640 * 359), "I422: the chroma planes must start behind the luma rows"),
    ]
    got = planar_layout_prog.check([c for c, _ in cases])
    for (c, text), (rc, msg) in zip(cases, got):
        if text is None:
            assert rc == 0, (c, msg)
        else:
            assert (rc, msg) == (1, "stage: " + text), c
