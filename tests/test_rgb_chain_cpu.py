"""Roll correction and auto zoom/crop on interleaved colour frames, the parts that need no device: the six entry points are declared,
exported and bound and refuse a null object; vs_op_scale_jobs_rgb_plan answers as the staging rule says; and the reference of
tests/rgb_chain_inputs.py is pinned to the oracle on every scene the GPU tests use, with the scenes' branches asserted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import azc_size_inputs as sizes
import ref16_geom as geom
import rgb_chain_inputs as inputs
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
SYMBOLS = ["vs_roll_correct_rgb_dev", "vs_roll_correct_rgb_dev_n", "vs_azc_apply_rgb_dev", "vs_azc_apply_rgb_dev_n", "vs_op_scale_jobs_rgb",
           "vs_op_scale_jobs_rgb_plan"]


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_declared_exported_and_bound(vs):
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\s*\(" % name, header, re.M), name
        f = getattr(vs.lib, name)                      # exported (ctypes resolves the symbol here)
        assert f.argtypes, name                        # bound in vsamd/capi.py
    assert vs.lib.vs_abi_version() == 2


def test_every_new_entry_point_refuses_a_null_object(vs):
    L = vs.lib
    p = C.c_void_p(4096)
    arr = (C.c_void_p * 1)(4096)
    t = C.c_int64(-1)
    assert L.vs_roll_correct_rgb_dev(None, capi.FMT_BGR8, p, 16, 16, 64, p, 64) == INVALID
    assert L.vs_roll_correct_rgb_dev_n(None, capi.FMT_BGRA8, arr, arr, 1, 16, 16, 64, 64) == INVALID
    assert L.vs_azc_apply_rgb_dev(None, capi.FMT_RGB8, p, 16, 16, 64, p, 4096, C.byref(t)) == INVALID
    assert L.vs_azc_apply_rgb_dev_n(None, capi.FMT_RGBA8, arr, arr, 1, 16, 16, 64, 4096, C.byref(t)) == INVALID
    assert L.vs_op_scale_jobs_rgb(None, 1, 0, None) == INVALID
    assert L.vs_op_scale_jobs_rgb_plan(None, 1, None) == INVALID
    assert t.value == -1


# ---- 2. vs_op_scale_jobs_rgb_plan ------------------------------------------------------------------------------------------------
def _jobs(cn, cases=sizes.OP_CASES):
    return [(4096, sw * cn, sw, sh, 1 << 20, dw * cn, dw, dh, cn) for (sw, sh), (dw, dh) in cases]


@pytest.mark.parametrize("cn", [3, 4])
def test_plan_answers_as_the_staging_rule_says(vs, cn):
    assert vs.scale_jobs_rgb_plan(_jobs(cn)).tolist() == sizes.OP_STAGED
    mixed = [j[:8] + (3 + i % 2,) for i, j in enumerate(_jobs(4))]          # cn 3 and 4 in one call (strides of 4 bytes per pixel hold both)
    assert vs.scale_jobs_rgb_plan(mixed).tolist() == sizes.OP_STAGED
    # the 8-bit operator of the YUV planes keeps refusing colour jobs, and this one theirs
    staged = np.zeros(24, np.int32)
    assert vs.lib.vs_op_scale_jobs_plan(vs._scale_job_array(_jobs(cn)), 24, 1, capi._p(staged, capi.i32p)) == INVALID


def test_plan_refusals(vs):
    ok = (4096, 400, 100, 50, 1 << 20, 520, 130, 66, 4)
    staged = np.zeros(32, np.int32)

    def rc(jobs, n=None, reserved=0, out=staged):
        arr = vs._scale_job_array(jobs)
        for a in arr:
            a.reserved = reserved
        return vs.lib.vs_op_scale_jobs_rgb_plan(arr, len(jobs) if n is None else n, capi._p(out, capi.i32p) if out is not None else None)

    assert rc([ok]) == 0 and staged[0] == 1
    for cn in (1, 2, 5, 0):
        assert rc([ok[:8] + (cn,)]) == INVALID, cn
    for k in (2, 3, 6, 7):                                  # zero sizes
        bad = list(ok)
        bad[k] = 0
        assert rc([tuple(bad)]) == INVALID, k
    assert rc([ok], reserved=1) == INVALID
    assert rc([ok[:1] + (399,) + ok[2:]]) == INVALID        # strides below a row
    assert rc([ok[:5] + (519,) + ok[6:]]) == INVALID
    assert rc([ok[:1] + (299,) + ok[2:8] + (3,)]) == INVALID
    assert rc([ok] * 25) == INVALID and rc([ok], n=0) == INVALID and rc([ok], out=None) == INVALID
    assert rc([(0,) + ok[1:]]) == INVALID and rc([ok[:4] + (0,) + ok[5:]]) == INVALID
    assert b"scale_jobs_rgb_plan" in vs.lib.vs_last_error()


# ---- 3. the reference is the oracle's ----------------------------------------------------------------------------------------------
def _permuted(ref_bgr, fmt):
    return ref_bgr if fmt in (inputs.BGR8, inputs.BGRA8) else ref_bgr[..., ::-1]


@pytest.mark.parametrize("size,slope,padded", inputs.ROLL_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_roll_reference_is_pinned_to_the_oracle(oracle, size, slope, padded):
    w, h = size
    bgr = inputs.roll_bgr(size, slope)
    ro = oracle.roll_correction(oracle.roll_params(hough_threshold=inputs.roll_hough_threshold(w)))
    want, states = [], []
    for f in bgr:
        want.append(ro.correct(f))
        states.append(ro.state())
    ro.close()
    ref_bgr, ref_states = inputs.roll_refs(oracle, size, slope, inputs.BGR8)
    assert ref_states == states and all(np.array_equal(a, b) for a, b in zip(ref_bgr, want))
    # the scene: the smoothed angle moves from frame to frame - in both batches, 8 + 3 - and ends away from zero; frames with lines
    # and frames without (the flat one among them: the decay branch)
    angles = [s[0] for s in states]
    assert angles[-1] != 0.0 and angles[-1] != angles[-2] != angles[-3] and len(set(angles[:8])) >= 6
    assert any(s[3] > 0 for s in states) and any(s[2] == 0 for s in states)
    assert (states[5][2] == 0 or states[5][3] == 0) and angles[5] == angles[4] * 0.995
    for fmt in (inputs.RGB8, inputs.BGRA8, inputs.RGBA8):
        ref, st = inputs.roll_refs(oracle, size, slope, fmt)
        assert st == states, fmt
        frames = inputs.roll_frames(size, slope, fmt)
        for i, (r, f) in enumerate(zip(ref, frames)):
            assert np.array_equal(r[..., :3], _permuted(ref_bgr[i], fmt)), (fmt, i)
            if inputs.CN[fmt] == 4:
                M = geom.roll_matrices(w, h, states[i][0])[0]
                assert np.array_equal(r[..., 3], oracle.warp_affine_d(f[..., 3], M, border=geom.REPLICATE)), (fmt, i)


@pytest.mark.parametrize("size", inputs.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_zoom_reference_is_pinned_to_the_oracle(oracle, size):
    w, h = size
    bgr = inputs.zoom_bgr(oracle, size)
    ref_bgr = inputs.zoom_refs(oracle, size, inputs.BGR8, (640, 360))
    infos = []
    for f, (r, info) in zip(bgr, ref_bgr):
        z, winfo = oracle.auto_zoom_crop(f)
        assert info.tolist() == winfo.tolist() and r.shape == z.shape and np.array_equal(r, z)
        infos.append(winfo)
    # the scenes: both fall-back branches (no contour: the black frame; a contour and an empty crop: the line frame) and the cropped one
    assert len(infos) == 13 and not infos[3][7] and infos[3][0] == 0 and not infos[12][7] and infos[12][0] == 1
    assert sum(int(i[7]) for i in infos) >= 9
    looked = 0
    for fmt in (inputs.RGB8, inputs.BGRA8, inputs.RGBA8):
        frames = inputs.zoom_frames(oracle, size, fmt)
        # (every scene in every format at the reference's output size; the other output sizes with the four-channel BGRA8)
        for out_size in (inputs.OUT_SIZES if fmt == inputs.BGRA8 else inputs.OUT_SIZES[:1]):
            ref = inputs.zoom_refs(oracle, size, fmt, out_size)
            base = inputs.zoom_refs(oracle, size, inputs.BGR8, out_size)
            for i, ((r, info), (b, binfo)) in enumerate(zip(ref, base)):
                assert info.tolist() == binfo.tolist() == infos[i].tolist(), (fmt, i)
                assert r.shape[:2] == b.shape[:2] == ((sizes.resolved(out_size, w, h)[::-1]) if info[7] else (h, w)), (fmt, out_size, i)
                assert np.array_equal(r[..., :3], _permuted(b, fmt)), (fmt, out_size, i)
                if inputs.CN[fmt] == 4:
                    a = frames[i][..., 3]
                    if info[7]:
                        cx, cy, cw, ch = (int(v) for v in info[2:6])
                        a = sizes.reference(a[cy:cy + ch, cx:cx + cw], sizes.resolved(out_size, w, h))
                        looked += 1
                    assert np.array_equal(r[..., 3], a), (fmt, out_size, i)
    assert looked >= (3 + 1) * 9                               # (cropped frames with a fourth channel were looked at)


def test_one_channel_reference_equals_the_oracle_warp(oracle):
    """azc_size_inputs.reference on a plane by itself is the oracle's warp of it: the pin of the fourth channel's statement."""
    plane = inputs.alpha_plane(66, 130, 5)
    for dsize in [(130, 66), (258, 130)]:
        M = sizes.scale_matrix((130, 66), dsize)
        want = geom.warp(plane, M, dsize, geom.CONSTANT, geom.HALF_UP)
        assert np.array_equal(sizes.reference(plane, dsize), want)
    M = geom.roll_matrices(130, 66, 2.75)[0]
    for img in (plane, np.dstack([plane, plane[::-1], plane[:, ::-1]]), np.dstack([plane, plane[::-1], plane[:, ::-1], inputs.alpha_plane(66, 130, 6)])):
        for border in (geom.CONSTANT, geom.REPLICATE):
            assert np.array_equal(geom.warp(img, M, None, border, geom.HALF_UP), oracle.warp_affine_d(img, M, border=border))


def test_chain_scene_makes_the_roll_stage_and_the_zoom_stage_work(oracle):
    frames = inputs.chain_bgr(8)
    ro = oracle.roll_correction()
    rolled = [ro.correct(f) for f in frames]
    assert ro.state()[0] != 0.0
    ro.close()
    assert rolled[0].shape == (inputs.CHAIN_SIZE[1], inputs.CHAIN_SIZE[0], 3)
    a, b = inputs.chain_frames(8, inputs.BGRA8), inputs.chain_frames(8, inputs.RGBA8)
    assert np.array_equal(a[7][..., :3], frames[0]) and np.array_equal(b[1][..., 2::-1], frames[1]) and np.array_equal(a[2][..., 3], b[2][..., 3])
    assert len(np.unique(a[0][..., 3])) == 256
