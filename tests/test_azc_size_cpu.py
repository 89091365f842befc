"""Auto zoom/crop at a chosen output size: what holds without a GPU.

(a) the four entry points and struct vs_scale_job are declared in include/vs_stab.h, exported and bound in vsamd/capi.py; without a
    device and without an object the setter, the getter and vs_op_scale_jobs answer VS_ERR_INVALID_ARG, and vs_op_scale_jobs_plan
    works (it is host arithmetic);
(b) the reference the GPU tests use - azc_size_inputs.reference: ref16_geom.warp with the reference's CV_32F scale matrix - equals the
    oracle's warp_affine_d through the black-canvas form of tests/test_i420_chain_cpu.py, cn 1 and 2, on the crop -> output pairs of
    azc_size_inputs.PAIRS; the 16-bit random planes of the same pairs hold rounding ties, so half-even is told from half-up;
(c) the plan: every pair that does not shrink is staged, 3840 x 2160 -> 640 x 360 is not, and the case list of the GPU operator test
    holds jobs of both classes, on the sides of the limit its docstring states;
(d) for p010_chain_inputs.zoom_surfaces the oracle alone says "cropped" for the ten rotated scenes and "not cropped" for the
    all-black one: the cap on the fall-back path for the stage tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import azc_size_inputs as inp
import p010_chain_inputs
import ref16_geom as geom
from test_i420_chain_cpu import _oracle_sized
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vs_azc_set_output_size", "vs_azc_get_output_size", "vs_op_scale_jobs", "vs_op_scale_jobs_plan"]
INVALID = 1
Job = capi.VsScaleJob          # struct vs_scale_job: the jobs of every test below that talks to the library
PAIR_IDS = ["%dx%d_to_%dx%d" % (s + d) for s, d in inp.PAIRS]


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exist_are_declared_and_bound(vs):
    with open(os.path.join(ROOT, "include", "vs_stab.h")) as f:
        hdr = f.read()
    with open(capi.__file__) as f:
        binding = f.read()
    for name in NEW:
        assert hasattr(vs.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(vs.lib, name).argtypes, name
        assert re.search(r"L\.%s\.argtypes" % name, binding), name
    m = re.search(r"typedef struct vs_scale_job \{(.*?)\} vs_scale_job;", hdr, re.S)
    want = "const void* src; size_t src_stride; int32_t sw, sh; void* dst; size_t dst_stride; int32_t dw, dh; int32_t cn, reserved;"
    assert m and m.group(1).split() == want.split()
    assert [f[0] for f in capi.VsScaleJob._fields_] == ["src", "src_stride", "sw", "sh", "dst", "dst_stride", "dw", "dh", "cn", "reserved"]
    assert C.sizeof(capi.VsScaleJob) == 2 * (C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t) + 8) + 8
    assert vs.lib.vs_abi_version() == 2 and "#define VS_STAB_ABI_VERSION 2" in hdr
    for n in ("set_output_size", "output_size"):
        assert hasattr(capi.AutoZoomCrop, n)
    assert callable(vs.scale_jobs) and callable(vs.scale_jobs_plan)


def test_calls_without_an_object_or_without_jobs_are_refused(vs):
    w, h = C.c_int(-1), C.c_int(-1)
    assert vs.lib.vs_azc_set_output_size(None, 640, 360) == INVALID
    assert vs.lib.vs_azc_get_output_size(None, C.byref(w), C.byref(h)) == INVALID and (w.value, h.value) == (-1, -1)
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    good = Job(p, 16, 8, 8, p + 2048, 32, 16, 16, 1, 0)
    one = (Job * 1)(good)
    assert vs.lib.vs_op_scale_jobs(None, 1, 1, 0, None) == INVALID
    assert vs.lib.vs_op_scale_jobs(one, 0, 1, 0, None) == INVALID and vs.lib.vs_op_scale_jobs(one, 25, 1, 0, None) == INVALID
    assert vs.lib.vs_op_scale_jobs(one, 1, 3, 0, None) == INVALID and vs.lib.vs_op_scale_jobs(one, 1, 1, 2, None) == INVALID
    bad = [dict(cn=3), dict(cn=0), dict(sw=0), dict(dh=0), dict(dw=40000), dict(src_stride=7), dict(dst_stride=15), dict(reserved=1), dict(src=None), dict(dst=None)]
    staged = np.full(1, -1, np.int32)
    for kw in bad:
        j = Job(p, 16, 8, 8, p + 2048, 32, 16, 16, 1, 0)
        for k, v in kw.items():
            setattr(j, k, v)
        arr = (Job * 1)(j)
        assert vs.lib.vs_op_scale_jobs(arr, 1, 1, 0, None) == INVALID, kw
        assert vs.lib.vs_op_scale_jobs_plan(arr, 1, 1, staged.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID and staged[0] == -1, kw
    assert b"scale_jobs" in vs.lib.vs_last_error()
    odd = (Job * 1)(Job(p + 1, 16, 8, 8, p + 2048, 32, 16, 16, 1, 0))          # 16-bit samples on an odd address
    assert vs.lib.vs_op_scale_jobs(odd, 1, 2, 0, None) == INVALID
    assert vs.lib.vs_op_scale_jobs_plan(odd, 1, 2, staged.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    assert vs.lib.vs_op_scale_jobs_plan(one, 1, 1, None) == INVALID
    assert vs.scale_jobs_plan([(p, 16, 8, 8, p + 2048, 32, 16, 16, 1)]).tolist() == [1]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("pair", inp.PAIRS, ids=PAIR_IDS)
def test_reference_equals_the_oracle_and_the_16_bit_planes_hold_ties(oracle, pair, cn):
    ssize, dsize = pair
    M = inp.scale_matrix(ssize, dsize)
    roi8 = inp.random_plane(ssize, cn, np.uint8, 100 + cn)
    assert np.array_equal(inp.reference(roi8, dsize), _oracle_sized(oracle, roi8, M, dsize))
    roi16 = inp.random_plane(ssize, cn, np.uint16, 200 + cn)
    ties = int(geom.tie_mask(roi16, M, dsize, geom.CONSTANT).sum())
    assert ties >= 1
    even, up = inp.reference(roi16, dsize), geom.warp(roi16, M, dsize, geom.CONSTANT, geom.HALF_UP)
    assert int((even != up).sum()) == ties


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def _plan(vs, cases, sb=1, cn=1):
    return vs.scale_jobs_plan([(4096, 65536, sw, sh, 1 << 30, 65536, dw, dh, cn) for (sw, sh), (dw, dh) in cases], sb).tolist()


def test_the_plan(vs):
    for sb in (1, 2):
        for cn in (1, 2):
            got = _plan(vs, inp.PAIRS, sb, cn)
            for ((sw, sh), (dw, dh)), s in zip(inp.PAIRS, got):
                if dw >= sw and dh >= sh:
                    assert s == 1, ((sw, sh), (dw, dh))
            assert _plan(vs, [((3840, 2160), (640, 360)), ((1920, 1080), (320, 180))], sb, cn) == [0, 0]
            # the GPU operator test's list: 24 jobs, both classes, each limit case on the side azc_size_inputs states
            assert len(inp.OP_CASES) == 24 and _plan(vs, inp.OP_CASES, sb, cn) == inp.OP_STAGED
    assert 0 in inp.OP_STAGED and 1 in inp.OP_STAGED
    # a zoom-in of the benchmark chain's surface at its own size: what the staged kernel is for
    assert _plan(vs, [((3400, 1912), (3840, 2160)), ((1700, 956), (1920, 1080))]) == [1, 1]


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", inp.STAGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_zoom_scenes_take_both_branches_by_the_oracle_alone(oracle, size):
    w, h = size
    surfs = p010_chain_inputs.zoom_surfaces(oracle, size)
    cropped = [int(oracle.auto_zoom_crop_nv12(geom.high_bytes(s), w, h)[1][7]) for s in surfs]
    assert len(cropped) == 12 and cropped[3] == 0                     # the all-black surface
    assert all(cropped[i] for i in range(12) if i not in (3, 8))      # the ten rotated scenes (8: the all-content one)
    assert sum(cropped) >= 10
