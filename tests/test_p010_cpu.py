"""P010 without a GPU: the 16-bit warp reference (tests/ref16.py) pinned by the 8-bit oracle, known answers on 16-bit data, the
rounding ties the GPU tests rely on, and the format at the ABI and in the binding."""
import os
import re

import numpy as np
import pytest

import ref16
from p010_inputs import MATS, NON_INTEGER, random_plane, random_surface
from vsamd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (6, 4), (38, 24), (130, 18), (322, 200)]


# ---- the reference is pinned by the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("name", list(MATS))
def test_half_up_on_8bit_planes_is_the_oracle(oracle, size, cn, name):
    w, h = size
    img = np.random.default_rng(w * 31 + h + cn).integers(0, 256, (h, w) if cn == 1 else (h, w, cn), np.uint8)
    want = oracle.warp_affine(img, MATS[name])
    assert np.array_equal(ref16.warp_affine(img, MATS[name], ref16.HALF_UP), want)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(MATS))
def test_half_up_on_nv12_surfaces_is_the_oracle(oracle, size, name):
    w, h = size
    surf = np.random.default_rng(w * 17 + h).integers(0, 256, (h * 3 // 2, w), np.uint8)
    assert np.array_equal(ref16.warp_two_planes(surf, w, h, MATS[name], ref16.HALF_UP), oracle.warp_affine_nv12(surf, w, h, MATS[name]))


# ---- known answers on 16-bit data --------------------------------------------------------------------------------------------
def test_identity_and_integer_shifts_return_the_samples():
    img = random_plane(1, 40, 64, ten_bit=False)
    assert np.array_equal(ref16.warp_affine(img, MATS["identity"]), img)
    got = ref16.warp_affine(img, MATS["int_shift"])           # dst(x, y) = src(x - 7, y + 3)
    want = np.zeros_like(img)
    want[:37, 7:] = img[3:, :57]
    assert np.array_equal(got, want)


def test_constant_plane_fades_to_zero_across_the_border_by_the_weights():
    img = np.full((16, 16), 65535, np.uint16)
    got = ref16.warp_affine(img, [1, 0, 0.25, 0, 1, 0])      # source x = x - 0.25: sx = x - 1, fx = 24
    assert np.all(got[:, 1:] == 65535)
    # column 0: taps (-1, y) = 0 and (0, y) = 65535 with weights 8 / 32 and 24 / 32: S = 65535 * 768
    S = 65535 * 768
    assert np.all(got[:, 0] == (S + 511 + ((S >> 10) & 1)) >> 10)
    assert got[0, 0] == 49151


def test_half_pixel_shift_over_a_ramp():
    img = np.tile((np.arange(32, dtype=np.uint16) * 64)[None, :], (4, 1))
    got = ref16.warp_affine(img, [1, 0, 0.5, 0, 1, 0])       # dst(x) = (src(x - 1) + src(x)) / 2 = 64 x - 32, exact
    assert np.array_equal(got[:, 1:], np.tile((np.arange(1, 32) * 64 - 32)[None, :], (4, 1)))
    assert np.all(got[:, 0] == 0)


def test_half_even_and_half_up_differ_exactly_on_even_ties():
    M = [1, 0, 0.5, 0, 1, 0]                                  # n = (512, 512, 0, 0)
    even = np.array([[0, 4, 5, 0]], np.uint16)                # x = 2: S = (4 + 5) * 512 = 4 * 1024 + 512, S >> 10 = 4 (even)
    odd = np.array([[0, 5, 6, 0]], np.uint16)                 # x = 2: S = 11 * 512 = 5 * 1024 + 512, S >> 10 = 5 (odd)
    assert ref16.warp_sum(even, np.float64(M))[0, 2] == 4 * 1024 + 512
    assert ref16.warp_affine(even, M, ref16.HALF_EVEN)[0, 2] == 4 and ref16.warp_affine(even, M, ref16.HALF_UP)[0, 2] == 5
    assert ref16.warp_sum(odd, np.float64(M))[0, 2] == 5 * 1024 + 512
    assert ref16.warp_affine(odd, M, ref16.HALF_EVEN)[0, 2] == 6 and ref16.warp_affine(odd, M, ref16.HALF_UP)[0, 2] == 6
    assert ref16.tie_mask(even, M)[0, 2] and not ref16.tie_mask(odd, M)[0, 2]


@pytest.mark.parametrize("name", NON_INTEGER)
def test_the_gpu_tests_inputs_hold_ties_that_tell_the_rounding_rules_apart(name):
    """A condition on the inputs, not a measurement: at least one output sample in a hundred on which half-even and half-up
    give different values, on the ten-bit surface the GPU tests warp at 322 x 200 - so a kernel with the wrong tie rule fails."""
    w, h = 322, 200
    surf = random_surface(322, w, h)
    a = ref16.warp_two_planes(surf, w, h, MATS[name], ref16.HALF_EVEN)
    b = ref16.warp_two_planes(surf, w, h, MATS[name], ref16.HALF_UP)
    frac = np.mean(a != b)
    print("%s: %.2f %% of the samples differ between half-even and half-up" % (name, 100 * frac))
    assert frac >= 0.01
    luma = ref16.tie_mask(surf[:h], MATS[name])
    assert np.array_equal(luma, a[:h] != b[:h])


def test_p010_clip_helper_keeps_the_nv12_clip_in_the_high_bytes():
    nv12 = np.random.default_rng(3).integers(0, 256, (36, 32), np.uint8)
    p = synth.nv12_to_p010(nv12, seed=9)
    assert p.dtype == np.uint16 and p.shape == nv12.shape
    assert np.array_equal((p >> 8).astype(np.uint8), nv12)
    assert np.all((p & 63) == 0) and len(np.unique((p >> 6) & 3)) == 4
    assert np.array_equal(p, synth.nv12_to_p010(nv12, seed=9))


# ---- header and binding ------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vs_stab.h")).read()


def test_p010_enum_value_in_the_header_and_the_binding():
    body = re.search(r"typedef enum vs_pixfmt16 \{(.*?)\} vs_pixfmt16;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert {k: int(v) for k, v in re.findall(r"(VS_\w+)\s*=\s*(\d+)", body)} == {"VS_FMT_P010": 6}
    assert capi.FMT_P010 == 6
    assert capi.FMT_SAMPLE_BYTES == {capi.FMT_P010: 2}
    assert capi.FMT_P010 not in capi.FMT_CHANNELS
    assert "#define VS_STAB_ABI_VERSION 2" in _header()


def test_p010_operator_is_declared():
    assert re.search(r"\bint\s+vs_op_warp_affine_p010\s*\(", _header())


def test_shape_helpers_of_p010():
    import test_pixfmt_cpu
    s = test_pixfmt_cpu._stub_stabilizer()
    assert s._geom(np.zeros((36, 32), np.uint16), capi.FMT_P010) == (32, 24, 2)
    assert s.out_shape(32, 24, capi.FMT_P010) == (66, 52)
    assert capi.fmt_dtype(capi.FMT_P010) == np.uint16 and capi.fmt_dtype(capi.FMT_NV12) == np.uint8
