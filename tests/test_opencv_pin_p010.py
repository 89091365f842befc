"""Pins the 16-bit warp definition (tests/ref16.py, half-to-even) to a real OpenCV: cv2.warpAffine on uint16 arrays.

This image has no OpenCV, so the whole module SKIPS here and on the GPU box, like tests/test_opencv_pin.py.  On any machine
with `cv2` (4.x) importable, `python -m pytest tests/test_opencv_pin_p010.py -q` decides the row "warpAffine, 16-bit" of
docs/opencv_semantics.md: the source followed is remapBilinear<Cast<float, ushort>, RemapNoVec, float>, whose float sum is
exact for ten-bit content - there the comparison is sample for sample.  For full-range 16-bit content the float sum depends on
the build (order, FMA); the library's definition is the exact integer sum rounded once, and the test reports how far a given
OpenCV is from it (at most one unit)."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import ref16                                                    # noqa: E402
from p010_inputs import MATS, random_plane                      # noqa: E402


def _cv(img, M):
    M = np.asarray(M, np.float32).reshape(2, 3)
    return cv2.warpAffine(img, M, (img.shape[1], img.shape[0]), flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT, borderValue=0)


@pytest.mark.parametrize("name", list(MATS))
@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("size", [(2, 2), (38, 24), (322, 200)], ids=lambda s: "%dx%d" % s)
def test_ten_bit_content_equals_cv2(name, cn, size):
    w, h = size
    img = random_plane(w + cn, h, w, cn)
    assert np.array_equal(ref16.warp_affine(img, MATS[name]), _cv(img, MATS[name]))


@pytest.mark.parametrize("name", list(MATS))
def test_full_range_content_is_within_one_unit_of_cv2(name):
    img = random_plane(5, 200, 322, 1, ten_bit=False)
    a, b = ref16.warp_affine(img, MATS[name]).astype(np.int64), _cv(img, MATS[name]).astype(np.int64)
    print("%s: %d of %d samples differ from this OpenCV's float blend" % (name, int(np.count_nonzero(a != b)), a.size))
    assert np.max(np.abs(a - b)) <= 1


def test_the_tie_rule_is_half_to_even():
    even = np.array([[0, 4, 5, 0]], np.uint16)
    odd = np.array([[0, 5, 6, 0]], np.uint16)
    M = [1, 0, 0.5, 0, 1, 0]
    assert _cv(even, M)[0, 2] == 4 and _cv(odd, M)[0, 2] == 6
