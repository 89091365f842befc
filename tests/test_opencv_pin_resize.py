"""Pins the resize's definition (tests/resizeref.py) to a real OpenCV: cv2.resize with INTER_LANCZOS4 and INTER_LINEAR on uint8.

This image has no OpenCV, so the whole module SKIPS here and on the GPU box, like tests/test_opencv_pin_cvt.py.  On any machine with
`cv2` (4.x) importable, `python -m pytest tests/test_opencv_pin_resize.py -q` decides the row "resize INTER_LANCZOS4 8U" of
docs/opencv_semantics.md (confidence "medium": interpolateLanczos4, the coordinate rule and the rounding were restated from memory of
imgproc/src/resize.cpp) and confirms the INTER_LINEAR row for downscales.  OpenCV's CV_16U resize blends with float coefficients:
the 16-bit form is the library's own definition and nothing here can pin it."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import resizeref as rr                                          # noqa: E402

SHAPES = [((1, 1), (5, 3)), ((3, 2), (1, 1)), ((7, 5), (7, 5)), ((9, 9), (8, 8)), ((66, 50), (33, 25)), ((130, 96), (97, 61)), ((97, 61), (322, 200)),
          ((322, 200), (64, 36)), ((2046, 70), (1920, 64))]


def picture(sw, sh, cn, seed):
    return np.random.default_rng(seed).integers(0, 256, (sh, sw * cn), np.uint8)


@pytest.mark.parametrize("interp", [(rr.LINEAR, "INTER_LINEAR"), (rr.LANCZOS4, "INTER_LANCZOS4")], ids=lambda v: v[1])
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_resize_equals_cv2(shape, cn, interp):
    (sw, sh), (dw, dh) = shape
    p = picture(sw, sh, cn, sw + dh + cn)
    src = p.reshape(sh, sw) if cn == 1 else p.reshape(sh, sw, cn)
    want = cv2.resize(src, (dw, dh), interpolation=getattr(cv2, interp[1]))
    assert np.array_equal(rr.resize(p, cn, dw, dh, interp[0]), np.asarray(want).reshape(dh, dw * cn))


def test_lanczos_checkerboard_and_flat_areas_equal_cv2():
    """Both clamps, and the coefficients that are not renormalised: a flat 255 area may come out as 254."""
    board = (np.indices((24, 40)).sum(0) % 2 * 255).astype(np.uint8)
    flat = np.full((24, 40), 255, np.uint8)
    for p in (board, flat):
        assert np.array_equal(rr.resize(p, 1, 52, 31, rr.LANCZOS4), cv2.resize(p, (52, 31), interpolation=cv2.INTER_LANCZOS4))
