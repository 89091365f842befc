"""Pins the colour conversion's definition (tests/cvtref.py) to a real OpenCV: cv2.cvtColor with COLOR_YUV2BGR_NV12,
COLOR_YUV2BGR_I420, COLOR_YUV2RGBA_NV12 and COLOR_BGR2YUV_I420.

This image has no OpenCV, so the whole module SKIPS here and on the GPU box, like tests/test_opencv_pin.py.  On any machine with
`cv2` (4.x) importable, `python -m pytest tests/test_opencv_pin_cvt.py -q` decides the two rows "cvtColor YUV 4:2:0 -> BGR" and
"cvtColor BGR -> YUV I420" of docs/opencv_semantics.md (confidence "medium": the constants and the rounding were restated from
memory of imgproc/src/color_yuv.simd.hpp).  OpenCV has no planar 4:2:2 / 4:4:4 and no 16-bit YUV conversion: those are the
library's own definition and nothing here can pin them."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import cvtref                                                   # noqa: E402


def surface(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h // 2, w // 2), np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), np.uint8))


def nv12(y, u, v):
    uv = np.empty((y.shape[0] // 2, y.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return np.vstack([y, uv])


def i420(y, u, v):
    h, w = y.shape
    return np.vstack([y, u.reshape(h // 4, w), v.reshape(h // 4, w)])


@pytest.mark.parametrize("size", [(2, 4), (34, 8), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_yuv420_to_bgr_equals_cv2(size):
    w, h = size
    y, u, v = surface(w, h, 1)
    assert np.array_equal(cvtref.yuv_to_rgb(y, u, v, 1, 1, "BGR8"), cv2.cvtColor(nv12(y, u, v), cv2.COLOR_YUV2BGR_NV12))
    assert np.array_equal(cvtref.yuv_to_rgb(y, u, v, 1, 1, "BGR8"), cv2.cvtColor(i420(y, u, v), cv2.COLOR_YUV2BGR_I420))
    assert np.array_equal(cvtref.yuv_to_rgb(y, u, v, 1, 1, "RGBA8"), cv2.cvtColor(nv12(y, u, v), cv2.COLOR_YUV2RGBA_NV12))


def test_every_chroma_pair_at_the_luma_extremes_equals_cv2():
    """The clamp on both sides, the max(0, Y - 16) floor and the rounding of negative sums."""
    u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    for luma in (0, 15, 16, 17, 128, 235, 236, 255):
        y = np.full((512, 512), luma, np.uint8)
        assert np.array_equal(cvtref.yuv_to_rgb(y, u, v, 1, 1, "BGR8"), cv2.cvtColor(nv12(y, u, v), cv2.COLOR_YUV2BGR_NV12)), luma


@pytest.mark.parametrize("size", [(2, 4), (34, 8), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_bgr_to_i420_equals_cv2(size):
    """... the chroma of the top-left pixel of each 2 x 2 block included (no averaging)."""
    w, h = size
    frame = np.random.default_rng(2).integers(0, 256, (h, w, 3), np.uint8)
    y, u, v = cvtref.rgb_to_yuv(frame, 1, 1, "BGR8")
    assert np.array_equal(i420(y, u, v), cv2.cvtColor(frame, cv2.COLOR_BGR2YUV_I420))


def test_known_answers_equal_cv2():
    for bgr, yuv in (((0, 0, 255), (82, 90, 240)), ((255, 0, 0), (41, 240, 110)), ((255, 255, 255), (235, 128, 128))):
        frame = np.full((4, 4, 3), bgr, np.uint8)
        got = cv2.cvtColor(frame, cv2.COLOR_BGR2YUV_I420)
        assert (int(got[0, 0]), int(got[4, 0]), int(got[5, 0])) == yuv
