"""The numpy / scipy statements of tests/lineref.py against the CPU oracle (oracle/vso_roll.cpp, oracle/vso_azc.cpp): Canny, HoughLines,
the roll stage's state over frame sequences and the zoom stage's content mask.  Every comparison is exact.  The statements are written
from OpenCV's definitions, the oracle from its loops: a difference means one of the two misreads cv::Canny / cv::HoughLines /
cv::morphologyEx (docs/opencv_semantics.md says which was wrong the last time).  tests/test_gpu_lineref.py holds the HIP kernels to
the same statements without the oracle in between.

Every case states that it is not trivial: edge pixels, lines, set and unset mask pixels wherever the shape allows."""
import math

import numpy as np
import pytest

import lineref
import lineref_cases as cases
from lineref_cases import THETA


def same_lines(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- Sobel, Canny ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_sobel_equals_the_oracle(oracle, shape):
    for kind in cases.KINDS:
        g = cases.gray(kind, shape)
        dx, dy = lineref.sobel(g)
        odx, ody = oracle.sobel16(g)
        assert np.array_equal(dx, odx) and np.array_equal(dy, ody), kind


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_canny_equals_the_oracle(oracle, shape, kind):
    g = cases.gray(kind, shape)
    any_edge = False
    for lo, hi in cases.THRESHOLDS:
        ref = lineref.canny(g, lo, hi)
        assert set(np.unique(ref)) <= {0, 255}
        assert np.array_equal(ref, oracle.canny(g, lo, hi)), (lo, hi, int((ref != oracle.canny(g, lo, hi)).sum()))
        any_edge |= bool(ref.any())
    if shape[0] >= 8 and shape[1] >= 8 and (kind == "binary" or shape[0] > 8):
        assert any_edge
    if kind == "noisy" and min(shape) >= 62:
        cand, strong = lineref.canny_candidates(g, 10, 30)
        assert (cand & ~strong).any() and strong.any()          # hysteresis has something to decide


def test_canny_swaps_and_floors_its_thresholds():
    g = cases.gray("noisy", (135, 240))
    assert np.array_equal(lineref.canny(g, 150, 50), lineref.canny(g, 50, 150))
    assert np.array_equal(lineref.canny(g, 10.9, 30.2), lineref.canny(g, 10, 30))
    assert not np.array_equal(lineref.canny(g, 10, 30), lineref.canny(g, 12, 33))


def test_canny_finds_both_diagonals(oracle):
    """A clean 45-degree step in either direction is one thin line: the diagonal sector compares along the gradient (up-left and
    down-right when dx and dy have equal signs), not along the edge, where the magnitudes are equal and nothing is a strict maximum."""
    y, x = np.mgrid[:40, :40]
    for g in (np.where(x + y > 40, 200, 20), np.where(x - y > 0, 200, 20)):
        g = g.astype(np.uint8)
        e = lineref.canny(g, 50, 150)
        inner = e[5:35, 5:35]
        assert inner.any() and (inner != 0).sum(axis=1).max() <= 2
        assert np.array_equal(e, oracle.canny(g, 50, 150))


def test_canny_on_the_serpentine_equals_the_oracle(oracle):
    lo, hi = cases.SERPENTINE_THRESHOLDS
    ref = lineref.canny(cases.serpentine(), lo, hi)
    row, cols = cases.SERPENTINE_FAR_END
    assert any(ref[row, c] for c in cols)                       # the growth reaches the far end
    assert np.array_equal(ref, oracle.canny(cases.serpentine(), lo, hi))
    weak = lineref.canny(cases.serpentine(strong=False), lo, hi)
    assert not weak.any() and not oracle.canny(cases.serpentine(strong=False), lo, hi).any()


def test_canny_on_rendered_frames_equals_the_oracle(oracle):
    for g in cases.rendered_grays():
        ref = lineref.canny(g, 50, 150)
        assert ref.any() and np.array_equal(ref, oracle.canny(g, 50, 150))


# ---- HoughLines --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,rho,theta,thr", cases.hough_cases())
def test_hough_equals_the_oracle(oracle, shape, rho, theta, thr):
    if shape in cases.TINY:
        for full in (True, False):
            e = cases.tiny_edges(shape, full)
            ref = lineref.hough_lines(e, rho, theta, thr)
            assert len(ref) == cases.TINY_COUNTS[shape][0 if full else 1]
            assert same_lines(ref, oracle.hough_lines(e, rho, theta, thr))
        return
    e = cases.edge_map(shape)
    ref = lineref.hough_lines(e, rho, theta, thr)
    assert 0 < len(ref) < lineref.HOUGH_CAP
    assert same_lines(ref, oracle.hough_lines(e, rho, theta, thr))


def test_hough_geometry_of_the_cases():
    assert lineref.hough_geometry(240, 135, 1.0, THETA) == (180, 751)
    assert lineref.hough_geometry(240, 135, 2.0, THETA) == (180, 376)              # 375.5 rounds to even
    assert lineref.hough_geometry(240, 135, 1.0, np.float32(math.pi / 90)) == (90, 751)
    assert lineref.hough_geometry(240, 135, 0.5, np.float32(math.pi / 360)) == (360, 1502)
    assert lineref.hough_geometry(520, 260, 0.1, THETA) == (180, cases.FINE_RHO_NUMRHO)


def test_hough_at_a_fine_rho_equals_the_oracle(oracle):
    rho, theta, thr = cases.FINE_RHO
    ref = lineref.hough_lines(cases.fine_rho_edges(), rho, theta, thr)
    assert len(ref) == 5
    assert same_lines(ref, oracle.hough_lines(cases.fine_rho_edges(), rho, theta, thr))


def test_hough_ties_are_listed_by_accumulator_index():
    e = np.zeros((60, 90), np.uint8)
    e[10, 5:85] = 255
    e[40, 5:85] = 255                  # two lines with 80 votes each at theta 90
    e[5:55, 30] = 255                  # and one of 50 at theta 0
    lines = lineref.hough_lines(e, 1.0, THETA, 45)
    assert lines[:2].tolist() == [[10.0, float(np.float32(90) * THETA)], [40.0, float(np.float32(90) * THETA)]]
    assert [30.0, 0.0] in lines.tolist()


def test_hough_cap_keeps_the_head_of_the_order(oracle):
    """The definition of the library's peak cap: the first 8192 lines of cv::HoughLines' order."""
    e = lineref.canny(cases.over_cap_gray(), *cases.OVER_CAP_CANNY)
    full = lineref.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD)
    assert len(full) > lineref.HOUGH_CAP + 2000
    assert np.degrees(full[:2, 1]).min() >= 150.0               # the strongest peaks come late in a scan by angle
    capped = lineref.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD, cap=lineref.HOUGH_CAP)
    assert len(capped) == lineref.HOUGH_CAP and same_lines(capped, full[:lineref.HOUGH_CAP])
    assert same_lines(full, oracle.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD))


# ---- roll state --------------------------------------------------------------------------------------------------------
def _oracle_states(oracle, frames, nv12, **kw):
    w, h = cases.ROLL_SIZE
    ro = oracle.roll_correction(oracle.roll_params(**kw))
    out = []
    for f in frames:
        ro.correct_nv12(f, w, h) if nv12 else ro.correct(f)
        out.append(ro.state())
    ro.close()
    return out


def _check_sequence(states):
    assert len(states) >= 6
    assert states[3][2] == 0 and states[3][0] == states[2][0] * 0.995 and states[2][0] != 0.0          # flat frame: decay
    assert states[6][2] > 0 and states[6][3] == 0 and states[6][0] == states[5][0] * 0.995                # lines, none inside the filter
    assert all(s[2] < lineref.HOUGH_CAP for s in states) and max(s[3] for s in states) >= 2


@pytest.mark.parametrize("nv12,scale", [(True, 0.25), (True, 0.5), (True, 1.0), (False, 0.5), (False, 1.0)])
def test_roll_state_equals_the_oracle(oracle, nv12, scale):
    h = cases.ROLL_SIZE[1]
    frames = cases.roll_surfaces() if nv12 else cases.roll_frames()
    p = dict(scale_factor=scale, hough_threshold=cases.roll_threshold(scale))
    ref = lineref.roll_run([lineref.analysis_image(f[:h] if nv12 else f, scale) for f in frames], lineref.roll_params(**p))
    _check_sequence(ref)
    assert ref == _oracle_states(oracle, frames, nv12, **p)


@pytest.mark.parametrize("nv12", [True, False])
def test_roll_state_with_other_parameters_equals_the_oracle(oracle, nv12):
    """Another alpha, decay and filter, and no clamp on the step (max_angle_change_deg = 0)."""
    h = cases.ROLL_SIZE[1]
    frames = cases.roll_surfaces() if nv12 else cases.roll_frames()
    p = dict(scale_factor=0.5, hough_threshold=cases.roll_threshold(0.5), **cases.OTHER_PARAMS)
    ref = lineref.roll_run([lineref.analysis_image(f[:h] if nv12 else f, 0.5) for f in frames], lineref.roll_params(**p))
    assert ref[3][0] == ref[2][0] * 0.9 and ref[3][2] == 0
    assert max(abs(b[0] - a[0]) for a, b in zip(ref, ref[1:])) > 0.5           # a step the default clamp would have cut
    assert any(0 < s[3] < s[2] for s in ref)                                    # the filter drops some lines of a frame and keeps others
    assert ref == _oracle_states(oracle, frames, nv12, **p)


def test_roll_state_on_the_serpentine_equals_the_oracle(oracle):
    ref = cases.serpentine_states(2)
    assert ref[0][2] > 4 and ref[0][3] == ref[0][2]
    g = cases.serpentine()
    ro = oracle.roll_correction(oracle.roll_params(**cases.SERPENTINE_ROLL))
    got = []
    for _ in range(2):
        ro.correct(np.repeat(g[:, :, None], 3, axis=2))
        got.append(ro.state())
    assert got == ref


def test_roll_state_over_the_cap_equals_the_oracle(oracle):
    """The roll stage is defined with the library's cap: statistics over the first 8192 lines of the order, n_lines = 8192."""
    g = cases.over_cap_gray()
    pictures = [g, np.ascontiguousarray(g[:, ::-1])]
    ref = lineref.roll_run(pictures, lineref.roll_params(**cases.over_cap_params()))
    assert all(s[2] == lineref.HOUGH_CAP and s[3] == lineref.HOUGH_CAP for s in ref)
    uncapped = lineref.roll_run(pictures, lineref.roll_params(**cases.over_cap_params()), cap=None)
    assert uncapped[0][2] > lineref.HOUGH_CAP + 2000 and uncapped[0][1] != ref[0][1]
    h, w = g.shape
    for nv12 in (True, False):
        ro = oracle.roll_correction(oracle.roll_params(**cases.over_cap_params()))
        for i, pic in enumerate(pictures):
            ro.correct_nv12(cases.gray_surface(pic), w, h) if nv12 else ro.correct(np.repeat(pic[:, :, None], 3, axis=2))
            assert ro.state() == ref[i], (nv12, i)
        ro.close()


# ---- content mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("shape", cases.MASK_SHAPES)
def test_content_mask_equals_the_oracle(oracle, shape, cn):
    img = cases.mask_picture(shape, cn)
    ref = lineref.content_mask(img)
    if shape[0] >= 9 and shape[1] >= 9:
        assert 0 < int((ref != 0).sum()) < ref.size
    assert np.array_equal(ref, oracle.content_mask(img))


def test_content_mask_closes_gaps_and_ignores_what_lies_outside():
    g = np.zeros((9, 16), np.uint8)
    g[:, :5] = 9
    g[:, 9:] = 9                       # a gap of four pixels: the dilation fills it from both sides
    assert lineref.content_mask(g).all()
    g[:, 5:11] = 0                     # six pixels: stays open
    m = lineref.content_mask(g)
    assert not m[:, 5:11].any() and m[:, :5].all() and m[:, 11:].all()
    one = np.zeros((5, 5), np.uint8)
    one[0, 0] = 2                      # a corner pixel survives its own closing: the erosion does not see the outside as empty
    assert lineref.content_mask(one)[0, 0] == 255 and (lineref.content_mask(one) != 0).sum() == 1
    assert not lineref.content_mask(np.ones((5, 5), np.uint8)).any()          # 1 is not above the threshold
