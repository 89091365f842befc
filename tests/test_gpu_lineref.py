"""The HIP kernels of the roll stage's line search (k_roll.hip: Sobel, Canny on bit planes, edge lists, both Hough accumulators, peaks,
the sort, the angle statistics) and of the zoom stage's content mask (k_azc.hip) against the numpy / scipy statements of
tests/lineref.py - no oracle in between (tests/test_lineref_oracle.py holds the oracle to the same statements on the CPU).

Every comparison is exact: edge maps and masks with array_equal, line lists as bit patterns, the roll objects' state() as tuples.
Rotated pixels stay with test_roll.py; these tests compare what the line search found."""
import functools

import numpy as np
import pytest

from vsamd import capi

import i010_inputs
import lineref
import lineref_cases as cases
import p010_chain_inputs
import ref16_geom
from lineref_cases import THETA

pytestmark = pytest.mark.gpu


def same_lines(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- vs_op_canny -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_canny_equals_the_statement(gpu, shape, kind):
    g = cases.gray(kind, shape)
    for lo, hi in cases.THRESHOLDS:
        ref = lineref.canny(g, lo, hi)
        got = gpu.canny(g, lo, hi)
        assert np.array_equal(ref, got), (lo, hi, int((ref != got).sum()))
    assert min(shape) < 62 or lineref.canny(g, 10, 30).any()


def test_canny_both_diagonals(gpu):
    y, x = np.mgrid[:40, :40]
    for g in (np.where(x + y > 40, 200, 20), np.where(x - y > 0, 200, 20)):
        g = g.astype(np.uint8)
        ref = lineref.canny(g, 50, 150)
        assert ref[5:35, 5:35].any() and np.array_equal(ref, gpu.canny(g, 50, 150))


def test_canny_pitched_input_and_result(gpu):
    """Input and edge pitch differ from the width and from each other; the poison behind the rows of the result stays."""
    h, w = 62, 65
    g = cases.gray("noisy", (h, w))
    pitch, epitch = w + 37, w + 11
    buf = np.full((h, pitch), 0xA5, np.uint8)
    buf[:, :w] = g
    d_in = capi.DevBuf.from_array(gpu, buf)
    d_out = capi.DevBuf.from_array(gpu, np.full((h, epitch), 0x5A, np.uint8))
    gpu.check(gpu.lib.vs_op_canny(d_in.ptr, pitch, w, h, 10.0, 30.0, d_out.ptr, epitch, None))
    gpu.sync()
    got = d_out.download((h, epitch), np.uint8)
    ref = lineref.canny(g, 10, 30)
    assert ref.any() and np.array_equal(got[:, :w], ref) and (got[:, w:] == 0x5A).all()


def test_canny_growth_along_the_serpentine(gpu):
    """Growth across the 62-row bands and through several groups of passes."""
    lo, hi = cases.SERPENTINE_THRESHOLDS
    ref = lineref.canny(cases.serpentine(), lo, hi)
    row, cols = cases.SERPENTINE_FAR_END
    assert any(ref[row, c] for c in cols)
    assert np.array_equal(ref, gpu.canny(cases.serpentine(), lo, hi))
    assert not gpu.canny(cases.serpentine(strong=False), lo, hi).any()


def test_canny_on_rendered_frames(gpu):
    for g in cases.rendered_grays():
        ref = lineref.canny(g, 50, 150)
        assert ref.any() and np.array_equal(ref, gpu.canny(g, 50, 150))


# ---- vs_op_hough_lines -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,rho,theta,thr", cases.hough_cases())
def test_hough_equals_the_statement(gpu, shape, rho, theta, thr):
    if shape in cases.TINY:
        for full in (True, False):
            e = cases.tiny_edges(shape, full)
            ref = lineref.hough_lines(e, rho, theta, thr)
            assert len(ref) == cases.TINY_COUNTS[shape][0 if full else 1]
            assert same_lines(ref, gpu.hough_lines(e, rho, theta, thr))
        return
    e = cases.edge_map(shape)
    ref = lineref.hough_lines(e, rho, theta, thr)
    assert 0 < len(ref) < lineref.HOUGH_CAP
    assert same_lines(ref, gpu.hough_lines(e, rho, theta, thr))


def _hough_pitched(gpu, e, pitch, rho, theta, thr, max_lines=lineref.HOUGH_CAP):
    h, w = e.shape
    buf = np.full((h, pitch), 255, np.uint8)              # (poison that would be an edge if it were read)
    buf[:, :w] = e
    d_in = capi.DevBuf.from_array(gpu, buf)
    d_lines, d_cnt = capi.DevBuf(gpu, max_lines * 8), capi.DevBuf(gpu, 16)
    gpu.check(gpu.lib.vs_op_hough_lines(d_in.ptr, pitch, w, h, rho, theta, thr, d_lines.ptr, max_lines, d_cnt.ptr, None))
    gpu.sync()
    n = int(d_cnt.download((1,), np.int32)[0])
    return d_lines.download((max_lines, 2), np.float32)[:n].copy()


@pytest.mark.parametrize("shape", [(135, 240), (62, 65)])
def test_hough_edge_map_on_an_odd_pitch(gpu, shape):
    """Rows that start at every alignment: the edge list's 8-byte loads and its byte-by-byte path."""
    e = cases.edge_map(shape)
    thr = cases.HOUGH_SHAPES[shape][0]
    ref = lineref.hough_lines(e, 1.0, THETA, thr)
    assert 0 < len(ref) < lineref.HOUGH_CAP
    assert same_lines(ref, _hough_pitched(gpu, e, shape[1] + 37, 1.0, THETA, thr))


def test_hough_accum_kernel_at_a_fine_rho(gpu):
    """rho = 0.1 on 520 x 260: rows of 15610 cells do not fit LDS, the votes go to the accumulator in HBM (hough_accum_kernel)."""
    rho, theta, thr = cases.FINE_RHO
    assert lineref.hough_geometry(520, 260, rho, theta)[1] * 4 > 60 * 1024
    ref = lineref.hough_lines(cases.fine_rho_edges(), rho, theta, thr)
    assert len(ref) == 5
    assert same_lines(ref, gpu.hough_lines(cases.fine_rho_edges(), rho, theta, thr))


def test_hough_empty_map(gpu):
    e = np.zeros((64, 67), np.uint8)
    assert len(lineref.hough_lines(e, 1.0, THETA, 0)) == 0 and len(gpu.hough_lines(e, 1.0, THETA, 0)) == 0


# ---- roll objects: state() against roll_step ---------------------------------------------------------------------------------------
def _gpu_params(gpu, **kw):
    return gpu.roll_params(**{k: (float(v) if isinstance(v, np.floating) else v) for k, v in kw.items()})


@functools.lru_cache(maxsize=None)
def _nv12_states(scale):
    h = cases.ROLL_SIZE[1]
    p = lineref.roll_params(scale_factor=scale, hough_threshold=cases.roll_threshold(scale))
    return lineref.roll_run([lineref.analysis_image(s[:h], scale) for s in cases.roll_surfaces()], p)


@functools.lru_cache(maxsize=None)
def _bgr_states(scale):
    p = lineref.roll_params(scale_factor=scale, hough_threshold=cases.roll_threshold(scale))
    return lineref.roll_run([lineref.analysis_image(f, scale) for f in cases.roll_frames()], p)


def _run_async(gpu, surfs, w, h, params, call="nv12", sample_bytes=1):
    """The surfaces through the asynchronous entry point without a sync in between; the state after the last one."""
    host = np.stack(surfs)
    sb = host[0].nbytes
    d_in, d_out = capi.DevBuf.from_array(gpu, host), capi.DevBuf(gpu, host.nbytes)
    rg = gpu.roll_correction(_gpu_params(gpu, **params))
    pitch = w * sample_bytes
    try:
        for i in range(len(surfs)):
            if call == "nv12":
                rg.correct_nv12_dev(d_in.ptr + i * sb, w, h, pitch, d_out.ptr + i * sb, pitch)
            elif call == "p010":
                rg.correct_p010_dev(d_in.ptr + i * sb, w, h, pitch, d_out.ptr + i * sb, pitch)
            else:
                lay = capi.i420_layout(pitch)
                rg.correct_i420_dev(call, d_in.ptr + i * sb, w, h, lay, d_out.ptr + i * sb, lay)
        rg.sync()
        return rg.state()
    finally:
        rg.close()
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("scale", [0.5, 1.0])
def test_roll_synchronous_bgr_state(gpu, scale):
    ref = _bgr_states(scale)
    assert ref[3][2] == 0 and ref[6][2] > 0 and ref[6][3] == 0 and max(s[3] for s in ref) >= 2
    rg = gpu.roll_correction(gpu.roll_params(scale_factor=scale, hough_threshold=cases.roll_threshold(scale)))
    w, h = cases.ROLL_SIZE
    d_in, d_out = capi.DevBuf(gpu, w * h * 3), capi.DevBuf(gpu, w * h * 3)
    for i, f in enumerate(cases.roll_frames()):
        if i == 4:                       # once through the device entry point
            d_in.upload(f)
            rg.correct_dev(d_in.ptr, w, h, w * 3, d_out.ptr, w * 3)
            rg.sync()
        else:
            rg.correct(f)
        assert rg.state() == ref[i], i
    rg.close()


@pytest.mark.parametrize("scale", [0.25, 0.5, 1.0])
def test_roll_asynchronous_nv12_state(gpu, scale):
    """Eleven surfaces without a sync: a batch of eight and one of three (blockIdx.z, counters cleared once per batch), the flat and the
    filtered-out frame inside; and the first seven alone, which end on the frame whose lines all fall outside the filter."""
    ref = _nv12_states(scale)
    assert ref[3][2] == 0 and ref[6][2] > 0 and ref[6][3] == 0 and ref[-1][3] > 0
    w, h = cases.ROLL_SIZE
    p = dict(scale_factor=scale, hough_threshold=cases.roll_threshold(scale))
    assert _run_async(gpu, cases.roll_surfaces(), w, h, p) == ref[-1]
    assert _run_async(gpu, cases.roll_surfaces()[:7], w, h, p) == ref[6]


def test_roll_asynchronous_other_parameters(gpu):
    h = cases.ROLL_SIZE[1]
    p = dict(scale_factor=0.5, hough_threshold=cases.roll_threshold(0.5), **cases.OTHER_PARAMS)
    ref = lineref.roll_run([lineref.analysis_image(s[:h], 0.5) for s in cases.roll_surfaces()], lineref.roll_params(**p))
    assert any(0 < s[3] < s[2] for s in ref)
    assert _run_async(gpu, cases.roll_surfaces(), cases.ROLL_SIZE[0], h, p) == ref[-1]


def test_roll_asynchronous_redo_branch_on_the_serpentine(gpu):
    """The growth along the serpentine outlasts the batch's twelve hysteresis passes: every frame is finished and searched again."""
    ref = cases.serpentine_states(6)
    assert ref[-1][2] > 4
    h, w = cases.serpentine().shape
    assert _run_async(gpu, [cases.gray_surface(cases.serpentine())] * 6, w, h, cases.SERPENTINE_ROLL) == ref[-1]


def test_roll_synchronous_redo_on_the_serpentine(gpu):
    ref = cases.serpentine_states(2)
    rg = gpu.roll_correction(gpu.roll_params(**cases.SERPENTINE_ROLL))
    f = np.repeat(cases.serpentine()[:, :, None], 3, axis=2)
    for i in range(2):
        rg.correct(f)
        assert rg.state() == ref[i]
    rg.close()


def test_roll_asynchronous_hough_accum_kernel_at_a_fine_rho(gpu):
    """hough_rho = 0.1 at 520 x 260, scale 1: the accumulator in HBM with several frames per launch."""
    w, h = cases.FINE_RHO_SIZE
    surfs = cases.fine_rho_surfaces()
    ref = lineref.roll_run([s[:h] for s in surfs], lineref.roll_params(**dict(cases.FINE_RHO_ROLL, hough_rho=np.float32(0.1))))
    assert all(0 < s[2] < lineref.HOUGH_CAP for s in ref) and len({s[1] for s in ref}) > 2
    assert _run_async(gpu, surfs, w, h, cases.FINE_RHO_ROLL) == ref[-1]
    assert _run_async(gpu, surfs[:3], w, h, cases.FINE_RHO_ROLL) == ref[2]


def test_roll_p010_state(gpu):
    """P010 surfaces: the line search sees the luma samples' high bytes."""
    (w, h), slope, _ = p010_chain_inputs.ROLL_CASES[0]
    surfs = p010_chain_inputs.roll_surfaces((w, h), slope)
    p = dict(hough_threshold=60)          # (160 x 90 analysis image: every horizon gives lines)
    ref = lineref.roll_run([lineref.analysis_image(ref16_geom.high_bytes(s)[:h], 0.25) for s in surfs], lineref.roll_params(**p))
    assert ref[-1][0] != 0.0 and ref[-1][3] > 0 and ref[5][2] == 0
    assert _run_async(gpu, surfs, w, h, p, call="p010", sample_bytes=2) == ref[-1]


def test_roll_i010_state(gpu):
    """I010 frames: the line search sees min(sample >> 2, 255); some samples lie above the 10-bit range."""
    (w, h), slope, _ = p010_chain_inputs.ROLL_CASES[0]
    rng = np.random.default_rng(77)
    frames = []
    for s in p010_chain_inputs.roll_surfaces((w, h), slope):
        f = i010_inputs.random_frame(5, w, h)
        f[:h] = (s[:h] >> 6) | (rng.random((h, w)) < 0.001) * np.uint16(0x4000)
        frames.append(f)
    p = dict(hough_threshold=60)          # (160 x 90 analysis image: every horizon gives lines)
    ref = lineref.roll_run([lineref.analysis_image(i010_inputs.analysis_byte(f[:h], 10), 0.25) for f in frames], lineref.roll_params(**p))
    assert ref[-1][0] != 0.0 and ref[-1][3] > 0 and ref[5][2] == 0
    assert _run_async(gpu, frames, w, h, p, call=capi.FMT_I010, sample_bytes=2) == ref[-1]


# ---- the peak cap ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _over_cap_pictures():
    g = cases.over_cap_gray()
    return [g, np.ascontiguousarray(g[:, ::-1]), g]


@functools.lru_cache(maxsize=None)
def _over_cap_states():
    return lineref.roll_run(_over_cap_pictures(), lineref.roll_params(**cases.over_cap_params()))


def test_hough_over_cap_branch_keeps_the_head_of_the_order(gpu):
    """Well over 8192 peaks, the strongest late in a scan of the accumulator: the 8192 lines cv::HoughLines lists first, in its order."""
    e = lineref.canny(cases.over_cap_gray(), *cases.OVER_CAP_CANNY)
    full = lineref.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD)
    assert len(full) > lineref.HOUGH_CAP + 2000 and np.degrees(full[:2, 1]).min() >= 150.0
    ref = lineref.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD, cap=lineref.HOUGH_CAP)
    got = gpu.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD, max_lines=lineref.HOUGH_CAP)
    assert len(got) == lineref.HOUGH_CAP and same_lines(ref, got)
    assert same_lines(got, gpu.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD, max_lines=lineref.HOUGH_CAP))      # the input alone decides
    few = gpu.hough_lines(e, 1.0, THETA, cases.OVER_CAP_THRESHOLD, max_lines=100)
    assert same_lines(ref[:100], few)


def test_roll_over_cap_branch_synchronous(gpu):
    ref = _over_cap_states()
    assert all(s[2] == lineref.HOUGH_CAP and s[3] == lineref.HOUGH_CAP for s in ref)
    rg = gpu.roll_correction(gpu.roll_params(**cases.over_cap_params()))
    for i, g in enumerate(_over_cap_pictures()):
        rg.correct(np.repeat(g[:, :, None], 3, axis=2))
        assert rg.state() == ref[i], i
    rg.close()


def test_roll_over_cap_branch_asynchronous(gpu):
    ref = _over_cap_states()
    h, w = cases.over_cap_gray().shape
    surfs = [cases.gray_surface(g) for g in _over_cap_pictures()]
    assert _run_async(gpu, surfs, w, h, cases.over_cap_params()) == ref[-1]
    assert _run_async(gpu, surfs[:2], w, h, cases.over_cap_params()) == ref[1]


# ---- vs_op_content_mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("shape", cases.MASK_SHAPES)
def test_content_mask_equals_the_statement(gpu, shape, cn):
    img = cases.mask_picture(shape, cn)
    ref = lineref.content_mask(img)
    if shape[0] >= 9 and shape[1] >= 9:
        assert 0 < int((ref != 0).sum()) < ref.size
    assert np.array_equal(ref, gpu.content_mask(img))
