"""The numpy statement of cv::goodFeaturesToTrack's selection (tests/gfttref.py) against the CPU oracle (oracle/vso_gftt.cpp),
and the tie pictures of tests/gftt_tie_inputs.py against what they are for.  Every comparison is exact.  The statement is
written from OpenCV's definition, the oracle from its loops (a sort with greaterThanPtr, the grid of cells): a difference
means one of the two misreads goodFeaturesToTrack.  tests/test_gpu_gftt_ties.py holds the HIP kernels to both.

The pictures fail HERE, on the CPU, when they stop being degenerate (another generator, another oracle): the GPU file would
otherwise go on passing on pictures without a tie in them."""
import numpy as np
import pytest

import gfttref
import gftt_tie_inputs as ties
from vsamd import synth

_maps = {}


def eig_map(oracle, name, bs):
    if (name, bs) not in _maps:
        e = oracle.min_eigen(ties.picture(name), bs)
        e.setflags(write=False)
        _maps[(name, bs)] = e
    return _maps[(name, bs)]


def same_selection(oracle, g, eig, args, bs, what):
    pts, nc = gfttref.select(eig, *args)
    pts_o, nc_o = oracle.gftt(g, *args, bs)
    assert nc == nc_o, (what, args, nc, nc_o)
    assert pts.shape == pts_o.shape and np.array_equal(pts, pts_o), (what, args, len(pts), len(pts_o))
    return pts, nc


@pytest.mark.parametrize("name,bs", ties.CASES)
def test_tie_pictures_hold_what_they_are_for(oracle, name, bs):
    g = ties.picture(name)
    assert g.dtype == np.uint8 and g.shape == ({"tile16": (242, 322), "tile16_vga": (480, 640)}.get(name, (120, 160)))
    total, values, pairs = ties.conditions(name, bs, eig_map(oracle, name, bs))
    assert total == oracle.gftt(g, 1, 1e-4, 0.0, bs)[1]


def test_conditions_reject_a_picture_without_ties(oracle):
    g = np.random.default_rng(5).integers(0, 256, (120, 160), dtype=np.uint8)
    for name in ties.NAMES:
        with pytest.raises(AssertionError):
            ties.conditions(name, 3, oracle.min_eigen(g, 3))


@pytest.mark.parametrize("name,bs", ties.CASES)
def test_selection_on_tie_pictures_equals_the_oracle(oracle, name, bs):
    g, eig = ties.picture(name), eig_map(oracle, name, bs)
    lengths = []
    for args in ties.PARAMS:
        pts, _ = same_selection(oracle, g, eig, args, bs, name)
        lengths.append(len(pts))
    assert lengths[0] >= lengths[3] >= lengths[4] > lengths[5] == 1 and lengths[0] > lengths[4]


def test_order_among_equal_values_is_by_descending_address(oracle):
    """On the plateau the head of the list without a distance test is the plateau read backwards."""
    g, eig = ties.picture("plateau3"), eig_map(oracle, "plateau3", 3)
    h, w = g.shape
    pts, nc = gfttref.select(eig, 4096, 1e-4, 0.0)
    assert nc == (w - 4) * (h - 4)
    ys, xs = np.divmod(np.arange(h * w)[::-1], w)
    keep = (xs >= 2) & (xs < w - 2) & (ys >= 2) & (ys < h - 2)
    want = np.stack([xs[keep], ys[keep]], axis=1)[:4096].astype(np.float32)
    assert np.array_equal(pts, want)
    # and with minDistance 1 nothing is rejected: distinct pixels are at least one apart
    assert np.array_equal(gfttref.select(eig, 4096, 1e-4, 1.0)[0], want)


def test_selection_on_clip_grays_equals_the_oracle(oracle):
    clip = synth.make_clip(synth.SEED_CONFIG1, 320, 240, 6)
    for k in (0, 3):
        g = oracle.analysis_gray(clip[k], 480, 360)
        for bs in (3, 5):
            eig = oracle.min_eigen(g, bs)
            for args in ties.PARAMS:
                same_selection(oracle, g, eig, args, bs, ("clip", k, bs))


def test_selection_on_the_noise_picture_equals_the_oracle(oracle):
    """The picture of test_gftt_many_candidates_chunked_sort (tests/test_gpu_parity.py) with its own arguments."""
    g = np.random.default_rng(99).integers(0, 256, (480, 640), dtype=np.uint8)
    eig = oracle.min_eigen(g, 3)
    pts, nc = same_selection(oracle, g, eig, (3000, 0.0001, 3.0), 3, "noise")
    assert nc > 8192 and len(pts) == 3000
    same_selection(oracle, g, eig, (4096, 1e-4, 0.0), 3, "noise")


def test_plateau_clip_overflows_the_old_list_at_the_analysis_size(oracle):
    """The stream's detector call (200, 0.02, 15.0, block size 3) on the analysis gray of the clip's frames: every interior
    pixel but the ring next to the frame is a candidate, four times what w * h / 4 + 64 holds."""
    w, h = ties.CLIP_SIZE
    clip = ties.plateau_clip()
    assert len(clip) == ties.CLIP_FRAMES and 8 <= len(clip) <= 12
    for k, f in enumerate(clip):
        assert f.shape == (h, w, 3)
        assert np.array_equal(f[:, 3:], f[:, :-3]) and np.array_equal(f[3:], f[:-3]), k        # period 3 both ways
        assert k == 0 or not np.array_equal(f, clip[k - 1])                                    # and it moves
    for k in (0, 5, len(clip) - 1):
        g = oracle.analysis_gray(clip[k], w, h)
        assert np.array_equal(g, clip[k][:, :, 0]), k
        pts, nc = oracle.gftt(g, 200, 0.02, 15.0, 3)
        assert (w - 4) * (h - 5) <= nc <= (w - 2) * (h - 2) and nc > 3 * ties.old_cap(w, h) and len(pts) == 200, (k, nc, len(pts))
    small = oracle.analysis_gray(clip[0], 480, 270)            # the first frame's own detection image
    assert oracle.gftt(small, 200, 0.01, 30.0, 3)[1] > 3 * ties.old_cap(480, 270)


def test_threshold_is_strict_and_taken_in_double():
    eig = np.zeros((5, 7), np.float32)
    eig[2, 2], eig[2, 4] = 8.0, 4.0
    assert len(gfttref.select(eig, 10, 0.5, 0.0)[0]) == 1               # 4 > 8 * 0.5 is false
    assert len(gfttref.select(eig, 10, 0.49, 0.0)[0]) == 2
    eig[0, 0] = 100.0                                                   # the maximum counts where it lies, the frame included
    assert gfttref.select(eig, 10, 0.05, 0.0)[1] == 1 and gfttref.select(eig, 10, 0.01, 0.0)[1] == 2
    assert gfttref.select(np.zeros((5, 7), np.float32), 10, 0.01, 3.0)[1] == 0
