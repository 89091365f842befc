"""The LK tracker computes the Scharr derivatives of its template patch itself, from the staged previous image (k_lk.hip
lk_track); the pyramid writes no derivative images.  What the oracle reads is cv::calcOpticalFlowPyrLK's derivative image:
the Scharr stencil with REFLECT_101 neighbours inside the level image, 0 outside it (copyMakeBorder BORDER_CONSTANT).
These cases put the template patch and its one-pixel rim on every border and corner of every level, for every window
class, on level sizes that are odd or only a few pixels wider than the window, on full-contrast content that drives the
derivatives to their extremes, and with motion that restages the search region.  Points, status and err must be
bit-identical to the oracle's."""
import numpy as np
import pytest

from vsamd import capi, synth

pytestmark = pytest.mark.gpu

WINS = [5, 9, 15, 21, 31]        # window classes: 1, 2, 4, 7 and 16 pixels per lane


def _texture(w, h, seed):
    """Smooth random texture with a full-contrast 4-pixel checkerboard in the upper left quarter and random 0 / 255
    pixels in the lower right one: |dx| and |dy| reach 16 * 255 there."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h, w)).astype(np.float64)
    for _ in range(2):
        g = (g + np.roll(g, 1, 0) + np.roll(g, -1, 0) + np.roll(g, 1, 1) + np.roll(g, -1, 1)) / 5
    g = np.clip((g - 128) * 3 + 128, 0, 255)
    y, x = np.mgrid[0:h, 0:w]
    board = ((x // 4 + y // 4) & 1) * 255
    q = (x < w // 2) & (y < h // 2)
    g[q] = board[q]
    r = (x >= w // 2) & (y >= h // 2)
    g[r] = rng.integers(0, 2, int(r.sum())) * 255
    return np.ascontiguousarray(g.astype(np.uint8))


def _levels(w, h, win, max_level):
    """buildOpticalFlowPyramid's level sizes: stop when the next level would not exceed the window."""
    sizes = [(w, h)]
    for _ in range(max_level):
        nw, nh = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= win or nh <= win:
            break
        sizes.append((nw, nh))
    return sizes


def _border_points(w, h, win, max_level):
    """Points whose template window at level l starts at each of the positions that put the patch or its rim on a border
    (left / top edge -win .. 1, right / bottom edge from size - win - 1 to size - 1), every pairing of a column with a row:
    edges, corners and the interior next to them, at every level."""
    half = (win - 1) * 0.5
    pts = []
    for l, (lw, lh) in enumerate(_levels(w, h, win, max_level)):
        xs = sorted({e for e in (-win, -win + 1, -2, -1, 0, 1, 2, lw // 2, lw - win - 2, lw - win - 1, lw - win, lw - win + 1, lw - 2, lw - 1)
                     if -win <= e < lw})
        ys = sorted({e for e in (-win, -1, 0, 1, lh // 2, lh - win - 2, lh - win - 1, lh - win, lh - 1) if -win <= e < lh})
        for ex in xs:
            for ey in ys:
                pts.append(((ex + half + 0.37) * (1 << l), (ey + half + 0.61) * (1 << l)))
    return np.array(pts, np.float32)


def _check(gpu, oracle, g0, g1, pts, win, max_level, iters=20, eps=0.03):
    no, so, eo = oracle.pyr_lk(g0, g1, pts, win, max_level, iters, eps)
    ng, sg, eg = gpu.pyr_lk(g0, g1, pts, win, max_level, iters, eps)
    assert np.array_equal(sg, so)
    assert np.array_equal(ng.view(np.uint32), no.view(np.uint32))
    assert np.array_equal(eg.view(np.uint32), eo.view(np.uint32))
    return no, so


@pytest.mark.parametrize("win", WINS)
@pytest.mark.parametrize("odd", [False, True])
def test_lk_patches_on_every_border_of_every_level(gpu, oracle, win, odd):
    """Top level only a few pixels wider than the window (win + 3 .. win + 5); with `odd`, odd sizes at every level."""
    w, h = 4 * win + 11, 4 * win + 17
    if odd:
        w, h = w + 2, h - 6              # 4 win + 13 -> 2 win + 7 -> win + 4, 4 win + 11 -> 2 win + 6 -> win + 3
    g0 = _texture(w, h, 11 + win)
    g1 = np.roll(np.roll(g0, 2, axis=0), -1, axis=1)
    g1[h // 3:h // 3 + 5] = 255 - g1[h // 3:h // 3 + 5]               # not a pure shift: some tracks move off
    pts = _border_points(w, h, win, 2)
    assert len(_levels(w, h, win, 2)) == 3
    _, so = _check(gpu, oracle, g0, g1, pts, win, 2)
    assert so.any() and not so.all()


@pytest.mark.parametrize("win", WINS)
def test_lk_full_contrast_checkerboard(gpu, oracle, win):
    """A 0 / 255 checkerboard of 3- and 4-pixel squares over the whole frame, moved by a few pixels: every window holds
    derivatives of the largest magnitude, on the borders too."""
    w, h = 161, 123
    y, x = np.mgrid[0:h, 0:w]
    g0 = np.ascontiguousarray((((x // 4 + y // 3) & 1) * 255).astype(np.uint8))
    g1 = np.ascontiguousarray(np.roll(np.roll(g0, 1, axis=0), 3, axis=1))
    rng = np.random.default_rng(win)
    pts = np.vstack([_border_points(w, h, win, 1),
                     np.stack([rng.uniform(-5, w + 5, 200), rng.uniform(-5, h + 5, 200)], 1).astype(np.float32)])
    _check(gpu, oracle, g0, g1, pts, win, 1)


@pytest.mark.parametrize("win", WINS)
@pytest.mark.parametrize("shift", [(11, -9), (-25, 14)])
def test_lk_large_motion_next_to_the_borders(gpu, oracle, win, shift):
    """Motion of more than LK_MARGIN pixels: the search region is staged again, here for windows whose template patch
    sits on a border (so the template takes the reflected staging and the masked derivatives while the region moves)."""
    w, h = 6 * win + 21, 5 * win + 13
    g0 = _texture(w, h, 5 * win + 1)
    g1 = np.ascontiguousarray(np.roll(np.roll(g0, shift[1], axis=0), shift[0], axis=1))
    pts = _border_points(w, h, win, 2)
    no, so = _check(gpu, oracle, g0, g1, pts, win, 2)
    moved = np.abs(no - pts).max(axis=1)[so.astype(bool)]
    assert moved.size and moved.max() > 6                               # the case is what it claims to be


def test_batch_mode_at_the_bench_shapes_matches_per_frame_pipeline(gpu):
    """1920x1080 BGR, batches of 64, 200 corners, 3 levels, 21x21 windows (bench.py's configs[1]): the batch pyramid is
    pyrDown-only, the tracker derives the gradients in both pipelines.  Tracks after every batch and every output frame
    equal the per-frame pipeline's."""
    W, H, NF, B = 1920, 1080, 32, 64
    n = 2 * B + 8
    clip = synth.make_clip_dev(gpu, synth.SEED_CONFIG2, W, H, NF)
    fb = W * H * 3
    p = gpu.params(max_corners=200, lk_win_size=21, lk_max_level=2, lk_max_iters=20, lk_epsilon=0.03, smoothing_radius=9)
    s1, s2 = gpu.stabilizer(p), gpu.stabilizer(p)
    s2.set_batch(B)
    d_ref, d_got = capi.DevBuf(gpu, fb * (n + 4)), capi.DevBuf(gpu, fb * (n + 4))
    order = [i % NF if (i // NF) % 2 == 0 else NF - 1 - i % NF for i in range(n)]
    k1 = k2 = checked = 0
    for i in range(n):
        src = clip.ptr + order[i] * fb
        k1 += s1.push_dev(src, W, H, W * 3, capi.FMT_BGR8, d_ref.ptr + k1 * fb, W * 3)
        k2 += s2.push_dev(src, W, H, W * 3, capi.FMT_BGR8, d_got.ptr + k2 * fb, W * 3)
        if i % B == B - 1:                   # the batch has just run: its last frame's tracks against the per-frame pipeline's
            s1.sync(); s2.sync()
            a, b = s1.debug_arrays(), s2.debug_arrays()
            for key in ("prev", "curr", "status", "inliers", "gray"):
                assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), (i, key)
            assert a["status"].sum() > 100
            checked += 1
    while s1.flush_dev(d_ref.ptr + k1 * fb, W * 3):
        k1 += 1
    while s2.flush_dev(d_got.ptr + k2 * fb, W * 3):
        k2 += 1
    s1.sync(); s2.sync()
    assert checked == 2 and k1 == k2 == n
    for j in range(0, n, 16):                # (in chunks: n frames of 1080p BGR are 850 MB per side)
        m = min(16, n - j)
        assert np.array_equal(d_ref.download((m, H, W, 3), np.uint8, j * fb), d_got.download((m, H, W, 3), np.uint8, j * fb)), j
    s1.close(); s2.close()
    for b in (d_ref, d_got, clip):
        b.free()
