"""The min-eigenvalue column walk (k_gftt.hip: min_eigen_walk3 and the two-pixel frame of thin tiles around it) on a real
MI355X, bit for bit against the CPU oracle.

The geometry the sizes straddle: block size 3 and an image of at least 64 x 5 take the walk - strips of 60 output columns
(64 gray columns, the last strip of a row moved left to end at the image's edge) and 32 output rows (36 gray rows, three per
trip of the loop) over the outputs [2, w-2) x [2, h-2); the frame is done by 128 x 2 and 2 x 128 tiles.  Smaller images and
other block sizes take the tile kernel.  A wrong direction of the walk's lane shifts mirrors dx and the row sums: every
picture here but the flat one would show it.
"""
import numpy as np
import pytest

import roi
from test_gpu_roi import Call, same
from test_min_eigen_walk_cpu import residue_image
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

R, SW = 32, 60                   # output rows and columns of a strip
# (w, h): below the walk's minimum; the minimum; one strip exactly (64 = 60 + 4) and +- 1 column; two strips (124) and + 1;
# heights of R - 1, R, R + 1 and 2R + 3 output rows (+ 4); 125 x 70; the largest
SIZES = [(3, 3), (5, 4), (64, 5), (63, R + 4), (64, R + 3), (65, R + 4), (2 * SW + 4, R + 5), (2 * SW + 5, 2 * R + 7), (125, 70),
         (200, 140)]
ARGS = (100, 0.02, 5.0)
_cache = {}


def image(w, h):
    """Noise on a ramp: corners everywhere, the frame included."""
    if (w, h) not in _cache:
        rng = np.random.default_rng(roi.case_seed("walk", w, h))
        ramp = np.add.outer(np.arange(h) * 2, np.arange(w)) % 200
        g = (ramp + rng.integers(0, 56, (h, w))).astype(np.uint8)
        g.setflags(write=False)
        _cache[(w, h)] = g
    return _cache[(w, h)]


def reference(oracle, key, g, bs=3):
    if ("ref", key, bs) not in _cache:
        eig = oracle.min_eigen(g, bs)
        pts, _ = oracle.gftt(g, *ARGS, bs)
        eig.setflags(write=False)
        pts.setflags(write=False)
        _cache[("ref", key, bs)] = (eig, pts)
    return _cache[("ref", key, bs)]


def check(gpu, oracle, key, g, bs=3):
    eig_o, pts_o = reference(oracle, key, g, bs)
    pts_g, eig_g = gpu.gftt(g, *ARGS, bs, want_eig=True)
    same(eig_g.view(np.uint32), eig_o.view(np.uint32), (key, bs, "eig"))
    assert pts_g.shape == pts_o.shape, (key, bs, len(pts_g), len(pts_o))
    same(pts_g.view(np.uint32), pts_o.view(np.uint32), (key, bs, "corners"))


@pytest.mark.parametrize("w,h", SIZES)
def test_map_and_corners_equal_oracle(gpu, oracle, w, h):
    check(gpu, oracle, (w, h), image(w, h))


def test_flat_image(gpu, oracle):
    g = np.full((R + 9, 70), 140, np.uint8)
    check(gpu, oracle, "flat", g)


def test_residue_image(gpu, oracle):
    """Box sums that are not exact in float64 (tests/test_min_eigen_walk_cpu.py): the walk keeps the oracle's order."""
    check(gpu, oracle, "residue", residue_image())


def test_block_size_5_takes_the_tile_kernel(gpu, oracle):
    check(gpu, oracle, (125, 70), image(125, 70), bs=5)


@pytest.mark.parametrize("layout", ["padded16", "roi_off1", "odd_pitch", "tight_end"])
def test_roi_of_a_larger_surface(gpu, oracle, layout):
    """stride > w, random bytes around the picture and around every output: the maps stay exact and no guard byte changes."""
    max_corners = ARGS[0]
    for w, h in SIZES:
        g = image(w, h)
        what = (layout, w, h)
        src = roi.Surface(roi.LAYOUTS[layout][0], w, h, seed=roi.case_seed("walk_roi", what)).put(g)
        assert src.pitch > w
        d_pts, d_cnt, d_eig = roi.blob(max_corners * 8, 5), roi.blob(4, 6), roi.blob(w * h * 4, 7)
        with Call(gpu, [src], [d_pts, d_cnt, d_eig]) as c:
            outs = c.done(gpu.lib.vs_op_gftt(src.ptr, src.pitch, w, h, max_corners, ARGS[1], ARGS[2], 3, d_pts.ptr, d_cnt.ptr,
                                             d_eig.ptr, None), what)
        eig_o, pts_o = reference(oracle, (w, h), g)
        same(outs[2].view(np.uint32), eig_o.view(np.uint32), what + ("eig",))
        n = int(outs[1].view(np.int32).reshape(-1)[0])
        assert n == len(pts_o), what
        same(outs[0].view(np.float32).reshape(-1, 2)[:n].view(np.uint32), pts_o.view(np.uint32), what + ("corners",))


@pytest.mark.parametrize("w,h", [(250, 140), (384, 216)])
def test_batch_stream_equals_oracle(gpu, oracle, w, h):
    """min_eigen_batch_kernel: a stream in batch mode (8 frames a step, zero-copy), 40 pushes; the analysis images are
    125 x 70 and 192 x 108.  Every frame the stream has handed out equals the oracle's for the same pushes, byte for byte."""
    n = 40
    clip = synth.make_clip(synth.SEED_CONFIG1 + 3, w, h, n)
    p_g, p_o = gpu.params(smoothing_radius=6), oracle.params(smoothing_radius=6)
    s, so = gpu.stabilizer(p_g), oracle.stabilizer(p_o)
    s.set_batch(8)
    s.set_zero_copy(True)
    fb = clip[0].nbytes
    d_in, d_out = capi.DevBuf(gpu, fb * n), capi.DevBuf(gpu, fb * (n + 1))
    k, ref = 0, []
    for i, f in enumerate(clip):
        d_in.upload(f, i * fb)
        k += s.push_dev(d_in.ptr + i * fb, w, h, w * 3, capi.FMT_BGR8, d_out.ptr + k * fb, w * 3)
        r = so.push(f)
        if r is not None:
            ref.append(r)
    s.sync()
    m = min(k, len(ref))
    assert m >= 16, (k, len(ref))
    got = d_out.download((m, h, w, 3), np.uint8)
    for j in range(m):
        assert np.array_equal(got[j], ref[j]), (w, h, "output %d of %d" % (j, m))
    s.close()
    d_in.free()
    d_out.free()
