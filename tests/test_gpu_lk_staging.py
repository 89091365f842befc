"""The LK tracker stages interior template patches and search regions with unaligned dword loads (k_lk.hip lk_track): PP / 4
dwords per patch row, RD = ceil(RW / 4) dwords per region row at an LDS row pitch of 4 RD.  A region that is inside the
image by bytes but whose last dword column would leave the row, and everything that touches a border, takes a byte walk.
The first butterfly steps of the wave sums run in 32 bits.

Points, status and err of vs_op_pyr_lk must equal the oracle's bit for bit: no tolerance, no point left out.

The inputs are checked too, with the kernel's own inequalities restated in numpy (_qualifies): in the 320 x 240 cases at
least three quarters of the points take the dword path at every level, and the points that do not are the hazard points
placed for that purpose.  For a static pair (next == prev) the restatement is exact at every level: the tracker's b vector is
exactly zero, so a level's search region starts at the template's own position.  For the shifted pair it is exact for
the patches and for the top level's regions; below the top level it uses the nominal flow (the shift, halved per level)."""
import numpy as np
import pytest

from vsamd import capi, synth

pytestmark = pytest.mark.gpu

MARGIN = 6                       # LK_MARGIN
SHIFT = (9.3, -7.6)
BASE_W, BASE_H = 323, 240


def _levels(w, h, win, max_level):
    """buildOpticalFlowPyramid's level sizes: stop when the next level would not exceed the window."""
    sizes = [(w, h)]
    for _ in range(max_level):
        nw, nh = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= win or nh <= win:
            break
        sizes.append((nw, nh))
    return sizes


def _geometry(win):
    PW = win + 1
    PP = (PW + 2 + 3) & ~3
    RW = win + 1 + 2 * MARGIN
    RP = 4 * ((RW + 3) // 4)
    return PW, PP, RW, RP


def _qualifies(pts, w, h, win, max_level, flow=(0.0, 0.0)):
    """Per level: (patch staged as dwords, region staged as dwords at the level's first staging, region inside by the byte
    test), from lk_track's conditions in float32 as the kernel evaluates them.  `flow`: the guess at level 0 in pixels."""
    PW, PP, RW, RP = _geometry(win)
    half = np.float32((win - 1) * 0.5)
    sizes = _levels(w, h, win, max_level)
    top = len(sizes) - 1
    out = []
    for l, (lw, lh) in enumerate(sizes):
        scale = np.float32(1.0 / (1 << l))
        px = pts[:, 0].astype(np.float32) * scale - half
        py = pts[:, 1].astype(np.float32) * scale - half
        ipx, ipy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        patch = (ipx >= 1) & (ipy >= 1) & (ipx - 1 + PP <= lw) & (ipy + PW + 1 <= lh)
        fx, fy = (0.0, 0.0) if l == top else (flow[0] / (1 << l), flow[1] / (1 << l))
        rx0 = np.floor(px + np.float32(fx)).astype(np.int64) - MARGIN
        ry0 = np.floor(py + np.float32(fy)).astype(np.int64) - MARGIN
        rows = (rx0 >= 0) & (ry0 >= 0) & (ry0 + RW <= lh)
        out.append((patch, rows & (rx0 + RP <= lw), rows & (rx0 + RW <= lw)))
    return out


def _pair(w, shifted):
    """A smooth texture of BASE_W x BASE_H cropped to w columns, and either itself or the same content moved by SHIFT
    (bilinear, from a larger canvas, so no border is invented)."""
    rng = np.random.default_rng(20)
    pad = 32
    B = rng.integers(0, 256, (BASE_H + 2 * pad, BASE_W + 2 * pad)).astype(np.float64)
    for _ in range(3):
        B = (B + np.roll(B, 1, 0) + np.roll(B, -1, 0) + np.roll(B, 1, 1) + np.roll(B, -1, 1)) / 5
    B = np.clip((B - 128) * 4 + 128, 0, 255)
    g0 = np.ascontiguousarray(np.rint(B[pad:pad + BASE_H, pad:pad + w]).astype(np.uint8))
    if not shifted:
        return g0, g0.copy()
    ox, oy = pad - SHIFT[0], pad - SHIFT[1]              # g1(x, y) = g0(x - sx, y - sy)
    ix, iy = int(np.floor(ox)), int(np.floor(oy))
    ax, ay = ox - ix, oy - iy
    S = lambda dy, dx: B[iy + dy:iy + dy + BASE_H, ix + dx:ix + dx + w]
    g1 = (1 - ay) * ((1 - ax) * S(0, 0) + ax * S(0, 1)) + ay * ((1 - ax) * S(1, 0) + ax * S(1, 1))
    return g0, np.ascontiguousarray(np.rint(g1).astype(np.uint8))


def _grid(w, h, win, max_level):
    """200 points of a jittered 5-pixel grid, taken evenly from those that the inequalities put on the dword path at every
    level, for the static and for the shifted pair."""
    rng = np.random.default_rng(win)
    xs, ys = np.meshgrid(np.arange(2.5, w, 5.0), np.arange(2.5, h, 5.0))
    cand = np.stack([xs.ravel(), ys.ravel()], 1) + rng.uniform(-2.0, 2.0, (xs.size, 2))
    cand = cand.astype(np.float32)
    ok = np.ones(len(cand), bool)
    for flow in ((0.0, 0.0), SHIFT):
        for patch, region, _ in _qualifies(cand, w, h, win, max_level, flow):
            ok &= patch & region
    cand = cand[ok]
    assert len(cand) >= 200, len(cand)
    return cand[np.linspace(0, len(cand) - 1, 200).astype(int)]


def _hazards(w, h, win, max_level):
    """name -> points: within 2 px of each image edge, the top-left corner, and (where 4 RD > RW) the columns whose region
    is inside the level image by the byte test but not by the dword test, at every level."""
    PW, PP, RW, RP = _geometry(win)
    half = (win - 1) * 0.5
    hz = {
        "left": [(0.4, h * 0.5), (1.7, h * 0.4)],
        "right": [(w - 0.6, h * 0.5), (w - 2.3, h * 0.6)],
        "top": [(w * 0.5, 0.3), (w * 0.4, 1.8)],
        "bottom": [(w * 0.5, h - 0.7), (w * 0.6, h - 2.2)],
        "corner": [(0.2, 0.6), (1.5, 1.1), (3.2, 2.7)],
    }
    edge = []
    for l, (lw, lh) in enumerate(_levels(w, h, win, max_level)):
        for rx0 in range(lw - RP + 1, lw - RW + 1):                       # lw - RW >= rx0 > lw - 4 RD
            edge.append(((rx0 + MARGIN + half + 0.4) * (1 << l), (lh // 2 + 0.3) * (1 << l)))
    if edge:
        hz["dword-edge"] = edge
    return {k: np.array(v, np.float32) for k, v in hz.items()}


def _check(gpu, oracle, g0, g1, pts, win, max_level, iters=20, eps=0.03):
    no, so, eo = oracle.pyr_lk(g0, g1, pts, win, max_level, iters, eps)
    ng, sg, eg = gpu.pyr_lk(g0, g1, pts, win, max_level, iters, eps)
    assert np.array_equal(sg, so)
    assert np.array_equal(ng.view(np.uint32), no.view(np.uint32))
    assert np.array_equal(eg.view(np.uint32), eo.view(np.uint32))
    return no, so


def _points_and_precondition(w, h, win, max_level, shifted):
    grid, hz = _grid(w, h, win, max_level), _hazards(w, h, win, max_level)
    pts = np.vstack([grid] + list(hz.values()))
    n_grid = len(grid)
    q = _qualifies(pts, w, h, win, max_level, SHIFT if shifted else (0.0, 0.0))
    assert len(q) == max_level + 1
    fails = np.zeros(len(pts), bool)
    for patch, region, _ in q:
        fast = patch & region
        assert fast.mean() >= 0.75, fast.mean()
        assert fast[:n_grid].all()
        fails |= ~fast
    assert fails[n_grid:].all() and not fails[:n_grid].any()               # the hazard points, and only they
    if "dword-edge" in hz:                                                 # inside by bytes, not by dwords, at its level
        at = n_grid + sum(len(v) for k, v in hz.items() if k != "dword-edge")
        per_level = len(hz["dword-edge"]) // len(q)
        assert per_level >= 1
        for l, (patch, region, byte_region) in enumerate(_qualifies(pts, w, h, win, max_level)):
            sl = slice(at + l * per_level, at + (l + 1) * per_level)
            assert patch[sl].all() and byte_region[sl].all() and not region[sl].any(), l
    return pts


@pytest.mark.parametrize("win", [15, 21, 31])
@pytest.mark.parametrize("shifted", [False, True], ids=["static", "shifted"])
def test_lk_dword_staging_320x240(gpu, oracle, win, shifted):
    """All three instantiations; 4 RD > RW only for 21 x 21 (34 -> 36), so only that window has dword-edge columns."""
    w, h = 320, 240
    g0, g1 = _pair(w, shifted)
    pts = _points_and_precondition(w, h, win, 2, shifted)
    assert ("dword-edge" in _hazards(w, h, win, 2)) == (win == 21)
    no, so = _check(gpu, oracle, g0, g1, pts, win, 2)
    assert so[:200].sum() > 150
    if shifted:
        d = (no - pts)[:200][so[:200].astype(bool)]
        assert np.abs(np.median(d, axis=0) - np.array(SHIFT)).max() < 0.5


def test_lk_regions_staged_again_at_level_0(gpu, oracle):
    """One level only: the point walks more than LK_MARGIN pixels at level 0, so the region is staged again mid-iteration
    (interior points by dwords, the hazard points by bytes)."""
    w, h = 320, 240
    g0, g1 = _pair(w, True)
    pts = _points_and_precondition(w, h, 21, 2, True)
    no, so = _check(gpu, oracle, g0, g1, pts, 21, 0)
    moved = np.abs(no - pts).max(axis=1)[so.astype(bool)]
    assert moved.size and moved.max() > MARGIN


@pytest.mark.parametrize("w", [321, 322, 323])
def test_lk_row_starts_at_every_residue(gpu, oracle, w):
    """Level strides 321 / 161 / 81, 322 / 161 / 81, 323 / 162 / 81: rows start at every residue mod 4, and with them the
    unaligned dwords of patches and regions."""
    g0, g1 = _pair(w, True)
    pts = _points_and_precondition(w, 240, 21, 2, True)
    _, so = _check(gpu, oracle, g0, g1, pts, 21, 2)
    assert so[:200].sum() > 150


@pytest.mark.parametrize("w,h", [(96, 72), (100, 88)])
def test_lk_levels_smaller_than_a_patch(gpu, oracle, w, h):
    """96 x 72: the pyramid stops at 48 x 36 (the next level, 24 x 18, would not exceed the window), where only a few
    patches and regions are interior.  100 x 88 has a level 2 of 25 x 22, lower than a 24-row patch and a 34-row region:
    every staging there takes the reflected path."""
    g0, g1 = _pair(BASE_W, True)
    g0, g1 = np.ascontiguousarray(g0[40:40 + h, 60:60 + w]), np.ascontiguousarray(g1[40:40 + h, 60:60 + w])
    rng = np.random.default_rng(w)
    pts = np.stack([rng.uniform(-3, w + 3, 150), rng.uniform(-3, h + 3, 150)], 1).astype(np.float32)
    sizes = _levels(w, h, 21, 2)
    assert sizes[-1] == ((48, 36) if w == 96 else (25, 22))
    if w == 100:
        patch, region, _ = _qualifies(pts, w, h, 21, 2)[2]
        assert not patch.any() and not region.any()
    _, so = _check(gpu, oracle, g0, g1, pts, 21, 2)
    assert so.any()


@pytest.mark.parametrize("n", [1, 63])
def test_lk_few_points(gpu, oracle, n):
    g0, g1 = _pair(320, True)
    pts = _points_and_precondition(320, 240, 21, 2, True)
    pts = pts[np.linspace(0, len(pts) - 1, n).astype(int)] if n > 1 else pts[100:101]
    _check(gpu, oracle, g0, g1, pts, 21, 2)


def test_batch_mode_matches_per_frame_pipeline(gpu):
    """Batch mode hands the tracker (lk_batch_kernel, one argument block per frame) a device-side point count below the
    launch's capacity; batches of 8, zero-copy, 40 pushes: the last batch's tracks and every output frame equal the per-frame
    pipeline's."""
    n, W, H = 40, 320, 240
    clip = synth.make_clip(synth.SEED_CONFIG1 + 7, W, H, n)
    p = gpu.params(smoothing_radius=6, max_corners=200, lk_win_size=21, lk_max_level=2)
    s1, s2 = gpu.stabilizer(p), gpu.stabilizer(p)
    s2.set_batch(8)
    s2.set_zero_copy(True)
    fb = clip[0].nbytes
    d_in = capi.DevBuf(gpu, fb * n)
    for i, f in enumerate(clip):
        d_in.upload(f, i * fb)
    d_ref, d_got = capi.DevBuf(gpu, fb * n), capi.DevBuf(gpu, fb * n)
    k1 = k2 = 0
    for i in range(n):
        k1 += s1.push_dev(d_in.ptr + i * fb, W, H, W * 3, capi.FMT_BGR8, d_ref.ptr + k1 * fb, W * 3)
        k2 += s2.push_dev(d_in.ptr + i * fb, W, H, W * 3, capi.FMT_BGR8, d_got.ptr + k2 * fb, W * 3)
    s1.sync(); s2.sync()
    a, b = s1.debug_arrays(), s2.debug_arrays()
    for key in ("prev", "curr", "status"):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    assert 0 < len(b["status"]) < 200 and b["status"].sum() > 10           # device-side count below the capacity
    while s1.flush_dev(d_ref.ptr + k1 * fb, W * 3):
        k1 += 1
    while s2.flush_dev(d_got.ptr + k2 * fb, W * 3):
        k2 += 1
    s1.sync(); s2.sync()
    assert k1 == k2 == n
    assert np.array_equal(d_ref.download((n, H, W, 3), np.uint8), d_got.download((n, H, W, 3), np.uint8))
    s1.close(); s2.close()
    for buf in (d_in, d_ref, d_got):
        buf.free()
