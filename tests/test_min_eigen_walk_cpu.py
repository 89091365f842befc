"""The summation order of the min-eigenvalue column walk (k_gftt.hip, min_eigen_walk3), stated in numpy, against the oracle.

The walk forms every float32 term once (Sobel row terms r and t per gray row, dx, dy and the three products per covariance row),
every float64 box row sum once, (c[x-1] + c[x]) + c[x+1], and shares it between the three output rows that use it:
s = (rs[y-1] + rs[y]) + rs[y+1].  The oracle recomputes each row sum per output pixel and starts every sum from 0.0; the
operations on the values are the same ones in the same order, so the maps must agree bit for bit - including on pictures
where the sums are NOT exact: dy is the difference of two t values that are each a sum of two rounded products, rows with the
same 2*centre + (left + right) split differently give t one rounding apart, and dy*dy then lies far below the 53 bits of a sum
that also holds ordinary terms.  `test_residue_exists` shows such dy values and that another order (columns first) gives other
float64 sums on the residue picture: the order is part of the definition, not a freedom.
"""
import numpy as np
import pytest

F1 = np.float32(1.0 / (4 * 3 * 255.0))
F0 = np.float32(2.0) * F1


def cov_planes(g):
    """float32 covariance planes (dx*dx, dx*dy, dy*dy) of a uint8 picture, the gray picture reflected (REFLECT_101)."""
    p = np.pad(g.astype(np.int32), 1, mode="reflect")
    left, centre, right = p[:, :-2], p[:, 1:-1], p[:, 2:]
    r = (right - left).astype(np.float32)
    t = centre.astype(np.float32) * F0 + (left + right).astype(np.float32) * F1
    dx = (r[:-2] + r[2:]) * F1 + r[1:-1] * F0
    dy = t[2:] - t[:-2]
    assert dx.dtype == dy.dtype == np.float32
    return dx * dx, dx * dy, dy * dy, dy


def tail(s0, s1, s2):
    a, b, c = s0.astype(np.float32) * np.float32(0.5), s1.astype(np.float32), s2.astype(np.float32) * np.float32(0.5)
    d = (a - c) * (a - c) + b * b
    return (a + c) - np.sqrt(d)


def walk_box_sums(g):
    """The walk's order: row sums left to right, once per covariance row (the covariance planes reflected), rows top to bottom."""
    out = []
    for c in cov_planes(g)[:3]:
        p = np.pad(c.astype(np.float64), 1, mode="reflect")
        rs = (p[:, :-2] + p[:, 1:-1]) + p[:, 2:]
        out.append((rs[:-2] + rs[1:-1]) + rs[2:])
    return out


def walk_min_eigen(g):
    return tail(*walk_box_sums(g))


def columns_first_box_sums(g):
    """Another order of the same nine terms (column sums first): NOT the definition."""
    out = []
    for c in cov_planes(g)[:3]:
        p = np.pad(c.astype(np.float64), 1, mode="reflect")
        cs = (p[:-2] + p[1:-1]) + p[2:]
        out.append((cs[:, :-2] + cs[:, 1:-1]) + cs[:, 2:])
    return out


def residue_image(w=67, h=41, seed=5):
    """Rows 0, 4, 8, .. constant c, rows 2, 6, 10, .. alternating c + d, c - d around the c of the row two above: both have
    2*centre + left + right = 4c at every column, split differently, so dy of the rows between is a rounding residue (or 0).
    The odd rows are noise, which puts ordinary terms into the same box sums."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    x = np.arange(w)
    for y in range(0, h, 2):
        if y % 4 == 0:
            c, d = int(rng.integers(45, 210)), int(rng.integers(1, 45))
            g[y] = c
        else:
            g[y] = c + d * (1 - 2 * (x & 1))
    return g


def _images():
    rng = np.random.default_rng(11)
    yield "random 70x45", rng.integers(0, 256, (45, 70), dtype=np.uint8)
    yield "random 5x4", rng.integers(0, 256, (4, 5), dtype=np.uint8)
    yield "random 3x3", rng.integers(0, 256, (3, 3), dtype=np.uint8)
    yield "smooth 125x70", (np.add.outer(np.arange(70) * 3, np.arange(125) * 2) % 256).astype(np.uint8)
    yield "residue", residue_image()
    yield "flat", np.full((20, 66), 93, np.uint8)


@pytest.mark.parametrize("name,g", list(_images()), ids=[n for n, _ in _images()])
def test_walk_order_equals_oracle(oracle, name, g):
    want = oracle.min_eigen(g, 3)
    got = walk_min_eigen(g)
    assert got.dtype == np.float32
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (name, len(bad), bad[:5].tolist())


def test_residue_exists(oracle):
    # every (centre, left + right): equal 2*centre + sum, different t
    c, s = np.meshgrid(np.arange(256), np.arange(511), indexing="ij")
    t = c.astype(np.float32) * F0 + s.astype(np.float32) * F1
    key = (2 * c + s).ravel()
    order = np.argsort(key, kind="stable")
    tk, kk = t.ravel()[order], key[order]
    lo = np.minimum.reduceat(tk, np.flatnonzero(np.r_[True, kk[1:] != kk[:-1]]))
    hi = np.maximum.reduceat(tk, np.flatnonzero(np.r_[True, kk[1:] != kk[:-1]]))
    res = (hi - lo)[hi > lo]
    assert res.size > 0 and res.dtype == np.float32
    assert 0 < float(res.min()) <= 2.0 ** -30, float(res.min())
    # the residue picture holds such dy values, next to ordinary ones
    g = residue_image()
    dy = np.abs(cov_planes(g)[3])
    tiny = (dy > 0) & (dy <= 2.0 ** -24)
    assert tiny.sum() > 50 and (dy > 2.0 ** -10).sum() > 50
    # and there the float64 sums are not exact: another order of the same nine terms gives other bits (on a noise picture
    # every term is a multiple of f1 * f1 of ordinary size, and the orders agree)
    assert any((a.view(np.uint64) != b.view(np.uint64)).any() for a, b in zip(walk_box_sums(g), columns_first_box_sums(g)))
    noise = np.random.default_rng(1).integers(0, 256, (45, 70), dtype=np.uint8)
    assert all(np.array_equal(a, b) for a, b in zip(walk_box_sums(noise), columns_first_box_sums(noise)))
