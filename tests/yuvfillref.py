"""The reference of edge fill on YUV streams (vs_stab_set_yuv_edge_fill, vs_op_warp_affine_yuv_fill), in numpy integers:

    cv::warpAffine(plane, M, size, INTER_LINEAR, BORDER_CONSTANT, borderValue = fill)   per plane.

Coordinates and tap weights are tests/ref16.py's - ref16.coords is what the oracle pins (tests/test_p010_cpu.py) -, the four taps are
gathered with the plane's fill sample outside the plane, each tap decided by itself, and the exact integer

    S = sum v_i n_i,   n = ((32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy fx),   sum n_i = 1024

is rounded once: (S + 512) >> 10 for 8-bit samples (the fixed-point path of cv::warpAffine), half to even for 16-bit samples
(P010's blend).  With fill 0 this is ref16.warp_affine / the oracle's warp (tests/test_yuv_edge_fill_cpu.py).

A plane is (h, w), or (h, w, cn) with one fill sample per channel: the interleaved UV plane of NV12 / P010 reads the (U, V) pair."""
import numpy as np

import ref16


def warp_sum(img, M, fill):
    """S of every sample (int64, the shape of img).  M: the forward matrix in double; fill: a sample, or one per channel."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    src = img.reshape(h, w, -1).astype(np.int64)
    f = np.broadcast_to(np.asarray(fill, np.int64).reshape(-1), (src.shape[2],))
    sx, sy, fx, fy = ref16.coords(M, w, h)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok[..., None], v, f)

    n = [(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx]
    S = (tap(sx, sy) * n[0][..., None] + tap(sx + 1, sy) * n[1][..., None] + tap(sx, sy + 1) * n[2][..., None] +
         tap(sx + 1, sy + 1) * n[3][..., None])
    return S.reshape(img.shape)


def warp_plane(img, M, fill):
    """img: uint8 or uint16; M: the forward 2x3 matrix as float32 values.  Same shape and dtype out."""
    img = np.asarray(img)
    assert img.dtype in (np.uint8, np.uint16)
    top = 255 if img.dtype == np.uint8 else 65535
    assert np.all(np.asarray(fill) >= 0) and np.all(np.asarray(fill) <= top), fill
    S = warp_sum(img, np.asarray(M, np.float32).astype(np.float64), fill)
    return ref16.round_sum(S, ref16.HALF_UP if img.dtype == np.uint8 else ref16.HALF_EVEN).astype(img.dtype)


def chroma_matrix(M, sx, sy):
    """Mc = S^-1 M S, S = diag(2^sx, 2^sy), every product in float32 (all exact): the stream's chroma matrix."""
    m = np.asarray(M, np.float32).reshape(6).copy()
    half, two = np.float32(0.5), np.float32(2.0)
    if sx == 1 and sy == 1:
        m[2] *= half; m[5] *= half
    elif sx == 1 and sy == 0:
        m[1] *= half; m[2] *= half; m[3] *= two
    else:
        assert (sx, sy) == (0, 0)
    return m


def warp_surface(planes, sx, sy, M, fill):
    """planes: [Y, U, V] (three-plane formats) or [Y, UV] with UV of shape (h >> sy, w >> sx, 2) (NV12, P010); fill: (y, u, v).
    Y under M, chroma under the chroma matrix.  -> the warped planes."""
    y, u, v = (int(c) for c in fill)
    Mc = chroma_matrix(M, sx, sy)
    if len(planes) == 2:
        return [warp_plane(planes[0], M, y), warp_plane(planes[1], Mc, (u, v))]
    return [warp_plane(planes[0], M, y), warp_plane(planes[1], Mc, u), warp_plane(planes[2], Mc, v)]
