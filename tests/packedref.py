"""What vs_op_cvt_packed_to_yuv and vs_op_cvt_yuv_to_packed compute, stated in numpy from the text of include/vs_stab.h alone: where
the samples of a packed 4:2:2 frame lie (plain indexing), and between them and a surface format the two steps of
vs_op_cvt_yuv_to_yuv - yuvref.depth, yuvref.siting - with the packed side a 4:2:2 format, (sx, sy) = (1, 0).  Shares nothing with the
library (tests/test_packed_cvt_cpu.py holds it to things it shares no code with).

A packed frame is its rows: an (h, row_bytes) uint8 array.  Planes are (Y, U, V) as in yuvref: (h, w) and twice (h, w / 2)."""
import numpy as np

import yuvref

# name: (value bits b, dtype of the planes, positions of Y0, U, Y1, V in a macropixel of four words - None: v210 has groups)
FORMATS = {
    "YUY2": (8, np.uint8, (0, 1, 2, 3)), "UYVY": (8, np.uint8, (1, 0, 3, 2)), "YVYU": (8, np.uint8, (0, 3, 2, 1)),
    "Y210": (16, np.uint16, (0, 1, 2, 3)), "v210": (10, np.uint16, None),
}
ENUM = {"YUY2": 0, "UYVY": 1, "YVYU": 2, "Y210": 3, "v210": 4}          # enum vs_packed_fmt
ALIGN = {"YUY2": 1, "UYVY": 1, "YVYU": 1, "Y210": 2, "v210": 4}         # what pointers and pitches are multiples of


def row_bytes(name, w):
    if name == "v210":
        return 16 * ((w + 5) // 6)
    return w * 2 * np.dtype(FORMATS[name][1]).itemsize


def default_pitch(name, w):
    return 128 * ((w + 47) // 48) if name == "v210" else row_bytes(name, w)


def pack(name, planes):
    """(Y, U, V) -> the rows of the packed frame.  v210: the value's low ten bits go into the field."""
    y, u, v = (np.asarray(p) for p in planes)
    h, w = y.shape
    _, dt, order = FORMATS[name]
    if order:
        m = np.zeros((h, w // 2, 4), np.dtype(dt).newbyteorder("<"))
        m[:, :, order[0]], m[:, :, order[1]], m[:, :, order[2]], m[:, :, order[3]] = y[:, 0::2], u, y[:, 1::2], v
        return m.reshape(h, -1).view(np.uint8)
    g = (w + 5) // 6
    yp, up, vp = np.zeros((h, 6 * g), np.uint32), np.zeros((h, 3 * g), np.uint32), np.zeros((h, 3 * g), np.uint32)
    yp[:, :w], up[:, :w // 2], vp[:, :w // 2] = y & 1023, u & 1023, v & 1023
    words = np.zeros((h, g, 4), np.dtype("<u4"))
    words[:, :, 0] = up[:, 0::3] | yp[:, 0::6] << 10 | vp[:, 0::3] << 20
    words[:, :, 1] = yp[:, 1::6] | up[:, 1::3] << 10 | yp[:, 2::6] << 20
    words[:, :, 2] = vp[:, 1::3] | yp[:, 3::6] << 10 | up[:, 2::3] << 20
    words[:, :, 3] = yp[:, 4::6] | vp[:, 2::3] << 10 | yp[:, 5::6] << 20
    return words.reshape(h, -1).view(np.uint8)


def unpack(name, rows, w):
    """The rows of a packed frame (at least row_bytes wide) -> (Y, U, V).  v210: bits 30 - 31 and the fields of pixels >= w are ignored."""
    _, dt, order = FORMATS[name]
    rows = np.ascontiguousarray(np.asarray(rows, np.uint8)[:, :row_bytes(name, w)])
    h = rows.shape[0]
    if order:
        m = rows.view(np.dtype(dt).newbyteorder("<")).reshape(h, w // 2, 4).astype(dt)
        y = np.empty((h, w), dt)
        y[:, 0::2], y[:, 1::2] = m[:, :, order[0]], m[:, :, order[2]]
        return [y, np.ascontiguousarray(m[:, :, order[1]]), np.ascontiguousarray(m[:, :, order[3]])]
    g = (w + 5) // 6
    words = rows.view(np.dtype("<u4")).reshape(h, g, 4).astype(np.uint32)
    lo, mid, hi = words & 1023, (words >> 10) & 1023, (words >> 20) & 1023
    y, u, v = np.empty((h, 6 * g), dt), np.empty((h, 3 * g), dt), np.empty((h, 3 * g), dt)
    u[:, 0::3], y[:, 0::6], v[:, 0::3] = lo[:, :, 0], mid[:, :, 0], hi[:, :, 0]
    y[:, 1::6], u[:, 1::3], y[:, 2::6] = lo[:, :, 1], mid[:, :, 1], hi[:, :, 1]
    v[:, 1::3], y[:, 3::6], u[:, 2::3] = lo[:, :, 2], mid[:, :, 2], hi[:, :, 2]
    y[:, 4::6], v[:, 2::3], y[:, 5::6] = lo[:, :, 3], mid[:, :, 3], hi[:, :, 3]
    return [np.ascontiguousarray(y[:, :w]), np.ascontiguousarray(u[:, :w // 2]), np.ascontiguousarray(v[:, :w // 2])]


def _finish(planes, dt):
    out = []
    for p in planes:
        assert p.min() >= 0 and p.max() <= np.iinfo(dt).max
        out.append(np.ascontiguousarray(p.astype(dt)))
    return out


def packed_to_yuv(name, planes, dst_name, depth_down=yuvref.TRUNCATE, chroma_down=yuvref.TOPLEFT):
    """(Y, U, V) of the packed format `name` -> (Y, U, V) of the surface format dst_name, in its dtype."""
    b_in = FORMATS[name][0]
    b_out, _, dt, sx, sy = yuvref.FORMATS[dst_name]
    y, u, v = (yuvref.depth(p, b_in, False, b_out, depth_down) for p in planes)
    u, v = (yuvref.siting(c, 1, 0, sx, sy, chroma_down) for c in (u, v))
    return _finish((y, u, v), dt)


def yuv_to_packed(src_name, planes, name, depth_down=yuvref.TRUNCATE, chroma_down=yuvref.TOPLEFT):
    """(Y, U, V) of the surface format src_name -> (Y, U, V) of the packed format `name`.  A v210 field takes min(value, 1023), in step 1."""
    b_in, low, _, sx, sy = yuvref.FORMATS[src_name]
    b_out, dt, _ = FORMATS[name]
    y, u, v = (yuvref.depth(p, b_in, low, b_out, depth_down) for p in planes)
    if name == "v210":          # part of step 1: the mean of a block is taken of values that fit a field
        y, u, v = (np.minimum(p, 1023) for p in (y, u, v))
    u, v = (yuvref.siting(c, sx, sy, 1, 0, chroma_down) for c in (u, v))
    return _finish((y, u, v), dt)


def random_planes(name, w, h, seed):
    """Sample planes of a packed format: every bit of an 8-bit sample, of a Y210 word and of a v210 field live."""
    b, dt, _ = FORMATS[name]
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << b, (h, pw)).astype(dt) for pw in (w, w // 2, w // 2)]
