"""What vs_op_cvt_yuv_to_rgb and vs_op_cvt_rgb_to_yuv compute, stated in numpy (int64) from the text of include/vs_stab.h alone:
ITU-R BT.601 limited range in the fixed-point arithmetic of OpenCV's COLOR_YUV2BGR_NV12 / _I420 and COLOR_BGR2YUV_I420.  Shares
nothing with the library; the format table below is this file's own (tests/test_cvt_cpu.py holds it to the library's).

Planes are (rows, cols) arrays of bytes; the 16-bit formats enter and leave through sample_to_byte / byte_to_sample."""
import numpy as np

H = 1 << 19

# name: (kind, sample_bytes, bits, sx, sy); kind "uv": a luma plane and one plane of interleaved (U, V) pairs, "3p": three planes
YUV_FORMATS = {
    "NV12": ("uv", 1, 8, 1, 1), "P010": ("uv", 2, 10, 1, 1),
    "I420": ("3p", 1, 8, 1, 1), "I010": ("3p", 2, 10, 1, 1), "I012": ("3p", 2, 12, 1, 1),
    "I422": ("3p", 1, 8, 1, 0), "I444": ("3p", 1, 8, 0, 0),
    "I210": ("3p", 2, 10, 1, 0), "I212": ("3p", 2, 12, 1, 0), "I410": ("3p", 2, 10, 0, 0), "I412": ("3p", 2, 12, 0, 0),
}
# name: (channels, position of R, position of B); G is channel 1, alpha (channel 3) is written as 255 and ignored on input
RGB_FORMATS = {"BGR8": (3, 2, 0), "RGB8": (3, 0, 2), "BGRA8": (4, 2, 0), "RGBA8": (4, 0, 2)}


def sample_shift(name):
    kind, sb, bits, _, _ = YUV_FORMATS[name]
    return 0 if sb == 1 else 8 if kind == "uv" else bits - 8


def sample_to_byte(name, s):
    """A surface's sample as the byte the conversion reads: P010 sample >> 8, the low-bit formats min(sample >> (bits - 8), 255)."""
    return np.minimum(np.asarray(s, np.int64) >> sample_shift(name), 255)


def byte_to_sample(name, b):
    """... and the sample written for a byte: byte << 8 for P010, byte << (bits - 8) for the low-bit formats."""
    sb = YUV_FORMATS[name][1]
    return (np.asarray(b, np.int64) << sample_shift(name)).astype(np.uint16 if sb == 2 else np.uint8)


def _sat(v):
    return np.clip(v, 0, 255)


def yuv_to_rgb_unclamped(y, u, v):
    """(R, G, B) before the clamp, int64, for arrays of bytes of one shape."""
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    yp = np.maximum(0, y - 16) * 1220542
    u = u - 128
    v = v - 128
    return (yp + H + 1673527 * v) >> 20, (yp + H - 852492 * v - 409993 * u) >> 20, (yp + H + 2116026 * u) >> 20


def yuv_to_rgb_px(y, u, v):
    return tuple(_sat(c) for c in yuv_to_rgb_unclamped(y, u, v))


def rgb_to_yuv_unclamped(r, g, b):
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    return ((269484 * r + 528482 * g + 102760 * b + H + (16 << 20)) >> 20,
            (-155188 * r - 305135 * g + 460324 * b + H + (128 << 20)) >> 20,
            (460324 * r - 385875 * g - 74448 * b + H + (128 << 20)) >> 20)


def rgb_to_yuv_px(r, g, b):
    return tuple(_sat(c) for c in rgb_to_yuv_unclamped(r, g, b))


def yuv_to_rgb(y, u, v, sx, sy, rgb="BGR8"):
    """Byte planes Y (h, w), U and V (h >> sy, w >> sx) -> (h, w, cn) uint8: pixel (x, y) takes the chroma sample (x >> sx, y >> sy)."""
    h, w = np.shape(y)
    yi, xi = np.arange(h)[:, None] >> sy, np.arange(w)[None, :] >> sx
    r, g, b = yuv_to_rgb_px(y, np.asarray(u)[yi, xi], np.asarray(v)[yi, xi])
    cn, ri, bi = RGB_FORMATS[rgb]
    out = np.full((h, w, cn), 255, np.uint8)
    out[:, :, ri], out[:, :, 1], out[:, :, bi] = r, g, b
    return out


def rgb_to_yuv(frame, sx, sy, rgb="BGR8"):
    """(h, w, cn) uint8 -> byte planes (Y, U, V): Y of every pixel, U and V of the one pixel (cx << sx, cy << sy) of each block."""
    frame = np.asarray(frame)
    cn, ri, bi = RGB_FORMATS[rgb]
    assert frame.shape[2] == cn
    y, u, v = rgb_to_yuv_px(frame[:, :, ri], frame[:, :, 1], frame[:, :, bi])
    return y.astype(np.uint8), u[::1 << sy, ::1 << sx].astype(np.uint8), v[::1 << sy, ::1 << sx].astype(np.uint8)


def all_triples():
    """Three (4096, 4096) uint8 planes that hold every triple of bytes once: (i >> 16, (i >> 8) & 255, i & 255) at flat index i."""
    i = np.arange(1 << 24, dtype=np.int64).reshape(4096, 4096)
    return (i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)
