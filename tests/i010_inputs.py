"""Inputs and references shared by the I010 / I012 tests (tests/test_i010_cpu.py, tests/test_gpu_i010.py).

A packed frame is a (h * 3 / 2, w) uint16 array laid out as an I420 frame: h rows of Y, then the U plane and the V plane, h / 2 rows
of w / 2 samples each, the value in the low bits of every sample.  The reference of the warp is tests/ref16.py plane by plane
(the blend of P010, which tests/test_p010_cpu.py pins to the 8-bit oracle); the analysis byte is min(sample >> (bits - 8), 255)."""
import numpy as np

import ref16
from vsamd import synth

BLACK, REPLICATE = 0, 3                  # vs_border: VS_BORDER_BLACK, VS_BORDER_REPLICATE
CANARY = 0xA5C3


def random_frame(seed, w, h, bits=10, full_range=False):
    """A packed frame: samples below 2^bits (low-aligned content), or anywhere in the 16-bit range (what the saturation is for)."""
    return np.random.default_rng(seed).integers(0, 65536 if full_range else 1 << bits, (h * 3 // 2, w), np.uint16)


def planes(frame, w, h):
    """(Y, U, V) of a packed frame: (h, w), (h / 2, w / 2), (h / 2, w / 2)."""
    frame = np.asarray(frame, np.uint16)
    flat = frame.reshape(-1)
    n = (h // 2) * (w // 2)
    return frame[:h], flat[w * h:w * h + n].reshape(h // 2, w // 2), flat[w * h + n:].reshape(h // 2, w // 2)


def interleaved(frame, w, h):
    """The two-plane surface (h * 3 / 2, w) with the same samples: Y, then rows of (U, V) pairs - the layout of P010, no shift."""
    y, u, v = planes(frame, w, h)
    out = np.empty((h * 3 // 2, w), np.uint16)
    out[:h] = y
    out[h:, 0::2] = u
    out[h:, 1::2] = v
    return out


def warp_plane(img, M, border=BLACK):
    """ref16.warp_affine; BORDER_REPLICATE: the same coordinates, sum and rounding with the taps clamped into the picture
    (remapBilinear's clip()) instead of zeroed."""
    if border == BLACK:
        return ref16.warp_affine(img, M)
    img = np.asarray(img)
    h, w = img.shape
    src = img.astype(np.int64)
    sx, sy, fx, fy = ref16.coords(np.asarray(M, np.float32).astype(np.float64), w, h)

    def tap(xx, yy):
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]

    S = tap(sx, sy) * (32 - fy) * (32 - fx) + tap(sx + 1, sy) * (32 - fy) * fx + tap(sx, sy + 1) * fy * (32 - fx) + tap(sx + 1, sy + 1) * fy * fx
    return ref16.round_sum(S).astype(img.dtype)


def warp_three_planes(frame, w, h, M, border=BLACK):
    """The expected warp of a packed frame: Y under M, U and V each under the matrix with the halved translation."""
    y, u, v = planes(frame, w, h)
    Mc = ref16.chroma_matrix(M)
    return np.concatenate([warp_plane(y, M, border).reshape(-1), warp_plane(u, Mc, border).reshape(-1),
                           warp_plane(v, Mc, border).reshape(-1)]).reshape(h * 3 // 2, w)


def analysis_byte(y, bits):
    """The 8-bit plane the analysis sees of a luma plane."""
    return np.minimum(np.asarray(y, np.uint16) >> (bits - 8), 255).astype(np.uint8)


class Layout:
    """Where the planes of a surface lie, in BYTES: pitch, chroma pitch, plane offsets, surface size (None: the packed default at
    pitch 2 w).  pack / unpack move packed frames in and out of flat uint16 buffers with canaries wherever no sample lies."""

    def __init__(self, w, h, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None):
        self.w, self.h = w, h
        self.pitch, self.c_pitch, self.u_off, self.v_off = synth.i420_layout(2 * w, h, pitch, c_pitch, u_off, v_off)
        end = max(h * self.pitch, self.u_off + (h // 2) * self.c_pitch, self.v_off + (h // 2) * self.c_pitch)
        self.size = size or end
        self.args = (u_off or 0, v_off or 0, c_pitch or 0)            # what the library is told: 0 for a field left at its default

    def _views(self, buf):
        w, h, p, c = self.w, self.h, self.pitch // 2, self.c_pitch // 2
        u, v = self.u_off // 2, self.v_off // 2
        return (buf[:h * p].reshape(h, p)[:, :w], buf[u:u + (h // 2) * c].reshape(h // 2, c)[:, :w // 2],
                buf[v:v + (h // 2) * c].reshape(h // 2, c)[:, :w // 2])

    def pack(self, frame):
        buf = np.full(self.size // 2, CANARY, np.uint16)
        for d, s in zip(self._views(buf), planes(frame, self.w, self.h)):
            d[...] = s
        return buf

    def blank(self, n):
        return np.full((n, self.size // 2), CANARY, np.uint16)

    def unpack(self, buf):
        """The packed frame of a surface; every sample outside the three planes must still be the canary."""
        buf = np.asarray(buf, np.uint16).reshape(-1)
        y, u, v = (p.copy() for p in self._views(buf))
        rest = buf.copy()
        for p in self._views(rest):
            p[...] = CANARY
        assert np.all(rest == CANARY), "samples outside the planes were written"
        return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(self.h * 3 // 2, self.w)
