"""Inputs and references shared by the planar 4:2:2 / 4:4:4 tests (tests/test_planar_cpu.py, tests/test_gpu_planar.py).

A packed frame is a (rows, w) array, uint8 or uint16: h rows of Y, then the U plane and the V plane, (h >> sy) rows of (w >> sx)
samples each, with (sx, sy) = (1, 0) for 4:2:2 and (0, 0) for 4:4:4; 16-bit samples carry their value in the low bits.

The reference of the warp is per plane: Y under M, U and V under the chroma matrix Mc = S^-1 M S.  8-bit planes: the oracle's
cv::warpAffine (BORDER_CONSTANT: warp_affine; BORDER_REPLICATE: warp_affine_d); 16-bit planes: tests/ref16.py / i010_inputs.warp_plane,
the blend of P010.  tests/test_planar_cpu.py pins ref16 to the oracle for the sheared chroma matrix of 4:2:2."""
import numpy as np

import i010_inputs as ii
from p010_inputs import MATS
from vsamd import capi, synth

BLACK, REPLICATE = ii.BLACK, ii.REPLICATE
CANARY8, CANARY16 = 0xA5, ii.CANARY

# name -> (format value, sx, sy, bits), from the binding's table
def _rows(*names):
    return {n: (capi.PIXFMT_BY_NAME[n].fmt, capi.PIXFMT_BY_NAME[n].sx, capi.PIXFMT_BY_NAME[n].sy, capi.PIXFMT_BY_NAME[n].bits) for n in names}


FORMATS = _rows("I422", "I444", "I210", "I212", "I410", "I412")
OLD = _rows("I420", "I010", "I012")


def rotation(deg, tx=0.0, ty=0.0):
    """The forward matrix the stabilizer builds: [cos -sin tx; sin cos ty], float32 values."""
    a = np.deg2rad(deg)
    return [float(np.float32(np.cos(a))), float(np.float32(-np.sin(a))), tx, float(np.float32(np.sin(a))), float(np.float32(np.cos(a))), ty]


# The staging area of a plane tile holds THP + 9 source rows (PlaneCfg::ROWS).  A full tile of 128 columns under the inverse map has a
# source box of floor(D) + 2 or + 3 rows, D = (THP - 1) cos(a) + 127 |m3'|, with |m3'| = sin(a) for luma (and 4:4:4 chroma) and
# 2 sin(a) for 4:2:2 chroma.  So a full-width tile is always staged while 127 |m3'| < 8 and always direct once 127 |m3'| >= 9 + (THP - 1)
# (1 - cos a): luma 3.61 / 4.07 degrees, 4:2:2 chroma 1.80 / 2.04 degrees.  (A chroma tile of c < 128 columns: (c - 1) in place of 127.)
STAGING = {
    "rot_1.5deg": rotation(1.5, 2.25, -1.5),     # every tile staged, luma and 4:2:2 chroma
    "rot_2.5deg": rotation(2.5, -3.5, 2.75),     # luma staged; full-width 4:2:2 chroma tiles go direct
    "rot_3.4deg": rotation(3.4, 1.0, 4.5),       # the same, just below the luma limit
    "rot_5deg": rotation(5.0, -6.0, 3.0),        # full-width luma tiles direct; 4:2:2 chroma tiles of 55 columns and more direct
}
ALL_MATS = dict(MATS, **STAGING)


def chroma_matrix(M, sx, sy):
    """Mc = S^-1 M S, S = diag(2^sx, 2^sy), every product in float32 (all exact): 4:2:0 halves the translation, 4:2:2 also halves m1
    and doubles m3, 4:4:4 is M."""
    m = np.asarray(M, np.float32).reshape(6).copy()
    half, two = np.float32(0.5), np.float32(2.0)
    if sx == 1 and sy == 1:
        m[2] *= half; m[5] *= half
    elif sx == 1 and sy == 0:
        m[1] *= half; m[2] *= half; m[3] *= two
    else:
        assert (sx, sy) == (0, 0)
    return m


def frame_rows(h, sx, sy):
    return synth.yuv_frame_rows(h, sx, sy)


def random_frame(seed, name, w, h, full_range=False):
    """A packed frame of random samples: bytes, samples below 2^bits, or (16-bit, full_range) anywhere in the 16-bit range."""
    _, sx, sy, bits = dict(FORMATS, **OLD)[name]
    hi = 256 if bits == 8 else 65536 if full_range else 1 << bits
    return np.random.default_rng(seed).integers(0, hi, (frame_rows(h, sx, sy), w), np.uint8 if bits == 8 else np.uint16)


def planes(frame, name, w, h):
    _, sx, sy, _ = dict(FORMATS, **OLD)[name]
    return synth.yuv_unpack(frame, w, h, sx, sy)


def warp_plane(oracle, p, M, border=BLACK):
    """One plane under the forward matrix M (float32 values)."""
    p = np.ascontiguousarray(p)
    if p.dtype == np.uint16:
        return ii.warp_plane(p, M, border)
    if border == BLACK:
        return oracle.warp_affine(p, M)
    return oracle.warp_affine_d(p, np.asarray(M, np.float32).astype(np.float64), border)


def warp_frame(oracle, frame, name, w, h, M, border=BLACK):
    """The expected warp of a packed frame."""
    _, sx, sy, _ = dict(FORMATS, **OLD)[name]
    y, u, v = planes(frame, name, w, h)
    Mc = chroma_matrix(M, sx, sy)
    return synth.yuv_pack(warp_plane(oracle, y, M, border), warp_plane(oracle, u, Mc, border), warp_plane(oracle, v, Mc, border), sx, sy)


def analysis_byte(y, bits):
    return np.ascontiguousarray(y) if bits == 8 else ii.analysis_byte(y, bits)


class Layout:
    """Where the planes of a surface lie, in BYTES (None: the packed default of the format).  pack / unpack move packed frames in and
    out of flat buffers with canaries wherever no sample lies."""

    def __init__(self, name, w, h, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None):
        _, self.sx, self.sy, bits = dict(FORMATS, **OLD)[name]
        self.name, self.w, self.h = name, w, h
        self.dtype = np.uint8 if bits == 8 else np.uint16
        self.sb = 1 if bits == 8 else 2
        self.canary = CANARY8 if bits == 8 else CANARY16
        self.lay = dict(pitch=pitch, c_pitch=c_pitch, u_off=u_off, v_off=v_off)
        self.pitch, self.c_pitch, self.u_off, self.v_off = synth.yuv_layout(w, h, self.sx, self.sy, self.sb, pitch, c_pitch, u_off, v_off)
        ch = h >> self.sy
        self.size = size or max(h * self.pitch, self.u_off + ch * self.c_pitch, self.v_off + ch * self.c_pitch)
        self.args = (u_off or 0, v_off or 0, c_pitch or 0)            # what the library is told: 0 for a field left at its default

    def _flat(self, y, u, v, fill):
        return synth.yuv_pack(y, u, v, self.sx, self.sy, self.pitch, self.c_pitch, self.u_off, self.v_off, self.size, fill).reshape(-1)

    def pack(self, frame):
        return self._flat(*synth.yuv_unpack(np.asarray(frame, self.dtype), self.w, self.h, self.sx, self.sy), self.canary)

    def blank(self, n):
        return np.full((n, self.size // self.sb), self.canary, self.dtype)

    def unpack(self, buf):
        """The packed frame of a surface; every sample outside the three planes must still be the canary."""
        buf = np.asarray(buf, self.dtype).reshape(-1)
        z = [np.zeros_like(p) for p in synth.yuv_unpack(np.zeros((frame_rows(self.h, self.sx, self.sy), self.w), self.dtype), self.w, self.h, self.sx, self.sy)]
        hole = self._flat(*z, 1)
        assert np.all(buf[hole == 1] == self.canary), "samples outside the planes were written"
        return synth.yuv_pack(*synth.yuv_unpack(buf, self.w, self.h, self.sx, self.sy, self.pitch, self.c_pitch, self.u_off, self.v_off), self.sx, self.sy)
