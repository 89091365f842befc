"""What vs_op_cvt_yuv_to_yuv computes, stated in numpy (int64) from the text of include/vs_stab.h alone: exact integer arithmetic in
two steps - the depth of every sample, then the siting of the chroma samples.  Shares nothing with the library; the format table is
this file's own (tests/test_yuv_cvt_cpu.py holds it to the library's).

Planes are (Y, U, V): (h, w) and twice (h >> sy, w >> sx) arrays of the format's dtype.  NV12 / P010 interleave U and V in memory;
that is layout, and no business of this file."""
import numpy as np

# name: (value bits b, low-bit format, sample dtype, sx, sy).  P010: b = 16, the whole word.
FORMATS = {
    "NV12": (8, False, np.uint8, 1, 1), "P010": (16, False, np.uint16, 1, 1),
    "I420": (8, False, np.uint8, 1, 1), "I010": (10, True, np.uint16, 1, 1), "I012": (12, True, np.uint16, 1, 1),
    "I422": (8, False, np.uint8, 1, 0), "I444": (8, False, np.uint8, 0, 0),
    "I210": (10, True, np.uint16, 1, 0), "I212": (12, True, np.uint16, 1, 0),
    "I410": (10, True, np.uint16, 0, 0), "I412": (12, True, np.uint16, 0, 0),
}
TRUNCATE, ROUND = 0, 1          # vs_yuv_depth_down
TOPLEFT, MEAN = 0, 1            # vs_cvt_chroma
DESCRIPTORS = [(TRUNCATE, TOPLEFT), (TRUNCATE, MEAN), (ROUND, TOPLEFT), (ROUND, MEAN)]


def depth(sample, b_in, low_bit_in, b_out, depth_down=TRUNCATE):
    """Step 1 on an array of samples -> int64 values at the destination's depth."""
    v = np.asarray(sample, np.int64)
    d = b_in - b_out
    if d == 0:
        return v
    if low_bit_in:
        v = np.minimum(v, (1 << b_in) - 1)
    if d < 0:
        return v << -d
    if depth_down == TRUNCATE:
        return v >> d
    return np.minimum((v + (1 << (d - 1))) >> d, (1 << b_out) - 1)


def siting(c, sx_in, sy_in, sx_out, sy_out, chroma_down=TOPLEFT):
    """Step 2 on one chroma plane of step-1 values (int64) -> the destination's chroma plane."""
    dsx, dsy = sx_out - sx_in, sy_out - sy_in
    assert dsx * dsy >= 0, "no pair of formats goes down in one axis and up in the other"
    if dsx == 0 and dsy == 0:
        return c
    if dsx >= 0 and dsy >= 0:
        if chroma_down == TOPLEFT:
            return c[::1 << dsy, ::1 << dsx]
        s = dsx + dsy
        ch, cw = c.shape
        block = c.reshape(ch >> dsy, 1 << dsy, cw >> dsx, 1 << dsx).sum(axis=(1, 3))
        return (block + (1 << (s - 1))) >> s
    usx, usy = -dsx, -dsy
    ch, cw = c.shape
    return c[(np.arange(ch << usy) >> usy)[:, None], (np.arange(cw << usx) >> usx)[None, :]]


def convert(src_name, planes, dst_name, depth_down=TRUNCATE, chroma_down=TOPLEFT):
    """(Y, U, V) of src_name -> (Y, U, V) of dst_name, in the destination's dtype."""
    b_in, low_in, _, sx_in, sy_in = FORMATS[src_name]
    b_out, _, dt, sx_out, sy_out = FORMATS[dst_name]
    y, u, v = (depth(p, b_in, low_in, b_out, depth_down) for p in planes)
    u, v = (siting(c, sx_in, sy_in, sx_out, sy_out, chroma_down) for c in (u, v))
    out = []
    for p in (y, u, v):
        assert p.min() >= 0 and p.max() <= np.iinfo(dt).max
        out.append(np.ascontiguousarray(p.astype(dt)))
    return out
