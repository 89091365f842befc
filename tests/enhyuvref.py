"""What the enhancer computes on a YUV surface, stated without the library: the numpy conversion of tests/cvtref.py into BGR8, the CPU
oracle's enhanceImage (tests/oracle_lib.py), the numpy conversion back - the composition vs_enh_apply_yuv_dev is defined as.  Surfaces
are packed (rows, w) frames of the format's dtype or flat buffers in a layout (pitch, c_pitch, u_off, v_off) in bytes, 0 = the default
of a field; a result in a layout holds `fill` wherever no sample lies, so a whole destination buffer can be compared.

Formats are named as in cvtref.YUV_FORMATS; "YV12" is I420 with the V plane in front of the U plane."""
import numpy as np

import cvtref
from vsamd import synth


def fmt_of(name):
    return cvtref.YUV_FORMATS["I420" if name == "YV12" else name]


def yv12_layout(w, h, pitch=0):
    """YV12 through the offsets of an I420 layout: the V plane behind the luma rows, the U plane behind it."""
    pitch = pitch or w
    return (pitch, 0, h * pitch + (h // 2) * (pitch // 2), h * pitch)


def pack(name, y, u, v, layout=None, size=None, fill=0):
    """The surface of three sample planes: packed (rows, w), or a flat buffer of `size` bytes in `layout`."""
    kind, sb, bits, sx, sy = fmt_of(name)
    if kind == "3p":
        if not layout:
            return synth.yuv_pack(y, u, v, sx, sy)
        pitch, c_pitch, u_off, v_off = (x or None for x in layout)
        return synth.yuv_pack(y, u, v, sx, sy, pitch, c_pitch, u_off, v_off, size, fill)
    h, w = y.shape
    uv = np.empty((h // 2, w), y.dtype)
    uv[:, 0::2], uv[:, 1::2] = u, v
    if not layout:
        return np.vstack([y, uv])
    pitch, uv_off = layout[0], layout[2] or h * layout[0]
    buf = np.full(size // sb, fill, y.dtype)
    buf[:h * pitch // sb].reshape(h, pitch // sb)[:, :w] = y
    buf[uv_off // sb:(uv_off + h // 2 * pitch) // sb].reshape(h // 2, pitch // sb)[:, :w] = uv
    return buf


def unpack(name, surface, w, h, layout=None):
    """The three sample planes of a surface `pack` made."""
    kind, sb, bits, sx, sy = fmt_of(name)
    surface = np.asarray(surface)
    if kind == "3p":
        return synth.yuv_unpack(surface, w, h, sx, sy, *((x or None for x in layout) if layout else ()))
    flat = surface.reshape(-1)
    pitch = layout[0] if layout else w * sb
    uv_off = (layout[2] if layout else 0) or h * pitch
    y = flat[:h * pitch // sb].reshape(h, pitch // sb)[:, :w].copy()
    uv = flat[uv_off // sb:(uv_off + h // 2 * pitch) // sb].reshape(h // 2, pitch // sb)[:, :w]
    return y, uv[:, 0::2].copy(), uv[:, 1::2].copy()


def to_bgr(name, surface, w, h, layout=None):
    _, _, _, sx, sy = fmt_of(name)
    base = "I420" if name == "YV12" else name
    return cvtref.yuv_to_rgb(*(cvtref.sample_to_byte(base, p) for p in unpack(name, surface, w, h, layout)), sx, sy, "BGR8")


def from_bgr(name, bgr, layout=None, size=None, fill=0):
    """The surface vs_op_cvt_rgb_to_yuv makes of a BGR8 frame (test_gpu_cvt.want_surface)."""
    _, _, _, sx, sy = fmt_of(name)
    base = "I420" if name == "YV12" else name
    return pack(name, *(cvtref.byte_to_sample(base, p) for p in cvtref.rgb_to_yuv(bgr, sx, sy, "BGR8")), layout, size, fill)


def enhance_yuv(oracle, params, name, surface, w, h, layout=None, out_layout=None, out_size=None, fill=0):
    """The statement: cvtref.yuv_to_rgb -> the oracle's enhance -> cvtref.rgb_to_yuv, in out_layout (None: packed)."""
    return from_bgr(name, oracle.enhance(to_bgr(name, surface, w, h, layout), params), out_layout, out_size, fill)


def round_trip(name, surface, w, h, layout=None, out_layout=None, out_size=None, fill=0):
    """The two conversions alone: what an enhancer that changes no pixel leaves of a surface."""
    return from_bgr(name, to_bgr(name, surface, w, h, layout), out_layout, out_size, fill)
