"""Inputs shared by the P010 tests: the matrix classes of the warp tests and the random surfaces the GPU tests warp.
tests/test_p010_cpu.py asserts that these surfaces hold enough rounding ties to tell half-even from half-up."""
import numpy as np

from test_gpu_pixfmt import _MATS as MATS

NON_INTEGER = ("frac_shift", "small_rot", "rot_zoom_beyond_box")     # matrix classes whose taps carry fractions


def random_plane(seed, h, w, cn=1, ten_bit=True):
    """uint16 samples: ten-bit content with live low bits, (u8 << 8) | (r << 6), or the full 16-bit range."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if cn == 1 else (h, w, cn)
    if not ten_bit:
        return rng.integers(0, 65536, shape, np.uint16)
    hi = rng.integers(0, 256, shape, np.uint16)
    return (hi << 8) | (rng.integers(0, 4, shape, np.uint16) << 6)


def random_surface(seed, w, h, ten_bit=True):
    """A P010 surface (h * 3 / 2, w)."""
    return random_plane(seed, h * 3 // 2, w, 1, ten_bit)
