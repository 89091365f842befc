"""The four- and reversed-channel pixel formats (BGRA8, RGBA8, RGB8) at the ABI and in the Python binding: the enum of
include/vs_stab.h, the constants of vsamd.capi and the shapes its helpers give frames of each format.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(name):
    text = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    body = re.search(r"typedef enum %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"(VS_\w+)\s*=\s*(\d+)", body)}


def test_pixfmt_enum_values_in_the_header():
    assert _header_enum("vs_pixfmt") == {"VS_FMT_BGR8": 0, "VS_FMT_NV12": 1, "VS_FMT_GRAY8": 2,
                                         "VS_FMT_BGRA8": 3, "VS_FMT_RGBA8": 4, "VS_FMT_RGB8": 5}


def test_capi_constants_match_the_header():
    e = _header_enum("vs_pixfmt")
    for name in ("BGR8", "NV12", "GRAY8", "BGRA8", "RGBA8", "RGB8"):
        assert getattr(capi, "FMT_" + name) == e["VS_FMT_" + name], name
    assert capi.FMT_CHANNELS == {capi.FMT_BGR8: 3, capi.FMT_NV12: 1, capi.FMT_GRAY8: 1,
                                 capi.FMT_BGRA8: 4, capi.FMT_RGBA8: 4, capi.FMT_RGB8: 3}


class _StubLib:
    """vs_stab_out_size of a stream with a 10-pixel border: out = in + 20 in both directions."""

    def vs_stab_out_size(self, h, w, hh, ow, oh):
        ow._obj.value, oh._obj.value = w + 20, hh + 20
        return 0


class _StubVs:
    def check(self, status, h=None):
        assert status == 0


def _stub_stabilizer():
    s = capi.Stabilizer.__new__(capi.Stabilizer)
    s.vs, s.lib, s.h = _StubVs(), _StubLib(), C.c_void_p()
    return s


def test_shape_helpers_of_the_new_formats():
    s = _stub_stabilizer()
    for fmt, cn in ((capi.FMT_BGRA8, 4), (capi.FMT_RGBA8, 4), (capi.FMT_RGB8, 3)):
        frame = np.zeros((24, 32, cn), np.uint8)
        assert s._geom(frame, fmt) == (32, 24, cn)
        assert s.out_shape(32, 24, fmt) == (44, 52, cn)


def test_shape_helpers_of_the_existing_formats_are_unchanged():
    s = _stub_stabilizer()
    assert s._geom(np.zeros((24, 32, 3), np.uint8), capi.FMT_BGR8) == (32, 24, 3)
    assert s._geom(np.zeros((36, 32), np.uint8), capi.FMT_NV12) == (32, 24, 1)
    assert s._geom(np.zeros((24, 32), np.uint8), capi.FMT_GRAY8) == (32, 24, 1)
    assert s.out_shape(32, 24, capi.FMT_BGR8) == (44, 52, 3)
    assert s.out_shape(32, 24, capi.FMT_NV12) == (66, 52)
    assert s.out_shape(32, 24, capi.FMT_GRAY8) == (44, 52)
