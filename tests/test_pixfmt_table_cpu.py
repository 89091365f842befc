"""One pixel-format table on each side of the C ABI - csrc/pixfmt.h and vsamd/capi.py - and the enum of include/vs_stab.h: the three
agree, for every format and every column they share."""
import json
import os
import re

import pixfmt_check
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ("fmt", "name", "text", "kind", "cn", "sample_bytes", "bits", "sx", "sy", "gray_source", "border_modes")


def _c_table():
    return json.loads(pixfmt_check.run("table"))


def _header_enum():
    text = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    out = {}
    for enum in ("vs_pixfmt", "vs_pixfmt16", "vs_pixfmt_planar", "vs_pixfmt_planar16", "vs_pixfmt_planar4xx"):
        body = re.search(r"typedef enum %s \{(.*?)\} %s;" % (enum, enum), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out.update({k: int(v) for k, v in re.findall(r"(VS_FMT_\w+)\s*=\s*(\d+)", body)})
    return out


def test_c_table_equals_the_binding_table():
    c = _c_table()
    assert len(c) == len(capi.PIXFMTS) == 16
    for row, rec in zip(c, capi.PIXFMTS):
        assert {k: row[k] for k in SHARED} == {k: getattr(rec, k) for k in SHARED}, rec.name


def test_header_enum_equals_both_tables():
    enum = _header_enum()
    assert enum == {"VS_FMT_" + r["name"]: r["fmt"] for r in _c_table()}
    assert enum == {"VS_FMT_" + f.name: f.fmt for f in capi.PIXFMTS}
    assert all(getattr(capi, "FMT_" + f.name) == f.fmt for f in capi.PIXFMTS)


def test_what_the_c_side_derives_is_what_the_binding_derives():
    for row in _c_table():
        fmt = row["fmt"]
        assert row["rows_of_48"] == capi.fmt_frame_rows(fmt, 48), row["name"]
        assert capi.fmt_picture_rows(fmt, row["rows_of_48"]) == 48, row["name"]
        assert row["lo16_shift"] == (capi.FMT_PLANAR_BITS[fmt] - 8 if fmt in capi.FMT_PLANAR_BITS and row["sample_bytes"] == 2 else 0), row["name"]
        if fmt in capi.FMT_CHROMA_SHIFTS:
            assert row["chroma_row_bytes_of_64"] == (64 >> capi.FMT_CHROMA_SHIFTS[fmt][0]) * row["sample_bytes"], row["name"]
            assert row["default_chroma_pitch_is_half"] == (capi.FMT_CHROMA_SHIFTS[fmt][0] == 1), row["name"]
        else:
            assert not row["default_chroma_pitch_is_half"], row["name"]
        assert capi.fmt_px_bytes(fmt) == row["cn"] and capi.fmt_two_planes(fmt) == (row["kind"] == 1), row["name"]
