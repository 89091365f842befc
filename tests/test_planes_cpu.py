"""The plane list of a YUV surface (csrc/planar_layout.h, planes()): where the host code says the planes of a queued frame, a scratch
surface and a result lie.  The expected values are stated here in Python integers, for all eleven YUV formats, at the smallest sizes
at which a shift by sx / sy and an odd half-size can go wrong, packed and 256-aligned pitches, the default layout and explicit ones."""
import itertools

import pytest

import planes_prog
from vsamd import capi

# name: (VS_FMT_*, planes, sample bytes, sx, sy) - stated here, not read from the tables under test
FORMATS = {
    "NV12": (1, 2, 1, 1, 1), "P010": (6, 2, 2, 1, 1),
    "I420": (7, 3, 1, 1, 1), "I010": (8, 3, 2, 1, 1), "I012": (9, 3, 2, 1, 1),
    "I422": (10, 3, 1, 1, 0), "I444": (11, 3, 1, 0, 0),
    "I210": (12, 3, 2, 1, 0), "I212": (13, 3, 2, 1, 0), "I410": (14, 3, 2, 0, 0), "I412": (15, 3, 2, 0, 0),
}
SIZES = [(2, 2), (4, 2), (6, 4), (66, 50)]


def _layouts(name, w, h, pitch):
    """(label, uv_off, u_off, v_off, c_pitch) of the default layout and the explicit ones."""
    _, n, sb, sx, sy = FORMATS[name]
    out = [("default", 0, 0, 0, 0)]
    if n == 2:
        out.append(("uv gap", (h + 6) * pitch + 64, 0, 0, 0))
        return out
    ch, crow = h >> sy, (w >> sx) * sb
    cp = (crow + 63) // 64 * 64 + 64         # an explicit chroma pitch with room behind the row (even: 16-bit samples)
    dp = pitch >> sx                         # the default one
    out.append(("yv12 order", 0, (h + 2) * pitch + ch * dp, (h + 2) * pitch, 0))
    out.append(("chroma pitch", 0, 0, 0, cp))
    out.append(("yv12 order, chroma pitch", 0, h * pitch + ch * cp + 32, h * pitch, cp))
    return out


def _cases(name):
    sb = FORMATS[name][2]
    for (w, h), aligned in itertools.product(SIZES, (False, True)):
        pitch = (w * sb + 255) // 256 * 256 if aligned else w * sb
        for lay in _layouts(name, w, h, pitch):
            yield (w, h, pitch, aligned) + lay


def _expected(name, w, h, pitch, uv_off, u_off, v_off, c_pitch):
    _, n, sb, sx, sy = FORMATS[name]
    luma = dict(off=0, pitch=pitch, w=w, h=h, cn=1, sx=0, sy=0, row_bytes=w * sb)
    cw, ch = w >> sx, h >> sy
    if n == 2:
        return [luma, dict(off=uv_off or h * pitch, pitch=pitch, w=cw, h=ch, cn=2, sx=1, sy=1, row_bytes=cw * 2 * sb)], None
    cp = c_pitch or pitch >> sx
    u = u_off or h * pitch
    v = v_off or u + ch * cp
    chroma = dict(pitch=cp, w=cw, h=ch, cn=1, sx=sx, sy=sy, row_bytes=cw * sb)
    return [luma, dict(chroma, off=u), dict(chroma, off=v)], (pitch, cp, u, v)


@pytest.fixture(scope="module")
def answers():
    """Every case of every format through the program, once."""
    keys = [(name,) + c for name in FORMATS for c in _cases(name)]
    got = planes_prog.planes([(FORMATS[k[0]][0], k[1], k[2], k[3]) + k[6:] for k in keys])
    return dict(zip(keys, got))


def test_the_format_numbers_are_the_bindings():
    assert {name: f[0] for name, f in FORMATS.items()} == {name: getattr(capi, "FMT_" + name) for name in FORMATS}


@pytest.mark.parametrize("name", list(FORMATS))
def test_plane_list(answers, name):
    _, n, sb, sx, sy = FORMATS[name]
    ncases = 0
    for case in _cases(name):
        w, h, pitch, aligned, label = case[:5]
        what = (name, w, h, pitch, label)
        gn, gsb, got, from_list, from_i420_layout = answers[(name,) + case]
        want, want_i420 = _expected(name, w, h, pitch, *case[5:])
        assert (gn, gsb) == (n, sb) and got == want, (what, got, want)
        # the I420Layout of the launchers: derived from the list, and what i420_layout computes beside it
        assert from_list == from_i420_layout == want_i420, what
        # pairwise disjoint: [off, off + (h - 1) * pitch + row_bytes)
        ext = sorted((p["off"], p["off"] + (p["h"] - 1) * p["pitch"] + p["row_bytes"]) for p in got)
        assert all(a[1] <= b[0] for a, b in zip(ext, ext[1:])), (what, ext)
        assert all(p["row_bytes"] <= p["pitch"] for p in got), what
        if label == "default":
            # the planes tile the surface: each starts where the one before ends, rows(h) rows of `pitch` bytes in all
            rows = h * 3 // 2 if n == 2 else h + ((2 * (h >> sy)) >> sx)
            end = 0
            for p in got:
                assert p["off"] == end, what
                end += p["h"] * p["pitch"]
            assert end == rows * pitch, (what, end, rows)
            if not aligned:         # packed: every byte of every row is a sample's
                assert all(p["row_bytes"] == p["pitch"] for p in got), what
        ncases += 1
    assert ncases == len(SIZES) * 2 * (2 if n == 2 else 4)
