"""The fade border on YUV streams, the parts that need no GPU.

1. tests/yuvfaderef.py, the numpy statement: for uint8 with fill 0 it is compref's (fade_blend over copy_make_border, fade_update,
   fade_stream_step); for uint16 it equals exact rational arithmetic (fractions.Fraction, rounded to float32 by integer arithmetic)
   on ties at alpha = 0.5, saturation at 65535 and every alpha of a 0.1 / 30 ramp; alpha = 0 gives the BLACK pad.
2. The refusal rules (video-stab_amd/csrc/pixfmt.h through tests/cpp/yuv_fade_check.cpp): without the mode every answer is today's;
   with it an even border passes, an odd one on a subsampled format names the format, and the canvas, crop-and-zoom and the five
   pad modes keep their answers.
3. The ABI surface: the three new entry points are exported and declared, the job structs have their stated sizes, and the operators
   refuse on the host - without a device they answer VS_ERR_NO_DEVICE after their argument checks."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import compref
import plane_job_refusals as pjr
import refusal_cases
import yuvfaderef as yf
import yuvpadref as yp
from vsamd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- 1. the numpy statement --------------------------------------------------------------------------------------------------
def test_bytes_with_fill_0_are_comprefs_statements():
    rng = np.random.default_rng(5)
    for (w, h), b in (((1, 1), 3), ((5, 4), 7), ((64, 48), 8), ((33, 17), 0)):
        for cn in (1, 2, 3):
            shape = (h, w) if cn == 1 else (h, w, cn)
            plane = rng.integers(0, 256, shape, np.uint8)
            hist = rng.integers(0, 256, (h + 2 * b, w + 2 * b) + shape[2:], np.uint8)
            for alpha in (F(0), F(0.5), F(0.1), F(0.1) * (F(7) / F(30))):
                beta = F(1) - alpha
                want = compref.fade_blend(hist, compref.copy_make_border(plane, b, compref.BLACK), alpha, beta)
                assert np.array_equal(yf.blend_plane(plane, hist, b, b, [0] * cn if cn > 1 else 0, alpha, beta), want)
            res = rng.integers(0, 256, hist.shape, np.uint8)
            assert np.array_equal(yf.update_plane(hist, res), compref.fade_update(hist, res))
    # all byte pairs
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert np.array_equal(yf.update_plane(a, b), compref.fade_update(a, b))
    for alpha in (F(0.5), F(0.1)):
        assert np.array_equal(yf.blend_plane(b, a, 0, 0, 0, alpha, F(1) - alpha), compref.fade_blend(a, b, alpha, F(1) - alpha))


def test_the_stream_step_of_a_gray_surface_is_comprefs():
    """Y alone (a 4:4:4 surface whose three planes are one picture), fill 0, through a change of geometry: blended frame, history, count
    and alpha are compref.fade_stream_step's, frame after frame, with the history updated by a stand-in for the warp."""
    rng = np.random.default_rng(6)
    hist = chist = None
    count = ccount = 0
    for k in range(12):
        w, h = (40, 24) if k < 8 else (36, 24)
        frame = rng.integers(0, 256, (h, w), np.uint8)
        blended, hist, count, a = yf.stream_step(hist, count, [frame, frame, frame], 0, 0, 6, (0, 0, 0), 0.5, 4)
        cb, chist, ccount, ca = compref.fade_stream_step(chist, ccount, frame, 6, 0.5, 4)
        assert count == ccount and a == ca and (k not in (0, 8) or (count == 1 and a == 0))
        for p, hp in zip(blended, hist):
            assert np.array_equal(p, cb) and np.array_equal(hp, chist)
        result = np.roll(cb, 3, axis=1)
        hist = [yf.update_plane(hp, result) for hp in hist]
        chist = compref.fade_update(chist, result)


def _round_f32(x):
    """The float32 nearest to the non-negative Fraction x, ties to even, by integer arithmetic (normal range)."""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return n * ulp


def _exact_blend(h, f, alpha, beta, top):
    al, be = Fraction(float(F(alpha))), Fraction(float(F(beta)))
    v = _round_f32(int(h) * al + _round_f32(int(f) * be))
    return min(max(round(v), 0), top)          # round(Fraction): half to even


def test_words_are_exact_rational_arithmetic():
    rng = np.random.default_rng(7)
    ramp = [compref.fade_alpha(0.1, c, 30)[0] for c in range(31)]
    assert len(set(float(a) for a in ramp)) == 31 and ramp[0] == 0 and ramp[30] == F(0.1)
    cases = []
    # ties at alpha = 0.5 (an odd sum), both parities of the half
    ties = [(1, 0), (0, 1), (2, 1), (3, 0), (65535, 65534), (65534, 65533), (4097, 1024), (1023, 64), (0x8001, 0x8000), (5, 2), (7, 4)]
    cases += [(h, f, F(0.5), F(0.5)) for h, f in ties]
    # saturation: both weights 1
    cases += [(65535, 65535, F(1), F(1)), (65535, 1, F(1), F(1)), (40000, 30000, F(1), F(1)), (32768, 32767, F(1), F(1)), (32768, 32768, F(1), F(1))]
    special = [0, 1, 63, 64, 1023, 4095, 0x8000, 0xffc0, 65535]
    for a in ramp + [F(0.5)]:
        hs = np.concatenate([special, rng.integers(0, 65536, 60)])
        fs = np.concatenate([special[::-1], rng.integers(0, 65536, 60)])
        cases += [(int(h), int(f), a, F(1) - a) for h, f in zip(hs, fs)]
    assert any(_exact_blend(h, f, a, b, 1 << 20) > 65535 for h, f, a, b in cases)                       # saturation is in the sample
    assert sum((h + f) % 2 == 1 and a == F(0.5) for h, f, a, b in cases) >= len(ties)
    for h, f, a, b in cases:
        got = yf.blend_plane(np.array([[f]], np.uint16), np.array([[h]], np.uint16), 0, 0, 0, a, b)
        assert int(got[0, 0]) == _exact_blend(h, f, a, b, 65535), (h, f, float(a))
    assert int(yf.blend_plane(np.array([[0]], np.uint16), np.array([[1]], np.uint16), 0, 0, 0, F(0.5), F(0.5))[0, 0]) == 0      # 0.5 -> 0
    assert int(yf.blend_plane(np.array([[2]], np.uint16), np.array([[1]], np.uint16), 0, 0, 0, F(0.5), F(0.5))[0, 0]) == 2      # 1.5 -> 2
    # the update: exact products, each rounded, their sum rounded, truncated
    keep, rate = Fraction(float(F(1.0) - F(0.1))), Fraction(float(F(0.1)))
    hs, rs = rng.integers(0, 65536, 400), rng.integers(0, 65536, 400)
    hs[:9], rs[:9] = special, special[::-1]
    got = yf.update_plane(hs.astype(np.uint16), rs.astype(np.uint16))
    for h, r, g in zip(hs, rs, got):
        v = _round_f32(_round_f32(keep * int(h)) + _round_f32(rate * int(r)))
        assert int(g) == v.numerator // v.denominator, (h, r)


def test_weights_outside_the_exact_range_are_refused_by_the_statement():
    one = np.ones((1, 1), np.uint16)
    with pytest.raises(AssertionError):
        yf.blend_plane(one, one, 0, 0, 0, F(2.0 ** -13), F(1))
    with pytest.raises(AssertionError):
        yf.blend_plane(one, one, 0, 0, 0, F(0.5), F(1.5))


@pytest.mark.parametrize("cn", [1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_alpha_0_is_the_black_pad(dtype, cn):
    rng = np.random.default_rng(11 + cn)
    top = np.iinfo(dtype).max + 1
    for (w, h), (bx, by) in (((1, 1), (3, 3)), ((5, 4), (7, 7)), ((64, 48), (15, 30)), ((40, 40), (0, 0))):
        shape = (h, w) if cn == 1 else (h, w, cn)
        plane = rng.integers(0, top, shape, dtype=dtype)
        hist = rng.integers(0, top, (h + 2 * by, w + 2 * bx) + shape[2:], dtype=dtype)
        fill = [int(v) for v in rng.integers(1, top, cn)]
        fill = fill[0] if cn == 1 else fill
        assert np.array_equal(yf.blend_plane(plane, hist, bx, by, fill, F(0), F(1)), yp.pad_plane(plane, bx, by, yp.BLACK, fill))


def test_stream_step_pads_every_plane_by_its_shifts_and_starts_with_the_frame():
    rng = np.random.default_rng(12)
    y, uv = rng.integers(0, 65536, (48, 64), np.uint16), rng.integers(0, 65536, (24, 32, 2), np.uint16)
    fill = (0x1000, 0x8000, 0x7000)
    blended, hist, count, a = yf.stream_step(None, 5, [y, uv], 1, 1, 6, fill, 0.5, 4)
    assert count == 1 and a == 0 and blended[0].shape == (60, 76) and blended[1].shape == (30, 38, 2)
    for p, hp, q in zip(blended, hist, yp.pad_surface([y, uv], 1, 1, 6, yp.BLACK, fill)):
        assert np.array_equal(p, q) and np.array_equal(hp, q)
    assert blended[1][0, 0, 0] == 0x8000 and blended[1][0, 0, 1] == 0x7000
    blended2, hist2, count, a = yf.stream_step(hist, count, [y[::-1], uv[::-1]], 1, 1, 6, fill, 0.5, 4)
    assert count == 2 and a == F(0.5) * (F(1) / F(4)) and hist2 is hist
    assert np.array_equal(blended2[0], yf.blend_plane(y[::-1], hist[0], 6, 6, fill[0], a, F(1) - a))
    with pytest.raises(AssertionError):
        yf.stream_step(None, 0, [y, uv], 1, 1, 5, fill, 0.5, 4)


# ---- 2. the refusal rules ----------------------------------------------------------------------------------------------------
YUV = ("NV12", "P010", "I420", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412")
SUBSAMPLED = ("NV12", "P010", "I420", "I010", "I012", "I422", "I210", "I212")


def _rules(cases):
    """cases: [(fmt, w, h, pitch, border, crop, canvas, fade, pad_mode, fade_mode, out_c_pitch)] -> [((rc, text) with the modes, (rc,
    text) with the default arguments)]"""
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(ROOT, "tests", "cpp", "yuv_fade_check.cpp"), os.path.join(build, "yuv_fade_check")
    deps = [src, os.path.join(ROOT, "video-stab_amd", "csrc", "pixfmt.h"), os.path.join(ROOT, "include", "vs_stab.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split("|") for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases) and all(len(x) == 4 for x in rows), r.stdout
    return [((int(a), b), (int(c), d)) for a, b, c, d in rows]


def _pitch(name):
    return 64 * capi.fmt_px_bytes(getattr(capi, "FMT_" + name))


def test_without_the_mode_every_answer_is_todays():
    """The recorded answers of the border cases (tests/golden/stream_refusals.json), asked with the mode off and with the arguments
    left out; the mode on changes none of the crop-and-zoom and border-pad answers."""
    golden = refusal_cases.load_golden(os.path.join(ROOT, "tests", "golden", "stream_refusals.json"))
    todo = [c for c in refusal_cases.cases() if c.entry == "push_dev" and c.border > 0 and not refusal_cases.stateful(c) and not c.data_odd and not c.out_odd
            and c.nv12 == (0, 0) and c.i420 == (0,) * 6 and c.out_pitch == c.pitch]
    assert len(todo) >= 3 * 16
    for c, (with_mode, default) in zip(todo, _rules([(c.fmt, c.w, c.h, c.pitch, c.border, c.crop, c.canvas, c.fade, 0, 0, 0) for c in todo])):
        assert with_mode == default == golden[c.id], c.id
    same = [c for c in todo if c.crop or not c.fade]
    assert len(same) >= 2 * 16
    for c, (with_mode, default) in zip(same, _rules([(c.fmt, c.w, c.h, c.pitch, c.border, c.crop, c.canvas, c.fade, 0, 1, 0) for c in same])):
        assert with_mode == default == golden[c.id], c.id


@pytest.mark.parametrize("name", YUV)
def test_with_the_mode_the_fade_passes_and_the_other_border_modes_keep_their_texts(name):
    fmt, p = getattr(capi, "FMT_" + name), _pitch(name)
    rows = _rules([(fmt, 64, 48, p, 8, 0, 0, 1, 0, 1, 0),      # the fade, an even border
                   (fmt, 64, 48, p, 5, 0, 0, 1, 0, 1, 0),      # an odd one
                   (fmt, 64, 48, p, 8, 0, 0, 0, 0, 1, 0),      # a pad with only the fade mode on
                   (fmt, 64, 48, p, 8, 0, 0, 1, 1, 0, 0),      # the fade with only the pad mode on
                   (fmt, 64, 48, p, 8, 0, 1, 1, 0, 1, 0),      # the canvas on a fade stream
                   (fmt, 64, 48, p, 0, 0, 1, 1, 0, 1, 0),      # the canvas alone
                   (fmt, 64, 48, p, 8, 1, 0, 1, 0, 1, 0),      # crop-and-zoom (its mode off)
                   (fmt, 64, 48, p, 8, 0, 0, 1, 1, 1, 0),      # the fade with both modes on
                   (fmt, 64, 48, p, 8, 0, 0, 0, 1, 1, 0)])     # a pad with both modes on
    (even, d_even), (odd, d_odd), (pad, d_pad), (fadepad, d_fadepad), (canvas, _), (canvas0, d_canvas0), (crop, d_crop), (both, _), (padboth, _) = rows
    assert even == (0, "") and both == (0, "") and padboth == (0, "")
    assert d_even[0] == 4 and "colour format" in d_even[1]       # VS_ERR_UNSUPPORTED without the mode
    if name in SUBSAMPLED:
        assert odd[0] == 1 and name in odd[1] and "fade on" in odd[1] and "even border_size" in odd[1]
    else:
        assert odd == (0, "")
    assert d_odd == d_even
    assert pad == d_pad and pad[0] == 4
    assert fadepad == d_fadepad == d_even
    assert canvas0 == d_canvas0 and canvas0[0] == 4 and "enableVirtualCanvas needs a BGR8 stream" in canvas0[1]
    assert canvas == canvas0
    assert crop == d_crop and crop[0] == 4


@pytest.mark.parametrize("name", ["I420", "I210", "I444"])
def test_an_explicit_output_chroma_pitch_holds_a_padded_chroma_row(name):
    fmt, p = getattr(capi, "FMT_" + name), _pitch(name)
    info = capi.PIXFMT_BY_NAME[name]
    sb = 1 if info.bits == 8 else 2
    row = ((64 + 16) >> info.sx) * sb
    short, fits = _rules([(fmt, 64, 48, p, 8, 0, 0, 1, 0, 1, row - 2), (fmt, 64, 48, p, 8, 0, 0, 1, 0, 1, row)])
    assert short[0][0] == 1 and "padded chroma row" in short[0][1] and "fade on " + name in short[0][1]
    assert fits[0] == (0, "")


def test_with_the_mode_gray8_and_the_colour_formats_answer_as_before():
    for name in ("GRAY8", "BGR8", "BGRA8", "RGBA8", "RGB8"):
        fmt, p = getattr(capi, "FMT_" + name), _pitch(name)
        for a, d in _rules([(fmt, 64, 48, p, 8, 0, 0, 1, 0, 1, 0), (fmt, 64, 48, p, 5, 0, 0, 1, 0, 1, 0), (fmt, 64, 48, p, 8, 0, 0, 0, 0, 1, 0)]):
            assert a == d, name
    assert _rules([(capi.FMT_GRAY8, 64, 48, 64, 8, 0, 0, 1, 0, 1, 0)])[0][0][0] == 4


# ---- 3. the ABI surface ------------------------------------------------------------------------------------------------------
NEW = ("vs_stab_set_yuv_fade", "vs_op_fade_blend_jobs", "vs_op_fade_update_jobs")


def test_the_new_entry_points_are_exported_and_declared():
    vs = capi.load()
    header = open(os.path.join(ROOT, "include", "vs_stab.h")).read()
    for name in NEW:
        assert hasattr(vs.lib, name), name + " is not exported by libvideo-stab.so"
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/vs_stab.h"
    assert not hasattr(vs.lib, "vs_batch_set_yuv_fade")
    assert vs.lib.vs_abi_version() == 2
    assert C.sizeof(capi.VsFadeJob) == 80 and C.sizeof(capi.VsFadeUpdateJob) == 48 and C.sizeof(capi.VsYuvFill) == 8
    assert capi.VsFadeJob.fill.offset == 64 and capi.VsFadeJob.cn.offset == 68 and capi.VsFadeJob.reserved.offset == 72
    assert capi.VsFadeUpdateJob.w.offset == 32 and capi.VsFadeUpdateJob.reserved.offset == 44


def test_the_operators_refuse_on_the_host_and_need_a_device_after_that():
    """A bad argument is answered before a device is looked for, so the addresses below are never read; with good arguments and no
    device the answer is VS_ERR_NO_DEVICE.  (A stream cannot be created without a device, so the setter has no object to take: a
    null one is VS_ERR_INVALID_ARG.)"""
    L = capi.load().lib
    for make in (pjr.fade_blend, pjr.fade_update):
        op = make(pjr.FAKE_BASE)
        pjr.check_refusals(L, op)
        if L.vs_device_count() <= 0:
            pjr.check_accepted(L, op, pjr.NO_DEVICE)
    assert L.vs_stab_set_yuv_fade(None, 1, None) == 1
