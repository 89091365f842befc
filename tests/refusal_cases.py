"""The calls a stream answers with a code and a text instead of a frame - and, next to them, the calls of the same shape that it
accepts: one list of cases for tests/golden/make_stream_refusals.py (which records the answers), tests/test_gpu_stream_refusals.py
(which asks the library again) and tests/test_stream_refusals_cpu.py (which asks the rules alone, without a stream).

A case is a short script over ONE fresh stream (smoothing_radius 5, two buffers of 1 MiB): the stream's modes, the layouts stored
before the first frame, then the entry point under test with its geometry, pitches and pointer parities.  What is recorded is the
code and the text of the LAST call; the calls before it (`flush*`: one accepted push; `set_*`: an accepted push and the flush that
drains it) must succeed.  All frames are 64 x 48, variants use 63 and 47.  No case pushes more than two frames.

`probe` cases are stateful: the first push is refused, a valid 32 x 24 frame follows, and ITS answer is recorded - VS_OK if the
refused call left the stream unallocated, VS_ERR_SIZE_CHANGED if it allocated.  Only a stream can answer them."""
import collections
import ctypes as C

import numpy as np

from vsamd import capi

NAMES = ("BGR8", "NV12", "GRAY8", "BGRA8", "RGBA8", "RGB8", "P010", "I420", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412")
ENTRIES = ("push_dev", "flush_dev", "push", "flush", "set_i420", "set_nv12", "probe")
W, H = 64, 48
BUF = 1 << 20

Case = collections.namedtuple("Case", "id fmt entry w h pitch border crop fade canvas batch pipe zc nv12 i420 data_odd out_odd out_pitch setter")


def _facts(name):
    fmt = getattr(capi, "FMT_" + name)
    sb = 2 if capi.fmt_dtype(fmt) == np.uint16 else 1
    sx = capi.FMT_CHROMA_SHIFTS.get(fmt, (1, 1))[0]
    sy = capi.FMT_CHROMA_SHIFTS.get(fmt, (1, 1))[1]
    return fmt, sb, W * capi.fmt_px_bytes(fmt), (W >> sx) * sb, sy, fmt in capi.FMT_CHROMA_SHIFTS


def _format_cases(name):
    fmt, sb, p, crow, sy, planar = _facts(name)
    out_rule = sb == 2 or name in ("I420", "I422")      # an odd pitch or pointer of an output surface is refused (the other formats have no such rule)
    out = []

    def add(tag, entry="push_dev", **kw):
        d = dict(w=W, h=H, pitch=p, border=0, crop=0, fade=0, canvas=0, batch=1, pipe=0, zc=0, nv12=(0, 0), i420=(0,) * 6, data_odd=0, out_odd=0,
                 out_pitch=p, setter=(0,) * 6)
        d.update(kw)
        out.append(Case(id="%s/%s/%s" % (name, tag, entry), fmt=fmt, entry=entry, **d))

    # ---- accepted pushes (some formats refuse the odd sizes)
    for b in (1, 8):
        add("tight.b%d" % b, batch=b)
        add("w63.b%d" % b, batch=b, w=63)
        add("h47.b%d" % b, batch=b, h=47)
        add("w63h47.b%d" % b, batch=b, w=63, h=47)
        if planar:
            add("p+2.cp.b%d" % b, batch=b, pitch=p + 2, i420=(0, 0, crow, 0, 0, crow))
            add("p+2.cp+2.b%d" % b, batch=b, pitch=p + 2, out_pitch=p + 2, i420=(0, 0, crow + 2, 0, 0, crow + 2), zc=1 if b == 1 else 0)
    # ---- the input side
    add("p-1", pitch=p - 1)
    add("p+1", pitch=p + 1)
    add("p+1.b8", pitch=p + 1, batch=8)
    if planar:
        add("p+2", pitch=p + 2)
    add("in_cp-", i420=(0, 0, crow - sb, 0, 0, 0))
    add("out_cp-", i420=(0, 0, 0, 0, 0, crow - sb))
    add("in_u.odd", i420=(p * H + 1, 0, 0, 0, 0, 0))
    add("out_v.odd", i420=(0, 0, 0, 0, p * H + crow * (H >> sy) + 1, 0))
    if name in ("NV12", "P010"):
        add("in_uv.odd", nv12=(p * H + 1, 0))
        add("out_uv.odd", nv12=(0, p * H + 1))
    add("w0", w=0)
    # ---- modes
    add("border", border=8)
    add("border.crop", border=8, crop=1)
    add("border.fade", border=8, fade=1)
    add("canvas", canvas=1)
    add("canvas.b8", canvas=1, batch=8)
    # ---- the output side, through every entry point that takes an output
    for entry, pipe in (("push_dev", 0), ("flush_dev", 0), ("push", 0), ("flush", 0), ("push", 1), ("flush", 1)):
        t = ".pipe" if pipe else ""
        for d in (1, 3, 6, -1):
            # (a device pitch below the row bytes that no rule refuses goes to hipMemcpy2DAsync, which fails and leaves its error in
            # the runtime for the next stream's first launch to find: not a refusal of the library, and not asked)
            if d > 0 or entry != "flush_dev" or out_rule:
                add("out.p%+d%s" % (d, t), entry, pipe=pipe, out_pitch=p + d)
        add("out.odd%s" % t, entry, pipe=pipe, out_odd=1)
        if entry.startswith("push"):
            add("data.odd%s" % t, entry, pipe=pipe, data_odd=1)
        add("out.p+2.cp%s" % t, entry, pipe=pipe, out_pitch=p + 2, i420=(0, 0, 0, 0, 0, crow + 2))
    # ---- the setters once the geometry is known and the queue is empty
    add("cp-.in", "set_i420", setter=(0, 0, crow - sb, 0, 0, 0))
    add("cp-.out", "set_i420", setter=(0, 0, 0, 0, 0, crow - sb))
    for i, t in ((0, "in_u"), (1, "in_v"), (3, "out_u"), (4, "out_v")):
        s = [0] * 6
        s[i] = p * H + crow * (H >> sy) + 1
        add(t + ".odd", "set_i420", setter=tuple(s))
    add("valid", "set_i420", setter=(p * H, p * H + crow * (H >> sy), crow, p * H, p * H + crow * (H >> sy), crow + 2 * sb))
    add("in.odd", "set_nv12", setter=(p * H + 1, 0, 0, 0, 0, 0))
    add("out.odd", "set_nv12", setter=(0, p * H + 1, 0, 0, 0, 0))
    add("valid", "set_nv12", setter=(p * H, p * H + 2 * p, 0, 0, 0, 0))
    # ---- did the refused call allocate?  (stateful)
    add("in.refused", "probe", pitch=p - 1)
    if out_rule:
        add("out.refused", "probe", out_pitch=p + 1, out_odd=1)
    return out


def _pairs():
    """Two violations in one call: the order of the checks decides the text."""
    out = []

    def add(name, tag, entry="push_dev", **kw):
        fmt, sb, p, crow, sy, planar = _facts(name)
        d = dict(w=W, h=H, pitch=p, border=0, crop=0, fade=0, canvas=0, batch=1, pipe=0, zc=0, nv12=(0, 0), i420=(0,) * 6, data_odd=0, out_odd=0,
                 out_pitch=p, setter=(0,) * 6)
        for k, v in kw.items():
            d[k] = v(p, crow, sb) if callable(v) else v
        out.append(Case(id="%s/two.%s/%s" % (name, tag, entry), fmt=fmt, entry=entry, **d))

    for name in ("I420", "I210", "NV12"):
        add(name, "w63+p+1", w=63, pitch=lambda p, c, s: p + 1)
    for name in ("I010", "I422", "P010", "GRAY8"):
        add(name, "p+1+border", pitch=lambda p, c, s: p + 1, border=8)
    for name in ("I420", "I412", "I012"):
        add(name, "in_cp-+border", i420=lambda p, c, s: (0, 0, c - s, 0, 0, 0), border=8)
    add("P010", "in_uv.odd+w63", w=63, nv12=lambda p, c, s: (p * H + 1, 0))
    for name in ("I010", "P010", "I410"):
        add(name, "out.p+1+out.odd", out_pitch=lambda p, c, s: p + 1, out_odd=1)
        add(name, "out.p+1+out.odd", "flush_dev", out_pitch=lambda p, c, s: p + 1, out_odd=1)
    add("NV12", "border+p-1", border=8, pitch=lambda p, c, s: p - 1)
    add("I444", "canvas+border", canvas=1, border=8)
    add("I420", "canvas+out.p+1", canvas=1, out_pitch=lambda p, c, s: p + 1)
    add("I210", "in_u.odd+in_cp-", i420=lambda p, c, s: (p * H + 1, 0, c - s, 0, 0, 0))
    add("GRAY8", "border+w0", border=8, w=0)
    add("I212", "cp-+odd", "set_i420", setter=lambda p, c, s: (p * H + 1, 0, c - s, 0, 0, 0))
    add("I422", "out.p-1+odd", "flush", out_pitch=lambda p, c, s: p - 1)
    return out


def _unknown():
    d = dict(entry="push_dev", w=W, h=H, pitch=W * 3, border=0, crop=0, fade=0, canvas=0, batch=1, pipe=0, zc=0, nv12=(0, 0), i420=(0,) * 6, data_odd=0,
             out_odd=0, out_pitch=W * 3, setter=(0,) * 6)
    return [Case(id="unknown/fmt16/push_dev", fmt=16, **d), Case(id="unknown/fmt-1/push_dev", fmt=-1, **d)]


def cases(name=None):
    """All cases, or those filed under one format name ("unknown": the two format values the library does not know)."""
    if name == "unknown":
        return _unknown()
    if name is not None:
        return _format_cases(name) + [c for c in _pairs() if c.id.startswith(name + "/")]
    return [c for n in NAMES for c in cases(n)] + _unknown()


def stateful(case):
    return case.entry == "probe"


def line(case):
    """The case as pixfmt_check reads it: the id, then integers."""
    v = [case.fmt, ENTRIES.index(case.entry), case.w, case.h, case.pitch, case.border, case.crop, case.fade, case.canvas, case.batch, case.pipe, case.zc]
    v += list(case.nv12) + list(case.i420) + [case.data_odd, case.out_odd, case.out_pitch] + list(case.setter)
    return case.id + " " + " ".join(str(int(x)) for x in v)


def drive(vs, case):
    """The case through the C ABI -> (code, text) of its last call; text "" with VS_OK."""
    L = vs.lib
    kw = dict(smoothing_radius=5, border_size=case.border, crop_n_zoom=case.crop, enable_virtual_canvas=case.canvas)
    if case.fade:
        kw["border_type"] = capi.BORDER_FADE
    h = C.c_void_p()
    vs.check(L.vs_stab_create(C.byref(vs.params(**kw)), 0, C.byref(h)))
    d_in, d_out = capi.DevBuf(vs, BUF), capi.DevBuf(vs, BUF)
    host_in, host_out = np.zeros(BUF, np.uint8), np.zeros(BUF, np.uint8)
    produced = C.c_int32(0)

    def must(rc):
        assert rc == 0, (case.id, rc, (L.vs_stab_last_error(h) or b"").decode())

    def push_dev(w, hh, pitch, fmt, data_odd, out_odd, out_pitch):
        return L.vs_stab_push_dev(h, C.c_void_p(d_in.ptr + data_odd), w, hh, pitch, fmt, C.c_void_p(d_out.ptr + out_odd), out_pitch, C.byref(produced))

    def push_host(w, hh, pitch, fmt, data_odd, out_odd, out_pitch):
        return L.vs_stab_push(h, C.cast(host_in.ctypes.data + data_odd, capi.u8p), w, hh, pitch, fmt, C.cast(host_out.ctypes.data + out_odd, capi.u8p),
                              out_pitch, C.byref(produced))

    try:
        d_in.zero()
        must(L.vs_stab_set_batch(h, case.batch))
        must(L.vs_stab_set_host_pipeline(h, case.pipe))
        must(L.vs_stab_set_zero_copy(h, case.zc))
        if any(case.nv12):
            must(L.vs_stab_set_nv12_layout(h, *case.nv12))
        if any(case.i420):
            must(L.vs_stab_set_i420_layout(h, *case.i420))
        tight = W * capi.fmt_px_bytes(case.fmt) if case.entry != "push_dev" else 0
        if case.entry == "push_dev":
            rc = push_dev(case.w, case.h, case.pitch, case.fmt, case.data_odd, case.out_odd, case.out_pitch)
        elif case.entry == "push":
            rc = push_host(case.w, case.h, case.pitch, case.fmt, case.data_odd, case.out_odd, case.out_pitch)
        elif case.entry == "flush_dev":
            must(push_dev(W, H, tight, case.fmt, 0, 0, tight))
            rc = L.vs_stab_flush_dev(h, C.c_void_p(d_out.ptr + case.out_odd), case.out_pitch, C.byref(produced))
        elif case.entry == "flush":
            must(push_host(W, H, tight, case.fmt, 0, 0, tight))
            rc = L.vs_stab_flush(h, C.cast(host_out.ctypes.data + case.out_odd, capi.u8p), case.out_pitch, C.byref(produced))
        elif case.entry in ("set_i420", "set_nv12"):
            must(push_dev(W, H, tight, case.fmt, 0, 0, tight))
            must(L.vs_stab_flush_dev(h, C.c_void_p(d_out.ptr), tight, C.byref(produced)))
            assert produced.value == 1
            rc = L.vs_stab_set_i420_layout(h, *case.setter) if case.entry == "set_i420" else L.vs_stab_set_nv12_layout(h, *case.setter[:2])
        else:
            rc = push_dev(case.w, case.h, case.pitch, case.fmt, case.data_odd, case.out_odd, case.out_pitch)
            assert rc != 0, (case.id, "the first push of a probe must be refused")
            rc = push_dev(32, 24, tight // 2, case.fmt, 0, 0, tight // 2)
        text = (L.vs_stab_last_error(h) or b"").decode() if rc != 0 else ""
        return rc, text
    finally:
        L.vs_stab_sync(h)
        L.vs_stab_destroy(h)
        d_in.free()
        d_out.free()


def load_golden(path):
    """stream_refusals.json -> {id: (code, text)}"""
    import json
    with open(path) as f:
        g = json.load(f)
    return {k: tuple(g["answers"][i]) for k, i in g["cases"].items()}
