"""What the sixteen asynchronous entry points of the roll and the zoom/crop stage - vs_roll_correct_{nv12,p010,i420,rgb}_dev[_n],
vs_azc_apply_{nv12,p010,i420,rgb}_dev[_n] - refuse, and next to each group of refusals a call of the same shape that they accept: one
case table for tests/golden/make_stage_refusals.py (which records code and text) and tests/test_gpu_stage_refusals.py (which holds the
library to the record).

Every case is a 64 x 48 frame on zeroed device buffers, asked of a FRESH object (a stale text cannot leak into the record), and
followed by a sync.  A case changes arguments of the entry's good call: a value, or a function of the arguments so far (changes apply
in the order written).  Keys beside the arguments: fmt (read first: the good call depends on it), size (vs_azc_set_output_size before
the call), src_add / dst_add (bytes added to the pointers), src_null / dst_null / obj_null / in_null / out_null, and for the _n forms
n, srcs_null / dsts_null and hole (the surface of the list that is a null pointer).  No refused call reaches the device, so the sizes
of the limit cases need no memory."""
import collections
import ctypes as C

from vsamd import capi

OK, INVALID = 0, 1
W, H = 64, 48
SRC_BYTES, DST_BYTES = 1 << 20, 4 << 20
FAMILIES = ("nv12", "p010", "i420", "rgb")
ENTRIES = [(stage, fam, many) for stage in ("roll", "azc") for fam in FAMILIES for many in (False, True)]

Case = collections.namedtuple("Case", "name rc word ch")


def entry_name(stage, fam, many):
    return "vs_%s_%s_dev%s" % ("roll_correct" if stage == "roll" else "azc_apply", fam, "_n" if many else "")


def _c(name, rc=INVALID, word="", **ch):
    return Case(name, rc, word, ch)


def good_call(stage, fam, fmt, size):
    """The arguments of the entry's good call; mw x mh: what the result must hold."""
    ow, oh = (W, H) if stage == "roll" or size == (0, 0) else size
    mw, mh = max(W, ow), max(H, oh)
    f = capi.PIXFMT[fmt]
    px = f.cn if fam == "rgb" else f.sample_bytes
    a = dict(fmt=fmt, w=W, h=H, mw=mw, mh=mh, pitch=W * px, opitch=mw * px)
    if fam in ("nv12", "p010"):
        a.update(uv=0, ouv=mh * a["opitch"] if stage == "azc" else 0)
    if fam == "i420":
        a.update(cp=0, u=0, v=0, ocp=0, ou=0, ov=0)
    return a


def _full(a):        # the out_uv_offset that goes with the arguments' out_pitch
    return a["mh"] * a["opitch"]


def _geometry():
    return [_c("w-odd", w=63), _c("h-odd", h=47), _c("w-0", w=0), _c("h-0", h=0), _c("w-neg", w=-2),
            _c("pitch-short", pitch=lambda a: a["pitch"] - 2), _c("opitch-short", opitch=lambda a: a["opitch"] - 2)]


def _nulls():
    return [_c("src-null", src_null=True), _c("dst-null", dst_null=True), _c("obj-null", obj_null=True)]


def _azc_limits(fam):
    """w > 65535, h > 32767 with everything else large enough to get there; the colour entry's 4 GiB rule."""
    px = 4 if fam == "rgb" else 2 if fam == "p010" else 1
    wide = dict(w=65536, pitch=65536 * px, opitch=65536 * px)
    tall = dict(h=32768)
    if fam in ("nv12", "p010"):
        wide["ouv"] = 360 * 65536 * px
        tall["ouv"] = lambda a: 32768 * a["opitch"]
    L = [_c("w-65536", word="too large", **wide), _c("h-32768", word="too large", **tall)]
    if fam == "rgb":
        L += [_c("stride-4g", word="4 GiB", pitch=1 << 32), _c("out-stride-4g", word="4 GiB", opitch=1 << 32)]
    return L


def _azc_sizes(fam):
    L = []
    for size in ((32, 24), (128, 96), (0, 0)):
        t = "%dx%d" % size
        L += [_c("size-" + t, OK, size=size), _c("size-%s-opitch-short" % t, size=size, opitch=lambda a: a["opitch"] - 2)]
        if fam in ("nv12", "p010"):
            L.append(_c("size-%s-ouv-short" % t, size=size, ouv=lambda a: a["ouv"] - 2))
        if fam == "i420":
            L.append(_c("size-%s-ou-short" % t, size=size, word="behind the luma rows", ou=lambda a: _full(a) - 2))
    return L


def _luma_uv(stage, fam):
    azc = stage == "azc"
    L = [_c("good", OK),
         _c("explicit-offsets", OK, uv=lambda a: a["h"] * a["pitch"] + 64, ouv=lambda a: _full(a) + 64),
         _c("wide-pitches", OK, pitch=lambda a: a["pitch"] + 64, opitch=lambda a: a["opitch"] + 64, ouv=lambda a: _full(a) if azc else 0)]
    L += _geometry() + _nulls()
    if azc:
        L += [_c("ouv-short", ouv=lambda a: a["ouv"] - 2), _c("ouv-0", ouv=0)]
    if fam == "p010":
        L += [_c("src-odd", word="even", src_add=1), _c("dst-odd", word="even", dst_add=1),
              _c("pitch-odd", word="even", pitch=lambda a: a["pitch"] + 1),
              _c("uv-odd", word="even", uv=lambda a: a["h"] * a["pitch"] + 1),
              _c("opitch-odd", word="even", opitch=lambda a: a["opitch"] + 1, ouv=lambda a: (_full(a) + 1) & ~1 if azc else 0),
              _c("ouv-odd", word="even", ouv=lambda a: _full(a) + 1)]
    return L


def _three_planes(stage):
    I420, I010, I444, I422 = capi.FMT_I420, capi.FMT_I010, capi.FMT_I444, capi.FMT_I422
    L = [_c("good", OK), _c("good-i010", OK, fmt=I010), _c("good-i422", OK, fmt=I422), _c("good-i444", OK, fmt=I444),
         _c("yv12", OK, v=lambda a: a["h"] * a["pitch"], u=lambda a: a["v"] + (a["h"] // 2) * (a["pitch"] // 2),
            ov=lambda a: _full(a), ou=lambda a: a["ov"] + (a["mh"] // 2) * (a["opitch"] // 2)),
         _c("explicit-chroma-pitch", OK, cp=lambda a: a["pitch"] // 2 + 16, ocp=lambda a: a["opitch"] // 2 + 16)]
    L += _geometry() + _nulls()
    L += [_c("in-null", in_null=True), _c("out-null", out_null=True),
          _c("cp-short", word="chroma pitch", cp=30), _c("ocp-short", word="chroma pitch", ocp=30),
          _c("cp-short-i444", word="chroma row", fmt=I444, cp=62),
          _c("u-in-luma", word="behind the luma rows", u=lambda a: a["h"] * a["pitch"] - 2),
          _c("ov-in-luma", word="behind the luma rows", ov=lambda a: _full(a) - 2),
          _c("uv-overlap", word="overlap", u=lambda a: a["h"] * a["pitch"], v=lambda a: a["u"] + 2),
          _c("pitch-odd", word="even pitch", pitch=65), _c("opitch-odd", word="even pitch", opitch=lambda a: a["opitch"] + 1),
          _c("src-odd-16", word="even", fmt=I010, src_add=1), _c("dst-odd-16", word="even", fmt=I010, dst_add=1),
          _c("pitch-130-16", word="multiple of 4", fmt=I010, pitch=130), _c("pitch-odd-16", word="even", fmt=I010, pitch=129),
          _c("cp-odd-16", word="even", fmt=I010, cp=65), _c("u-odd-16", word="even", fmt=I010, u=lambda a: a["h"] * a["pitch"] + 1),
          _c("v-odd-16", word="even", fmt=I010, v=lambda a: a["h"] * a["pitch"] * 2 + 1),
          _c("ou-odd-16", word="even", fmt=I010, ou=lambda a: _full(a) + 1)]
    L += [_c("fmt-%s" % n, word="three-plane format", fmt=f) for n, f in
          (("nv12", capi.FMT_NV12), ("p010", capi.FMT_P010), ("bgr8", capi.FMT_BGR8), ("gray8", capi.FMT_GRAY8), ("99", 99), ("neg", -1))]
    return L


def _colour(stage):
    L = [_c("good-%s" % n, OK, fmt=f) for n, f in
         (("bgr8", capi.FMT_BGR8), ("rgb8", capi.FMT_RGB8), ("bgra8", capi.FMT_BGRA8), ("rgba8", capi.FMT_RGBA8))]
    L.append(_c("wide-strides", OK, pitch=lambda a: a["pitch"] + 64, opitch=lambda a: a["opitch"] + 64))
    L += [c for c in _geometry() if c.name not in ("w-odd", "h-odd")] + _nulls()
    L += [_c("fmt-%s" % n, word="not an interleaved colour format", fmt=f) for n, f in
          (("nv12", capi.FMT_NV12), ("gray8", capi.FMT_GRAY8), ("i420", capi.FMT_I420), ("p010", capi.FMT_P010), ("99", 99), ("neg", -1))]
    return L


def cases(stage, fam, many):
    L = _luma_uv(stage, fam) if fam in ("nv12", "p010") else _three_planes(stage) if fam == "i420" else _colour(stage)
    if stage == "azc":
        L += _azc_limits(fam) + _azc_sizes(fam)
    if many:
        L += [_c("n-0", INVALID if fam == "rgb" else OK, n=0), _c("n-neg", n=-1), _c("n-1", OK, n=1), _c("n-3", OK, n=3),
              _c("srcs-null", srcs_null=True), _c("dsts-null", dsts_null=True), _c("hole", n=3, hole=1)]
    assert len(set(c.name for c in L)) == len(L)
    return L


DEFAULT_FMT = dict(nv12=capi.FMT_NV12, p010=capi.FMT_P010, i420=capi.FMT_I420, rgb=capi.FMT_BGRA8)


def arguments(stage, fam, case):
    """(the call's arguments as a dict, the changes that are not arguments)."""
    ch = dict(case.ch)
    fmt = ch.pop("fmt", DEFAULT_FMT[fam])
    # (a format the table does not know: the good call of the family's default, asked with that format)
    a = good_call(stage, fam, fmt if fmt in capi.PIXFMT and (fam != "rgb" or capi.PIXFMT[fmt].cn >= 3) else DEFAULT_FMT[fam], ch.get("size", (640, 360)))
    a["fmt"] = fmt
    rest = {}
    for k, v in ch.items():
        if k in a:
            a[k] = v(a) if callable(v) else v
        else:
            rest[k] = v
    return a, rest


def ask(vs, stage, fam, many, case, src, dst):
    """(rc, text of the object's last error) of the case's call on a fresh object; src, dst: zeroed DevBufs of SRC_BYTES / DST_BYTES."""
    lib = vs.lib
    a, r = arguments(stage, fam, case)
    obj = None if r.get("obj_null") else (vs.roll_correction() if stage == "roll" else vs.auto_zoom_crop())
    h = obj.h if obj else None
    if obj and "size" in r:
        assert lib.vs_azc_set_output_size(h, *r["size"]) == OK
    s = None if r.get("src_null") else src.ptr + r.get("src_add", 0)
    d = None if r.get("dst_null") else dst.ptr + r.get("dst_add", 0)
    if fam in ("nv12", "p010"):
        geo, lay = [a["w"], a["h"]], [[a["pitch"], a["uv"]], [a["opitch"], a["ouv"]]]
    elif fam == "i420":
        lin = None if r.get("in_null") else C.byref(capi.i420_layout(a["pitch"], a["cp"], a["u"], a["v"]))
        lout = None if r.get("out_null") else C.byref(capi.i420_layout(a["opitch"], a["ocp"], a["ou"], a["ov"]))
        geo, lay = [a["w"], a["h"]], [[lin], [lout]]
    else:
        geo, lay = [a["w"], a["h"]], [[a["pitch"]], [a["opitch"]]]
    head = [h] + ([a["fmt"]] if fam in ("i420", "rgb") else [])
    if many:
        n = r.get("n", 2)
        k = max(n, 1)
        ss, dd = (C.c_void_p * k)(*[s] * k), (C.c_void_p * k)(*[d] * k)
        if "hole" in r:
            ss[r["hole"]] = None
        tickets = [(C.c_int64 * k)()] if stage == "azc" else []
        args = head + [None if r.get("srcs_null") else ss, None if r.get("dsts_null") else dd, n] + geo + lay[0] + lay[1] + tickets
    else:
        args = head + [s] + geo + lay[0] + [d] + lay[1] + ([C.byref(C.c_int64())] if stage == "azc" else [])
    rc = getattr(lib, entry_name(stage, fam, many))(*args)
    last = lib.vs_roll_last_error if stage == "roll" else lib.vs_azc_last_error
    text = (last(h) or b"").decode()
    if obj:
        (lib.vs_roll_sync if stage == "roll" else lib.vs_azc_sync)(h)
        obj.close()
    return rc, text


def every_case():
    for stage, fam, many in ENTRIES:
        for c in cases(stage, fam, many):
            yield stage, fam, many, c


def buffers(vs):
    src, dst = capi.DevBuf(vs, SRC_BYTES), capi.DevBuf(vs, DST_BYTES)
    src.zero()
    dst.zero()
    return src, dst


def recorded(vs):
    """[entry, case, rc, text] of every case."""
    src, dst = buffers(vs)
    return [[entry_name(stage, fam, many), c.name] + list(ask(vs, stage, fam, many, c, src, dst)) for stage, fam, many, c in every_case()]
