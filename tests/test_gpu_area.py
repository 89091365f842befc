"""Area-averaging downscale on the device, bit for bit against tests/arearef.py: vs_op_area_jobs on the three classes in one launch,
vs_op_area_yuv on the eleven surface formats, vs_op_area_rgb, and the recipe "border pad -> area downscale to a proxy size" behind
a stream without a host synchronisation.

Every source lies inside a larger buffer of random bytes at an odd pitch (16-bit: an even one that is no multiple of 4) with its
first sample 1 and 3 bytes (16-bit: 2) off alignment, so a tap that leaves the sw x sh samples changes the result; every destination
is prefilled and the whole allocation is compared, so a byte written outside dw x dh is seen.  The kernel's tile is 256 bytes x 16
rows: the shapes lie on both sides of it.  There is one kernel body, so no path argument.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import arearef as ar
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

SHAPES = [((1, 1), (1, 1)), ((7, 5), (7, 5)), ((9, 9), (8, 8)), ((66, 50), (33, 25)), ((99, 60), (33, 20)), ((131, 40), (130, 37)), ((650, 100), (271, 37)),
          ((600, 90), (200, 37)), ((300, 100), (300, 41)), ((2048, 64), (37, 3)), ((1023, 35), (341, 35))]


class Jobs:
    """Planes to downscale, laid out in one source and one destination buffer."""

    def __init__(self, seed, sb):
        self.rng, self.sb, self.dtype = np.random.default_rng(seed), sb, (np.uint8 if sb == 1 else np.uint16)
        self.jobs, self.so, self.do = [], 0, 0

    def add(self, sw, sh, dw, dh, cn, off):
        """A source of sw x sh pixels inside (sh + 4) rows of random bytes, its first sample `off` bytes off alignment."""
        px, sb = self.sb * cn, self.sb
        sp = (sw + 4) * px + (3 if sb == 1 else 2)
        sp += (sp % 2 == 0) if sb == 1 else (2 if sp % 4 == 0 else 0)
        dp = dw * px + (7 if sb == 1 else 6)
        self.jobs.append(dict(a=self.so + 2 * sp + 2 * px + off, sp=sp, sw=sw, sh=sh, b=self.do + dp + off, dp=dp, dw=dw, dh=dh, cn=cn))
        self.so = (self.so + (sh + 4) * sp + 16 + 255) // 256 * 256
        self.do = (self.do + (dh + 2) * dp + 16 + 255) // 256 * 256

    def build(self):
        self.src = self.rng.integers(0, 256, self.so, np.uint8)          # (16-bit samples: the whole range, 0 .. 65535)
        self.fill = self.rng.integers(0, 256, self.do, np.uint8)
        return self

    def plane_bytes(self, buf, at, pitch, w, h, cn):
        return np.lib.stride_tricks.as_strided(buf[at:], (h, w * cn * self.sb), (pitch, 1))

    def source(self, j):
        return self.plane_bytes(self.src, j["a"], j["sp"], j["sw"], j["sh"], j["cn"]).copy().view(self.dtype)

    def tuples(self, s_ptr, d_ptr):
        return [(s_ptr + j["a"], j["sp"], j["sw"], j["sh"], d_ptr + j["b"], j["dp"], j["dw"], j["dh"], j["cn"]) for j in self.jobs]

    def expected(self, max_value=0):
        """-> the whole destination buffer, and the largest sample of any result."""
        want, top = self.fill.copy(), 0
        for j in self.jobs:
            o = ar.resize(self.source(j), j["cn"], j["dw"], j["dh"], max_value)
            self.plane_bytes(want, j["b"], j["dp"], j["dw"], j["dh"], j["cn"])[...] = o.view(np.uint8)
            top = max(top, int(o.max()))
        return want, top

    def run(self, gpu, max_value=0, stream=None):
        d_src, d_dst = capi.DevBuf.from_array(gpu, self.src), capi.DevBuf.from_array(gpu, self.fill)
        try:
            gpu.area_jobs(self.tuples(d_src.ptr, d_dst.ptr), self.sb, max_value, stream)
            gpu.sync()
            assert np.array_equal(d_src.download((self.so,), np.uint8), self.src), "the sources were written"
            return d_dst.download((self.do,), np.uint8)
        finally:
            d_src.free(); d_dst.free()

    def compare(self, got, want):
        for i, j in enumerate(self.jobs):
            g = self.plane_bytes(got, j["b"], j["dp"], j["dw"], j["dh"], j["cn"])
            w = self.plane_bytes(want, j["b"], j["dp"], j["dw"], j["dh"], j["cn"])
            assert np.array_equal(g, w), ("job %d: %dx%d -> %dx%d, cn %d" % (i, j["sw"], j["sh"], j["dw"], j["dh"], j["cn"]), np.argwhere(g != w)[:4])
        assert np.array_equal(got, want), "bytes outside dw x dh were written"


# ---- 1. the job operator -------------------------------------------------------------------------------------------------------
_cases = {}


def shapes_case(sb, cn):
    """Every shape at both base offsets; built once per (sample size, cn)."""
    if (sb, cn) not in _cases:
        J = Jobs(2000 + 100 * sb + 10 * cn, sb)
        for off in ((1, 3) if sb == 1 else (2,)):
            for (sw, sh), (dw, dh) in SHAPES:
                J.add(sw, sh, dw, dh, cn, off)
        _cases[(sb, cn)] = J.build()
    return _cases[(sb, cn)]


@pytest.mark.parametrize("case", [(1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 1, 0), (2, 2, 0), (2, 1, 1023), (2, 2, 1023), (2, 1, 4095), (2, 2, 4095)],
                         ids=lambda v: "u%d-cn%d-max%d" % (8 * v[0], v[1], v[2]))
def test_jobs_against_the_numpy_statement(gpu, case):
    sb, cn, max_value = case
    J = shapes_case(sb, cn)
    cls = gpu.area_jobs_plan(J.tuples(1 << 20, 1 << 30), sb)
    assert set(cls.tolist()) == {0, 1, 2}                            # this launch runs the three classes
    want, top = J.expected(max_value)
    if max_value:                                                    # the sources reach 65535: the limit is what clamps
        assert top == max_value and J.expected(0)[1] > max_value
    J.compare(J.run(gpu, max_value), want)


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_96_mixed_jobs_in_one_launch_and_97_refused(gpu, sb):
    shapes = [((66, 50), (33, 25)), ((99, 60), (33, 20)), ((7, 5), (7, 5)), ((61, 30), (40, 23)), ((300, 9), (60, 4)), ((131, 40), (130, 37)), ((96, 61), (24, 61))]
    J = Jobs(196 + sb, sb)
    for i in range(96):
        (sw, sh), (dw, dh) = shapes[i % len(shapes)]
        J.add(sw, sh, dw, dh, 1 + (i // 2) % 2, sb * (1 + 2 * (i % 2)) if sb == 1 else 2)
    J.build()
    cls = gpu.area_jobs_plan(J.tuples(1 << 20, 1 << 30), sb)
    assert set(cls.tolist()) == {0, 1, 2}
    J.compare(J.run(gpu), J.expected()[0])
    # 97 jobs: refused, nothing written
    d_src, d_dst = capi.DevBuf.from_array(gpu, J.src), capi.DevBuf.from_array(gpu, J.fill)
    try:
        t = J.tuples(d_src.ptr, d_dst.ptr)
        with pytest.raises(capi.VsError, match="vs_op_area_jobs: invalid argument"):
            gpu.area_jobs(t + t[:1], sb)
        gpu.sync()
        assert np.array_equal(d_dst.download((J.do,), np.uint8), J.fill)
    finally:
        d_src.free(); d_dst.free()


# ---- 2. surfaces ---------------------------------------------------------------------------------------------------------------
YUV = ["NV12", "P010", "I420", "YV12", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412"]


class Surface:
    """A w x h surface of a YUV format with padded pitches (odd ones for 8-bit samples) and explicit plane offsets; YV12 = I420 with
    the offsets swapped."""

    def __init__(self, name, w, h, pad):
        self.f = f = capi.PIXFMT_BY_NAME["I420" if name == "YV12" else name]
        sb = self.sb = f.sample_bytes
        self.dtype = np.uint8 if sb == 1 else np.uint16
        self.w, self.h, self.cw, self.ch = w, h, w >> f.sx, h >> f.sy
        self.pitch = (w + pad) * sb
        if f.kind == capi.KIND_LUMA_UV:
            u = self.pitch * (h + 3)
            self.layout, self.planes = (self.pitch, 0, u, 0), [(0, self.pitch, w, h, 1), (u, self.pitch, self.cw, self.ch, 2)]
            self.size = u + self.ch * self.pitch
        else:
            cp = (self.cw + pad // 2 + 2) * sb
            u = self.pitch * (h + 1)
            v = u + cp * (self.ch + 2)
            if name == "YV12":
                u, v = v, u
            self.layout, self.planes = (self.pitch, cp, u, v), [(0, self.pitch, w, h, 1), (u, cp, self.cw, self.ch, 1), (v, cp, self.cw, self.ch, 1)]
            self.size = max(u, v) + self.ch * cp
        self.size += 32

    def view(self, buf, k):
        off, pitch, w, h, cn = self.planes[k]
        return np.lib.stride_tricks.as_strided(buf[off:], (h, w * cn * self.sb), (pitch, 1))

    def random(self, rng):
        """The surface as bytes: 16-bit samples over the whole word in every format, so the low-bit formats' clamp acts."""
        return rng.integers(0, 256, self.size, np.uint8)


def surfaces_case(gpu, name, sw, sh, dw, dh, n, seed):
    """n surfaces through vs_op_area_yuv -> (got, want) whole destination buffers, and the clamp of the format."""
    rng = np.random.default_rng(seed)
    S, D = Surface(name, sw, sh, 7), Surface(name, dw, dh, 11)
    src, fill = [S.random(rng) for _ in range(n)], [rng.integers(0, 256, D.size, np.uint8) for _ in range(n)]
    mv = (1 << S.f.bits) - 1 if S.f.kind == capi.KIND_THREE_PLANES and S.sb == 2 else 0
    want = [x.copy() for x in fill]
    for i in range(n):
        for k, (_, _, w, h, cn) in enumerate(S.planes):
            D.view(want[i], k)[...] = ar.resize(S.view(src[i], k).copy().view(S.dtype), cn, D.planes[k][2], D.planes[k][3], mv).view(np.uint8)
    d_src, d_dst = [capi.DevBuf.from_array(gpu, x) for x in src], [capi.DevBuf.from_array(gpu, x) for x in fill]
    try:
        gpu.area_yuv(S.f.fmt, [d.ptr for d in d_src], S.layout, sw, sh, [d.ptr for d in d_dst], D.layout, dw, dh)
        gpu.sync()
        got = [d.download((D.size,), np.uint8) for d in d_dst]
        assert all(np.array_equal(d.download((S.size,), np.uint8), x) for d, x in zip(d_src, src))
    finally:
        for d in d_src + d_dst:
            d.free()
    return got, want, mv, D


@pytest.mark.parametrize("name", YUV)
def test_surfaces_of_every_format(gpu, name):
    for (sw, sh), (dw, dh) in (((390, 204), (130, 68)), ((322, 200), (214, 134))):
        got, want, mv, D = surfaces_case(gpu, name, sw, sh, dw, dh, 2, zlib.crc32(("%s %d" % (name, dw)).encode()) % 1000)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (name, dw, dh, i, np.flatnonzero(g != w)[:6])
        if mv:                                                   # the low-bit formats: the clamp is the format's depth, and it acted
            assert D.view(want[0], 0).copy().view(np.uint16).max() == mv, name


@pytest.mark.parametrize("name", ["NV12", "P010"])
def test_32_surfaces_in_one_call_and_33_refused(gpu, name):
    got, want, _, _ = surfaces_case(gpu, name, 66, 50, 44, 26, 32, 132)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (name, i)
    assert len({g.tobytes() for g in got}) == 32                 # every surface different
    d = capi.DevBuf(gpu, 1 << 16)
    sb = capi.PIXFMT_BY_NAME[name].sample_bytes
    with pytest.raises(capi.VsError, match="vs_op_area_yuv.*n must be 1 .. 32"):
        gpu.area_yuv(capi.PIXFMT_BY_NAME[name].fmt, [d.ptr] * 33, (66 * sb, 0, 0, 0), 66, 50, [d.ptr + (1 << 15)] * 33, (44 * sb, 0, 0, 0), 44, 26)
    d.free()


@pytest.mark.parametrize("name", ["BGR8", "RGB8", "BGRA8", "RGBA8", "GRAY8"])
def test_rgb_frames(gpu, name):
    f = capi.PIXFMT_BY_NAME[name]
    sw, sh, dw, dh, n, cn = 650, 100, 271, 37, 2, f.cn
    rng = np.random.default_rng(15 + f.fmt)
    sp, dp = sw * cn + 5, dw * cn + 3
    src = [rng.integers(0, 256, sh * sp, np.uint8) for _ in range(n)]
    fill = [rng.integers(0, 256, dh * dp, np.uint8) for _ in range(n)]
    d_src, d_dst = [capi.DevBuf.from_array(gpu, x) for x in src], [capi.DevBuf.from_array(gpu, x) for x in fill]
    try:
        gpu.area_rgb(f.fmt, [d.ptr for d in d_src], sp, sw, sh, [d.ptr for d in d_dst], dp, dw, dh)
        gpu.sync()
        got = [d.download((dh * dp,), np.uint8) for d in d_dst]
    finally:
        for d in d_src + d_dst:
            d.free()
    for g, s, x in zip(got, src, fill):
        want = x.copy().reshape(dh, dp)
        want[:, :dw * cn] = ar.resize(s.reshape(sh, sp)[:, :sw * cn], cn, dw, dh)
        assert np.array_equal(g.reshape(dh, dp), want), name


# ---- 3. behind a stream --------------------------------------------------------------------------------------------------------
def test_border_pad_then_area_down_to_a_proxy_without_a_host_sync(gpu):
    """An NV12 stream with border pad, b = 8, at 144 x 96 returns 160 x 112 surfaces; vs_op_area_yuv queued on the stream's own
    stream right behind every push brings them down to 96 x 64, 2/3 of the frame size (5 : 3, general on both axes).  One
    vs_stab_sync at the end; the results equal arearef applied to the stream's outputs, read back in a second run of the same clip."""
    w, h, b, n = 144, 96, 8, 12
    pw, ph, ow, oh = w + 2 * b, h + 2 * b, 96, 64
    clip = [synth.bgr_to_nv12(x) for x in synth.make_clip(synth.SEED_CONFIG3 + 72, w, h, n)]
    pbytes, obytes = pw * ph * 3 // 2, ow * oh * 3 // 2

    def run(area):
        s = gpu.stabilizer(gpu.params(border_size=b, smoothing_radius=4))
        s.set_yuv_border_pad(True)
        d_in, d_pad = capi.DevBuf.from_array(gpu, np.stack(clip)), capi.DevBuf.from_array(gpu, np.full(n * pbytes, 0xA5, np.uint8))
        d_out = capi.DevBuf.from_array(gpu, np.full(n * obytes, 0x5A, np.uint8))
        st = gpu.lib.vs_stab_stream(s.h)
        try:
            k = 0
            for i in range(n):
                p = s.push_dev(d_in.ptr + i * clip[0].nbytes, w, h, w, capi.FMT_NV12, d_pad.ptr + k * pbytes, pw)
                if p and area:
                    gpu.area_yuv(capi.FMT_NV12, [d_pad.ptr + k * pbytes], (pw, 0, 0, 0), pw, ph, [d_out.ptr + k * obytes], (ow, 0, 0, 0), ow, oh, st)
                k += p
            s.sync()
            return k, d_pad.download((n, ph * 3 // 2, pw), np.uint8), d_out.download((n, oh * 3 // 2, ow), np.uint8)
        finally:
            s.close(); d_in.free(); d_pad.free(); d_out.free()
    k, _, got = run(True)
    k2, padded, untouched = run(False)
    assert k == k2 and k >= 4 and np.all(untouched == 0x5A)
    assert ar.job_class(pw, ph, ow, oh) == 0
    for i in range(k):
        want = np.vstack([ar.resize(padded[i][:ph], 1, ow, oh), ar.resize(padded[i][ph:], 2, ow // 2, oh // 2)])
        assert np.array_equal(got[i], want), i
    assert np.all(got[k:] == 0x5A)
