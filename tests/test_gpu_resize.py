"""Resize to an output size on the device, bit for bit against tests/resizeref.py (8-bit LINEAR also against the oracle's cv::resize):
vs_op_resample_jobs through both paths, vs_op_resize_yuv on the eleven surface formats, vs_op_resize_rgb, the recipe "border pad ->
Lanczos back to the frame size" behind a stream without a host synchronisation, and the table cache under two streams.

Every source lies inside a larger buffer of random bytes at an odd pitch (16-bit: an even one that is no multiple of 4) with its
first sample 1 and 3 bytes (16-bit: 2) off alignment, so a tap that leaves the sw x sh samples changes the result; every destination
is prefilled and the whole allocation is compared, so a byte written outside dw x dh is seen.  tests/test_resize_cpu.py shows that
path 0 runs the staged kernel for 130 x 96 -> 97 x 61 and the direct kernel for 322 x 200 -> 64 x 36.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import resizeref as rr
from vsamd import capi, synth

pytestmark = pytest.mark.gpu

LINEAR, LANCZOS4 = rr.LINEAR, rr.LANCZOS4
SHAPES = [((1, 1), (5, 3)), ((3, 2), (1, 1)), ((7, 5), (7, 5)), ((9, 9), (8, 8)), ((66, 50), (33, 25)), ((130, 96), (97, 61)), ((97, 61), (322, 200)),
          ((322, 200), (64, 36)), ((2046, 70), (1920, 64)), ((70, 2046), (64, 1920))]


class Jobs:
    """Planes to resize, laid out in one source and one destination buffer."""

    def __init__(self, seed, sb):
        self.rng, self.sb, self.dtype = np.random.default_rng(seed), sb, (np.uint8 if sb == 1 else np.uint16)
        self.jobs, self.so, self.do = [], 0, 0

    def add(self, sw, sh, dw, dh, cn, off, content=None):
        """A source of sw x sh pixels inside (sh + 4) rows of random bytes, its first sample `off` bytes off alignment."""
        px, sb = self.sb * cn, self.sb
        sp = (sw + 4) * px + (3 if sb == 1 else 2)
        sp += (sp % 2 == 0) if sb == 1 else (2 if sp % 4 == 0 else 0)
        dp = dw * px + (7 if sb == 1 else 6)
        a = self.so + 2 * sp + 2 * px + off
        b = self.do + dp + off
        self.jobs.append(dict(a=a, sp=sp, sw=sw, sh=sh, b=b, dp=dp, dw=dw, dh=dh, cn=cn, content=content))
        self.so = (self.so + (sh + 4) * sp + 16 + 255) // 256 * 256
        self.do = (self.do + (dh + 2) * dp + 16 + 255) // 256 * 256

    def build(self, top=None):
        self.src = self.rng.integers(0, 256, self.so, np.uint8)
        if top is not None:                      # samples of 0 .. top
            self.src = self.rng.integers(0, top + 1, self.so // 2, np.uint16).view(np.uint8)
        for j in self.jobs:
            if j["content"] is not None:
                self.plane_bytes(self.src, j["a"], j["sp"], j["sw"], j["sh"], j["cn"])[...] = j["content"].view(np.uint8)
        self.fill = self.rng.integers(0, 256, self.do, np.uint8)
        return self

    def plane_bytes(self, buf, at, pitch, w, h, cn):
        return np.lib.stride_tricks.as_strided(buf[at:], (h, w * cn * self.sb), (pitch, 1))

    def source(self, j):
        return self.plane_bytes(self.src, j["a"], j["sp"], j["sw"], j["sh"], j["cn"]).copy().view(self.dtype)

    def tuples(self, s_ptr, d_ptr):
        return [(s_ptr + j["a"], j["sp"], j["sw"], j["sh"], d_ptr + j["b"], j["dp"], j["dw"], j["dh"], j["cn"]) for j in self.jobs]

    def expected(self, interp, max_value=0):
        """-> the whole destination buffer, and the result of every job."""
        want, outs = self.fill.copy(), []
        for j in self.jobs:
            o = rr.resize(self.source(j), j["cn"], j["dw"], j["dh"], interp, max_value)
            self.plane_bytes(want, j["b"], j["dp"], j["dw"], j["dh"], j["cn"])[...] = o.view(np.uint8)
            outs.append(o)
        return want, outs

    def run(self, gpu, interp, max_value=0, path=0, stream=None):
        d_src, d_dst = capi.DevBuf.from_array(gpu, self.src), capi.DevBuf.from_array(gpu, self.fill)
        try:
            gpu.resample_jobs(self.tuples(d_src.ptr, d_dst.ptr), self.sb, interp, max_value, path, stream)
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


def shapes_case(sb, cn, interp):
    """Every shape at both base offsets, and its reference: computed once, shared by both paths."""
    key = (sb, cn, interp)
    if key not in _cases:
        J = Jobs(1000 + 100 * sb + 10 * cn + interp, sb)
        for off in ((1, 3) if sb == 1 else (2,)):
            for (sw, sh), (dw, dh) in SHAPES:
                J.add(sw, sh, dw, dh, cn, off)
        J.build()
        _cases[key] = (J, J.expected(interp)[0])
    return _cases[key]


@pytest.mark.parametrize("path", [0, 1], ids=["path0", "path1"])
@pytest.mark.parametrize("interp", [LINEAR, LANCZOS4], ids=["linear", "lanczos4"])
@pytest.mark.parametrize("sbcn", [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2)], ids=lambda v: "u%d-cn%d" % (8 * v[0], v[1]))
def test_jobs_against_the_numpy_statement(gpu, oracle, sbcn, interp, path):
    sb, cn = sbcn
    J, want = shapes_case(sb, cn, interp)
    if path == 0:
        staged = gpu.resample_jobs_plan(J.tuples(1 << 20, 1 << 30), sb, interp)
        assert 0 < staged.sum() < len(J.jobs)                    # this launch runs both kernels
    J.compare(J.run(gpu, interp, path=path), want)
    if sb == 1 and interp == LINEAR and path == 0:                # ... and the statement is the oracle's cv::resize
        for j in J.jobs[:len(SHAPES)]:
            src = J.source(j).reshape(j["sh"], j["sw"]) if cn == 1 else J.source(j).reshape(j["sh"], j["sw"], cn)
            o = np.asarray(oracle.resize(src, j["dw"], j["dh"])).reshape(j["dh"], j["dw"] * cn)
            assert np.array_equal(J.plane_bytes(want, j["b"], j["dp"], j["dw"], j["dh"], cn), o), j


@pytest.mark.parametrize("path", [0, 1], ids=["path0", "path1"])
@pytest.mark.parametrize("case", [(1, 255, 0), (2, 65535, 0), (2, 1023, 1023)], ids=["255", "65535", "1023"])
def test_lanczos_checkerboards_hit_both_clamps(gpu, case, path):
    sb, top, max_value = case
    J = Jobs(77 + top, sb)
    board = (np.indices((24, 40)).sum(0) % 2 * top).astype(J.dtype)
    J.add(40, 24, 52, 31, 1, sb, board)
    J.add(20, 24, 26, 31, 2, sb, board)
    J.build()
    want, outs = J.expected(LANCZOS4, max_value)
    assert all(o.min() == 0 and o.max() == top for o in outs)
    if max_value:
        assert J.expected(LANCZOS4)[1][0].max() > top             # the limit is what clamps
    J.compare(J.run(gpu, LANCZOS4, max_value, path), want)


@pytest.mark.parametrize("interp", [LINEAR, LANCZOS4], ids=["linear", "lanczos4"])
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_96_mixed_jobs_in_one_launch_and_97_refused(gpu, sb, interp):
    shapes = [((20, 4), (64, 48)), ((2, 2), (3, 7)), ((66, 50), (33, 25)), ((126, 92), (130, 96)), ((61, 30), (40, 33)), ((300, 9), (60, 40)), ((33, 70), (301, 16))]
    J = Jobs(96 + sb + 10 * interp, sb)
    for i in range(96):
        (sw, sh), (dw, dh) = shapes[i % len(shapes)]
        J.add(sw, sh, dw, dh, 1 + (i // 2) % 2, sb * (1 + 2 * (i % 2)) if sb == 1 else 2)
    J.build()
    staged = gpu.resample_jobs_plan(J.tuples(1 << 20, 1 << 30), sb, interp)
    assert 0 < staged.sum() < 96
    J.compare(J.run(gpu, interp), J.expected(interp)[0])
    # 97 jobs: refused, nothing written
    d_src, d_dst = capi.DevBuf.from_array(gpu, J.src), capi.DevBuf.from_array(gpu, J.fill)
    try:
        t = J.tuples(d_src.ptr, d_dst.ptr)
        with pytest.raises(capi.VsError, match="vs_op_resample_jobs: invalid argument"):
            gpu.resample_jobs(t + t[:1], sb, interp)
        gpu.sync()
        assert np.array_equal(d_dst.download((J.do,), np.uint8), J.fill)
    finally:
        d_src.free(); d_dst.free()


# ---- 2. surfaces ---------------------------------------------------------------------------------------------------------------
YUV = ["NV12", "P010", "I420", "YV12", "I010", "I012", "I422", "I444", "I210", "I212", "I410", "I412"]


class Surface:
    """A w x h surface of a YUV format with padded pitches and explicit plane offsets; YV12 = I420 with the offsets swapped."""

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
            cp = (self.cw + pad // 2 + 1) * sb
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
        """The surface as bytes: samples of the format's depth in the planes (P010: the whole word), random bytes elsewhere."""
        buf = rng.integers(0, 256, self.size, np.uint8)
        top = 255 if self.sb == 1 else 65535 if self.f.kind == capi.KIND_LUMA_UV else (1 << self.f.bits) - 1
        for k, (_, _, w, h, cn) in enumerate(self.planes):
            self.view(buf, k)[...] = rng.integers(0, top + 1, (h, w * cn), self.dtype).view(np.uint8)
        return buf


def surfaces_case(gpu, name, sw, sh, dw, dh, n, interp, seed):
    """n surfaces through vs_op_resize_yuv -> (got, want) whole destination buffers, and the unclamped reference of surface 0's luma."""
    rng = np.random.default_rng(seed)
    S, D = Surface(name, sw, sh, 6), Surface(name, dw, dh, 10)
    src, fill = [S.random(rng) for _ in range(n)], [rng.integers(0, 256, D.size, np.uint8) for _ in range(n)]
    low_bit = S.f.kind == capi.KIND_THREE_PLANES and S.sb == 2
    mv = rr.lanczos_max_value(S.f.bits, low_bit) if interp == LANCZOS4 else 0
    want = [x.copy() for x in fill]
    for i in range(n):
        for k, (_, _, w, h, cn) in enumerate(S.planes):
            D.view(want[i], k)[...] = rr.resize(S.view(src[i], k).copy().view(S.dtype), cn, D.planes[k][2], D.planes[k][3], interp, mv).view(np.uint8)
    d_src, d_dst = [capi.DevBuf.from_array(gpu, x) for x in src], [capi.DevBuf.from_array(gpu, x) for x in fill]
    try:
        gpu.resize_yuv(S.f.fmt, [d.ptr for d in d_src], S.layout, sw, sh, [d.ptr for d in d_dst], D.layout, dw, dh, interp)
        gpu.sync()
        got = [d.download((D.size,), np.uint8) for d in d_dst]
        assert all(np.array_equal(d.download((S.size,), np.uint8), x) for d, x in zip(d_src, src))
    finally:
        for d in d_src + d_dst:
            d.free()
    raw = rr.resize(S.view(src[0], 0).copy().view(S.dtype), 1, dw, dh, interp) if mv else None
    return got, want, raw, mv


@pytest.mark.parametrize("interp", [LINEAR, LANCZOS4], ids=["linear", "lanczos4"])
@pytest.mark.parametrize("name", YUV)
def test_surfaces_of_every_format(gpu, name, interp):
    for dw, dh in ((98, 64), (260, 192)):
        got, want, raw, mv = surfaces_case(gpu, name, 130, 96, dw, dh, 3, interp, zlib.crc32(("%s %d" % (name, dw)).encode()) % 1000)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (name, dw, dh, i, np.flatnonzero(g != w)[:6])
        if mv:                                                   # the low-bit formats under LANCZOS4: the clamp is the format's depth
            assert raw.max() > mv, name


@pytest.mark.parametrize("name", ["NV12", "P010"])
def test_32_surfaces_in_one_call_and_33_refused(gpu, name):
    for interp in (LINEAR, LANCZOS4):
        got, want, _, _ = surfaces_case(gpu, name, 66, 50, 34, 26, 32, interp, 32 + interp)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (name, interp, i)
        assert len({g.tobytes() for g in got}) == 32             # every surface different
    d = capi.DevBuf(gpu, 1 << 16)
    sb = capi.PIXFMT_BY_NAME[name].sample_bytes
    with pytest.raises(capi.VsError, match="vs_op_resize_yuv.*n must be 1 .. 32"):
        gpu.resize_yuv(capi.PIXFMT_BY_NAME[name].fmt, [d.ptr] * 33, (66 * sb, 0, 0, 0), 66, 50, [d.ptr + (1 << 15)] * 33, (34 * sb, 0, 0, 0), 34, 26)
    d.free()


@pytest.mark.parametrize("interp", [LINEAR, LANCZOS4], ids=["linear", "lanczos4"])
@pytest.mark.parametrize("name", ["BGR8", "BGRA8", "GRAY8"])
def test_rgb_frames(gpu, oracle, name, interp):
    f = capi.PIXFMT_BY_NAME[name]
    sw, sh, dw, dh, n, cn = 130, 96, 97, 61, 2, f.cn
    rng = np.random.default_rng(5 + f.fmt + interp)
    sp, dp = sw * cn + 5, dw * cn + 3
    src = [rng.integers(0, 256, sh * sp, np.uint8) for _ in range(n)]
    fill = [rng.integers(0, 256, dh * dp, np.uint8) for _ in range(n)]
    d_src, d_dst = [capi.DevBuf.from_array(gpu, x) for x in src], [capi.DevBuf.from_array(gpu, x) for x in fill]
    try:
        gpu.resize_rgb(f.fmt, [d.ptr for d in d_src], sp, sw, sh, [d.ptr for d in d_dst], dp, dw, dh, interp)
        gpu.sync()
        got = [d.download((dh * dp,), np.uint8) for d in d_dst]
    finally:
        for d in d_src + d_dst:
            d.free()
    for g, s, x in zip(got, src, fill):
        frame = s.reshape(sh, sp)[:, :sw * cn]
        want = x.copy().reshape(dh, dp)
        want[:, :dw * cn] = rr.resize(frame, cn, dw, dh, interp)
        assert np.array_equal(g.reshape(dh, dp), want), name
        if interp == LINEAR:
            o = oracle.resize(np.ascontiguousarray(frame).reshape((sh, sw) if cn == 1 else (sh, sw, cn)), dw, dh)
            assert np.array_equal(want[:, :dw * cn], np.asarray(o).reshape(dh, dw * cn))


# ---- 3. behind a stream, and the table cache -------------------------------------------------------------------------------------
def test_border_pad_then_lanczos_back_to_the_frame_size_without_a_host_sync(gpu):
    """An NV12 stream with border pad, b = 8, at 130 x 96 returns 146 x 112 surfaces; vs_op_resize_yuv(LANCZOS4) queued on the
    stream's own stream right behind every push brings them back to 130 x 96.  One vs_stab_sync at the end; the results equal
    resizeref applied to the stream's outputs, read back in a second run of the same clip."""
    w, h, b, n = 130, 96, 8, 12
    pw, ph = w + 2 * b, h + 2 * b
    clip = [synth.bgr_to_nv12(x) for x in synth.make_clip(synth.SEED_CONFIG3 + 71, w, h, n)]
    pbytes, obytes = pw * ph * 3 // 2, w * h * 3 // 2

    def run(resize):
        s = gpu.stabilizer(gpu.params(border_size=b, smoothing_radius=4))
        s.set_yuv_border_pad(True)
        d_in, d_pad = capi.DevBuf.from_array(gpu, np.stack(clip)), capi.DevBuf.from_array(gpu, np.full(n * pbytes, 0xA5, np.uint8))
        d_out = capi.DevBuf.from_array(gpu, np.full(n * obytes, 0x5A, np.uint8))
        st = gpu.lib.vs_stab_stream(s.h)
        try:
            k = 0
            for i in range(n):
                p = s.push_dev(d_in.ptr + i * clip[0].nbytes, w, h, w, capi.FMT_NV12, d_pad.ptr + k * pbytes, pw)
                if p and resize:
                    gpu.resize_yuv(capi.FMT_NV12, [d_pad.ptr + k * pbytes], (pw, 0, 0, 0), pw, ph, [d_out.ptr + k * obytes], (w, 0, 0, 0), w, h, LANCZOS4, st)
                k += p
            s.sync()
            return k, d_pad.download((n, ph * 3 // 2, pw), np.uint8), d_out.download((n, h * 3 // 2, w), np.uint8)
        finally:
            s.close(); d_in.free(); d_pad.free(); d_out.free()
    k, _, got = run(True)
    k2, padded, untouched = run(False)
    assert k == k2 and k >= 4 and np.all(untouched == 0x5A)
    for i in range(k):
        want = np.vstack([rr.resize(padded[i][:ph], 1, w, h, LANCZOS4), rr.resize(padded[i][ph:], 2, w // 2, h // 2, LANCZOS4)])
        assert np.array_equal(got[i], want), i
    assert np.all(got[k:] == 0x5A)


def test_a_new_axis_pair_on_another_stream_right_behind_the_first(gpu):
    """Two calls back to back on two streams, the second with axes the device has not met: it builds and uploads tables while the
    first may still run.  Neither result changes - a table, once placed, is only read."""
    A, B = Jobs(501, 1), Jobs(502, 1)
    for i in range(24):
        A.add(1283, 211, 1117, 197, 1 + i % 2, 1)
    B.add(1117, 197, 1291, 223, 1, 3)
    B.add(211, 1283, 193, 1301, 2, 1)
    A.build(); B.build()
    want_a, want_b = A.expected(LANCZOS4)[0], B.expected(LANCZOS4)[0]
    owners = [gpu.stabilizer(gpu.params())]
    sa, sb_ = gpu.lib.vs_stab_stream(owners[0].h), None          # a stream object's non-blocking stream, and the default stream
    assert sa
    bufs = [capi.DevBuf.from_array(gpu, x) for x in (A.src, A.fill, B.src, B.fill)]
    try:
        gpu.resample_jobs(A.tuples(bufs[0].ptr, bufs[1].ptr), 1, LANCZOS4, 0, 0, sa)
        gpu.resample_jobs(B.tuples(bufs[2].ptr, bufs[3].ptr), 1, LANCZOS4, 0, 0, sb_)
        gpu.resample_jobs(A.tuples(bufs[0].ptr, bufs[1].ptr), 1, LANCZOS4, 0, 1, sa)     # (again, through the direct kernel: the same bytes)
        gpu.sync()
        A.compare(bufs[1].download((A.do,), np.uint8), want_a)
        B.compare(bufs[3].download((B.do,), np.uint8), want_b)
    finally:
        for d in bufs:
            d.free()
        for o in owners:
            o.close()
