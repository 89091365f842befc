"""The deinterlacer and the weave on the device, byte for byte against tests/deintref.py: vs_op_deint_jobs in both modes at every
(keep, second), vs_op_deint_yuv and vs_op_interlace_yuv on the eleven surface formats, and a call on a non-default stream followed
by a resize without a host synchronisation.

Every source lies inside a larger buffer of random bytes at an odd pitch (16-bit: an even one that is no multiple of 4) with its
first sample 1 or 3 bytes (16-bit: 2) off alignment; every destination is prefilled and the whole allocation is compared, so a
byte written outside w x h is seen; the sources are compared with themselves afterwards.  16-bit samples span 0 .. 65535.  The
kernel's tile is 256 bytes x 256 rows, a lane owns 16 bytes: the shapes lie on both sides of them.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import deintref as dr
import resizeref as rr
from vsamd import capi

pytestmark = pytest.mark.gpu

TILE_BYTES, TILE_ROWS = 256, 256


def shapes_of(sb, cn):
    """(w, h): the smallest at which the kernel can go wrong, for pixels of sb * cn bytes."""
    tw = -(-TILE_BYTES // (sb * cn))
    s = [(w, h) for w in (1, 6, 7, 8) for h in (2, 3, 4, 5)]
    s += [(w, h) for w in (tw - 1, tw, tw + 1, 2 * tw + 3) for h in (3, 6)]
    s += [(9, TILE_ROWS - 1), (9, TILE_ROWS + 1), (tw + 1, TILE_ROWS + 2)]
    return s


class Jobs:
    """Planes to deinterlace: P, C and N of every job inside one source buffer of random bytes, the destinations in another."""

    def __init__(self, seed, sb):
        self.rng, self.sb, self.dtype = np.random.default_rng(seed), sb, (np.uint8 if sb == 1 else np.uint16)
        self.jobs, self.so, self.do = [], 0, 0

    def _plane(self, w, h, cn, off):
        """-> (offset of the first sample, pitch) of w x h pixels inside (h + 4) rows of the source buffer."""
        px, sb = self.sb * cn, self.sb
        sp = (w + 4) * px + (3 if sb == 1 else 2)
        sp += (sp % 2 == 0) if sb == 1 else (2 if sp % 4 == 0 else 0)
        at = self.so + 2 * sp + 2 * px + off
        self.so = (self.so + (h + 4) * sp + 16 + 255) // 256 * 256
        return at, sp

    def add(self, w, h, cn, off, keep, second, variant="pcn"):
        c = self._plane(w, h, cn, off)
        p = c if variant == "same" else None if variant in ("null_p", "null_pn") else self._plane(w, h, cn, off)
        n = c if variant == "same" else None if variant in ("null_n", "null_pn") else self._plane(w, h, cn, off)
        dp = w * self.sb * cn + (7 if self.sb == 1 else 6)
        self.jobs.append(dict(p=p, c=c, n=n, d=self.do + dp + off, dp=dp, w=w, h=h, cn=cn, keep=keep, second=second))
        self.do = (self.do + (h + 2) * dp + 16 + 255) // 256 * 256

    def build(self):
        self.src = self.rng.integers(0, 256, self.so, np.uint8)          # (16-bit samples: the whole range, 0 .. 65535)
        self.fill = self.rng.integers(0, 256, self.do, np.uint8)
        return self

    def plane_bytes(self, buf, at, pitch, w, h, cn):
        return np.lib.stride_tricks.as_strided(buf[at:], (h, w * cn * self.sb), (pitch, 1))

    def source(self, j, k):
        return None if j[k] is None else self.plane_bytes(self.src, j[k][0], j[k][1], j["w"], j["h"], j["cn"]).copy().view(self.dtype)

    def tuples(self, s_ptr, d_ptr):
        def ps(j, k):
            return (None, 0) if j[k] is None else (s_ptr + j[k][0], j[k][1])
        return [ps(j, "p") + ps(j, "c") + ps(j, "n") + (d_ptr + j["d"], j["dp"], j["w"], j["h"], j["cn"], j["keep"], j["second"]) for j in self.jobs]

    def expected(self, mode, counts=None):
        want = self.fill.copy()
        for j in self.jobs:
            full = j["w"] >= 7 and j["h"] >= 3
            o = dr.deint(self.source(j, "p"), self.source(j, "c"), self.source(j, "n"), j["cn"], j["keep"], j["second"], mode,
                         counts if full and mode == dr.YADIF else None)
            self.plane_bytes(want, j["d"], j["dp"], j["w"], j["h"], j["cn"])[...] = o.view(np.uint8)
        return want

    def run(self, gpu, mode, stream=None):
        d_src, d_dst = capi.DevBuf.from_array(gpu, self.src), capi.DevBuf.from_array(gpu, self.fill)
        try:
            gpu.deint_jobs(self.tuples(d_src.ptr, d_dst.ptr), self.sb, mode, stream)
            gpu.sync()
            assert np.array_equal(d_src.download((self.so,), np.uint8), self.src), "the sources were written"
            return d_dst.download((self.do,), np.uint8)
        finally:
            d_src.free(); d_dst.free()

    def compare(self, got, want):
        for i, j in enumerate(self.jobs):
            g = self.plane_bytes(got, j["d"], j["dp"], j["w"], j["h"], j["cn"])
            w = self.plane_bytes(want, j["d"], j["dp"], j["w"], j["h"], j["cn"])
            assert np.array_equal(g, w), ("job %d: %dx%d, cn %d, keep %d, second %d" % (i, j["w"], j["h"], j["cn"], j["keep"], j["second"]), np.argwhere(g != w)[:4])
        assert np.array_equal(got, want), "bytes outside w x h were written"


# ---- 1. the job operator -------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2)]
_cases = {}


def shapes_case(sb, cn, keep, second):
    """Every shape, the base offsets in turn; built once per (sample size, cn, keep, second) and shared by both modes."""
    key = (sb, cn, keep, second)
    if key not in _cases:
        J = Jobs(3000 + 100 * sb + 10 * cn + 2 * keep + second, sb)
        for i, (w, h) in enumerate(shapes_of(sb, cn)):
            J.add(w, h, cn, (1, 3)[i % 2] if sb == 1 else 2, keep, second)
        _cases[key] = J.build()
    return _cases[key]


@pytest.mark.parametrize("mode", [dr.LINEAR, dr.YADIF], ids=["linear", "yadif"])
@pytest.mark.parametrize("size", SIZES, ids=lambda v: "u%d-cn%d" % (8 * v[0], v[1]))
def test_jobs_against_the_numpy_statement(gpu, size, mode):
    sb, cn = size
    counts = {}
    for keep in (0, 1):
        for second in (0, 1):
            J = shapes_case(sb, cn, keep, second)
            J.compare(J.run(gpu, mode), J.expected(mode, counts))
    if mode == dr.YADIF:                                                 # the inputs reach every branch of the statement
        assert all(counts[k] > 0 for k in dr.BRANCHES), counts


@pytest.mark.parametrize("variant", ["null_p", "null_n", "null_pn", "same"])
@pytest.mark.parametrize("size", SIZES, ids=lambda v: "u%d-cn%d" % (8 * v[0], v[1]))
def test_jobs_without_a_previous_or_next_frame_and_on_one_buffer(gpu, size, variant):
    sb, cn = size
    J = Jobs(4000 + 100 * sb + 10 * cn + len(variant), sb)
    for i, (w, h) in enumerate(shapes_of(sb, cn)[8:]):
        J.add(w, h, cn, (1, 3)[i % 2] if sb == 1 else 2, i & 1, (i >> 1) & 1, variant)
    J.build()
    counts = {}
    J.compare(J.run(gpu, dr.YADIF), J.expected(dr.YADIF, counts))
    assert all(counts[k] > 0 for k in dr.BRANCHES if variant != "same" or k in ("pick_0", "pick_m1", "pick_p1", "clamp_none")), counts


@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_96_mixed_jobs_in_one_launch_and_97_refused(gpu, sb):
    shapes = [(66, 50), (7, 5), (259, 9), (33, 2), (17, 33), (131, 40), (96, 61)]
    J = Jobs(296 + sb, sb)
    for i in range(96):
        w, h = shapes[i % len(shapes)]
        J.add(w, h, 1 + (i // 2) % (4 if sb == 1 else 2), (1, 3)[i % 2] if sb == 1 else 2, i % 2, (i // 3) % 2, ("pcn", "null_p", "pcn", "null_n", "same")[i % 5])
    J.build()
    assert len({(j["w"], j["h"], j["cn"], j["keep"], j["second"]) for j in J.jobs}) > 40
    J.compare(J.run(gpu, dr.YADIF), J.expected(dr.YADIF))
    # 97 jobs: refused, nothing written
    d_src, d_dst = capi.DevBuf.from_array(gpu, J.src), capi.DevBuf.from_array(gpu, J.fill)
    try:
        t = J.tuples(d_src.ptr, d_dst.ptr)
        with pytest.raises(capi.VsError, match="vs_op_deint_jobs: invalid argument"):
            gpu.deint_jobs(t + t[:1], sb, dr.YADIF)
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

    def plane(self, buf, k):
        return None if buf is None else self.view(buf, k).copy().view(self.dtype)

    def random(self, rng):
        return rng.integers(0, 256, self.size, np.uint8)


def deint_surfaces(gpu, name, w, h, n, seed, tff, mode, double, ends):
    """A batch of n frames chained as prev[i] = cur[i - 1], next[i] = cur[i + 1] through vs_op_deint_yuv; ends: the batch's first
    prev and last next are frames of their own (True) or missing (False: once a NULL entry, once a NULL array).
    -> (got, want) lists of whole destination buffers, first fields then second fields."""
    rng = np.random.default_rng(seed)
    S, D = Surface(name, w, h, 7), Surface(name, w, h, 11)
    cur = [S.random(rng) for _ in range(n)]
    before, after = (S.random(rng), S.random(rng)) if ends else (None, None)
    prev, nxt = [before] + cur[:-1], cur[1:] + [after]
    fill = [rng.integers(0, 256, D.size, np.uint8) for _ in range(2 * n if double else n)]
    want = [x.copy() for x in fill]
    k0 = 0 if tff else 1
    for i in range(n):
        for f in range(2 if double else 1):
            for k, (_, _, _, _, cn) in enumerate(S.planes):
                D.view(want[f * n + i], k)[...] = dr.deint(S.plane(prev[i], k), S.plane(cur[i], k), S.plane(nxt[i], k), cn, k0 ^ f, f, mode).view(np.uint8)
    d_cur = [capi.DevBuf.from_array(gpu, x) for x in cur]
    d_ends = [capi.DevBuf.from_array(gpu, x) for x in (before, after) if x is not None]
    d_dst = [capi.DevBuf.from_array(gpu, x) for x in fill]
    try:
        c = [d.ptr for d in d_cur]
        p = [d_ends[0].ptr if ends else None] + c[:-1]
        q = c[1:] + [d_ends[1].ptr if ends else None]
        if not ends and n == 1:
            p = q = None                                         # the arrays themselves may be missing
        out = [d.ptr for d in d_dst]
        gpu.deint_yuv(S.f.fmt, p, c, q, S.layout, w, h, out[:n], out[n:] if double else None, D.layout, tff, mode)
        gpu.sync()
        got = [d.download((D.size,), np.uint8) for d in d_dst]
        assert all(np.array_equal(d.download((S.size,), np.uint8), x) for d, x in zip(d_cur, cur))
    finally:
        for d in d_cur + d_ends + d_dst:
            d.free()
    return got, want


@pytest.mark.parametrize("name", YUV)
def test_surfaces_of_every_format(gpu, name):
    sizes = [(130, 96), (322, 200)] + ([(131, 96)] if name in ("I444", "I410", "I412") else [])
    cases = [(sizes[0], 5, 1, dr.YADIF, True, True), (sizes[1], 2, 0, dr.YADIF, True, False), (sizes[0], 1, 1, dr.YADIF, False, False),
             (sizes[1], 2, 1, dr.LINEAR, True, True), (sizes[0], 3, 0, dr.LINEAR, False, False)]
    cases += [(s, 2, 1, dr.YADIF, True, False) for s in sizes[2:]]
    for (w, h), n, tff, mode, double, ends in cases:
        got, want = deint_surfaces(gpu, name, w, h, n, zlib.crc32(("%s %d %d" % (name, w, n)).encode()) % 1000, tff, mode, double, ends)
        for i, (g, x) in enumerate(zip(got, want)):
            assert np.array_equal(g, x), (name, w, h, n, tff, mode, double, ends, i, np.flatnonzero(g != x)[:6])


def test_16_frames_at_double_rate_and_17_refused(gpu):
    got, want = deint_surfaces(gpu, "I420", 66, 50, 16, 216, 1, dr.YADIF, True, True)           # 96 jobs
    for i, (g, x) in enumerate(zip(got, want)):
        assert np.array_equal(g, x), i
    d = capi.DevBuf(gpu, 1 << 16)
    with pytest.raises(capi.VsError, match="vs_op_deint_yuv.*n must be 1 .. 16"):
        gpu.deint_yuv(capi.FMT_NV12, None, [d.ptr] * 17, None, (66, 0, 0, 0), 66, 50, [d.ptr + (1 << 15)] * 17, None, (66, 0, 0, 0))
    d.free()


@pytest.mark.parametrize("name", YUV)
def test_the_weave_and_the_round_trip(gpu, name):
    for (w, h), n, tff in (((130, 96), 3, 1), ((322, 200), 2, 0)):
        rng = np.random.default_rng(zlib.crc32(("weave %s %d" % (name, w)).encode()) % 1000)
        S, D = Surface(name, w, h, 7), Surface(name, w, h, 11)
        first, second, cur = ([S.random(rng) for _ in range(n)] for _ in range(3))
        fill = [rng.integers(0, 256, D.size, np.uint8) for _ in range(n)]
        want = [x.copy() for x in fill]
        for i in range(n):
            for k in range(len(S.planes)):
                D.view(want[i], k)[...] = dr.weave(S.view(first[i], k), S.view(second[i], k), tff)
        bufs = [[capi.DevBuf.from_array(gpu, x) for x in group] for group in (first, second, fill, cur, first, second, fill)]
        d_first, d_second, d_dst, d_cur, d_f, d_s, d_back = ([d.ptr for d in group] for group in bufs)
        try:
            gpu.interlace_yuv(S.f.fmt, d_first, d_second, S.layout, w, h, d_dst, D.layout, tff)
            # interlace(deint(C)) == C: same layout on every side, so the whole planes come back
            for mode in (dr.YADIF, dr.LINEAR):
                gpu.deint_yuv(S.f.fmt, d_first, d_cur, d_second, S.layout, w, h, d_f, d_s, S.layout, tff, mode)
                gpu.interlace_yuv(S.f.fmt, d_f, d_s, S.layout, w, h, d_back, D.layout, tff)
                gpu.sync()
                for i in range(n):
                    back = bufs[6][i].download((D.size,), np.uint8)
                    for k in range(len(S.planes)):
                        assert np.array_equal(D.view(back, k), S.view(cur[i], k)), (name, w, mode, i, k)
            for i in range(n):
                g = bufs[2][i].download((D.size,), np.uint8)
                assert np.array_equal(g, want[i]), (name, w, h, i, np.flatnonzero(g != want[i])[:6])
                assert np.array_equal(bufs[0][i].download((S.size,), np.uint8), first[i]) and np.array_equal(bufs[1][i].download((S.size,), np.uint8), second[i])
        finally:
            for group in bufs:
                for d in group:
                    d.free()


@pytest.mark.parametrize("name", ["NV12", "I010"])
def test_32_pairs_woven_in_one_call_and_33_refused(gpu, name):
    w, h, n = 66, 50, 32
    rng = np.random.default_rng(332)
    S = Surface(name, w, h, 5)
    first, second = ([S.random(rng) for _ in range(n)] for _ in range(2))
    fill = [rng.integers(0, 256, S.size, np.uint8) for _ in range(n)]
    bufs = [[capi.DevBuf.from_array(gpu, x) for x in group] for group in (first, second, fill)]
    try:
        a, b, d = ([x.ptr for x in group] for group in bufs)
        gpu.interlace_yuv(S.f.fmt, a, b, S.layout, w, h, d, S.layout, 1)
        gpu.sync()
        for i in range(n):
            want = fill[i].copy()
            for k in range(len(S.planes)):
                S.view(want, k)[...] = dr.weave(S.view(first[i], k), S.view(second[i], k), 1)
            assert np.array_equal(bufs[2][i].download((S.size,), np.uint8), want), i
        with pytest.raises(capi.VsError, match="vs_op_interlace_yuv.*n must be 1 .. 32"):
            gpu.interlace_yuv(S.f.fmt, a + a[:1], b + b[:1], S.layout, w, h, d + d[:1], S.layout, 1)
    finally:
        for group in bufs:
            for x in group:
                x.free()


# ---- 3. behind a stream --------------------------------------------------------------------------------------------------------
def test_on_a_stream_followed_by_a_resize_without_a_host_sync(gpu):
    """Three NV12 frames deinterlaced to double rate on a stream that is not the default one; vs_op_resize_yuv, queued on the same
    stream right behind, halves the six progressive frames.  One synchronisation at the end."""
    w, h, n = 144, 96, 3
    rng = np.random.default_rng(77)
    frame = w * h * 3 // 2
    cur = [rng.integers(0, 256, frame, np.uint8) for _ in range(n)]
    s = gpu.stabilizer(gpu.params(smoothing_radius=4))
    st = gpu.lib.vs_stab_stream(s.h)
    assert st
    d_cur = [capi.DevBuf.from_array(gpu, x) for x in cur]
    d_prog = [capi.DevBuf.from_array(gpu, np.full(frame, 0xA5, np.uint8)) for _ in range(2 * n)]
    d_half = [capi.DevBuf.from_array(gpu, np.full(frame // 4, 0x5A, np.uint8)) for _ in range(2 * n)]
    try:
        c, p, q = [d.ptr for d in d_cur], [d.ptr for d in d_prog], [d.ptr for d in d_half]
        gpu.deint_yuv(capi.FMT_NV12, [None] + c[:-1], c, c[1:] + [None], (w, 0, 0, 0), w, h, p[:n], p[n:], (w, 0, 0, 0), 1, dr.YADIF, st)
        gpu.resize_yuv(capi.FMT_NV12, p, (w, 0, 0, 0), w, h, q, (w // 2, 0, 0, 0), w // 2, h // 2, capi.INTERP_LINEAR, st)
        s.sync()
        prev, nxt = [None] + cur[:-1], cur[1:] + [None]

        def planes(x):
            return (None, None) if x is None else (x[:w * h].reshape(h, w), x[w * h:].reshape(h // 2, w))
        for i in range(n):
            for f in range(2):
                (py, puv), (cy, cuv), (ny, nuv) = planes(prev[i]), planes(cur[i]), planes(nxt[i])
                y, uv = dr.deint(py, cy, ny, 1, f, f, dr.YADIF), dr.deint(puv, cuv, nuv, 2, f, f, dr.YADIF)
                got = d_prog[f * n + i].download((frame,), np.uint8)
                assert np.array_equal(got, np.concatenate([y.ravel(), uv.ravel()])), (i, f)
                half = d_half[f * n + i].download((frame // 4,), np.uint8)
                want = np.concatenate([rr.resize(y, 1, w // 2, h // 2, rr.LINEAR).ravel(), rr.resize(uv, 2, w // 4, h // 4, rr.LINEAR).ravel()])
                assert np.array_equal(half, want), (i, f)
    finally:
        s.close()
        for d in d_cur + d_prog + d_half:
            d.free()
