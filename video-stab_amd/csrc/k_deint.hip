// Interlaced sources on YUV surfaces: vs_op_deint_jobs, vs_op_deint_yuv (deinterlace: VS_DEINT_LINEAR, VS_DEINT_YADIF) and
// vs_op_interlace_yuv (the weave).  include/vs_stab.h defines what they compute, tests/deintref.py states it in numpy.  A job is
// one plane of w x h pixels of cn channels: rows of parity `keep` are copies of the current frame C, the others are computed from
// C's rows above and below (LINEAR), with the previous and next frame P and N as well (YADIF), or copied from the other
// progressive frame (the weave, an internal third mode: C = the first frame in time, N = the second).
//
// One launch takes up to DI_MAX_JOBS jobs in the scheme of plane_jobs.h.  A job's record is 56 bytes - four pointers with a stride
// each - so 96 of them are 5.3 KB of kernel arguments: more than the 4 KB the other plane-job operators keep to.  The kernel
// argument segment of a gfx9 code object has no such bound (the dispatch packet holds its address, scalar loads reach all of it).
//
// A tile is 256 bytes x 256 rows.  A lane owns the PJ_LB = 16 bytes at one place of a row; a wave is 16 lanes side by side times 4
// strips, and a lane walks DOWN its strip of DI_R row pairs (one kept row, one missing row each) with a window of rows in registers:
// the missing row y needs C, P and N at up / dn (y -+ 1) and the temporal pair (A, B) at y and at upp / dnn (y -+ 2); the step to
// y + 2 keeps dn as the new up and y, dnn as the new upp, y, so a step loads one row of C (with 3 pixels of halo on either side:
// the lane's own 16 bytes and the 16 before and behind), one of P, one of N and one each of A and B.  The kept row is C's dn (or
// up) row, which the window holds: a 16-byte copy without a load of its own.  At the top and bottom of a plane up / dn / upp / dnn
// fold back as the definition says; the folded row is the window's other one, not a load.
//
// Loads are 16 bytes at any address where the lane's 16 bytes lie inside the row, else sample by sample (pj_gather); a halo that
// leaves the row reads nothing and holds zeros - the search needs it only for 3 <= x < w - 3, where it is inside.  Stores are
// 16-byte non-temporal where the 16 bytes are inside the row and aligned, else sample by sample.  No load touches a byte outside
// w x h of a source, no store a byte outside w x h of the destination.  Nothing waits on data; every loop bound is a constant.
#include <hip/hip_runtime.h>

#include <vector>

#include "plane_jobs.h"

namespace vsd {
namespace {

constexpr int DI_R = 8;                      // row pairs per lane
constexpr int DI_WAVES = 4;
constexpr int DI_CL = 16;                    // lanes side by side
constexpr int DI_STRIPS = 64 / DI_CL;        // strips per wave
constexpr int DI_TB = pj_tb(DI_CL);                            // 256 bytes
constexpr int DI_TR = DI_WAVES * DI_STRIPS * DI_R * 2;         // 256 rows
constexpr int DI_WEAVE = 2;                  // the kernel's third mode, behind vs_deint_mode

struct DiJob {
    const uint8_t *p, *c, *n;                // previous, current, next (never null here: the host puts c for a null p or n)
    uint8_t* dst;
    uint32_t pstride, cstride, nstride, dstride;
    uint32_t wh;                             // w | h << 16
    uint32_t t0f;                            // the job's first tile in the launch's sequence (24 bits) | (cn - 1) << 24 | keep << 26 | second << 27
};
struct DiArgs {
    DiJob j[DI_MAX_JOBS];
    uint32_t n, tiles, mode;
};
static_assert(sizeof(DiJob) == 56, "four pointers, four strides, two words");
constexpr uint32_t DI_T0_MASK = 0xffffffu;
// 96 jobs of at most 512 x 128 tiles (32767 pixels of 4 bytes, 32767 rows)
static_assert(96ull * ((32767ull * 4 + DI_TB - 1) / DI_TB) * ((32767 + DI_TR - 1) / DI_TR) <= DI_T0_MASK, "a launch's tiles fit 24 bits");

// sample i of packed samples (i: a constant once the loops are unrolled)
template <int SB>
__device__ __forceinline__ int di_get(const uint32_t* q, int i) {
    if constexpr (SB == 1) return (int)((q[i >> 2] >> (8 * (i & 3))) & 0xffu);
    else return (int)((q[i >> 1] >> (16 * (i & 1))) & 0xffffu);
}
__device__ __forceinline__ int di_abs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ void di_copy4(uint32_t* d, const uint32_t* s) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3]; }

// The 16 bytes at p, of which the first nvb lie inside the row (nvb <= 0: none - zeros)
template <int SB>
__device__ __forceinline__ void di_load(const uint8_t* p, int nvb, uint32_t* o) {
    uint32_t t[4];
    if (nvb >= PJ_LB) pj_load16<pj_q1>(p, t);
    else pj_gather<SB>(p, nvb, t);
    di_copy4(o, t);
}
template <int SB>
__device__ __forceinline__ void di_store(uint8_t* p, int nvb, const uint32_t* o) {
    const uint32_t t[4] = {o[0], o[1], o[2], o[3]};
    if (nvb == PJ_LB && ((uintptr_t)p & 15) == 0) __builtin_nontemporal_store(pj_pack16(t), reinterpret_cast<pj_u4*>(p));
    else pj_scatter<SB>(p, nvb, t);
}

// The lane's place in a row
struct DiLane {
    int e0, nvb;             // its first byte, its bytes inside the row
    int nl, nr;              // the bytes inside the row of the 16 before it (0 or 16) and of the 16 behind it
};

// A row of C with its halo (q[0 .. 3] before, q[4 .. 7] the lane's, q[8 .. 11] behind) or without (q[4 .. 7] only)
template <int SB>
__device__ __forceinline__ void di_load_c(const uint8_t* row, const DiLane& L, bool halo, uint32_t* q) {
    di_load<SB>(row + L.e0, L.nvb, q + 4);
    if (halo) {
        di_load<SB>(row + L.e0 - PJ_LB, L.nl, q);
        di_load<SB>(row + L.e0 + PJ_LB, L.nr, q + 8);
    }
}

template <int SB, int CN>
__device__ __forceinline__ void di_tile(const DiJob& J, int mode, int tx, int ty) {
    constexpr int NEL = PJ_LB / SB;                   // samples of a lane per row
    constexpr int SPD = 4 / SB;                       // samples per dword
    const int w = J.wh & 0xffffu, h = J.wh >> 16;
    const int keep = (J.t0f >> 26) & 1u, second = (J.t0f >> 27) & 1u;
    const int rowb = w * CN * SB;
    const int lane = threadIdx.x & (DI_CL - 1), strip = threadIdx.x / DI_CL, wave = threadIdx.y;
    DiLane L;
    L.e0 = (tx * DI_CL + lane) * PJ_LB;
    L.nvb = min(PJ_LB, rowb - L.e0);
    if (L.nvb <= 0) return;
    L.nl = L.e0 >= PJ_LB ? PJ_LB : 0;
    L.nr = min(PJ_LB, rowb - L.e0 - PJ_LB);
    const int pair0 = ((ty * DI_WAVES + wave) * DI_STRIPS + strip) * DI_R;
    if (2 * pair0 >= h) return;
    const size_t cs = J.cstride, ps = J.pstride, ns = J.nstride, ds = J.dstride;
    const uint8_t* __restrict__ C = J.c + L.e0;
    const uint8_t* __restrict__ N = J.n + L.e0;
    uint8_t* __restrict__ D = J.dst + L.e0;

    if (mode == DI_WEAVE) {                           // rows of parity keep from C, the others from N
#pragma unroll 1
        for (int r = 0; r < 2 * DI_R; r++) {
            const int y = 2 * pair0 + r;
            if (y >= h) break;
            uint32_t q[4];
            di_load<SB>((y & 1) == keep ? C + (size_t)y * cs : N + (size_t)y * ns, L.nvb, q);
            di_store<SB>(D + (size_t)y * ds, L.nvb, q);
        }
        return;
    }

    const bool yadif = mode == VS_DEINT_YADIF;
    const uint8_t* __restrict__ P = J.p + L.e0;
    // the temporal pair
    const uint8_t* __restrict__ A = second ? C : P;
    const uint8_t* __restrict__ B = second ? N : C;
    const size_t as = second ? cs : ps, bs = second ? ns : cs;
    const int s0 = L.e0 / SB;                         // the lane's first sample in the row

    // the window: C with halo, P and N at up / dn; A and B at upp / y / dnn
    uint32_t cu[12] = {}, cd[12] = {}, pu[4] = {}, pd[4] = {}, nu[4] = {}, nd[4] = {};
    uint32_t aU[4] = {}, bU[4] = {}, aY[4] = {}, bY[4] = {}, aD[4] = {}, bD[4] = {};
    {
        const int y = 2 * pair0 + (1 - keep);         // the strip's first missing row (y > h - 1: an odd h's last kept row only)
        if (y > 0) {
            di_load_c<SB>(J.c + (size_t)(y - 1) * cs, L, yadif, cu);
            if (yadif) {
                di_load<SB>(P + (size_t)(y - 1) * ps, L.nvb, pu);
                di_load<SB>(N + (size_t)(y - 1) * ns, L.nvb, nu);
            }
        }
        if (yadif && y < h) {
            di_load<SB>(A + (size_t)y * as, L.nvb, aY);
            di_load<SB>(B + (size_t)y * bs, L.nvb, bY);
            if (y >= 2) {
                di_load<SB>(A + (size_t)(y - 2) * as, L.nvb, aU);
                di_load<SB>(B + (size_t)(y - 2) * bs, L.nvb, bU);
            }
        }
    }

#pragma unroll 1
    for (int r = 0; r < DI_R; r++) {
        const int y = 2 * (pair0 + r) + (1 - keep);
        if (y >= h) {                                 // no missing row; keep 0 and an odd h: the kept row h - 1 is the up row
            if (!keep && y == h) di_store<SB>(D + (size_t)(y - 1) * ds, L.nvb, cu + 4);
            break;
        }
        // dn: row y + 1, or up again at the bottom
        if (y + 1 < h) {
            di_load_c<SB>(J.c + (size_t)(y + 1) * cs, L, yadif, cd);
            if (yadif) {
                di_load<SB>(P + (size_t)(y + 1) * ps, L.nvb, pd);
                di_load<SB>(N + (size_t)(y + 1) * ns, L.nvb, nd);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) cd[k] = cu[k];
            di_copy4(pd, pu); di_copy4(nd, nu);
        }
        if (y == 0) {                                 // up: dn again at the top
#pragma unroll
            for (int k = 0; k < 12; k++) cu[k] = cd[k];
            di_copy4(pu, pd); di_copy4(nu, nd);
        }
        // the kept row of the pair
        if (keep) {
            if (y + 1 < h) di_store<SB>(D + (size_t)(y + 1) * ds, L.nvb, cd + 4);
        } else {
            di_store<SB>(D + (size_t)(y - 1) * ds, L.nvb, cu + 4);
        }

        uint32_t o[4] = {0, 0, 0, 0};
        if (!yadif) {
#pragma unroll
            for (int i = 0; i < NEL; i++) {
                const int v = (di_get<SB>(cu + 4, i) + di_get<SB>(cd + 4, i) + 1) >> 1;
                o[i / SPD] |= (uint32_t)v << (8 * SB * (i % SPD));
            }
        } else {
            // dnn: row y + 2, or upp again at the bottom; upp: dnn again at the top
            if (y + 2 < h) {
                di_load<SB>(A + (size_t)(y + 2) * as, L.nvb, aD);
                di_load<SB>(B + (size_t)(y + 2) * bs, L.nvb, bD);
            } else {
                di_copy4(aD, aU); di_copy4(bD, bU);
            }
            if (y == 0) { di_copy4(aU, aD); di_copy4(bU, bD); }
            const bool chk = !(y == 1 || y + 2 == h);
#pragma unroll
            for (int i = 0; i < NEL; i++) {
                const int x = (s0 + i) / CN;
                // C's up and dn rows, j pixels from x (index NEL = the lane's first sample)
                auto U = [&](int j) { return di_get<SB>(cu, NEL + i + j * CN); };
                auto E = [&](int j) { return di_get<SB>(cd, NEL + i + j * CN); };
                const int c = U(0), e = E(0);
                const int a = di_get<SB>(aY, i), b = di_get<SB>(bY, i);
                const int d = (a + b) >> 1;
                const int td0 = di_abs(a - b);
                const int td1 = (di_abs(di_get<SB>(pu, i) - c) + di_abs(di_get<SB>(pd, i) - e)) >> 1;
                const int td2 = (di_abs(di_get<SB>(nu, i) - c) + di_abs(di_get<SB>(nd, i) - e)) >> 1;
                int diff = max(max(td0 >> 1, td1), td2);
                int sp = (c + e) >> 1;
                // the edge-directed search (a lane's pixels with x < 3 or x >= w - 3 compute it on whatever the halo holds and drop it)
                auto score = [&](int j) { return di_abs(U(-1 + j) - E(-1 - j)) + di_abs(U(j) - E(-j)) + di_abs(U(1 + j) - E(1 - j)); };
                const bool inner = x >= 3 && x < w - 3;
                int best = score(0) - 1;
#pragma unroll
                for (int g = -1; g <= 1; g += 2) {
                    const int s1 = score(g), s2 = score(2 * g);
                    const bool m1 = inner && s1 < best;
                    best = m1 ? s1 : best;
                    sp = m1 ? (U(g) + E(-g)) >> 1 : sp;
                    const bool m2 = m1 && s2 < best;
                    best = m2 ? s2 : best;
                    sp = m2 ? (U(2 * g) + E(-2 * g)) >> 1 : sp;
                }
                // the spatial interlacing check
                const int bb = (di_get<SB>(aU, i) + di_get<SB>(bU, i)) >> 1, ff = (di_get<SB>(aD, i) + di_get<SB>(bD, i)) >> 1;
                const int mx = max(max(d - e, d - c), min(bb - c, ff - e));
                const int mn = min(min(d - e, d - c), max(bb - c, ff - e));
                diff = chk ? max(max(diff, mn), -mx) : diff;
                const int v = sp > d + diff ? d + diff : sp < d - diff ? d - diff : sp;
                o[i / SPD] |= (uint32_t)v << (8 * SB * (i % SPD));
            }
            // the step to y + 2
            di_copy4(aU, aY); di_copy4(bU, bY);
            di_copy4(aY, aD); di_copy4(bY, bD);
        }
        di_store<SB>(D + (size_t)y * ds, L.nvb, o);
#pragma unroll
        for (int k = 0; k < 12; k++) cu[k] = cd[k];
        di_copy4(pu, pd); di_copy4(nu, nd);
    }
}

template <int SB>
__global__ __launch_bounds__(64 * DI_WAVES) void deint_kernel(const DiArgs a) {
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const DiJob J = a.j[pj_find(a, seq, [](const DiJob& j) { return j.t0f & DI_T0_MASK; })];
    const uint32_t cn = ((J.t0f >> 24) & 3u) + 1u;
    const PjTile t = pj_split(seq - (J.t0f & DI_T0_MASK), (J.wh & 0xffffu) * cn * SB, DI_TB);
    const int mode = (int)a.mode;
    if (cn == 1) di_tile<SB, 1>(J, mode, t.tx, t.ty);
    else if (cn == 2) di_tile<SB, 2>(J, mode, t.tx, t.ty);
    else if constexpr (SB == 1) {
        if (cn == 3) di_tile<SB, 3>(J, mode, t.tx, t.ty);
        else di_tile<SB, 4>(J, mode, t.tx, t.ty);
    }
}

// What the operators refuse about a job by itself; nullptr = accepted
const char* di_job_refusal(const vs_deint_job& s, int sample_bytes, bool weave) {
    if (!s.cur || !s.dst || (weave && !s.next)) return "a null cur or dst";
    if (const char* why = pj_bad_sizes({s.w, s.h})) return why;
    if (s.h < 2) return "h must be at least 2 (a plane of one row has no second field)";
    if (s.reserved != 0) return "reserved must be 0";
    if (s.cn < 1 || s.cn > (sample_bytes == 1 ? 4 : 2)) return sample_bytes == 1 ? "cn must be 1 .. 4 with 8-bit samples" : "cn must be 1 or 2 with 16-bit samples";
    if (s.keep != 0 && s.keep != 1) return "keep must be 0 or 1";
    if (s.second != 0 && s.second != 1) return "second must be 0 or 1";
    const size_t row = (size_t)s.w * s.cn * sample_bytes;
    if (const char* why = pj_bad_strides({{s.cur_stride, row}, {s.dst_stride, row}, {s.prev ? s.prev_stride : row, row}, {s.next ? s.next_stride : row, row}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.cur | (uintptr_t)s.dst | (uintptr_t)s.prev | (uintptr_t)s.next | s.cur_stride | s.dst_stride |
                                                          (s.prev ? s.prev_stride : 0) | (s.next ? s.next_stride : 0)))
        return why;
    return nullptr;
}

struct DiSpan { uintptr_t a, b; };
DiSpan di_span(const void* p, size_t stride, const vs_deint_job& s, int sample_bytes) {
    return {(uintptr_t)p, pj_end(p, stride, s.h, (size_t)s.w * s.cn * sample_bytes)};
}

// The launch, every job by itself, then the destinations against every source and every other destination of the call
int di_check(const char* name, const vs_deint_job* jobs, int n, int sample_bytes, int mode) {
    auto refuse = [&](const std::string& why) {
        set_last_error(std::string(name) + ": " + why);
        return (int)VS_ERR_INVALID_ARG;
    };
    if (!pj_launch_ok(jobs, n, DI_MAX_JOBS, sample_bytes)) return refuse("invalid argument (1 .. " + std::to_string(DI_MAX_JOBS) + " jobs of one sample size, 1 or 2 bytes)");
    if (mode != VS_DEINT_LINEAR && mode != VS_DEINT_YADIF && mode != DI_WEAVE) return refuse("mode = " + std::to_string(mode) + " is not a vs_deint_mode (0, 1)");
    for (int i = 0; i < n; i++)
        if (const char* why = di_job_refusal(jobs[i], sample_bytes, mode == DI_WEAVE)) return refuse("job " + std::to_string(i) + ": " + why);
    for (int i = 0; i < n; i++) {
        const DiSpan d = di_span(jobs[i].dst, jobs[i].dst_stride, jobs[i], sample_bytes);
        for (int k = 0; k < n; k++) {
            const vs_deint_job& s = jobs[k];
            const void* src[3] = {s.cur, s.prev, s.next};
            const size_t stride[3] = {s.cur_stride, s.prev_stride, s.next_stride};
            for (int q = 0; q < 3; q++) {
                if (!src[q]) continue;
                const DiSpan r = di_span(src[q], stride[q], s, sample_bytes);
                if (pj_overlap(d.a, d.b, r.a, r.b))
                    return refuse("job " + std::to_string(i) + ": the destination overlaps " + (q == 0 ? "cur" : q == 1 ? "prev" : "next") + " of job " + std::to_string(k));
            }
            if (k < i) {
                const DiSpan r = di_span(s.dst, s.dst_stride, s, sample_bytes);
                if (pj_overlap(d.a, d.b, r.a, r.b)) return refuse("job " + std::to_string(i) + ": the destination overlaps the destination of job " + std::to_string(k));
            }
        }
    }
    return VS_OK;
}

}  // namespace

int launch_deint(const char* name, const vs_deint_job* jobs, int n, int sample_bytes, int mode, hipStream_t st) {
    VS_TRY(di_check(name, jobs, n, sample_bytes, mode));
    DiArgs a{};
    a.mode = (uint32_t)mode;
    return pj_launch(
        name, jobs, n, DI_MAX_JOBS, sample_bytes, a, [](const vs_deint_job&, int, int*) -> const char* { return nullptr; },
        [&](const vs_deint_job& s, DiJob& j, uint32_t tile0) {
            j.c = (const uint8_t*)s.cur; j.cstride = (uint32_t)s.cur_stride;
            j.p = s.prev ? (const uint8_t*)s.prev : j.c; j.pstride = s.prev ? (uint32_t)s.prev_stride : j.cstride;
            j.n = s.next ? (const uint8_t*)s.next : j.c; j.nstride = s.next ? (uint32_t)s.next_stride : j.cstride;
            j.dst = (uint8_t*)s.dst; j.dstride = (uint32_t)s.dst_stride;
            j.wh = (uint32_t)s.w | (uint32_t)s.h << 16;
            j.t0f = tile0 | (uint32_t)(s.cn - 1) << 24 | (uint32_t)s.keep << 26 | (uint32_t)s.second << 27;
            return pj_tiles((size_t)s.w * s.cn * sample_bytes, s.h, DI_TB, DI_TR);
        },
        [&](auto sb, const DiArgs& args, unsigned tiles) { hipLaunchKernelGGL(deint_kernel<decltype(sb)::value>, dim3(tiles), dim3(64, DI_WAVES), 0, st, args); });
}

}  // namespace vsd

// ---- the C entry points (include/vs_stab.h) -------------------------------------------------------------------------------
namespace {

using namespace vsd;

int di_refuse(const std::string& why) {
    set_last_error(why);
    return VS_ERR_INVALID_ARG;
}

// The planes of a surface as jobs see them: luma; the interleaved (U, V) plane as cn 2, or U and V as planes of their own
struct DiPlane { size_t ioff, ipitch, ooff, opitch; int sx, sy, cn; };
int di_planes(const PixFmt& f, const I420Layout& li, const I420Layout& lo, DiPlane (&planes)[3]) {
    int np = 0;
    planes[np++] = DiPlane{0, li.pitch, 0, lo.pitch, 0, 0, 1};
    if (f.luma_uv()) planes[np++] = DiPlane{li.u, li.cpitch, lo.u, lo.cpitch, f.sx, f.sy, 2};
    else {
        planes[np++] = DiPlane{li.u, li.cpitch, lo.u, lo.cpitch, f.sx, f.sy, 1};
        planes[np++] = DiPlane{li.v, li.cpitch, lo.v, lo.cpitch, f.sx, f.sy, 1};
    }
    return np;
}

// What both surface calls refuse before their sides' own rules: the format, the count, tff, the plane heights
int di_check_call(const char* call, int fmt, int n, int limit, int w, int h, int tff, std::string* head) {
    const PixFmt* f = pixfmt(fmt);
    if (!f || f->kind == PIX_INTERLEAVED)
        return di_refuse(std::string(call) + ": " + (f ? std::string(f->name) : "format " + std::to_string(fmt)) + " is not a YUV surface format (NV12, P010, I420 ... I412)");
    *head = std::string(call) + ": " + f->name + ": ";
    if (n < 1 || n > limit) return di_refuse(*head + "n must be 1 .. " + std::to_string(limit) + " frames");
    if (tff != 0 && tff != 1) return di_refuse(*head + "tff must be 0 or 1");
    if (pj_bad_sizes({w, h})) return di_refuse(*head + "sizes must be 1 .. 32767");
    if ((h >> f->sy) < 2) return di_refuse(*head + "every plane needs at least 2 rows (h must be at least " + std::to_string(2 << f->sy) + ")");
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_op_deint_jobs(const vs_deint_job* jobs, int n, int sample_bytes, int mode, void* stream) {
    if (mode != VS_DEINT_LINEAR && mode != VS_DEINT_YADIF) return di_refuse("vs_op_deint_jobs: mode = " + std::to_string(mode) + " is not a vs_deint_mode (0, 1)");
    return vsd::launch_deint("vs_op_deint_jobs", jobs, n, sample_bytes, mode, (hipStream_t)stream);
}

int vs_op_deint_yuv(int fmt, const void* const* d_prev, const void* const* d_cur, const void* const* d_next, const vs_i420_layout* in, int w, int h,
                    void* const* d_first, void* const* d_second, const vs_i420_layout* out, int tff, int mode, int n, void* stream) {
    static const char call[] = "vs_op_deint_yuv";
    std::string head, msg;
    if (int rc = di_check_call(call, fmt, n, 16, w, h, tff, &head)) return rc;
    if (mode != VS_DEINT_LINEAR && mode != VS_DEINT_YADIF) return di_refuse(head + "mode = " + std::to_string(mode) + " is not a vs_deint_mode (0, 1)");
    if (!d_cur || !d_first) return di_refuse(head + "null pointer");
    // a NULL previous or next frame stands for the current one
    std::vector<const void*> prev(n), next(n);
    for (int i = 0; i < n; i++) {
        prev[i] = d_prev && d_prev[i] ? d_prev[i] : d_cur[i];
        next[i] = d_next && d_next[i] ? d_next[i] : d_cur[i];
    }
    I420Layout li, lo;
    if (cvt_check_yuv((std::string(call) + ": source (cur)").c_str(), fmt, d_cur, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": source (prev)").c_str(), fmt, prev.data(), n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": source (next)").c_str(), fmt, next.data(), n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": destination (first)").c_str(), fmt, d_first, n, out, w, h, &lo, &msg) != VS_OK ||
        (d_second && cvt_check_yuv((std::string(call) + ": destination (second)").c_str(), fmt, d_second, n, out, w, h, &lo, &msg) != VS_OK))
        return di_refuse(msg);
    const PixFmt& f = *pixfmt(fmt);
    DiPlane planes[3];
    const int np = di_planes(f, li, lo, planes);
    std::vector<vs_deint_job> jobs;
    for (int i = 0; i < n; i++)
        for (int field = 0; field < (d_second ? 2 : 1); field++)
            for (int k = 0; k < np; k++) {
                const DiPlane& p = planes[k];
                void* dst = field ? d_second[i] : d_first[i];
                jobs.push_back(vs_deint_job{(const uint8_t*)prev[i] + p.ioff, p.ipitch, (const uint8_t*)d_cur[i] + p.ioff, p.ipitch,
                                            (const uint8_t*)next[i] + p.ioff, p.ipitch, (uint8_t*)dst + p.ooff, p.opitch, w >> p.sx, h >> p.sy, p.cn,
                                            (tff ? 0 : 1) ^ field, field, 0});
            }
    return vsd::launch_deint((std::string(call) + ": " + f.name).c_str(), jobs.data(), (int)jobs.size(), f.sample_bytes, mode, (hipStream_t)stream);
}

int vs_op_interlace_yuv(int fmt, const void* const* d_first, const void* const* d_second, const vs_i420_layout* in, int w, int h, void* const* d_dst,
                        const vs_i420_layout* out, int tff, int n, void* stream) {
    static const char call[] = "vs_op_interlace_yuv";
    std::string head, msg;
    if (int rc = di_check_call(call, fmt, n, 32, w, h, tff, &head)) return rc;
    I420Layout li, lo;
    if (cvt_check_yuv((std::string(call) + ": source (first)").c_str(), fmt, d_first, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": source (second)").c_str(), fmt, d_second, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": destination").c_str(), fmt, d_dst, n, out, w, h, &lo, &msg) != VS_OK)
        return di_refuse(msg);
    const PixFmt& f = *pixfmt(fmt);
    DiPlane planes[3];
    const int np = di_planes(f, li, lo, planes);
    std::vector<vs_deint_job> jobs;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < np; k++) {
            const DiPlane& p = planes[k];
            jobs.push_back(vs_deint_job{nullptr, 0, (const uint8_t*)d_first[i] + p.ioff, p.ipitch, (const uint8_t*)d_second[i] + p.ioff, p.ipitch,
                                        (uint8_t*)d_dst[i] + p.ooff, p.opitch, w >> p.sx, h >> p.sy, p.cn, tff ? 0 : 1, 0, 0});
        }
    return vsd::launch_deint((std::string(call) + ": " + f.name).c_str(), jobs.data(), (int)jobs.size(), f.sample_bytes, 2, (hipStream_t)stream);
}

}  // extern "C"
