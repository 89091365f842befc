// The fade border on YUV surfaces: vs_op_fade_blend_jobs and vs_op_fade_update_jobs, the two launches a stream with
// vs_stab_set_yuv_fade queues around its warp.  Planes of 8- or 16-bit samples, one job per plane, cn 1 (Y, U, V) or 2 (the
// interleaved UV plane of NV12 / P010); tests/yuvfaderef.py in numpy.
//
//   blend   pad and blend in one pass: dst = addWeighted(hist, alpha, inside ? src : fill, beta) over the padded plane of
//           (sw + 2 bx) x (sh + 2 by) samples - v = fma(hist, alpha, fl32(frame * beta)) in float, rounded half to even, saturated
//           to the sample (fade_blend_kernel of k_traj.hip for bytes; the same three operations for words).  The padded frame is
//           never written unblended.
//   update  hist = (T)((1.0f - 0.1f) * hist + 0.1f * result): two float products, one float sum, truncation (fade_update_kernel);
//           the library is built without contraction, so they stay three operations.
//
// Both launches follow k_yuvpad.hip: the jobs travel as kernel arguments, a launch is a flat sequence of (job, tile row, tile
// column) tiles in the XCD-aware order of k_warp.hip (tile_id), a workgroup finds its job by bisection over the jobs' first tiles.
// A lane owns YF_LB = 16 bytes at one place of YF_R rows; a wave is yf_cl lanes side by side times 64 / yf_cl rows.
//
//   blend, interior lanes (all 16 bytes inside the picture): their 16 source bytes in ONE 16-byte load at the source's own
//     alignment; lanes wholly in the border take the fill without a load; lanes across the left or right edge of the picture go
//     sample by sample ("inside or fill": there is no index map).
//   history: 16-byte loads (and, in the update, stores) where the lane's 16 bytes are inside the row and 16-byte aligned - always
//     in a stream, whose history has the layout of its padded scratch surface - else sample by sample.
//   blend destination: 16-byte non-temporal stores under the same condition, else sample by sample.
//   update, result plane: the caller's output surface at any alignment: ONE 16-byte load of exactly the lane's bytes, sample by
//     sample at a row's end.
//
// No load touches a byte outside the source, history or result planes, no store a byte outside the destination or history plane.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "vs_common.h"

namespace vsd {
namespace {

constexpr int YF_LB = 16;                    // bytes per lane and row
constexpr int YF_R = 8;                      // rows per lane
constexpr int YF_WAVES = 4;
// A wave is cl lanes side by side times 64 / cl rows ("Fade on YUV", has the shapes that were measured).
#ifndef YF_CL_8
#define YF_CL_8 16
#endif
#ifndef YF_CL_16
#define YF_CL_16 32
#endif
constexpr int yf_cl(int sb) { return sb == 1 ? YF_CL_8 : YF_CL_16; }
constexpr int yf_tb(int sb) { return yf_cl(sb) * YF_LB; }                        // tile: bytes ...
constexpr int yf_tr(int sb) { return YF_WAVES * YF_R * (64 / yf_cl(sb)); }       // ... and rows

struct YfJob {                               // blend
    const uint8_t* src;
    const uint8_t* hist;
    uint8_t* dst;
    uint32_t sstride, hstride, dstride;
    uint32_t swh;                            // sw | sh << 16
    uint32_t bxy;                            // bx | by << 16
    uint32_t t0f;                            // the job's first tile in the launch's sequence (24 bits) | (cn - 1) << 24
    uint32_t fill;                           // fill[0] | fill[1] << 16
    uint32_t pad_;
};
struct YfArgs {
    YfJob j[YF_MAX_JOBS];
    uint32_t n, tiles;
    float alpha, beta;
};
struct YfuJob {                              // update
    uint8_t* hist;
    const uint8_t* res;
    uint32_t hstride, rstride;
    uint32_t rowb, rows;                     // bytes of a row (w * cn * sample bytes), rows
    uint32_t t0;
    uint32_t pad_;
};
struct YfuArgs {
    YfuJob j[YF_MAX_JOBS];
    uint32_t n, tiles;
};
static_assert(sizeof(YfJob) == 56 && sizeof(YfArgs) <= 4096 && sizeof(YfuJob) == 40 && sizeof(YfuArgs) <= 4096, "the jobs travel as kernel arguments");
constexpr uint32_t YF_T0_MASK = 0xffffffu;
// 32 jobs of at most 32767 pixels of 2 or 4 bytes by 32767 rows
static_assert(32ull * ((32767ull * 2 + yf_tb(1) - 1) / yf_tb(1)) * ((32767 + yf_tr(1) - 1) / yf_tr(1)) <= YF_T0_MASK &&
                  32ull * ((32767ull * 4 + yf_tb(2) - 1) / yf_tb(2)) * ((32767 + yf_tr(2) - 1) / yf_tr(2)) <= YF_T0_MASK,
              "a launch's tiles fit 24 bits");

typedef uint32_t yf_u4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) yf_q1 { uint32_t x, y, z, w; };    // 16 bytes at any address: ONE global_load_dwordx4

template <int SB>
__device__ __forceinline__ uint32_t yf_ld(const uint8_t* p) {
    if constexpr (SB == 1) return *p;
    else return *reinterpret_cast<const uint16_t*>(p);
}

// the first nvb bytes at p, sample by sample (the rest 0)
template <int SB>
__device__ __forceinline__ void yf_gather(const uint8_t* p, int nvb, uint32_t (&o)[4]) {
    constexpr int NEL = YF_LB / SB, SPD = 4 / SB;
    o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
    for (int i = 0; i < NEL; i++)
        if (i * SB < nvb) o[i / SPD] |= yf_ld<SB>(p + i * SB) << (8 * SB * (i % SPD));
}

template <int SB>
__device__ __forceinline__ void yf_scatter(uint8_t* p, int nvb, const uint32_t (&o)[4]) {
    constexpr int NEL = YF_LB / SB, SPD = 4 / SB;
#pragma unroll
    for (int i = 0; i < NEL; i++) {
        if (i * SB < nvb) {
            const uint32_t v = o[i / SPD] >> (8 * SB * (i % SPD));
            if constexpr (SB == 1) p[i] = (uint8_t)v;
            else reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)v;
        }
    }
}

// The tile sequence: workgroup `lin` of n takes tile seq (XCD c = lin mod 8 the c-th contiguous eighth)
__device__ __forceinline__ uint32_t yf_seq(uint32_t lin, uint32_t n) {
    const uint32_t c = lin & 7u, k = lin >> 3, q = n >> 3, r = n & 7u;
    return c * q + (c < r ? c : r) + k;
}

template <int SB, int CN>
__device__ __forceinline__ void yf_blend_tile(const YfJob& J, int tx, int ty, float alpha, float beta) {
    constexpr int NEL = YF_LB / SB;                   // samples of a lane per row
    constexpr int NPX = NEL / CN;                     // pixels
    constexpr int PB = SB * CN;                       // bytes of a pixel
    constexpr int SPD = 4 / SB;                       // samples per dword
    constexpr uint32_t SMASK = SB == 1 ? 0xffu : 0xffffu;
    constexpr int SMAX = SB == 1 ? 255 : 65535;
    constexpr int CL = yf_cl(SB), RW = 64 / CL, TR = yf_tr(SB);
    const int sw = J.swh & 0xffffu, sh = J.swh >> 16, bx = J.bxy & 0xffffu, by = J.bxy >> 16;
    const int dw = sw + 2 * bx, dh = sh + 2 * by;
    const int lane = threadIdx.x & (CL - 1), sub = threadIdx.x / CL, wave = threadIdx.y;
    const uint32_t fills[2] = {J.fill & 0xffffu, J.fill >> 16};

    const int e0 = (tx * CL + lane) * YF_LB;          // first byte of the lane in the padded row
    const int nvb = min(YF_LB, dw * PB - e0);         // its bytes inside the row (a multiple of PB)
    if (nvb <= 0) return;
    const int px0 = e0 / PB;                          // its first pixel
    const bool interior = px0 >= bx && px0 + NPX <= bx + sw;      // (then nvb == YF_LB)
    const bool outside = px0 + NPX <= bx || px0 >= bx + sw;       // every pixel of the lane is border
    const bool full = nvb == YF_LB;

    // the fill of a lane's 16 bytes
    uint32_t fq;
    if constexpr (SB == 1 && CN == 1) fq = fills[0] * 0x01010101u;
    else if constexpr (SB == 1) fq = (fills[0] | fills[1] << 8) * 0x00010001u;
    else if constexpr (CN == 1) fq = fills[0] * 0x00010001u;
    else fq = J.fill;

#pragma unroll 1
    for (int r = 0; r < YF_R; r++) {
        const int dy = ty * TR + (wave * YF_R + r) * RW + sub;
        if (dy >= dh) break;
        const int sy = dy - by;
        const uint8_t* __restrict__ hp = J.hist + (size_t)dy * J.hstride + (size_t)e0;
        uint8_t* __restrict__ dp = J.dst + (size_t)dy * J.dstride + (size_t)e0;
        uint32_t hq[4], fr[4], o[4];
        if (full && ((uintptr_t)hp & 15) == 0) {
            const yf_u4 q = *reinterpret_cast<const yf_u4*>(hp);
            hq[0] = q.x; hq[1] = q.y; hq[2] = q.z; hq[3] = q.w;
        } else {
            yf_gather<SB>(hp, nvb, hq);
        }
        if ((unsigned)sy >= (unsigned)sh || outside) {
            fr[0] = fr[1] = fr[2] = fr[3] = fq;
        } else {
            const uint8_t* __restrict__ rp = J.src + (size_t)sy * J.sstride;
            if (interior) {
                // exactly the lane's 16 source bytes, wherever they start
                const yf_q1 q = *reinterpret_cast<const yf_q1*>(rp + (size_t)(px0 - bx) * PB);
                fr[0] = q.x; fr[1] = q.y; fr[2] = q.z; fr[3] = q.w;
            } else {
                fr[0] = fr[1] = fr[2] = fr[3] = 0;
#pragma unroll
                for (int k = 0; k < NPX; k++) {
                    const int sx = px0 + k - bx;
                    const bool in = (unsigned)sx < (unsigned)sw && k * PB < nvb;
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const int i = k * CN + c;
                        const uint32_t v = in ? yf_ld<SB>(rp + ((size_t)sx * CN + c) * SB) : fills[c];
                        fr[i / SPD] |= v << (8 * SB * (i % SPD));
                    }
                }
            }
        }
        o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
        for (int i = 0; i < NEL; i++) {
            const float a = (float)((hq[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            const float b = (float)((fr[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            int v = __float2int_rn(fmaf(a, alpha, __fmul_rn(b, beta)));
            v = v < 0 ? 0 : (v > SMAX ? SMAX : v);
            o[i / SPD] |= (uint32_t)v << (8 * SB * (i % SPD));
        }
        if (full && ((uintptr_t)dp & 15) == 0) {
            yf_u4 q;
            q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
            __builtin_nontemporal_store(q, reinterpret_cast<yf_u4*>(dp));
        } else {
            yf_scatter<SB>(dp, nvb, o);
        }
    }
}

template <int SB>
__global__ __launch_bounds__(64 * YF_WAVES) void yuvfade_blend_kernel(const YfArgs a) {
    const uint32_t seq = yf_seq(blockIdx.x, a.tiles);
    // the job of tile seq: the last one whose first tile is not behind it
    uint32_t jl = 0, jh = a.n - 1;
    while (jl < jh) {
        const uint32_t mid = (jl + jh + 1) >> 1;
        if ((a.j[mid].t0f & YF_T0_MASK) <= seq) jl = mid;
        else jh = mid - 1;
    }
    const YfJob J = a.j[jl];
    const uint32_t t = seq - (J.t0f & YF_T0_MASK);
    const uint32_t cn = ((J.t0f >> 24) & 1u) + 1u;
    const uint32_t dw = (J.swh & 0xffffu) + 2u * (J.bxy & 0xffffu);
    const uint32_t gx = (dw * cn * SB + yf_tb(SB) - 1) / yf_tb(SB);
    const int ty = (int)(t / gx), tx = (int)(t - (uint32_t)ty * gx);
    if (cn == 1) yf_blend_tile<SB, 1>(J, tx, ty, a.alpha, a.beta);
    else yf_blend_tile<SB, 2>(J, tx, ty, a.alpha, a.beta);
}

template <int SB>
__global__ __launch_bounds__(64 * YF_WAVES) void yuvfade_update_kernel(const YfuArgs a) {
    constexpr int NEL = YF_LB / SB, SPD = 4 / SB;
    constexpr uint32_t SMASK = SB == 1 ? 0xffu : 0xffffu;
    constexpr int CL = yf_cl(SB), RW = 64 / CL, TR = yf_tr(SB);
    const uint32_t seq = yf_seq(blockIdx.x, a.tiles);
    uint32_t jl = 0, jh = a.n - 1;
    while (jl < jh) {
        const uint32_t mid = (jl + jh + 1) >> 1;
        if (a.j[mid].t0 <= seq) jl = mid;
        else jh = mid - 1;
    }
    const YfuJob J = a.j[jl];
    const uint32_t t = seq - J.t0;
    const uint32_t gx = (J.rowb + yf_tb(SB) - 1) / yf_tb(SB);
    const int ty = (int)(t / gx), tx = (int)(t - (uint32_t)ty * gx);
    const int lane = threadIdx.x & (CL - 1), sub = threadIdx.x / CL, wave = threadIdx.y;
    const int e0 = (tx * CL + lane) * YF_LB;
    const int nvb = min(YF_LB, (int)J.rowb - e0);
    if (nvb <= 0) return;
    const bool full = nvb == YF_LB;
    const float rate = 0.1f, keep = 1.0f - rate;
#pragma unroll 1
    for (int r = 0; r < YF_R; r++) {
        const int y = ty * TR + (wave * YF_R + r) * RW + sub;
        if (y >= (int)J.rows) break;
        uint8_t* hp = J.hist + (size_t)y * J.hstride + (size_t)e0;
        const uint8_t* rp = J.res + (size_t)y * J.rstride + (size_t)e0;
        const bool vec = full && ((uintptr_t)hp & 15) == 0;
        uint32_t hq[4], rq[4], o[4];
        if (vec) {
            const yf_u4 q = *reinterpret_cast<const yf_u4*>(hp);
            hq[0] = q.x; hq[1] = q.y; hq[2] = q.z; hq[3] = q.w;
        } else {
            yf_gather<SB>(hp, nvb, hq);
        }
        if (full) {
            const yf_q1 q = *reinterpret_cast<const yf_q1*>(rp);
            rq[0] = q.x; rq[1] = q.y; rq[2] = q.z; rq[3] = q.w;
        } else {
            yf_gather<SB>(rp, nvb, rq);
        }
        o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
        for (int i = 0; i < NEL; i++) {
            const float h = (float)((hq[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            const float s = (float)((rq[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            const float v = __fadd_rn(__fmul_rn(keep, h), __fmul_rn(rate, s));
            o[i / SPD] |= ((uint32_t)(int)v & SMASK) << (8 * SB * (i % SPD));
        }
        if (vec) {
            yf_u4 q;
            q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
            *reinterpret_cast<yf_u4*>(hp) = q;
        } else {
            yf_scatter<SB>(hp, nvb, o);
        }
    }
}

inline bool yf_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }
inline uintptr_t yf_end(const void* p, size_t stride, int rows, size_t row) { return (uintptr_t)p + (size_t)(rows - 1) * stride + row; }

// What the operators refuse about a job, decided before any device call; "" = accepted.
std::string yf_blend_refusal(const vs_fade_job& s, int sample_bytes) {
    if (!s.src || !s.hist || !s.dst) return "a null src, hist or dst";
    if (s.sw < 1 || s.sh < 1 || s.bx < 0 || s.by < 0 || s.bx > 32767 || s.by > 32767 || (int64_t)s.sw + 2 * (int64_t)s.bx > 32767 ||
        (int64_t)s.sh + 2 * (int64_t)s.by > 32767)
        return "sizes must be at least 1, borders at least 0 and padded sizes at most 32767";
    if ((s.cn != 1 && s.cn != 2) || s.reserved != 0) return "cn must be 1 or 2 and reserved 0";
    if (sample_bytes == 1 && (s.fill[0] > 255 || s.fill[1] > 255)) return "a fill sample above 255 for 8-bit samples";
    const int dh = s.sh + 2 * s.by;
    const size_t srow = (size_t)s.sw * s.cn * sample_bytes, drow = (size_t)(s.sw + 2 * s.bx) * s.cn * sample_bytes;
    if (s.src_stride > UINT32_MAX || s.hist_stride > UINT32_MAX || s.dst_stride > UINT32_MAX || s.src_stride < srow || s.hist_stride < drow ||
        s.dst_stride < drow)
        return "a stride does not hold a row (or exceeds 32 bits)";
    if (sample_bytes == 2 && (((uintptr_t)s.src | (uintptr_t)s.hist | (uintptr_t)s.dst | s.src_stride | s.hist_stride | s.dst_stride) & 1))
        return "16-bit pointers and strides must be even";
    const uintptr_t d0 = (uintptr_t)s.dst, d1 = yf_end(s.dst, s.dst_stride, dh, drow);
    if (yf_overlap((uintptr_t)s.src, yf_end(s.src, s.src_stride, s.sh, srow), d0, d1)) return "source and destination overlap";
    if (yf_overlap((uintptr_t)s.hist, yf_end(s.hist, s.hist_stride, dh, drow), d0, d1)) return "history and destination overlap";
    return std::string();
}

std::string yf_update_refusal(const vs_fade_update_job& s, int sample_bytes) {
    if (!s.hist || !s.res) return "a null hist or res";
    if (s.w < 1 || s.h < 1 || s.w > 32767 || s.h > 32767) return "sizes must be 1 .. 32767";
    if ((s.cn != 1 && s.cn != 2) || s.reserved != 0) return "cn must be 1 or 2 and reserved 0";
    const size_t row = (size_t)s.w * s.cn * sample_bytes;
    if (s.hist_stride > UINT32_MAX || s.res_stride > UINT32_MAX || s.hist_stride < row || s.res_stride < row)
        return "a stride does not hold a row (or exceeds 32 bits)";
    if (sample_bytes == 2 && (((uintptr_t)s.hist | (uintptr_t)s.res | s.hist_stride | s.res_stride) & 1)) return "16-bit pointers and strides must be even";
    if (yf_overlap((uintptr_t)s.hist, yf_end(s.hist, s.hist_stride, s.h, row), (uintptr_t)s.res, yf_end(s.res, s.res_stride, s.h, row)))
        return "history and result overlap";
    return std::string();
}

}  // namespace

int launch_yuvfade_blend(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, hipStream_t st) {
    if (!jobs || n < 1 || n > YF_MAX_JOBS || (sample_bytes != 1 && sample_bytes != 2)) {
        set_last_error("vs_op_fade_blend_jobs: invalid argument (1 .. 32 jobs of one sample size, 1 or 2 bytes)");
        return VS_ERR_INVALID_ARG;
    }
    if (!(alpha >= 0.0f && alpha <= 1.0f && beta >= 0.0f && beta <= 1.0f)) {
        set_last_error("vs_op_fade_blend_jobs: weights must be in [0,1]");
        return VS_ERR_INVALID_ARG;
    }
    YfArgs a{};
    uint64_t tiles = 0;
    const int tb = yf_tb(sample_bytes), tr = yf_tr(sample_bytes);
    for (int i = 0; i < n; i++) {
        const vs_fade_job& s = jobs[i];
        const std::string why = yf_blend_refusal(s, sample_bytes);
        if (!why.empty()) {
            set_last_error("vs_op_fade_blend_jobs: job " + std::to_string(i) + ": " + why);
            return VS_ERR_INVALID_ARG;
        }
        YfJob& j = a.j[i];
        j.src = (const uint8_t*)s.src; j.hist = (const uint8_t*)s.hist; j.dst = (uint8_t*)s.dst;
        j.sstride = (uint32_t)s.src_stride; j.hstride = (uint32_t)s.hist_stride; j.dstride = (uint32_t)s.dst_stride;
        j.swh = (uint32_t)s.sw | (uint32_t)s.sh << 16; j.bxy = (uint32_t)s.bx | (uint32_t)s.by << 16;
        j.t0f = (uint32_t)tiles | (uint32_t)(s.cn - 1) << 24;
        j.fill = (uint32_t)s.fill[0] | (uint32_t)s.fill[1] << 16;
        const int dw = s.sw + 2 * s.bx, dh = s.sh + 2 * s.by;
        tiles += (uint64_t)(((size_t)dw * s.cn * sample_bytes + tb - 1) / tb) * (uint64_t)((dh + tr - 1) / tr);
    }
    a.n = (uint32_t)n; a.tiles = (uint32_t)tiles;
    a.alpha = alpha; a.beta = beta;
    VS_TRY(ensure_device());
    if (sample_bytes == 1) hipLaunchKernelGGL(yuvfade_blend_kernel<1>, dim3((unsigned)tiles), dim3(64, YF_WAVES), 0, st, a);
    else hipLaunchKernelGGL(yuvfade_blend_kernel<2>, dim3((unsigned)tiles), dim3(64, YF_WAVES), 0, st, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

int launch_yuvfade_update(const vs_fade_update_job* jobs, int n, int sample_bytes, hipStream_t st) {
    if (!jobs || n < 1 || n > YF_MAX_JOBS || (sample_bytes != 1 && sample_bytes != 2)) {
        set_last_error("vs_op_fade_update_jobs: invalid argument (1 .. 32 jobs of one sample size, 1 or 2 bytes)");
        return VS_ERR_INVALID_ARG;
    }
    YfuArgs a{};
    uint64_t tiles = 0;
    const int tb = yf_tb(sample_bytes), tr = yf_tr(sample_bytes);
    for (int i = 0; i < n; i++) {
        const vs_fade_update_job& s = jobs[i];
        const std::string why = yf_update_refusal(s, sample_bytes);
        if (!why.empty()) {
            set_last_error("vs_op_fade_update_jobs: job " + std::to_string(i) + ": " + why);
            return VS_ERR_INVALID_ARG;
        }
        YfuJob& j = a.j[i];
        j.hist = (uint8_t*)s.hist; j.res = (const uint8_t*)s.res;
        j.hstride = (uint32_t)s.hist_stride; j.rstride = (uint32_t)s.res_stride;
        j.rowb = (uint32_t)s.w * (uint32_t)s.cn * (uint32_t)sample_bytes; j.rows = (uint32_t)s.h;
        j.t0 = (uint32_t)tiles;
        tiles += (uint64_t)((j.rowb + tb - 1) / tb) * (uint64_t)((s.h + tr - 1) / tr);
    }
    a.n = (uint32_t)n; a.tiles = (uint32_t)tiles;
    VS_TRY(ensure_device());
    if (sample_bytes == 1) hipLaunchKernelGGL(yuvfade_update_kernel<1>, dim3((unsigned)tiles), dim3(64, YF_WAVES), 0, st, a);
    else hipLaunchKernelGGL(yuvfade_update_kernel<2>, dim3((unsigned)tiles), dim3(64, YF_WAVES), 0, st, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace vsd

extern "C" int vs_op_fade_blend_jobs(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, void* stream) {
    return vsd::launch_yuvfade_blend(jobs, n, sample_bytes, alpha, beta, (hipStream_t)stream);
}

extern "C" int vs_op_fade_update_jobs(const vs_fade_update_job* jobs, int n, int sample_bytes, void* stream) {
    return vsd::launch_yuvfade_update(jobs, n, sample_bytes, (hipStream_t)stream);
}
