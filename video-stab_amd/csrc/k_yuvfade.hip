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
// Both launches follow the scheme of plane_jobs.h.  A lane owns PJ_LB = 16 bytes at one place of YF_R rows; a wave is yf_cl lanes side
// by side times 64 / yf_cl rows.
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

#include "plane_jobs.h"

namespace vsd {
namespace {

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
constexpr int yf_tb(int sb) { return pj_tb(yf_cl(sb)); }
constexpr int yf_tr(int sb) { return pj_tr(YF_WAVES, YF_R, yf_cl(sb)); }

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

template <int SB, int CN>
__device__ __forceinline__ void yf_blend_tile(const YfJob& J, int tx, int ty, float alpha, float beta) {
    constexpr int NEL = PJ_LB / SB;                   // samples of a lane per row
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

    const PjLane L = pj_lane<CL, PB>(tx, lane, dw);          // the lane in the padded row
    if (L.nvb <= 0) return;
    const int e0 = L.e0, nvb = L.nvb, px0 = L.px0(PB);
    const bool interior = px0 >= bx && px0 + NPX <= bx + sw;      // (then full)
    const bool outside = px0 + NPX <= bx || px0 >= bx + sw;       // every pixel of the lane is border
    const bool full = L.full();
    const uint32_t fq = pj_fill_dword<SB, CN>(fills, J.fill);

#pragma unroll 1
    for (int r = 0; r < YF_R; r++) {
        const int dy = ty * TR + (wave * YF_R + r) * RW + sub;
        if (dy >= dh) break;
        const int sy = dy - by;
        const uint8_t* __restrict__ hp = J.hist + (size_t)dy * J.hstride + (size_t)e0;
        uint8_t* __restrict__ dp = J.dst + (size_t)dy * J.dstride + (size_t)e0;
        uint32_t hq[4], fr[4], o[4];
        if (full && ((uintptr_t)hp & 15) == 0) pj_load16<pj_u4>(hp, hq);
        else pj_gather<SB>(hp, nvb, hq);
        if ((unsigned)sy >= (unsigned)sh || outside) {
            fr[0] = fr[1] = fr[2] = fr[3] = fq;
        } else {
            const uint8_t* __restrict__ rp = J.src + (size_t)sy * J.sstride;
            if (interior) {
                // exactly the lane's 16 source bytes, wherever they start
                pj_load16<pj_q1>(rp + (size_t)(px0 - bx) * PB, fr);
            } else {
                fr[0] = fr[1] = fr[2] = fr[3] = 0;
#pragma unroll
                for (int k = 0; k < NPX; k++) {
                    const int sx = px0 + k - bx;
                    const bool in = (unsigned)sx < (unsigned)sw && k * PB < nvb;
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const int i = k * CN + c;
                        const uint32_t v = in ? pj_ld<SB>(rp + ((size_t)sx * CN + c) * SB) : fills[c];
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
        if (full && ((uintptr_t)dp & 15) == 0) __builtin_nontemporal_store(pj_pack16(o), reinterpret_cast<pj_u4*>(dp));
        else pj_scatter<SB>(dp, nvb, o);
    }
}

template <int SB>
__global__ __launch_bounds__(64 * YF_WAVES) void yuvfade_blend_kernel(const YfArgs a) {
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const YfJob J = a.j[pj_find(a, seq, [](const YfJob& j) { return j.t0f & YF_T0_MASK; })];
    const uint32_t cn = ((J.t0f >> 24) & 1u) + 1u;
    const uint32_t dw = (J.swh & 0xffffu) + 2u * (J.bxy & 0xffffu);
    const PjTile t = pj_split(seq - (J.t0f & YF_T0_MASK), dw * cn * SB, yf_tb(SB));
    if (cn == 1) yf_blend_tile<SB, 1>(J, t.tx, t.ty, a.alpha, a.beta);
    else yf_blend_tile<SB, 2>(J, t.tx, t.ty, a.alpha, a.beta);
}

template <int SB>
__global__ __launch_bounds__(64 * YF_WAVES) void yuvfade_update_kernel(const YfuArgs a) {
    constexpr int NEL = PJ_LB / SB, SPD = 4 / SB;
    constexpr uint32_t SMASK = SB == 1 ? 0xffu : 0xffffu;
    constexpr int CL = yf_cl(SB), RW = 64 / CL, TR = yf_tr(SB);
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const YfuJob J = a.j[pj_find(a, seq, [](const YfuJob& j) { return j.t0; })];
    const PjTile t = pj_split(seq - J.t0, J.rowb, yf_tb(SB));
    const int ty = t.ty;
    const int lane = threadIdx.x & (CL - 1), sub = threadIdx.x / CL, wave = threadIdx.y;
    const PjLane L = pj_lane<CL, 1>(t.tx, lane, (int)J.rowb);
    if (L.nvb <= 0) return;
    const int e0 = L.e0, nvb = L.nvb;
    const bool full = L.full();
    const float rate = 0.1f, keep = 1.0f - rate;
#pragma unroll 1
    for (int r = 0; r < YF_R; r++) {
        const int y = ty * TR + (wave * YF_R + r) * RW + sub;
        if (y >= (int)J.rows) break;
        uint8_t* hp = J.hist + (size_t)y * J.hstride + (size_t)e0;
        const uint8_t* rp = J.res + (size_t)y * J.rstride + (size_t)e0;
        const bool vec = full && ((uintptr_t)hp & 15) == 0;
        uint32_t hq[4], rq[4], o[4];
        if (vec) pj_load16<pj_u4>(hp, hq);
        else pj_gather<SB>(hp, nvb, hq);
        if (full) pj_load16<pj_q1>(rp, rq);
        else pj_gather<SB>(rp, nvb, rq);
        o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
        for (int i = 0; i < NEL; i++) {
            const float h = (float)((hq[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            const float s = (float)((rq[i / SPD] >> (8 * SB * (i % SPD))) & SMASK);
            const float v = __fadd_rn(__fmul_rn(keep, h), __fmul_rn(rate, s));
            o[i / SPD] |= ((uint32_t)(int)v & SMASK) << (8 * SB * (i % SPD));
        }
        if (vec) *reinterpret_cast<pj_u4*>(hp) = pj_pack16(o);
        else pj_scatter<SB>(hp, nvb, o);
    }
}

// What the operators refuse about a job, decided before any device call; nullptr = accepted.
const char* yf_blend_refusal(const vs_fade_job& s, int sample_bytes, int*) {
    if (!s.src || !s.hist || !s.dst) return "a null src, hist or dst";
    if (const char* why = pj_bad_padded_sizes(s.sw, s.sh, s.bx, s.by)) return why;
    if (const char* why = pj_bad_cn(s.cn, s.reserved)) return why;
    if (const char* why = pj_bad_fill(s.fill, sample_bytes)) return why;
    const int dh = s.sh + 2 * s.by;
    const size_t srow = (size_t)s.sw * s.cn * sample_bytes, drow = (size_t)(s.sw + 2 * s.bx) * s.cn * sample_bytes;
    if (const char* why = pj_bad_strides({{s.src_stride, srow}, {s.hist_stride, drow}, {s.dst_stride, drow}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.src | (uintptr_t)s.hist | (uintptr_t)s.dst | s.src_stride | s.hist_stride | s.dst_stride)) return why;
    const uintptr_t d0 = (uintptr_t)s.dst, d1 = pj_end(s.dst, s.dst_stride, dh, drow);
    if (pj_overlap((uintptr_t)s.src, pj_end(s.src, s.src_stride, s.sh, srow), d0, d1)) return "source and destination overlap";
    if (pj_overlap((uintptr_t)s.hist, pj_end(s.hist, s.hist_stride, dh, drow), d0, d1)) return "history and destination overlap";
    return nullptr;
}

const char* yf_update_refusal(const vs_fade_update_job& s, int sample_bytes, int*) {
    if (!s.hist || !s.res) return "a null hist or res";
    if (const char* why = pj_bad_sizes({s.w, s.h})) return why;
    if (const char* why = pj_bad_cn(s.cn, s.reserved)) return why;
    const size_t row = (size_t)s.w * s.cn * sample_bytes;
    if (const char* why = pj_bad_strides({{s.hist_stride, row}, {s.res_stride, row}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.hist | (uintptr_t)s.res | s.hist_stride | s.res_stride)) return why;
    if (pj_overlap((uintptr_t)s.hist, pj_end(s.hist, s.hist_stride, s.h, row), (uintptr_t)s.res, pj_end(s.res, s.res_stride, s.h, row)))
        return "history and result overlap";
    return nullptr;
}

}  // namespace

int launch_yuvfade_blend(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, hipStream_t st) {
    // (behind the launch's own check, in front of the jobs')
    if (pj_launch_ok(jobs, n, YF_MAX_JOBS, sample_bytes) && !(alpha >= 0.0f && alpha <= 1.0f && beta >= 0.0f && beta <= 1.0f)) {
        set_last_error("vs_op_fade_blend_jobs: weights must be in [0,1]");
        return VS_ERR_INVALID_ARG;
    }
    YfArgs a{};
    a.alpha = alpha; a.beta = beta;
    return pj_launch(
        "vs_op_fade_blend_jobs", jobs, n, YF_MAX_JOBS, sample_bytes, a, yf_blend_refusal,
        [&](const vs_fade_job& s, YfJob& j, uint32_t tile0) {
            j.src = (const uint8_t*)s.src; j.hist = (const uint8_t*)s.hist; j.dst = (uint8_t*)s.dst;
            j.sstride = (uint32_t)s.src_stride; j.hstride = (uint32_t)s.hist_stride; j.dstride = (uint32_t)s.dst_stride;
            j.swh = (uint32_t)s.sw | (uint32_t)s.sh << 16; j.bxy = (uint32_t)s.bx | (uint32_t)s.by << 16;
            j.t0f = tile0 | (uint32_t)(s.cn - 1) << 24;
            j.fill = (uint32_t)s.fill[0] | (uint32_t)s.fill[1] << 16;
            return pj_tiles((size_t)(s.sw + 2 * s.bx) * s.cn * sample_bytes, s.sh + 2 * s.by, yf_tb(sample_bytes), yf_tr(sample_bytes));
        },
        [&](auto sb, const YfArgs& args, unsigned tiles) { hipLaunchKernelGGL(yuvfade_blend_kernel<decltype(sb)::value>, dim3(tiles), dim3(64, YF_WAVES), 0, st, args); });
}

int launch_yuvfade_update(const vs_fade_update_job* jobs, int n, int sample_bytes, hipStream_t st) {
    YfuArgs a{};
    return pj_launch(
        "vs_op_fade_update_jobs", jobs, n, YF_MAX_JOBS, sample_bytes, a, yf_update_refusal,
        [&](const vs_fade_update_job& s, YfuJob& j, uint32_t tile0) {
            j.hist = (uint8_t*)s.hist; j.res = (const uint8_t*)s.res;
            j.hstride = (uint32_t)s.hist_stride; j.rstride = (uint32_t)s.res_stride;
            j.rowb = (uint32_t)s.w * (uint32_t)s.cn * (uint32_t)sample_bytes; j.rows = (uint32_t)s.h;
            j.t0 = tile0;
            return pj_tiles(j.rowb, s.h, yf_tb(sample_bytes), yf_tr(sample_bytes));
        },
        [&](auto sb, const YfuArgs& args, unsigned tiles) { hipLaunchKernelGGL(yuvfade_update_kernel<decltype(sb)::value>, dim3(tiles), dim3(64, YF_WAVES), 0, st, args); });
}

}  // namespace vsd

extern "C" int vs_op_fade_blend_jobs(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, void* stream) {
    return vsd::launch_yuvfade_blend(jobs, n, sample_bytes, alpha, beta, (hipStream_t)stream);
}

extern "C" int vs_op_fade_update_jobs(const vs_fade_update_job* jobs, int n, int sample_bytes, void* stream) {
    return vsd::launch_yuvfade_update(jobs, n, sample_bytes, (hipStream_t)stream);
}
