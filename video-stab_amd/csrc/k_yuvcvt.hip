// Conversion between YUV surface formats in HBM: vs_op_cvt_yuv_to_yuv (comp_op.cpp).  The definition is in include/vs_stab.h
// (exact integer arithmetic in two steps - the depth of every sample, then the siting of the chroma samples; tests/yuvref.py
// states it in numpy).  No colour matrix runs here and no RGB frame is written: a sample goes from its source word to its
// destination word.
//
// The kernel streams like cvt_yuv_to_rgb_kernel (k_cvt.hip): a lane covers YC_PX consecutive luma pixels in the 1 << max(sy_in,
// sy_out) rows that share a chroma row on the coarser side, with the chroma samples of both sides that belong to them, so every
// source sample is read once and every destination sample written once; a wave covers 512 pixels of those rows, a block four such
// row groups; blockIdx.z = surface, the surface pointers travel as kernel arguments.  A run whose address is aligned to its size
// and that lies inside the row moves as one dword / x2 / x4 access; any other run (the ragged right edge, a row at an odd pitch, a
// surface at an unaligned pointer) goes sample by sample and touches nothing beyond the row's samples.  Stores carry the
// non-temporal hint: nothing written here is read again by the kernel.  No LDS.
//
// Sample size and plane layout of each side are template parameters (2 x 4 per side: 64 instances); the depth step - clamp,
// rounding half, shifts - and the chroma rule are data (YuvDepth, YuvCvtArgs::mean).
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "vs_common.h"

namespace vsd {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int YC_PX = 8;           // luma pixels of a row per lane
constexpr int YC_BX = 64, YC_BY = 4;

// how the planes of a side lie: its interleave and chroma shifts
enum YuvLay { LAY_UV420 = 0, LAY_420 = 1, LAY_422 = 2, LAY_444 = 3 };
constexpr bool lay_il(int l) { return l == LAY_UV420; }
constexpr int lay_sx(int l) { return l != LAY_444; }
constexpr int lay_sy(int l) { return l == LAY_UV420 || l == LAY_420; }

struct YuvCvtArgs {
    const uint8_t* src[CVT_MAX_SURFACES];
    uint8_t* dst[CVT_MAX_SURFACES];
    I420Layout in, out;            // NV12 / P010: u = the interleaved plane, cpitch = pitch
    int w, h;
    YuvDepth d;
    int mean;                      // chroma of a block going down: 1 the rounded mean, 0 its top-left sample
};

// step 1: the value of a sample at the destination's depth
__device__ __forceinline__ uint32_t yc_depth(const YuvDepth& d, uint32_t s) {
    return min(((min(s, d.in_max) + d.add) >> d.down) << d.up, d.out_max);
}

// N samples of SB bytes at p, the first `valid` of them inside the row, as they are stored
template <int SB, int N>
__device__ __forceinline__ void load_samples(const uint8_t* __restrict__ p, int valid, uint32_t (&v)[N]) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one load");
    if (valid == N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[BYTES / 4];
        if constexpr (BYTES == 4) q[0] = *reinterpret_cast<const uint32_t*>(p);
        else if constexpr (BYTES == 8) { const u32x2 t = *reinterpret_cast<const u32x2*>(p); q[0] = t.x; q[1] = t.y; }
        else { const u32x4 t = *reinterpret_cast<const u32x4*>(p); q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w; }
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) v[i] = (q[i / 4] >> (8 * (i % 4))) & 255u;
            else v[i] = (q[i / 2] >> (16 * (i % 2))) & 0xffffu;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            v[i] = 0;
            if (i < valid) {
                if constexpr (SB == 1) v[i] = p[i];
                else v[i] = reinterpret_cast<const uint16_t*>(p)[i];
            }
        }
    }
}

template <int SB, int N>
__device__ __forceinline__ void store_samples(uint8_t* __restrict__ p, int valid, const uint32_t (&v)[N]) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one store");
    if (valid == N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[BYTES / 4] = {};
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) q[i / 4] |= v[i] << (8 * (i % 4));
            else q[i / 2] |= v[i] << (16 * (i % 2));
        }
        if constexpr (BYTES == 4) __builtin_nontemporal_store(q[0], reinterpret_cast<uint32_t*>(p));
        else if constexpr (BYTES == 8) __builtin_nontemporal_store(u32x2{q[0], q[1]}, reinterpret_cast<u32x2*>(p));
        else __builtin_nontemporal_store(u32x4{q[0], q[1], q[2], q[3]}, reinterpret_cast<u32x4*>(p));
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (i < valid) {
                if constexpr (SB == 1) p[i] = (uint8_t)v[i];
                else reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)v[i];
            }
        }
    }
}

// SBI / SBO: bytes per sample; LI / LO: YuvLay of the source and the destination
template <int SBI, int LI, int SBO, int LO>
__global__ __launch_bounds__(YC_BX * YC_BY) void yuv_cvt_kernel(const YuvCvtArgs a) {
    constexpr int SXI = lay_sx(LI), SYI = lay_sy(LI), SXO = lay_sx(LO), SYO = lay_sy(LO);
    constexpr int SYM = SYI > SYO ? SYI : SYO;                     // the rows of a lane share a chroma row on the coarser side
    constexpr int RI = 1 << (SYM - SYI), RO = 1 << (SYM - SYO);    // chroma rows of a lane on either side
    constexpr int NCI = YC_PX >> SXI, NCO = YC_PX >> SXO;          // chroma samples of a lane per row
    // the format set moves both axes the same way: down (D) or up (U) or neither, never one of each
    constexpr int DSX = SXO > SXI ? SXO - SXI : 0, DSY = SYO > SYI ? SYO - SYI : 0, USX = SXI > SXO ? SXI - SXO : 0, USY = SYI > SYO ? SYI - SYO : 0;
    constexpr int S = DSX + DSY;
    static_assert(S == 0 || USX + USY == 0, "no pair goes down in one axis and up in the other");

    const int x0 = (int)(blockIdx.x * YC_BX + threadIdx.x) * YC_PX;
    const int gy = (int)(blockIdx.y * YC_BY + threadIdx.y);
    if (x0 >= a.w || gy >= (a.h >> SYM)) return;
    const uint8_t* __restrict__ s = a.src[blockIdx.z];
    uint8_t* __restrict__ d = a.dst[blockIdx.z];
    const int valid = min(YC_PX, a.w - x0);        // a multiple of 1 << max(SXI, SXO), as w is

#pragma unroll
    for (int r = 0; r < (1 << SYM); r++) {
        const size_t y = ((size_t)gy << SYM) + r;
        uint32_t yy[YC_PX];
        load_samples<SBI, YC_PX>(s + y * a.in.pitch + (size_t)x0 * SBI, valid, yy);
#pragma unroll
        for (int i = 0; i < YC_PX; i++) yy[i] = yc_depth(a.d, yy[i]);
        store_samples<SBO, YC_PX>(d + y * a.out.pitch + (size_t)x0 * SBO, valid, yy);
    }

    uint32_t u[RI][NCI], v[RI][NCI];
    const int cvi = valid >> SXI;
    const size_t cxi = (size_t)(x0 >> SXI);
#pragma unroll
    for (int r = 0; r < RI; r++) {
        const size_t cy = (size_t)gy * RI + r;
        if constexpr (lay_il(LI)) {
            uint32_t uv[2 * NCI];
            load_samples<SBI, 2 * NCI>(s + a.in.u + cy * a.in.cpitch + cxi * (2 * SBI), 2 * cvi, uv);
#pragma unroll
            for (int k = 0; k < NCI; k++) { u[r][k] = uv[2 * k]; v[r][k] = uv[2 * k + 1]; }
        } else {
            load_samples<SBI, NCI>(s + a.in.u + cy * a.in.cpitch + cxi * SBI, cvi, u[r]);
            load_samples<SBI, NCI>(s + a.in.v + cy * a.in.cpitch + cxi * SBI, cvi, v[r]);
        }
#pragma unroll
        for (int k = 0; k < NCI; k++) { u[r][k] = yc_depth(a.d, u[r][k]); v[r][k] = yc_depth(a.d, v[r][k]); }
    }

    const int cvo = valid >> SXO;
    const size_t cxo = (size_t)(x0 >> SXO);
#pragma unroll
    for (int r = 0; r < RO; r++) {
        const size_t cy = (size_t)gy * RO + r;
        uint32_t ou[NCO], ov[NCO];
#pragma unroll
        for (int k = 0; k < NCO; k++) {
            if constexpr (S > 0) {
                // down: the block of (1 << DSX) x (1 << DSY) source samples at (k << DSX, r << DSY)
                const int r0 = r << DSY, c0 = k << DSX;
                uint32_t su = u[r0][c0], sv = v[r0][c0];
                if (a.mean) {
                    su = sv = 1u << (S - 1);
#pragma unroll
                    for (int j = 0; j < (1 << DSY); j++)
#pragma unroll
                        for (int i = 0; i < (1 << DSX); i++) { su += u[r0 + j][c0 + i]; sv += v[r0 + j][c0 + i]; }
                    su >>= S;
                    sv >>= S;
                }
                ou[k] = su;
                ov[k] = sv;
            } else {
                ou[k] = u[r >> USY][k >> USX];       // up: nearest; same shifts: the sample itself
                ov[k] = v[r >> USY][k >> USX];
            }
        }
        if constexpr (lay_il(LO)) {
            uint32_t uv[2 * NCO];
#pragma unroll
            for (int k = 0; k < NCO; k++) { uv[2 * k] = ou[k]; uv[2 * k + 1] = ov[k]; }
            store_samples<SBO, 2 * NCO>(d + a.out.u + cy * a.out.cpitch + cxo * (2 * SBO), 2 * cvo, uv);
        } else {
            store_samples<SBO, NCO>(d + a.out.u + cy * a.out.cpitch + cxo * SBO, cvo, ou);
            store_samples<SBO, NCO>(d + a.out.v + cy * a.out.cpitch + cxo * SBO, cvo, ov);
        }
    }
}

int lay_of(const PixFmt& f) { return f.luma_uv() ? LAY_UV420 : f.sy ? LAY_420 : f.sx ? LAY_422 : LAY_444; }

template <int SBI, int LI, int SBO, int LO>
void launch_one(dim3 grid, hipStream_t st, const YuvCvtArgs& a) {
    hipLaunchKernelGGL((yuv_cvt_kernel<SBI, LI, SBO, LO>), grid, dim3(YC_BX, YC_BY), 0, st, a);
}

template <int SBI, int LI, int SBO>
void launch_dst_lay(int lo, dim3 grid, hipStream_t st, const YuvCvtArgs& a) {
    if (lo == LAY_UV420) launch_one<SBI, LI, SBO, LAY_UV420>(grid, st, a);
    else if (lo == LAY_420) launch_one<SBI, LI, SBO, LAY_420>(grid, st, a);
    else if (lo == LAY_422) launch_one<SBI, LI, SBO, LAY_422>(grid, st, a);
    else launch_one<SBI, LI, SBO, LAY_444>(grid, st, a);
}

template <int SBI, int LI>
void launch_dst(int sbo, int lo, dim3 grid, hipStream_t st, const YuvCvtArgs& a) {
    if (sbo == 1) launch_dst_lay<SBI, LI, 1>(lo, grid, st, a);
    else launch_dst_lay<SBI, LI, 2>(lo, grid, st, a);
}

template <int SBI>
void launch_src_lay(int li, int sbo, int lo, dim3 grid, hipStream_t st, const YuvCvtArgs& a) {
    if (li == LAY_UV420) launch_dst<SBI, LAY_UV420>(sbo, lo, grid, st, a);
    else if (li == LAY_420) launch_dst<SBI, LAY_420>(sbo, lo, grid, st, a);
    else if (li == LAY_422) launch_dst<SBI, LAY_422>(sbo, lo, grid, st, a);
    else launch_dst<SBI, LAY_444>(sbo, lo, grid, st, a);
}

}  // namespace

int launch_cvt_yuv_to_yuv(const PixFmt& sf, const void* const* src, const I420Layout& in, const PixFmt& df, void* const* dst, const I420Layout& out,
                          int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st) {
    YuvCvtArgs a{};
    for (int k = 0; k < n; k++) { a.src[k] = (const uint8_t*)src[k]; a.dst[k] = (uint8_t*)dst[k]; }
    a.in = in; a.out = out;
    a.w = w; a.h = h;
    a.d = depth;
    a.mean = mean;
    const int sym = std::max(sf.sy, df.sy);
    const dim3 grid((unsigned)((w + YC_BX * YC_PX - 1) / (YC_BX * YC_PX)), (unsigned)(((h >> sym) + YC_BY - 1) / YC_BY), (unsigned)n);
    if (sf.sample_bytes == 1) launch_src_lay<1>(lay_of(sf), df.sample_bytes, lay_of(df), grid, st, a);
    else launch_src_lay<2>(lay_of(sf), df.sample_bytes, lay_of(df), grid, st, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace vsd
