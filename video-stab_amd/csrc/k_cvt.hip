// Colour conversion between YUV surfaces and interleaved 8-bit RGB in HBM: vs_op_cvt_yuv_to_rgb[_cs], vs_op_cvt_rgb_to_yuv[_cs]
// (comp_op.cpp) and the two ends of vs_enh_apply_yuv_dev (k_enhance.hip).  The definition is in include/vs_stab.h (the fixed-point
// path of OpenCV's COLOR_YUV2BGR_NV12 / _I420 and COLOR_BGR2YUV_I420 with the integers of a colour space; tests/cvtref.py and
// tests/cvtref_cs.py state it in numpy).  The per-pixel arithmetic is in cvt_px.h, shared with the enhancer's YUV form; the
// colour space is data (CvtArgs::k), not a kernel instance.
//
// Both kernels stream: a lane covers CVT_PX consecutive pixels in the 1 << SY rows that share a chroma row, so every chroma sample
// is read (or computed and written) once; a wave covers 512 pixels of those rows, a block four chroma rows; blockIdx.z = surface,
// the surface pointers travel as kernel arguments.  A run whose address is aligned to its size and that lies inside the row moves
// as dwords - x2 and x4 for the samples, x3 / x4 per four pixels of BGR8 / BGRA8 -; any other run (the ragged right edge, a row
// at an odd pitch) goes sample by sample and touches nothing beyond the row's w samples.  Stores carry the non-temporal hint: nothing written here is read again by the
// kernel.  No LDS.
#include <hip/hip_runtime.h>

#include "cvt_px.h"
#include "launchers.h"
#include "vs_common.h"

namespace vsd {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int CVT_PX = 8;          // pixels of a row per lane (8-byte luma loads; with four the 8-bit directions ran on dword loads)
constexpr int CVT_BX = 64, CVT_BY = 4;

struct CvtArgs {
    const uint8_t* src[CVT_MAX_SURFACES];
    uint8_t* dst[CVT_MAX_SURFACES];
    size_t pitch, cpitch, u, v;    // the YUV side (NV12 / P010: u = the interleaved plane, cpitch = pitch)
    size_t rgb_stride;
    int w, h;
    int shift;                     // 16-bit samples: byte = min(sample >> shift, 255), sample = byte << shift
    int rgb_order;                 // 1: R first (RGB8, RGBA8)
    CvtCoef k;                     // the integers of the colour space; k.mean: chroma of a block from the sums over its pixels
};

// N samples of SB bytes at p, the first `valid` of them inside the row, as bytes
template <int SB, int N>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ p, int valid, int shift, int (&v)[N]) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 2 || BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one load");
    if (valid == N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[(BYTES + 3) / 4];
        if constexpr (BYTES == 2) q[0] = *reinterpret_cast<const uint16_t*>(p);
        else if constexpr (BYTES == 4) q[0] = *reinterpret_cast<const uint32_t*>(p);
        else if constexpr (BYTES == 8) { const u32x2 t = *reinterpret_cast<const u32x2*>(p); q[0] = t.x; q[1] = t.y; }
        else { const u32x4 t = *reinterpret_cast<const u32x4*>(p); q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w; }
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) v[i] = (int)((q[i / 4] >> (8 * (i % 4))) & 255u);
            else v[i] = cvt_sample_to_byte((int)((q[i / 2] >> (16 * (i % 2))) & 0xffffu), shift);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            v[i] = 0;
            if (i < valid) {
                if constexpr (SB == 1) v[i] = p[i];
                else v[i] = cvt_sample_to_byte((int)reinterpret_cast<const uint16_t*>(p)[i], shift);
            }
        }
    }
}

template <int SB, int N>
__device__ __forceinline__ void store_run(uint8_t* __restrict__ p, int valid, int shift, const int (&v)[N]) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 2 || BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one store");
    if (valid == N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[(BYTES + 3) / 4] = {};
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) q[i / 4] |= (uint32_t)v[i] << (8 * (i % 4));
            else q[i / 2] |= cvt_byte_to_sample((uint32_t)v[i], shift) << (16 * (i % 2));
        }
        if constexpr (BYTES == 2) __builtin_nontemporal_store((uint16_t)q[0], reinterpret_cast<uint16_t*>(p));
        else if constexpr (BYTES == 4) __builtin_nontemporal_store(q[0], reinterpret_cast<uint32_t*>(p));
        else if constexpr (BYTES == 8) __builtin_nontemporal_store(u32x2{q[0], q[1]}, reinterpret_cast<u32x2*>(p));
        else __builtin_nontemporal_store(u32x4{q[0], q[1], q[2], q[3]}, reinterpret_cast<u32x4*>(p));
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (i < valid) {
                if constexpr (SB == 1) p[i] = (uint8_t)v[i];
                else reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)cvt_byte_to_sample((uint32_t)v[i], shift);
            }
        }
    }
}

// c[i][0..2]: the three colour bytes of pixel i in memory order (alpha is not read).  A full aligned run moves in groups of four
// pixels: three dwords of BGR8, four of BGRA8.
template <int CN>
__device__ __forceinline__ void load_rgb(const uint8_t* __restrict__ p, int valid, int (&c)[CVT_PX][3]) {
    static_assert(CVT_PX % 4 == 0, "groups of four pixels");
    if (valid == CVT_PX && ((uintptr_t)p & (CN == 4 ? 15 : 3)) == 0) {
#pragma unroll
        for (int g = 0; g < CVT_PX / 4; g++) {
            if constexpr (CN == 4) {
                const u32x4 t = *reinterpret_cast<const u32x4*>(p + 16 * g);
                const uint32_t q[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int i = 0; i < 4; i++) { c[4 * g + i][0] = q[i] & 255u; c[4 * g + i][1] = (q[i] >> 8) & 255u; c[4 * g + i][2] = (q[i] >> 16) & 255u; }
            } else {
                const u32x3 t = *reinterpret_cast<const u32x3*>(p + 12 * g);
                const uint32_t q[3] = {t.x, t.y, t.z};
#pragma unroll
                for (int k = 0; k < 12; k++) c[4 * g + k / 3][k % 3] = (int)((q[k / 4] >> (8 * (k % 4))) & 255u);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < CVT_PX; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) c[i][k] = i < valid ? p[i * CN + k] : 0;
    }
}

template <int CN>
__device__ __forceinline__ void store_rgb(uint8_t* __restrict__ p, int valid, const int (&c)[CVT_PX][3]) {
    if (valid == CVT_PX && ((uintptr_t)p & (CN == 4 ? 15 : 3)) == 0) {
#pragma unroll
        for (int g = 0; g < CVT_PX / 4; g++) {
            if constexpr (CN == 4) {
                uint32_t q[4];
#pragma unroll
                for (int i = 0; i < 4; i++)
                    q[i] = (uint32_t)c[4 * g + i][0] | ((uint32_t)c[4 * g + i][1] << 8) | ((uint32_t)c[4 * g + i][2] << 16) | 0xff000000u;
                __builtin_nontemporal_store(u32x4{q[0], q[1], q[2], q[3]}, reinterpret_cast<u32x4*>(p + 16 * g));
            } else {
                uint32_t q[3] = {0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 12; k++) q[k / 4] |= (uint32_t)c[4 * g + k / 3][k % 3] << (8 * (k % 4));
                __builtin_nontemporal_store(u32x3{q[0], q[1], q[2]}, reinterpret_cast<u32x3*>(p + 12 * g));
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < CVT_PX; i++) {
            if (i < valid) {
#pragma unroll
                for (int k = 0; k < 3; k++) p[i * CN + k] = (uint8_t)c[i][k];
                if constexpr (CN == 4) p[i * CN + 3] = 255;
            }
        }
    }
}

// SB: bytes per sample; IL: one plane of interleaved (U, V) pairs (NV12, P010); a chroma plane has (w >> SX) x (h >> SY) samples
template <int SB, bool IL, int SX, int SY, int CN>
__global__ __launch_bounds__(CVT_BX * CVT_BY) void cvt_yuv_to_rgb_kernel(const CvtArgs a) {
    const int x0 = (int)(blockIdx.x * CVT_BX + threadIdx.x) * CVT_PX;
    const int cy = (int)(blockIdx.y * CVT_BY + threadIdx.y);
    if (x0 >= a.w || cy >= (a.h >> SY)) return;
    const uint8_t* __restrict__ s = a.src[blockIdx.z];
    uint8_t* __restrict__ d = a.dst[blockIdx.z];
    const int valid = min(CVT_PX, a.w - x0);
    constexpr int NC = CVT_PX >> SX;
    const int cvalid = valid >> SX;
    const size_t cx0 = (size_t)(x0 >> SX);
    int u[NC], v[NC];
    if constexpr (IL) {
        int uv[2 * NC];
        load_run<SB, 2 * NC>(s + a.u + (size_t)cy * a.cpitch + cx0 * (2 * SB), 2 * cvalid, a.shift, uv);
#pragma unroll
        for (int k = 0; k < NC; k++) { u[k] = uv[2 * k]; v[k] = uv[2 * k + 1]; }
    } else {
        load_run<SB, NC>(s + a.u + (size_t)cy * a.cpitch + cx0 * SB, cvalid, a.shift, u);
        load_run<SB, NC>(s + a.v + (size_t)cy * a.cpitch + cx0 * SB, cvalid, a.shift, v);
    }
    int ru[NC], gu[NC], bu[NC];                 // the chroma terms, with the rounding half
#pragma unroll
    for (int k = 0; k < NC; k++) cvt_chroma_terms(a.k, u[k], v[k], ru[k], gu[k], bu[k]);
#pragma unroll
    for (int r = 0; r < (1 << SY); r++) {
        const size_t y = ((size_t)cy << SY) + r;
        int yy[CVT_PX], c[CVT_PX][3];
        load_run<SB, CVT_PX>(s + y * a.pitch + (size_t)x0 * SB, valid, a.shift, yy);
#pragma unroll
        for (int i = 0; i < CVT_PX; i++) {
            int R, G, B;
            cvt_yuv_px(a.k, yy[i], ru[i >> SX], gu[i >> SX], bu[i >> SX], R, G, B);
            c[i][0] = a.rgb_order ? R : B;
            c[i][1] = G;
            c[i][2] = a.rgb_order ? B : R;
        }
        store_rgb<CN>(d + y * a.rgb_stride + (size_t)x0 * CN, valid, c);
    }
}

template <int SB, bool IL, int SX, int SY, int CN>
__global__ __launch_bounds__(CVT_BX * CVT_BY) void cvt_rgb_to_yuv_kernel(const CvtArgs a) {
    const int x0 = (int)(blockIdx.x * CVT_BX + threadIdx.x) * CVT_PX;
    const int cy = (int)(blockIdx.y * CVT_BY + threadIdx.y);
    if (x0 >= a.w || cy >= (a.h >> SY)) return;
    const uint8_t* __restrict__ s = a.src[blockIdx.z];
    uint8_t* __restrict__ d = a.dst[blockIdx.z];
    const int valid = min(CVT_PX, a.w - x0);
    constexpr int NC = CVT_PX >> SX;
    const int cvalid = valid >> SX;
    const size_t cx0 = (size_t)(x0 >> SX);
    // chroma: of the top-left pixel of each block (stored with the block's first row), or - mean - of the sums over the block's
    // pixels (stored behind its last row).  4:4:4 has one pixel per block: the two rules are one.
    const bool mean = (SX + SY) != 0 && a.k.mean;
    int sum[NC][3];
#pragma unroll
    for (int r = 0; r < (1 << SY); r++) {
        const size_t y = ((size_t)cy << SY) + r;
        int c[CVT_PX][3], yy[CVT_PX];
        load_rgb<CN>(s + y * a.rgb_stride + (size_t)x0 * CN, valid, c);
#pragma unroll
        for (int i = 0; i < CVT_PX; i++) {
            const int R = a.rgb_order ? c[i][0] : c[i][2], G = c[i][1], B = a.rgb_order ? c[i][2] : c[i][0];
            yy[i] = cvt_luma(a.k, R, G, B);
        }
        store_run<SB, CVT_PX>(d + y * a.pitch + (size_t)x0 * SB, valid, a.shift, yy);
        if (r == 0 || mean) {
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int i = k << SX;
                int t[3] = {c[i][0], c[i][1], c[i][2]};
                if (mean) {
                    if constexpr (SX) { t[0] += c[i + 1][0]; t[1] += c[i + 1][1]; t[2] += c[i + 1][2]; }
                    if (r) { t[0] += sum[k][0]; t[1] += sum[k][1]; t[2] += sum[k][2]; }
                }
                sum[k][0] = t[0]; sum[k][1] = t[1]; sum[k][2] = t[2];
            }
        }
        if (mean ? r == (1 << SY) - 1 : r == 0) {
            const int sh = mean ? SX + SY : 0;
            int u[NC], v[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int R = a.rgb_order ? sum[k][0] : sum[k][2], G = sum[k][1], B = a.rgb_order ? sum[k][2] : sum[k][0];
                cvt_chroma(a.k, R, G, B, sh, u[k], v[k]);
            }
            if constexpr (IL) {
                int uv[2 * NC];
#pragma unroll
                for (int k = 0; k < NC; k++) { uv[2 * k] = u[k]; uv[2 * k + 1] = v[k]; }
                store_run<SB, 2 * NC>(d + a.u + (size_t)cy * a.cpitch + cx0 * (2 * SB), 2 * cvalid, a.shift, uv);
            } else {
                store_run<SB, NC>(d + a.u + (size_t)cy * a.cpitch + cx0 * SB, cvalid, a.shift, u);
                store_run<SB, NC>(d + a.v + (size_t)cy * a.cpitch + cx0 * SB, cvalid, a.shift, v);
            }
        }
    }
}

template <bool TO_RGB, int SB, bool IL, int SX, int SY, int CN>
void launch_one(dim3 grid, hipStream_t st, const CvtArgs& a) {
    if constexpr (TO_RGB) hipLaunchKernelGGL((cvt_yuv_to_rgb_kernel<SB, IL, SX, SY, CN>), grid, dim3(CVT_BX, CVT_BY), 0, st, a);
    else hipLaunchKernelGGL((cvt_rgb_to_yuv_kernel<SB, IL, SX, SY, CN>), grid, dim3(CVT_BX, CVT_BY), 0, st, a);
}

template <bool TO_RGB, int SB, int CN>
void launch_layout(const PixFmt& yf, dim3 grid, hipStream_t st, const CvtArgs& a) {
    if (yf.luma_uv()) launch_one<TO_RGB, SB, true, 1, 1, CN>(grid, st, a);
    else if (yf.sy) launch_one<TO_RGB, SB, false, 1, 1, CN>(grid, st, a);
    else if (yf.sx) launch_one<TO_RGB, SB, false, 1, 0, CN>(grid, st, a);
    else launch_one<TO_RGB, SB, false, 0, 0, CN>(grid, st, a);
}

template <bool TO_RGB>
int launch_cvt(const PixFmt& yf, const I420Layout& l, const PixFmt& rf, size_t rgb_stride, const void* const* src, void* const* dst, int n, int w,
               int h, const CvtCoef& k, hipStream_t st) {
    CvtArgs a{};
    a.k = k;
    for (int k = 0; k < n; k++) { a.src[k] = (const uint8_t*)src[k]; a.dst[k] = (uint8_t*)dst[k]; }
    a.pitch = l.pitch; a.cpitch = l.cpitch; a.u = l.u; a.v = l.v;
    a.rgb_stride = rgb_stride;
    a.w = w; a.h = h;
    a.shift = yf.sample_bytes == 2 ? (yf.luma_uv() ? 8 : yf.bits - 8) : 0;
    a.rgb_order = rf.fmt == VS_FMT_RGB8 || rf.fmt == VS_FMT_RGBA8;
    const dim3 grid((unsigned)((w + CVT_BX * CVT_PX - 1) / (CVT_BX * CVT_PX)), (unsigned)(((h >> yf.sy) + CVT_BY - 1) / CVT_BY), (unsigned)n);
    if (yf.sample_bytes == 1) {
        if (rf.cn == 3) launch_layout<TO_RGB, 1, 3>(yf, grid, st, a);
        else launch_layout<TO_RGB, 1, 4>(yf, grid, st, a);
    } else {
        if (rf.cn == 3) launch_layout<TO_RGB, 2, 3>(yf, grid, st, a);
        else launch_layout<TO_RGB, 2, 4>(yf, grid, st, a);
    }
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace

int launch_cvt_yuv_to_rgb(const PixFmt& yf, const void* const* surfaces, const I420Layout& l, const PixFmt& rf, void* const* rgb, size_t rgb_stride,
                          int n, int w, int h, const CvtCoef& k, hipStream_t st) {
    return launch_cvt<true>(yf, l, rf, rgb_stride, surfaces, rgb, n, w, h, k, st);
}

int launch_cvt_rgb_to_yuv(const PixFmt& rf, const void* const* rgb, size_t rgb_stride, const PixFmt& yf, void* const* surfaces, const I420Layout& l,
                          int n, int w, int h, const CvtCoef& k, hipStream_t st) {
    return launch_cvt<false>(yf, l, rf, rgb_stride, rgb, surfaces, n, w, h, k, st);
}

}  // namespace vsd
