// Packed 4:2:2 capture formats in HBM to and from the YUV surface formats: vs_op_cvt_packed_to_yuv, vs_op_cvt_yuv_to_packed
// (comp_op.cpp).  The definition is in include/vs_stab.h: the two steps of vs_op_cvt_yuv_to_yuv - depth, then chroma siting - with
// the packed side a 4:2:2 format, (sx, sy) = (1, 0); tests/packedref.py states it in numpy.
//
// The kernel streams like yuv_cvt_kernel (k_yuvcvt.hip): a lane covers a run of luma pixels - YP_PX of an 8-bit order or of Y210,
// YP_PX_V210 (four groups of six) of v210 - in the 1 << sy rows that share a chroma row of the surface side, so every source byte
// is read once and every destination byte written once; a row of YP_BX / YP_BX_V210 lanes covers 512 / 768 pixels, a block of
// YP_THREADS lanes 4 / 8 such row groups; blockIdx.z = surface, the surface pointers travel as kernel arguments.  A run whose
// address is aligned to its size and that lies inside the row moves as one dword / x2 / x4 access; any other run (the ragged right
// edge, a row at an odd pitch, a surface at an unaligned pointer) goes sample by sample - on the packed side by the unit the format
// guarantees: byte, 16-bit word, dword - and touches nothing beyond the row's bytes.  The stores of the 8-pixel kernels carry the
// non-temporal hint, those of the v210 kernels do not (store_run says why).  No LDS.
//
// The three 8-bit orders are one body: a dword holds a macropixel, and v_perm_b32 with the selector of the order (PackedCvtArgs::sel,
// the same for both directions: each order is its own inverse) makes it Y0 U Y1 V or undoes that.  Y210 is that layout with 16-bit
// words, v210 a body of its own.  Template parameters: the packed kind, the direction, sample size and plane layout of the surface
// side (3 x 2 x 2 x 4: 48 instances); the depth step and the chroma rule are data (YuvDepth, PackedCvtArgs::mean).
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "vs_common.h"

namespace vsd {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int YP_PX = 8;             // luma pixels of a row per lane: the 8-bit orders (16 packed bytes) and Y210 (32)
constexpr int YP_PX_V210 = 24;       // v210: four groups of six pixels, 64 packed bytes
constexpr int YP_BX = 64;            // lanes along a row: the 8-bit orders and Y210
constexpr int YP_BX_V210 = 32;       // v210
constexpr int YP_THREADS = 256;      // a block is YP_THREADS / lanes-along-a-row row groups high
constexpr int pk_px(int pk) { return pk == PACKED_V210 ? YP_PX_V210 : YP_PX; }
constexpr int pk_bx(int pk) { return pk == PACKED_V210 ? YP_BX_V210 : YP_BX; }
constexpr int pk_bytes(int pk) { return pk == PACKED_8 ? 2 * YP_PX : pk == PACKED_16 ? 4 * YP_PX : 16 * (YP_PX_V210 / 6); }   // of a lane's run
constexpr int pk_unit(int pk) { return pk == PACKED_8 ? 1 : pk == PACKED_16 ? 2 : 4; }     // what pointer and pitch are multiples of

// how the planes of the surface side lie: its interleave and chroma shifts (as in k_yuvcvt.hip)
enum YuvLay { LAY_UV420 = 0, LAY_420 = 1, LAY_422 = 2, LAY_444 = 3 };
constexpr bool lay_il(int l) { return l == LAY_UV420; }
constexpr int lay_sx(int l) { return l != LAY_444; }
constexpr int lay_sy(int l) { return l == LAY_UV420 || l == LAY_420; }

struct PackedCvtArgs {
    const uint8_t* src[CVT_MAX_SURFACES];
    uint8_t* dst[CVT_MAX_SURFACES];
    I420Layout s;                  // the surface side (NV12 / P010: u = the interleaved plane, cpitch = pitch)
    size_t ppitch;                 // the packed side
    int w, h;
    YuvDepth d;
    int mean;                      // chroma of a block going down: 1 the rounded mean, 0 its top-left sample
    uint32_t sel;                  // 8-bit orders: byte i of Y0 U Y1 V is byte (sel >> 8 i) & 3 of the macropixel, and the reverse
};

// step 1: the value of a sample at the destination's depth
__device__ __forceinline__ uint32_t yp_depth(const YuvDepth& d, uint32_t s) {
    return min(((min(s, d.in_max) + d.add) >> d.down) << d.up, d.out_max);
}

// ---- the surface side: N samples of SB bytes at p, the first `valid` of them inside the row, as they are stored
template <int SB, int N>
__device__ __forceinline__ void load_samples(const uint8_t* __restrict__ p, int valid, uint32_t* v) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one load");
    if (valid >= N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[BYTES / 4];
        if constexpr (BYTES == 4) q[0] = *reinterpret_cast<const uint32_t*>(p);
        else if constexpr (BYTES == 8) { const u32x2 t = *reinterpret_cast<const u32x2*>(p); q[0] = t.x; q[1] = t.y; }
        else { const u32x4 t = *reinterpret_cast<const u32x4*>(p); q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w; }
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) v[i] = (q[i / 4] >> (8 * (i % 4))) & 255u;
            else v[i] = (q[i / 2] >> (16 * (i % 2))) & 0xffffu;
        }
    } else if (valid > 0) {
        // one branch for the run, not one per sample (those cost the v210 writers 194 VGPRs): a sample outside the row is read
        // from the run's first, which is inside, and set to 0
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int j = i < valid ? i : 0;
            if constexpr (SB == 1) v[i] = p[j];
            else v[i] = reinterpret_cast<const uint16_t*>(p)[j];
            if (i >= valid) v[i] = 0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = 0;
    }
}

// NT: the non-temporal hint.  It suits a store that fills its lines by itself - neighbouring lanes 4 to 32 bytes apart, the 8-pixel
// kernels - and not the v210 kernels', whose lanes are 12 to 64 bytes apart so that three or four instructions share a line: with
// the hint those partial lines are not merged on their way out, and the v210 kernels ran at 0.23 - 0.30 of the sibling conversion's
// bytes per second instead of 0.71 - 0.73 ("Packed capture formats").
template <bool NT, typename T>
__device__ __forceinline__ void store_run(T value, T* p) {
    if constexpr (NT) __builtin_nontemporal_store(value, p);
    else *p = value;
}

template <int SB, int N, bool NT>
__device__ __forceinline__ void store_samples(uint8_t* __restrict__ p, int valid, const uint32_t* v) {
    constexpr int BYTES = SB * N;
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "a run is one store");
    if (valid >= N && ((uintptr_t)p & (BYTES - 1)) == 0) {
        uint32_t q[BYTES / 4] = {};
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SB == 1) q[i / 4] |= v[i] << (8 * (i % 4));
            else q[i / 2] |= v[i] << (16 * (i % 2));
        }
        if constexpr (BYTES == 4) store_run<NT>(q[0], reinterpret_cast<uint32_t*>(p));
        else if constexpr (BYTES == 8) store_run<NT>(u32x2{q[0], q[1]}, reinterpret_cast<u32x2*>(p));
        else store_run<NT>(u32x4{q[0], q[1], q[2], q[3]}, reinterpret_cast<u32x4*>(p));
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

// A lane's N samples of a row as runs of the largest power of two of bytes, 16 at most, that divides them: 8 pixels are one run,
// the 24 luma pixels of a v210 lane three, its 12 chroma bytes three dwords.
constexpr int run_bytes(int bytes) { return (bytes & -bytes) < 16 ? (bytes & -bytes) : 16; }

template <int SB, int N>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ p, int valid, uint32_t (&v)[N]) {
    constexpr int RB = run_bytes(SB * N), RN = RB / SB;
#pragma unroll
    for (int c = 0; c < N / RN; c++) load_samples<SB, RN>(p + c * RB, valid - c * RN, v + c * RN);
}

template <int SB, int N, bool NT>
__device__ __forceinline__ void store_row(uint8_t* __restrict__ p, int valid, const uint32_t (&v)[N]) {
    constexpr int RB = run_bytes(SB * N), RN = RB / SB;
#pragma unroll
    for (int c = 0; c < N / RN; c++) store_samples<SB, RN, NT>(p + c * RB, valid - c * RN, v + c * RN);
}

// ---- the packed side: the ND dwords of a lane's run, the first `valid` bytes of them inside the row (a multiple of the
// macropixel - 4, 8 or 16 bytes - so a dword is inside or outside as a whole), in runs of 16 bytes
template <int UNIT, int ND>
__device__ __forceinline__ void load_packed(const uint8_t* __restrict__ p, int valid, uint32_t (&q)[ND]) {
#pragma unroll
    for (int c = 0; c < ND / 4; c++) {
        const uint8_t* __restrict__ pc = p + 16 * c;
        if (valid >= 16 * (c + 1) && ((uintptr_t)pc & 15) == 0) {
            const u32x4 t = *reinterpret_cast<const u32x4*>(pc);
            q[4 * c] = t.x; q[4 * c + 1] = t.y; q[4 * c + 2] = t.z; q[4 * c + 3] = t.w;
        } else {
#pragma unroll
            for (int i = 4 * c; i < 4 * c + 4; i++) {
                q[i] = 0;
                if (4 * i < valid) {
                    if constexpr (UNIT == 1) q[i] = p[4 * i] | p[4 * i + 1] << 8 | p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
                    else if constexpr (UNIT == 2) q[i] = reinterpret_cast<const uint16_t*>(p)[2 * i] | (uint32_t)reinterpret_cast<const uint16_t*>(p)[2 * i + 1] << 16;
                    else q[i] = reinterpret_cast<const uint32_t*>(p)[i];
                }
            }
        }
    }
}

template <int UNIT, int ND, bool NT>
__device__ __forceinline__ void store_packed(uint8_t* __restrict__ p, int valid, const uint32_t (&q)[ND]) {
#pragma unroll
    for (int c = 0; c < ND / 4; c++) {
        uint8_t* __restrict__ pc = p + 16 * c;
        if (valid >= 16 * (c + 1) && ((uintptr_t)pc & 15) == 0) {
            store_run<NT>(u32x4{q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]}, reinterpret_cast<u32x4*>(pc));
        } else {
#pragma unroll
            for (int i = 4 * c; i < 4 * c + 4; i++) {
                if (4 * i < valid) {
                    if constexpr (UNIT == 1) {
#pragma unroll
                        for (int b = 0; b < 4; b++) p[4 * i + b] = (uint8_t)(q[i] >> (8 * b));
                    } else if constexpr (UNIT == 2) {
                        reinterpret_cast<uint16_t*>(p)[2 * i] = (uint16_t)q[i];
                        reinterpret_cast<uint16_t*>(p)[2 * i + 1] = (uint16_t)(q[i] >> 16);
                    } else {
                        reinterpret_cast<uint32_t*>(p)[i] = q[i];
                    }
                }
            }
        }
    }
}

// the dwords of a run -> its samples.  v210: bits 30 - 31 of a word are not looked at.
template <int PK, int ND, int PX>
__device__ __forceinline__ void unpack_run(const uint32_t (&q)[ND], uint32_t sel, uint32_t (&y)[PX], uint32_t (&u)[PX / 2], uint32_t (&v)[PX / 2]) {
    if constexpr (PK == PACKED_8) {
#pragma unroll
        for (int i = 0; i < PX / 2; i++) {
            const uint32_t m = __builtin_amdgcn_perm(0u, q[i], sel);      // Y0 U Y1 V
            y[2 * i] = m & 255u; u[i] = (m >> 8) & 255u; y[2 * i + 1] = (m >> 16) & 255u; v[i] = m >> 24;
        }
    } else if constexpr (PK == PACKED_16) {
#pragma unroll
        for (int i = 0; i < PX / 2; i++) {
            y[2 * i] = q[2 * i] & 0xffffu; u[i] = q[2 * i] >> 16; y[2 * i + 1] = q[2 * i + 1] & 0xffffu; v[i] = q[2 * i + 1] >> 16;
        }
    } else {
#pragma unroll
        for (int g = 0; g < PX / 6; g++) {
            const uint32_t w0 = q[4 * g], w1 = q[4 * g + 1], w2 = q[4 * g + 2], w3 = q[4 * g + 3];
            u[3 * g] = w0 & 1023u;     y[6 * g] = (w0 >> 10) & 1023u;     v[3 * g] = (w0 >> 20) & 1023u;
            y[6 * g + 1] = w1 & 1023u; u[3 * g + 1] = (w1 >> 10) & 1023u; y[6 * g + 2] = (w1 >> 20) & 1023u;
            v[3 * g + 1] = w2 & 1023u; y[6 * g + 3] = (w2 >> 10) & 1023u; u[3 * g + 2] = (w2 >> 20) & 1023u;
            y[6 * g + 4] = w3 & 1023u; v[3 * g + 2] = (w3 >> 10) & 1023u; y[6 * g + 5] = (w3 >> 20) & 1023u;
        }
    }
}

// ... and back.  Every sample is within its field: an 8-bit value below 256, a v210 value below 1024 (the depth step sees to it).
template <int PK, int ND, int PX>
__device__ __forceinline__ void pack_run(const uint32_t (&y)[PX], const uint32_t (&u)[PX / 2], const uint32_t (&v)[PX / 2], uint32_t sel, uint32_t (&q)[ND]) {
    if constexpr (PK == PACKED_8) {
#pragma unroll
        for (int i = 0; i < PX / 2; i++) q[i] = __builtin_amdgcn_perm(0u, y[2 * i] | u[i] << 8 | y[2 * i + 1] << 16 | v[i] << 24, sel);
    } else if constexpr (PK == PACKED_16) {
#pragma unroll
        for (int i = 0; i < PX / 2; i++) { q[2 * i] = y[2 * i] | u[i] << 16; q[2 * i + 1] = y[2 * i + 1] | v[i] << 16; }
    } else {
#pragma unroll
        for (int g = 0; g < PX / 6; g++) {
            q[4 * g] = u[3 * g] | y[6 * g] << 10 | v[3 * g] << 20;
            q[4 * g + 1] = y[6 * g + 1] | u[3 * g + 1] << 10 | y[6 * g + 2] << 20;
            q[4 * g + 2] = v[3 * g + 1] | y[6 * g + 3] << 10 | u[3 * g + 2] << 20;
            q[4 * g + 3] = y[6 * g + 4] | v[3 * g + 2] << 10 | y[6 * g + 5] << 20;
        }
    }
}

// PK: the packed kind; OUT: surface -> packed; SB, LAY: bytes per sample and YuvLay of the surface side
template <int PK, bool OUT, int SB, int LAY>
__global__ __launch_bounds__(YP_THREADS) void yuv_packed_kernel(const PackedCvtArgs a) {
    constexpr int PX = pk_px(PK), BX = pk_bx(PK), BY = YP_THREADS / BX, ND = pk_bytes(PK) / 4, UNIT = pk_unit(PK);
    constexpr int SX = lay_sx(LAY), SY = lay_sy(LAY);
    constexpr int ROWS = 1 << SY;                // packed rows of a lane: they share a chroma row of the surface side
    constexpr int NCP = PX / 2, NCS = PX >> SX;  // chroma samples of a lane per row: packed side, surface side
    constexpr bool NT = PK != PACKED_V210;       // (store_run)

    const int x0 = (int)(blockIdx.x * BX + threadIdx.x) * PX;
    const int gy = (int)(blockIdx.y * BY + threadIdx.y);
    if (x0 >= a.w || gy >= (a.h >> SY)) return;
    const uint8_t* __restrict__ s = a.src[blockIdx.z];
    uint8_t* __restrict__ d = a.dst[blockIdx.z];
    const int valid = min(PX, a.w - x0);         // even, as w is
    // the bytes of the run inside the packed row: whole macropixels; v210: every group that holds a pixel of the picture
    const int pvalid = PK == PACKED_V210 ? 16 * ((valid + 5) / 6) : valid * (pk_bytes(PK) / PX);
    const size_t poff = (size_t)(x0 / PX) * pk_bytes(PK);
    const int cvs = valid >> SX;
    const size_t cxs = (size_t)(x0 >> SX);

    if constexpr (!OUT) {
        uint32_t u[ROWS][NCP], v[ROWS][NCP];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const size_t y = (size_t)gy * ROWS + r;
            uint32_t q[ND], yy[PX];
            load_packed<UNIT, ND>(s + y * a.ppitch + poff, pvalid, q);
            unpack_run<PK, ND, PX>(q, a.sel, yy, u[r], v[r]);
#pragma unroll
            for (int i = 0; i < PX; i++) yy[i] = yp_depth(a.d, yy[i]);
#pragma unroll
            for (int k = 0; k < NCP; k++) { u[r][k] = yp_depth(a.d, u[r][k]); v[r][k] = yp_depth(a.d, v[r][k]); }
            store_row<SB, PX, NT>(d + y * a.s.pitch + (size_t)x0 * SB, valid, yy);
        }
        // step 2, from (1, 0) to (SX, SY): 4:2:0 goes down by a row, 4:4:4 up by a column (nearest), 4:2:2 is the sample itself
        uint32_t ou[NCS], ov[NCS];
#pragma unroll
        for (int k = 0; k < NCS; k++) {
            if constexpr (SY) {
                ou[k] = a.mean ? (u[0][k] + u[ROWS - 1][k] + 1u) >> 1 : u[0][k];
                ov[k] = a.mean ? (v[0][k] + v[ROWS - 1][k] + 1u) >> 1 : v[0][k];
            } else {
                ou[k] = u[0][k >> (1 - SX)];
                ov[k] = v[0][k >> (1 - SX)];
            }
        }
        if constexpr (lay_il(LAY)) {
            uint32_t uv[2 * NCS];
#pragma unroll
            for (int k = 0; k < NCS; k++) { uv[2 * k] = ou[k]; uv[2 * k + 1] = ov[k]; }
            store_row<SB, 2 * NCS, NT>(d + a.s.u + (size_t)gy * a.s.cpitch + cxs * (2 * SB), 2 * cvs, uv);
        } else {
            store_row<SB, NCS, NT>(d + a.s.u + (size_t)gy * a.s.cpitch + cxs * SB, cvs, ou);
            store_row<SB, NCS, NT>(d + a.s.v + (size_t)gy * a.s.cpitch + cxs * SB, cvs, ov);
        }
    } else {
        uint32_t su[NCS], sv[NCS];
        if constexpr (lay_il(LAY)) {
            uint32_t uv[2 * NCS];
            load_row<SB, 2 * NCS>(s + a.s.u + (size_t)gy * a.s.cpitch + cxs * (2 * SB), 2 * cvs, uv);
#pragma unroll
            for (int k = 0; k < NCS; k++) { su[k] = uv[2 * k]; sv[k] = uv[2 * k + 1]; }
        } else {
            load_row<SB, NCS>(s + a.s.u + (size_t)gy * a.s.cpitch + cxs * SB, cvs, su);
            load_row<SB, NCS>(s + a.s.v + (size_t)gy * a.s.cpitch + cxs * SB, cvs, sv);
        }
#pragma unroll
        for (int k = 0; k < NCS; k++) { su[k] = yp_depth(a.d, su[k]); sv[k] = yp_depth(a.d, sv[k]); }
        // step 2, from (SX, SY) to (1, 0): 4:4:4 goes down by a column, 4:2:0 up by a row (nearest: both rows take the sample)
        uint32_t pu[NCP], pv[NCP];
#pragma unroll
        for (int k = 0; k < NCP; k++) {
            if constexpr (SX == 0) {
                pu[k] = a.mean ? (su[2 * k] + su[2 * k + 1] + 1u) >> 1 : su[2 * k];
                pv[k] = a.mean ? (sv[2 * k] + sv[2 * k + 1] + 1u) >> 1 : sv[2 * k];
            } else {
                pu[k] = su[k];
                pv[k] = sv[k];
            }
            // v210: the fields of pixels beyond the picture in the last group are written as 0
            if (PK == PACKED_V210 && 2 * k >= valid) pu[k] = pv[k] = 0;
        }
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const size_t y = (size_t)gy * ROWS + r;
            uint32_t q[ND], yy[PX];
            load_row<SB, PX>(s + y * a.s.pitch + (size_t)x0 * SB, valid, yy);
#pragma unroll
            for (int i = 0; i < PX; i++) {
                yy[i] = yp_depth(a.d, yy[i]);
                if (PK == PACKED_V210 && i >= valid) yy[i] = 0;
            }
            pack_run<PK, ND, PX>(yy, pu, pv, a.sel, q);
            store_packed<UNIT, ND, NT>(d + y * a.ppitch + poff, pvalid, q);
        }
    }
}

int lay_of(const PixFmt& f) { return f.luma_uv() ? LAY_UV420 : f.sy ? LAY_420 : f.sx ? LAY_422 : LAY_444; }

template <int PK, bool OUT, int SB>
void launch_lay(int lay, dim3 grid, hipStream_t st, const PackedCvtArgs& a) {
    const dim3 block(pk_bx(PK), YP_THREADS / pk_bx(PK));
    if (lay == LAY_UV420) hipLaunchKernelGGL((yuv_packed_kernel<PK, OUT, SB, LAY_UV420>), grid, block, 0, st, a);
    else if (lay == LAY_420) hipLaunchKernelGGL((yuv_packed_kernel<PK, OUT, SB, LAY_420>), grid, block, 0, st, a);
    else if (lay == LAY_422) hipLaunchKernelGGL((yuv_packed_kernel<PK, OUT, SB, LAY_422>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((yuv_packed_kernel<PK, OUT, SB, LAY_444>), grid, block, 0, st, a);
}

template <int PK, bool OUT>
void launch_kind(const PixFmt& f, hipStream_t st, int n, const PackedCvtArgs& a) {
    const int bx = pk_bx(PK), by = YP_THREADS / bx;
    const dim3 grid((unsigned)((a.w + bx * pk_px(PK) - 1) / (bx * pk_px(PK))), (unsigned)(((a.h >> f.sy) + by - 1) / by), (unsigned)n);
    if (f.sample_bytes == 1) launch_lay<PK, OUT, 1>(lay_of(f), grid, st, a);
    else launch_lay<PK, OUT, 2>(lay_of(f), grid, st, a);
}

template <bool OUT>
int launch_packed(int kind, uint32_t sel, const void* const* src, void* const* dst, size_t ppitch, const PixFmt& f, const I420Layout& l, int n, int w,
                  int h, const YuvDepth& depth, bool mean, hipStream_t st) {
    PackedCvtArgs a{};
    for (int k = 0; k < n; k++) { a.src[k] = (const uint8_t*)src[k]; a.dst[k] = (uint8_t*)dst[k]; }
    a.s = l;
    a.ppitch = ppitch;
    a.w = w; a.h = h;
    a.d = depth;
    a.mean = mean;
    a.sel = sel;
    if (kind == PACKED_8) launch_kind<PACKED_8, OUT>(f, st, n, a);
    else if (kind == PACKED_16) launch_kind<PACKED_16, OUT>(f, st, n, a);
    else launch_kind<PACKED_V210, OUT>(f, st, n, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace

int launch_cvt_packed_to_yuv(int kind, uint32_t sel, const void* const* src, size_t src_pitch, const PixFmt& df, void* const* dst, const I420Layout& out,
                             int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st) {
    return launch_packed<false>(kind, sel, src, dst, src_pitch, df, out, n, w, h, depth, mean, st);
}

int launch_cvt_yuv_to_packed(const PixFmt& sf, const void* const* src, const I420Layout& in, int kind, uint32_t sel, void* const* dst, size_t dst_pitch,
                             int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st) {
    return launch_packed<true>(kind, sel, src, dst, dst_pitch, sf, in, n, w, h, depth, mean, st);
}

}  // namespace vsd
