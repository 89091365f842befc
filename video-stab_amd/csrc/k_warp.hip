// warpAffine for gfx950: the device counterpart of
//   cv::warpAffine(src, dst, T, size, INTER_LINEAR, BORDER_CONSTANT)
// as called at /root/reference/src/Stabilizer.cpp:1056-1060 (and, with a scale
// matrix, src/AutoZoomCrop.cpp:270).  Integer fixed-point throughout:
//   inverse map in double (cv::warpAffine), AB_BITS=10 coordinates rounded per
//   row/column, 1/32-px fractions, 4-tap bilinear with weights summing to 2^15.
// The 4-tap sum is evaluated in its exactly-equivalent separable form
//   ((v00*(32-fx)+v01*fx)*(32-fy) + (v10*(32-fx)+v11*fx)*fy + 512) >> 10
// (the (0,0) table entry {32767,0,0,1} gives the same 8-bit result).
//
// HBM-bound stage: 2 x frame bytes of algorithmic traffic per frame.  One
// workgroup = one 128x16 output tile:
//   1. every wave evaluates, in ONE double-precision pass, its share of the tile's
//      coordinate terms (adelta/bdelta of 32 columns, X0/Y0 of 4 rows -> LDS) and, in four
//      spare lanes, the terms of the tile corners, from which the source bounding box of
//      the tile follows by v_readlane (the maps are monotone in x and in y);
//   2. the box is staged into LDS with coalesced 12-byte/lane loads, one dword per pixel;
//      tiles whose box lies inside the image take a branch-free version of this;
//   3. fast path (box at most 136 x 28, i.e. rotations up to ~4 degrees at scale ~1): lane L
//      of a 32-lane row blends the pixels L, L+32, L+64, L+96 (neighbouring lanes read
//      neighbouring LDS dwords: no bank conflicts), taps at immediate offsets of one
//      multiply-add address, horizontal lerps with v_dot4_u32_u8 on byte-permuted tap pairs,
//      vertical lerp in 24-bit multiply-adds whose byte 2 is the rounded result; the row is
//      transposed through a per-wave LDS buffer so that each lane stores 12 contiguous bytes;
//   4. other tiles: a generic LDS path (variable pitch) or, when the box does not fit the
//      LDS budget (large rotation / scale), direct global loads - the same arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "launchers.h"
#include "vs_common.h"
#include "warp_tab.h"

namespace vsd {

namespace {

constexpr int TW = WT_TW;    // output tile width  (pixels)
constexpr int TH = WT_TH;    // output tile height (rows)
constexpr int PX = 4;        // consecutive output pixels per lane
constexpr int NT = 256;      // threads per workgroup
constexpr int TXN = TW / PX; // 32 lanes along x
constexpr int TYN = NT / TXN;// 8 lane-rows
constexpr int MAXB = WARP_BATCH_MAX;   // frames per launch (frame pointers and, for host matrices, the maps travel as kernel arguments)
// fast path (near-identity maps): the source box of a tile is staged with a FIXED row pitch, so
// the lower taps sit at an immediate offset and the tap address is one multiply-add
constexpr int FDATA = 136;   // staged pixels of a row (128 + tap + shear + 12-byte alignment slack)
constexpr int FPITCH = 136;  // staged row pitch in pixels (= dwords).  (A pitch of 160 - a multiple of the 32 LDS banks, so that the lanes the
                             // map's rotation moves to the next source row keep their banks: what the plane kernels do - costs the
                             // BGR kernel its eighth workgroup per CU: 90.8 instead of 85 us per 32 frames, not kept.)
constexpr int FROWS = 25;    // staged rows (rotations up to ~3.5 degrees at scale ~1)
constexpr int LDS_PX = FPITCH * FROWS;   // 13.3 KiB of staged pixels per workgroup
constexpr int SG = FDATA / 4;            // 34 four-pixel groups per staged row
constexpr int SR = 7;                    // rows per staging pass (34 x 7 = 238 lanes)
constexpr int SPASS = (FROWS + SR - 1) / SR;   // 4 staging passes held in registers (the last one is partial)
constexpr int LUT_STRIDE = 32;           // bytes between the entries of the weight table (index = coordinate & 0x3E0)
constexpr int OBUF = (NT / 64) * 2 * TW; // per wave: two output rows, one dword per pixel

struct WarpCore {                // what the staging and output code needs of a launch (kept in scalar registers)
    size_t sstride, dstride;
    int sw, sh, dw, dh;
    int src_aligned, dst_aligned;
    int border;                  // VS_BORDER_BLACK (constant 0) or VS_BORDER_REPLICATE
};

struct WarpArgs {
    WarpCore c;
    const double* Minv_dev;      // inverse maps on the device (minv_stride doubles apart), or nullptr
    double Minv_val[MAXB * 6];   // used when Minv_dev == nullptr
    int minv_stride;             // doubles between the maps of consecutive frames in Minv_dev
    int32_t* tabs;               // coordinate tables of the frames of this launch (warp_tables_kernel), or nullptr
    int tab_stride;              // ints between the tables of consecutive frames
    int tab_row, tab_ad;         // offsets inside a frame's table (TabLayout)
    const uint8_t* srcs[MAXB];
    uint8_t* dsts[MAXB];
};

// One source pixel as a dword; outside the image: 0 (BORDER_CONSTANT) or the nearest
// edge pixel (BORDER_REPLICATE, remapBilinear's clip()).
// SB = 2: 16-bit samples (P010 planes; CN = 1 or 2): the sample, or the (U, V) pair, as the dword's halves.
template <int CN, int SB = 1>
__device__ __forceinline__ uint32_t load_px_checked(const uint8_t* src, size_t sstride, int sw,
                                                    int sh, int sx, int sy, int border = VS_BORDER_BLACK) {
    if (border == VS_BORDER_REPLICATE) {
        sx = sx < 0 ? 0 : (sx >= sw ? sw - 1 : sx);
        sy = sy < 0 ? 0 : (sy >= sh ? sh - 1 : sy);
    } else if ((unsigned)sx >= (unsigned)sw || (unsigned)sy >= (unsigned)sh) return 0u;
    if (SB == 2) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(src + (size_t)sy * sstride) + (size_t)sx * CN;
        uint32_t v16 = q[0];
        if (CN > 1) v16 |= (uint32_t)q[1] << 16;
        return v16;
    }
    const uint8_t* p = src + (size_t)sy * sstride + (size_t)sx * CN;
    uint32_t v = p[0];
    if (CN > 1) v |= (uint32_t)p[1] << 8;
    if (CN > 2) v |= (uint32_t)p[2] << 16;
    if (CN > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

// The same under VS_BORDER_FILL (edge fill on YUV surfaces): outside the plane the pixel is `fillpx`, the plane's fill in the form
// above - the sample, or the (U, V) pair.  Each tap is decided by itself.
template <int CN, int SB>
__device__ __forceinline__ uint32_t load_px_fill(const uint8_t* src, size_t sstride, int sw, int sh, int sx, int sy, uint32_t fillpx) {
    if ((unsigned)sx >= (unsigned)sw || (unsigned)sy >= (unsigned)sh) return fillpx;
    if (SB == 2) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(src + (size_t)sy * sstride) + (size_t)sx * CN;
        uint32_t v16 = q[0];
        if (CN > 1) v16 |= (uint32_t)q[1] << 16;
        return v16;
    }
    const uint8_t* p = src + (size_t)sy * sstride + (size_t)sx * CN;
    uint32_t v = p[0];
    if (CN > 1) v |= (uint32_t)p[1] << 8;
    return v;
}

// p00/p01 = taps of the upper row, p10/p11 of the lower row (one pixel per dword,
// channel c in byte c).  Horizontal lerps as byte dot products, vertical in 24 bits.
template <int CN>
__device__ __forceinline__ uint32_t blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11,
                                          uint32_t fx, uint32_t fy) {
    const uint32_t wlo = (32u - fx) | (fx << 8);     // weights against bytes 0,1
    const uint32_t whi = wlo << 16;                    // weights against bytes 2,3
    const uint32_t wy0 = 32u - fy, wy1 = fy;
    // (c0_a, c0_b, c1_a, c1_b): channels 0 and 1 of the two taps side by side
    const uint32_t x0 = __builtin_amdgcn_perm(p01, p00, 0x05010400u);
    const uint32_t x1 = __builtin_amdgcn_perm(p11, p10, 0x05010400u);
    uint32_t out;
    {
        const uint32_t t = __builtin_amdgcn_udot4(x0, wlo, 0u, false);
        const uint32_t b = __builtin_amdgcn_udot4(x1, wlo, 0u, false);
        out = (__umul24(t, wy0) + __umul24(b, wy1) + 512u) >> 10;
    }
    if (CN > 1) {
        const uint32_t t = __builtin_amdgcn_udot4(x0, whi, 0u, false);
        const uint32_t b = __builtin_amdgcn_udot4(x1, whi, 0u, false);
        out |= ((__umul24(t, wy0) + __umul24(b, wy1) + 512u) >> 10) << 8;
    }
    if (CN > 2) {
        // (c2_a, c2_b, 0, 0); four channels: (c2_a, c2_b, c3_a, c3_b)
        const uint32_t sel = CN > 3 ? 0x07030602u : 0x0C0C0602u;
        const uint32_t y0 = __builtin_amdgcn_perm(p01, p00, sel);
        const uint32_t y1 = __builtin_amdgcn_perm(p11, p10, sel);
        const uint32_t t = __builtin_amdgcn_udot4(y0, wlo, 0u, false);
        const uint32_t b = __builtin_amdgcn_udot4(y1, wlo, 0u, false);
        out |= ((__umul24(t, wy0) + __umul24(b, wy1) + 512u) >> 10) << 16;
        if (CN > 3) {
            const uint32_t ta = __builtin_amdgcn_udot4(y0, whi, 0u, false);
            const uint32_t ba = __builtin_amdgcn_udot4(y1, whi, 0u, false);
            out |= ((__umul24(ta, wy0) + __umul24(ba, wy1) + 512u) >> 10) << 24;
        }
    }
    return out;
}

// ---- 16-bit samples (P010) ---------------------------------------------------------------------------------------------------
// cv::warpAffine on CV_16U data blends with the float table w = n / 1024, n = ((32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy fx), and
// saturate_cast<ushort> rounds half to even.  Here: the exact integer S = sum v_i n_i (< 2^26) in its separable form, rounded once,
// half to even - for ten-bit content what the float form gives on any build, for arbitrary 16-bit content the definition.
// The fp32-on-denormals vertical lerp of the 8-bit kernels does not carry over (S needs 26 bits): integer throughout.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// pair = [v(x), v(x+1)] as the halves of a dword, w = (32 - fx) | fx << 16: the horizontal lerp in one v_dot2_u32_u16 (< 2^21)
__device__ __forceinline__ uint32_t hlerp16(uint32_t pair, uint32_t w) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pair), __builtin_bit_cast(u16x2, w), 0u, false);
}

// t, b: the horizontal sums of the upper and the lower tap row; S = t (32 - fy) + b fy = 32 t + fy (b - t)
__device__ __forceinline__ uint32_t vlerp16(uint32_t t, uint32_t b, uint32_t fy) {
    const uint32_t S = (t << 5) + (uint32_t)__mul24((int)fy, (int)b - (int)t);
    return (S + 511u + ((S >> 10) & 1u)) >> 10;
}

// Taps as load_px_checked<CN, 2> gives them -> the pixel in the same form.
template <int CN>
__device__ __forceinline__ uint32_t blend16(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx, uint32_t fy) {
    const uint32_t wx = (32u - fx) | (fx << 16);
    uint32_t out = vlerp16(hlerp16(__builtin_amdgcn_perm(p01, p00, 0x05040100u), wx), hlerp16(__builtin_amdgcn_perm(p11, p10, 0x05040100u), wx), fy);
    if (CN > 1)
        out |= vlerp16(hlerp16(__builtin_amdgcn_perm(p01, p00, 0x07060302u), wx), hlerp16(__builtin_amdgcn_perm(p11, p10, 0x07060302u), wx), fy) << 16;
    return out;
}

struct __attribute__((aligned(4))) U3 { uint32_t a, b, c; };
struct __attribute__((aligned(4))) U4 { uint32_t a, b, c, d; };

// 12 bytes with the non-temporal hint (global_store_dwordx3 ... nt)
__device__ __forceinline__ void store_nt3(uint8_t* p, const U3& v) {
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    __builtin_nontemporal_store(u32x3{v.a, v.b, v.c}, reinterpret_cast<u32x3*>(p));
}

template <int CN>
__device__ __forceinline__ uint4 stage_group(const WarpCore& c, const uint8_t* __restrict__ src, int sx, int sy) {
    uint4 px = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)sy < (unsigned)c.sh || c.border == VS_BORDER_REPLICATE) {
        if (c.src_aligned && sx >= 0 && sx + 3 < c.sw && (unsigned)sy < (unsigned)c.sh) {
            const uint8_t* p = src + (size_t)sy * c.sstride + (size_t)sx * CN;
            if (CN == 3) {
                const U3 d = *reinterpret_cast<const U3*>(p);
                px.x = d.a & 0xFFFFFFu;
                px.y = (d.a >> 24) | ((d.b & 0xFFFFu) << 8);
                px.z = (d.b >> 16) | ((d.c & 0xFFu) << 16);
                px.w = d.c >> 8;
            } else if (CN == 1) {
                const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
                px.x = d & 255u; px.y = (d >> 8) & 255u; px.z = (d >> 16) & 255u; px.w = d >> 24;
            } else if (CN == 4) {
                px = *reinterpret_cast<const uint4*>(p);
            } else {
                const uint2 d = *reinterpret_cast<const uint2*>(p);
                px.x = d.x & 0xFFFFu; px.y = d.x >> 16; px.z = d.y & 0xFFFFu; px.w = d.y >> 16;
            }
        } else {
            px.x = load_px_checked<CN>(src, c.sstride, c.sw, c.sh, sx, sy, c.border);
            px.y = load_px_checked<CN>(src, c.sstride, c.sw, c.sh, sx + 1, sy, c.border);
            px.z = load_px_checked<CN>(src, c.sstride, c.sw, c.sh, sx + 2, sy, c.border);
            px.w = load_px_checked<CN>(src, c.sstride, c.sw, c.sh, sx + 3, sy, c.border);
        }
    }
    return px;
}

// FILL (the VS_BORDER_FILL kernels, direct path only): a tap outside the picture is `fillpx` (load_px_fill)
template <int CN, bool USE_LDS, int SB = 1, bool FILL = false>
__device__ __forceinline__ void emit_rows(const WarpCore& c, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                          const uint32_t* tile, const int* s_ad, const int* s_bd, const int* s_x0,
                                          const int* s_y0, int x0, int y0, int x1, int y1, int bx0a, int by0, int bw, int tid, uint32_t fillpx = 0u) {
    const int tx = tid % TXN, ty = tid / TXN;
    const int x = x0 + PX * tx;
    if (x > x1) return;
    int ad[PX], bd[PX];
#pragma unroll
    for (int i = 0; i < PX; i++) { ad[i] = s_ad[PX * tx + i]; bd[i] = s_bd[PX * tx + i]; }
    uint32_t o[TH / TYN][PX];
#pragma unroll
    for (int r = 0; r < TH / TYN; r++) {
        const int yl = ty + TYN * r;
        const int X0 = s_x0[yl], Y0 = s_y0[yl];
        uint32_t p00[PX], p01[PX], p10[PX], p11[PX], fx[PX], fy[PX];
#pragma unroll
        for (int i = 0; i < PX; i++) {
            const int X = (X0 + ad[i]) >> 5, Y = (Y0 + bd[i]) >> 5;
            const int sx = sat_s16(X >> 5), sy = sat_s16(Y >> 5);
            fx[i] = X & 31; fy[i] = Y & 31;
            if (USE_LDS) {
                // rows beyond the tile (yl past y1) still index inside the staged box of a
                // full tile only; clamp them to the first row so the reads stay in bounds
                const int idx = y0 + yl <= y1 ? __mul24(sy - by0, bw) + (sx - bx0a) : 0;
                p00[i] = tile[idx]; p01[i] = tile[idx + 1];
                p10[i] = tile[idx + bw]; p11[i] = tile[idx + bw + 1];
            } else if constexpr (FILL) {
                p00[i] = load_px_fill<CN, SB>(src, c.sstride, c.sw, c.sh, sx, sy, fillpx);
                p01[i] = load_px_fill<CN, SB>(src, c.sstride, c.sw, c.sh, sx + 1, sy, fillpx);
                p10[i] = load_px_fill<CN, SB>(src, c.sstride, c.sw, c.sh, sx, sy + 1, fillpx);
                p11[i] = load_px_fill<CN, SB>(src, c.sstride, c.sw, c.sh, sx + 1, sy + 1, fillpx);
            } else {
                p00[i] = load_px_checked<CN, SB>(src, c.sstride, c.sw, c.sh, sx, sy, c.border);
                p01[i] = load_px_checked<CN, SB>(src, c.sstride, c.sw, c.sh, sx + 1, sy, c.border);
                p10[i] = load_px_checked<CN, SB>(src, c.sstride, c.sw, c.sh, sx, sy + 1, c.border);
                p11[i] = load_px_checked<CN, SB>(src, c.sstride, c.sw, c.sh, sx + 1, sy + 1, c.border);
            }
        }
#pragma unroll
        for (int i = 0; i < PX; i++) {
            if constexpr (SB == 2) o[r][i] = blend16<CN>(p00[i], p01[i], p10[i], p11[i], fx[i], fy[i]);
            else o[r][i] = blend<CN>(p00[i], p01[i], p10[i], p11[i], fx[i], fy[i]);
        }
    }
#pragma unroll
    for (int r = 0; r < TH / TYN; r++) {
        const int y = y0 + ty + TYN * r;
        if (y > y1) break;
        uint8_t* d = dst + (size_t)y * c.dstride + (size_t)x * (CN * SB);
        if (SB == 2) {             // a pixel is one (luma) or two (chroma) 16-bit samples: four pixels = 8 / 16 aligned bytes
            if (c.dst_aligned && x + PX - 1 <= x1) {
                if (CN == 1) {
                    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                    __builtin_nontemporal_store(u32x2{o[r][0] | (o[r][1] << 16), o[r][2] | (o[r][3] << 16)}, reinterpret_cast<u32x2*>(d));
                } else {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(u32x4{o[r][0], o[r][1], o[r][2], o[r][3]}, reinterpret_cast<u32x4*>(d));
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; i++) {
                    if (x + i > x1) break;
#pragma unroll
                    for (int c = 0; c < CN; c++) reinterpret_cast<uint16_t*>(d)[i * CN + c] = (uint16_t)(o[r][i] >> (16 * c));
                }
            }
            continue;
        }
        if (c.dst_aligned && x + PX - 1 <= x1) {
            if (CN == 3) {
                U3 v;
                v.a = o[r][0] | (o[r][1] << 24);
                v.b = (o[r][1] >> 8) | (o[r][2] << 16);
                v.c = (o[r][2] >> 16) | (o[r][3] << 8);
                store_nt3(d, v);
            } else if (CN == 1) {
                __builtin_nontemporal_store(o[r][0] | (o[r][1] << 8) | (o[r][2] << 16) | (o[r][3] << 24), reinterpret_cast<uint32_t*>(d));
            } else if (CN == 4) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(u32x4{o[r][0], o[r][1], o[r][2], o[r][3]}, reinterpret_cast<u32x4*>(d));
            } else {
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                __builtin_nontemporal_store(u32x2{o[r][0] | (o[r][1] << 16), o[r][2] | (o[r][3] << 16)}, reinterpret_cast<u32x2*>(d));
            }
        } else {
#pragma unroll
            for (int i = 0; i < PX; i++) {
                if (x + i > x1) break;
#pragma unroll
                for (int c = 0; c < CN; c++) d[i * CN + c] = (uint8_t)(o[r][i] >> (8 * c));
            }
        }
    }
}

// ---- fast path (BGR8, near-identity maps) ------------------------------------------------------------------
// Staged layout: one dword per source pixel x, E(x) = [B(x), B(x+1), G(x), R(x)].  The horizontal lerp of the B
// channel is then ONE byte dot product on the staged dword itself, and one byte permute of (E(x), E(x+1)) gives
// [G(x), G(x+1), R(x), R(x+1)] for the other two (two permutes per tap pair with a plain [B,G,R,-] layout).
//
// Weight table in LDS, 32 entries (one per 1/32-px fraction f) of 32 bytes: {wlo, whi, W0, W1}:
//   wlo = (32-f) | f << 8, whi = wlo << 16   byte weights of the horizontal lerp (against bytes 0,1 / 2,3)
//   W0 = (32-f) * 2^121, W1 = f * 2^121      float weights of the vertical lerp
// indexed with (coordinate & 0x3E0) - the fraction bits in place - so a pixel's weights cost two 2-cycle ANDs and
// two LDS reads instead of a bit-field extract, two multiply-adds, a shift and a subtraction.
//
// Vertical lerp in fp32.  gfx950 issues v_fma_f32 / v_add_f32 at twice the rate of the integer multiply-adds.  The
// horizontal sums t, b <= 8160 are used as they are: an integer bit pattern read as a float is the denormal
// t * 2^-149 (denormals run at full rate), so
//   u = fma(t, W0, 2^-29)       = (t*(32-f)     + 1/2) * 2^-28     exact (< 2^20 units of 2^-29)
//   v = fma(b, W1, u)           = (S            + 1/2) * 2^-28     S = t*(32-f) + b*f, exact
//   m = v + 32.0f               rounds to multiples of 2^-18 = 1024 * 2^-28: RNE((S + 1/2) / 1024), never a tie,
//                               = floor((S + 512) / 1024) = cv::warpAffine's (sum + 2^14) >> 15 of the 4-tap form
// and the 8-bit result is the low byte of m's bit pattern (checked exhaustively: scratch/denorm_probe.hip).
struct __attribute__((aligned(8))) LutX { uint32_t wlo, whi; };
struct __attribute__((aligned(8))) LutY { float w0, w1; };

__device__ __forceinline__ float vlerp(uint32_t t, uint32_t b, LutY w) {
    const float u = __builtin_fmaf(__uint_as_float(t), w.w0, 0x1p-29f);
    const float v = __builtin_fmaf(__uint_as_float(b), w.w1, u);
    return v + 32.0f;
}

__device__ __forceinline__ uint32_t blend3_fast(uint32_t e00, uint32_t e01, uint32_t e10, uint32_t e11, LutX wx, LutY wy) {
    const uint32_t q0 = __builtin_amdgcn_perm(e01, e00, 0x07030602u);   // [G00 G01 R00 R01]
    const uint32_t q1 = __builtin_amdgcn_perm(e11, e10, 0x07030602u);
    const float mb = vlerp(__builtin_amdgcn_udot4(e00, wx.wlo, 0u, false), __builtin_amdgcn_udot4(e10, wx.wlo, 0u, false), wy);
    const float mg = vlerp(__builtin_amdgcn_udot4(q0, wx.wlo, 0u, false), __builtin_amdgcn_udot4(q1, wx.wlo, 0u, false), wy);
    const float mr = vlerp(__builtin_amdgcn_udot4(q0, wx.whi, 0u, false), __builtin_amdgcn_udot4(q1, wx.whi, 0u, false), wy);
    const uint32_t bg = __builtin_amdgcn_perm(__float_as_uint(mg), __float_as_uint(mb), 0x0C0C0400u);   // (B, G, 0, 0)
    return __builtin_amdgcn_perm(__float_as_uint(mr), bg, 0x0C040100u);                                  // (B, G, R, 0)
}

// Staged dword of pixel x from the pixel itself and its right neighbour, both as [B, G, R, -].
__device__ __forceinline__ uint32_t pair_b(uint32_t cur, uint32_t next) { return __builtin_amdgcn_perm(next, cur, 0x02010400u); }

// Fast-path output (BGR8).  Lane L of a 32-lane row handles the pixels L, L+32, L+64, L+96 of its row, so that
// neighbouring lanes read neighbouring LDS dwords (no bank conflicts; with 4 consecutive pixels per lane the taps of a
// wave fall on 8 of the 32 banks).  The results are transposed through a small per-wave LDS buffer so that every lane
// still stores 4 consecutive pixels = 12 contiguous bytes.  `base` = -(by0*FPITCH + bx0a).
__device__ __forceinline__ void emit_fast(const WarpCore& c, uint8_t* __restrict__ dst, const uint32_t* tile,
                                          uint32_t* obuf, const uint8_t* lut, const int* s_ad, const int* s_bd, const int* s_x0,
                                          const int* s_y0, int x0, int y0, int x1, int y1, int base, int tid) {
    const int L = tid & 31, ty = tid >> 5;
    uint32_t* wb = obuf + (tid >> 6) * (2 * TW) + ((tid >> 5) & 1) * TW;
    int ad[4], bd[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { ad[i] = s_ad[L + 32 * i]; bd[i] = s_bd[L + 32 * i]; }
    // full tile, aligned rows: the stores need no per-lane checks (tile-uniform)
    const bool whole = c.dst_aligned && x1 - x0 == TW - 1 && y1 - y0 == TH - 1;
    const uint32_t dstride32 = (uint32_t)c.dstride;
    uint8_t* const dtile = dst + (size_t)y0 * c.dstride + (size_t)x0 * 3;      // wave-uniform base, 32-bit lane offsets
#pragma unroll
    for (int r = 0; r < TH / TYN; r++) {
        const int yl = ty + TYN * r;
        const int X0 = s_x0[yl], Y0 = s_y0[yl];
        uint32_t e00[4], e01[4], e10[4], e11[4];
        LutX wx[4];
        LutY wy[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int SX = X0 + ad[i], SY = Y0 + bd[i];              // 1/1024 px
            // byte address of the upper-left tap: one multiply-add and one shift-add
            int rowb = __mul24(SY >> 10, FPITCH * 4) + 4 * base;
            asm("" : "+v"(rowb));
            int sxi = SX >> 10;
            asm("" : "+v"(sxi));
            const uint32_t* t = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(tile) + ((sxi << 2) + rowb));
            e00[i] = t[0]; e01[i] = t[1];
            e10[i] = t[FPITCH]; e11[i] = t[FPITCH + 1];
            wx[i] = *reinterpret_cast<const LutX*>(lut + (SX & 0x3E0));
            wy[i] = *reinterpret_cast<const LutY*>(lut + 8 + (SY & 0x3E0));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) wb[L + 32 * i] = blend3_fast(e00[i], e01[i], e10[i], e11[i], wx[i], wy[i]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint4 q = *reinterpret_cast<const uint4*>(&wb[4 * L]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (whole) {
            U3 v;
            v.a = __builtin_amdgcn_perm(q.y, q.x, 0x04020100u);
            v.b = __builtin_amdgcn_perm(q.z, q.y, 0x05040201u);
            v.c = __builtin_amdgcn_perm(q.w, q.z, 0x06050402u);
            // the result is not read again by this launch: streaming stores (nt) leave the caches to the source rows
            // (measured: 96.1 -> 88.5 us per 32-frame launch; sc1 / sc0 sc1 stores and nt LOADS did not help)
            store_nt3(dtile + (__umul24((uint32_t)yl, dstride32) + 12u * L), v);
            continue;
        }
        const int y = y0 + yl, x = x0 + 4 * L;
        if (y <= y1 && x <= x1) {
            uint8_t* d = dst + (size_t)y * c.dstride + (size_t)x * 3;
            if (c.dst_aligned && x + 3 <= x1) {
                U3 v;
                v.a = __builtin_amdgcn_perm(q.y, q.x, 0x04020100u);
                v.b = __builtin_amdgcn_perm(q.z, q.y, 0x05040201u);
                v.c = __builtin_amdgcn_perm(q.w, q.z, 0x06050402u);
                store_nt3(d, v);
            } else {
                const uint32_t o[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (x + i > x1) break;
                    d[3 * i] = (uint8_t)o[i]; d[3 * i + 1] = (uint8_t)(o[i] >> 8); d[3 * i + 2] = (uint8_t)(o[i] >> 16);
                }
            }
        }
    }
}

// hal::warpAffine / WarpAffineInvoker coordinate terms in one form: round((p*v + q) * 1024)  (warp_tab.h)
__device__ __forceinline__ int coord_term(double p, double q, double v) { return wt_coord_term(p, q, v); }

// The inverse map of frame bz (wave-uniform: scalar loads or kernel arguments).
__device__ __forceinline__ void load_map(const WarpArgs& a, int bz, double* m) {
    if (a.Minv_dev) {
        const __attribute__((address_space(4))) double* mp =
            (const __attribute__((address_space(4))) double*)(a.Minv_dev + a.minv_stride * bz);
#pragma unroll
        for (int i = 0; i < 6; i++) m[i] = mp[i];
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) m[i] = a.Minv_val[6 * bz + i];
    }
}

// The coordinate terms of the tile (x0, y0) .. (x1, y1) from the inverse map m, in double: the first 128 lanes a column each (adelta,
// bdelta), the next 16 a row each (X0, Y0).  Columns and rows past the image repeat the last one.
__device__ __forceinline__ void map_terms(const double (&m)[6], int x0, int y0, int x1, int y1, int tid, int* s_ad, int* s_bd, int* s_x0, int* s_y0) {
    if (tid < TW) {
        const double dv = (double)min(x0 + tid, x1);
        s_ad[tid] = coord_term(m[0], 0.0, dv);
        s_bd[tid] = coord_term(m[3], 0.0, dv);
    } else if (tid < TW + TH) {
        const double dv = (double)min(y0 + (tid - TW), y1);
        s_x0[tid - TW] = coord_term(m[1], m[2], dv) + 16;
        s_y0[tid - TW] = coord_term(m[4], m[5], dv) + 16;
    }
}

// Coordinate tables of the frames of a launch, once per frame instead of once per tile (layout and arithmetic: warp_tab.h).
// The batch schedule has them built by the kernel that computes the inverse maps (k_ransac.hip, release workgroups); this
// launch serves the standalone operator, deferred warps and steps whose maps come out of a one-kernel tail (Kalman).
constexpr int TAB_COL = WT_COL;

__global__ __launch_bounds__(NT) void warp_tables_kernel(WarpArgs a) {
    const int bz = blockIdx.y;
    double m[6];
    load_map(a, bz, m);
    TabLayout L;
    L.row = a.tab_row; L.ad = a.tab_ad; L.stride = a.tab_stride;
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j < wt_entries(a.c.dw, a.c.dh))
        wt_build_entry(a.tabs + (size_t)bz * a.tab_stride, L, m, a.c.dw, a.c.dh, a.srcs[bz], a.dsts[bz], j);
}

// The table blocks of up to NVT_MAX NV12 surfaces, both planes, from inverse maps given on the host, in ONE launch
// (blockIdx.y = surface, blockIdx.z = plane): the rotations of a batch of roll-corrected surfaces.
constexpr int NVT_MAX = 16;
struct NvTabArgs {
    int32_t* tabs;
    int block, chroma;           // ints between the blocks of consecutive surfaces / offset of the chroma table inside a block
    int w, h;
    size_t src_uv, dst_uv;
    const uint8_t* ys[NVT_MAX];
    uint8_t* yd[NVT_MAX];
    double my[NVT_MAX * 6], muv[NVT_MAX * 6];
};

__global__ __launch_bounds__(NT) void warp_tables_nv12_kernel(NvTabArgs a) {
    const int bz = blockIdx.y, plane = blockIdx.z;
    const int dw = plane ? a.w / 2 : a.w, dh = plane ? a.h / 2 : a.h;
    TabLayout L = tab_layout(dw, dh);
    L.stride = a.block;
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = plane ? a.muv[6 * bz + i] : a.my[6 * bz + i];
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j < wt_entries(dw, dh))
        wt_build_entry(a.tabs + (size_t)bz * a.block + (plane ? a.chroma : 0), L, m, dw, dh, plane ? a.ys[bz] + a.src_uv : a.ys[bz],
                       plane ? a.yd[bz] + a.dst_uv : a.yd[bz], j);
}

template <int CN, bool TABS>
__global__ __launch_bounds__(NT) void warp_affine_kernel(WarpArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[LDS_PX];
    __shared__ __attribute__((aligned(16))) uint32_t obuf[OBUF];
    __shared__ int s_ad[TW], s_bd[TW], s_x0[TH], s_y0[TH];
    __shared__ __attribute__((aligned(16))) uint8_t lut[CN == 3 ? 32 * LUT_STRIDE : 16];
    const int bz = blockIdx.z;
    const uint8_t* __restrict__ src = a.srcs[bz];
    uint8_t* __restrict__ dst = a.dsts[bz];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int x1 = min(x0 + TW, a.c.dw) - 1, y1 = min(y0 + TH, a.c.dh) - 1;
    if (CN == 3 && tid >= NT - 32) {      // weight table of the fast path (see blend3_fast): the last 32 lanes of wave 3
        const uint32_t f = tid - (NT - 32);
        const uint32_t wlo = (32u - f) | (f << 8);
        *reinterpret_cast<uint4*>(lut + f * LUT_STRIDE) =
            make_uint4(wlo, wlo << 16, __float_as_uint((float)(32u - f) * 0x1p121f), __float_as_uint((float)f * 0x1p121f));
    }

    // ---- 1. coordinate terms of the tile (128 columns: adelta, bdelta; 16 rows: X0, Y0) -> LDS.  Columns and rows
    // past the image repeat the last one, so every lane of a partial tile stays inside the box.  The maps are
    // monotone in x and in y separately, so the source bounding box of the tile follows from the terms of its
    // first/last column and row.
    int ad0, ad1, bd0, bd1, Xa, Xb, Ya, Yb;
    int tv0 = 0, tv1 = 0;
    if (TABS) {
        // from the frame's tables: the corner terms with scalar loads, the tile's share with one vector load per
        // lane; they travel together with the staging loads of step 2 and reach LDS in front of the one barrier
        const size_t tb = (size_t)bz * a.tab_stride;
        const __attribute__((address_space(4))) int32_t* Ts = (const __attribute__((address_space(4))) int32_t*)(a.tabs + tb);
        const __attribute__((address_space(4))) int32_t* Cc = Ts + TAB_COL * blockIdx.x + 4;
        const __attribute__((address_space(4))) int32_t* Cr = Ts + a.tab_row + 4 * blockIdx.y;
        ad0 = Cc[0]; ad1 = Cc[1]; bd0 = Cc[2]; bd1 = Cc[3];
        Xa = Cr[0]; Xb = Cr[1]; Ya = Cr[2]; Yb = Cr[3];
        const int32_t* Tg = a.tabs + tb + a.tab_ad;
        if (wave < 2) {
            const int c = min(x0 + tid, x1);
            tv0 = Tg[c]; tv1 = Tg[a.c.dw + c];
        } else if (tid < 2 * 64 + TH) {
            const int r = min(y0 + (tid - 128), y1);
            tv0 = Tg[2 * a.c.dw + r]; tv1 = Tg[2 * a.c.dw + a.c.dh + r];
        }
    } else {
        // no tables (single launches of the image operators): waves 0 and 1 evaluate the columns, 16 lanes of
        // wave 2 the rows, in double; the corner terms come back through LDS
        double m[6];
        load_map(a, bz, m);
        map_terms(m, x0, y0, x1, y1, tid, s_ad, s_bd, s_x0, s_y0);
        __syncthreads();
        const int cl = x1 - x0, rl = y1 - y0;
        ad0 = __builtin_amdgcn_readfirstlane(s_ad[0]); ad1 = __builtin_amdgcn_readfirstlane(s_ad[cl]);
        bd0 = __builtin_amdgcn_readfirstlane(s_bd[0]); bd1 = __builtin_amdgcn_readfirstlane(s_bd[cl]);
        Xa = __builtin_amdgcn_readfirstlane(s_x0[0]); Xb = __builtin_amdgcn_readfirstlane(s_x0[rl]);
        Ya = __builtin_amdgcn_readfirstlane(s_y0[0]); Yb = __builtin_amdgcn_readfirstlane(s_y0[rl]);
    }
    int bx0, bx1, by0, by1;
    bool saturated;
    {
        const int sx00 = (Xa + ad0) >> 10, sx01 = (Xa + ad1) >> 10, sx10 = (Xb + ad0) >> 10, sx11 = (Xb + ad1) >> 10;
        const int sy00 = (Ya + bd0) >> 10, sy01 = (Ya + bd1) >> 10, sy10 = (Yb + bd0) >> 10, sy11 = (Yb + bd1) >> 10;
        const int rx0 = min(min(sx00, sx01), min(sx10, sx11)), rx1 = max(max(sx00, sx01), max(sx10, sx11));
        const int ry0 = min(min(sy00, sy01), min(sy10, sy11)), ry1 = max(max(sy00, sy01), max(sy10, sy11));
        saturated = rx0 < -32768 || ry0 < -32768 || rx1 > 32767 || ry1 > 32767;   // saturate_cast<short> acts
        bx0 = max(rx0, -32768); bx1 = min(rx1, 32767) + 1;                        // (values past the other end
        by0 = max(ry0, -32768); by1 = min(ry1, 32767) + 1;                        //  only occur when saturated)
    }
    const int bx0a = bx0 & ~3;                       // 4-pixel (12-byte) aligned start
    const int bw = (bx1 - bx0a + 1 + 3) & ~3;        // staged width, multiple of 4
    const int bh = by1 - by0 + 1;
    const bool fast = CN == 3 && !saturated && bw <= FDATA && bh <= FROWS;
    const bool use_lds = fast || (!saturated && (long long)bw * bh <= LDS_PX);
    // (the last group of a row loads 4 bytes past the box: inside the frame unless the box ends with the frame)
    const bool interior = fast && a.c.src_aligned && bx0a >= 0 && bx0a + bw <= a.c.sw && by0 >= 0 && by0 + bh <= a.c.sh &&
                          (bx0a + bw + 2 <= a.c.sw || by0 + bh < a.c.sh);

    // ---- 2. staging
    if (interior) {
        // branch-free: 4 passes of 7 rows x 34 groups; rows past the box repeat its last row.  A lane loads 16 bytes
        // = its 4 pixels and the B of the next one (the staged dword of a pixel carries its right neighbour's B)
        const int ly = tid / SG, lx = tid - ly * SG;
        if (tid < SG * SR && 4 * lx < bw) {
            // wave-uniform base + 32-bit lane offset (the box spans < 2^24 bytes of rows)
            const uint8_t* box = src + (size_t)bx0a * 3 + (size_t)by0 * a.c.sstride;
            const uint32_t stride32 = (uint32_t)a.c.sstride, col = 12u * lx;
            U4 d[SPASS];
#pragma unroll
            for (int k = 0; k < SPASS; k++)
                if (SR * k < bh)       // tile-uniform: small rotations need 3 passes (21 rows)
                    d[k] = *reinterpret_cast<const U4*>(box + (__umul24((uint32_t)min(ly + SR * k, bh - 1), stride32) + col));
#pragma unroll
            for (int k = 0; k < SPASS; k++) {
                if (SR * k < bh && (SR * (k + 1) <= FROWS || ly + SR * k < FROWS))
                    *reinterpret_cast<uint4*>(&tile[(ly + SR * k) * FPITCH + 4 * lx]) =
                        make_uint4(__builtin_amdgcn_perm(d[k].a, d[k].a, 0x02010300u),      // bytes 0,3,1,2
                                   __builtin_amdgcn_perm(d[k].b, d[k].a, 0x05040603u),      // bytes 3,6,4,5
                                   __builtin_amdgcn_perm(d[k].c, d[k].b, 0x04030502u),      // bytes 6,9,7,8
                                   __builtin_amdgcn_perm(d[k].d, d[k].c, 0x03020401u));     // bytes 9,12,10,11
            }
        }
    } else if (use_lds) {
        const int pitch = fast ? FPITCH : bw;
        const int gpr = bw >> 2;
        const int total = gpr * bh;
        for (int g = tid; g < total; g += NT) {
            const int row = g / gpr, gx = g - row * gpr;
            uint4 px = stage_group<CN>(a.c, src, bx0a + 4 * gx, by0 + row);
            if (CN == 3 && fast) {     // the fast path's layout (tiles at the image border)
                const uint32_t nx = load_px_checked<CN>(src, a.c.sstride, a.c.sw, a.c.sh, bx0a + 4 * gx + 4, by0 + row, a.c.border);
                px = make_uint4(pair_b(px.x, px.y), pair_b(px.y, px.z), pair_b(px.z, px.w), pair_b(px.w, nx));
            }
            *reinterpret_cast<uint4*>(&tile[row * pitch + 4 * gx]) = px;
        }
    }
    if (TABS) {
        if (wave < 2) { s_ad[tid] = tv0; s_bd[tid] = tv1; }
        else if (tid < 2 * 64 + TH) { s_x0[tid - 128] = tv0; s_y0[tid - 128] = tv1; }
    }
    __syncthreads();

    // ---- 3. output (the choice is tile-uniform)
    if (CN == 3 && fast) emit_fast(a.c, dst, tile, obuf, lut, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, -(by0 * FPITCH + bx0a), tid);
    else if (use_lds) emit_rows<CN, true>(a.c, src, dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
    else emit_rows<CN, false>(a.c, src, dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
}

// The general form for planes of 16-bit samples (CN = 1: P010 luma, CN = 2: interleaved chroma): single surfaces, launches without
// tables, chroma planes that do not lie one offset behind their luma planes, geometry outside what warp_nv12_kernel packs.  Terms
// from the frame's inverse map as in the kernel above, taps read directly (no staging): emit_rows' arithmetic for 16-bit samples.
template <int CN>
__global__ __launch_bounds__(NT) void warp_affine16_kernel(WarpArgs a) {
    __shared__ int s_ad[TW], s_bd[TW], s_x0[TH], s_y0[TH];
    const int bz = blockIdx.z;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int x1 = min(x0 + TW, a.c.dw) - 1, y1 = min(y0 + TH, a.c.dh) - 1;
    double m[6];
    load_map(a, bz, m);
    map_terms(m, x0, y0, x1, y1, tid, s_ad, s_bd, s_x0, s_y0);
    __syncthreads();
    emit_rows<CN, false, 2>(a.c, a.srcs[bz], a.dsts[bz], nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
}

// ---- several small warps of different geometry in ONE launch --------------------------------------------------------------
// AutoZoomCrop's crop-and-scale of a batch of NV12 surfaces (k_azc.hip): 2 x 8 jobs of 640 x 360 / 320 x 180 pixels, every one
// with its own crop rectangle, as one launch instead of sixteen (a launch costs the host 6 - 7 us on this runtime).  The jobs
// travel as kernel arguments; blockIdx.z = job, a job's tiles beyond its own size return at once.  Terms and taps as the
// general kernel's direct path (no staging: a scale map spreads the taps of a tile over a box that no staging area holds).
// SB = 2: jobs on planes of 16-bit samples (the crop-and-scale of P010 surfaces: cn 1 and 2, P010's blend) - a kernel of its own,
// so that the 8-bit launch keeps its code and its registers; the jobs of a launch share one sample size.
// Planar 4:2:0 surfaces (I420 / I010 / I012) are three jobs of cn 1 each: 3 x 8 = WARP_JOBS_MAX jobs per batch, still one launch.
struct WarpJobsArg { WarpJob j[WARP_JOBS_MAX]; };

// RGB: the jobs of interleaved colour frames (8-bit, cn 3 or 4: AutoZoomCrop on BGR8 / RGB8 / BGRA8 / RGBA8, every channel a channel
// of its own) - a kernel of its own as well, for the same reason.
template <int SB, bool RGB = false>
__device__ __forceinline__ void warp_jobs_tile(const WarpJobsArg& a) {
    __shared__ int s_ad[TW], s_bd[TW], s_x0[TH], s_y0[TH];
    const WarpJob& j = a.j[blockIdx.z];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    if (x0 >= j.dw || y0 >= j.dh) return;                 // (workgroup-uniform)
    const int x1 = min(x0 + TW, j.dw) - 1, y1 = min(y0 + TH, j.dh) - 1;
    map_terms(j.m, x0, y0, x1, y1, tid, s_ad, s_bd, s_x0, s_y0);
    __syncthreads();
    WarpCore c;
    c.sstride = j.sstride; c.dstride = j.dstride;
    c.sw = j.sw; c.sh = j.sh; c.dw = j.dw; c.dh = j.dh;
    c.src_aligned = 0;
    const int galign = SB == 2 ? 8 * j.cn : j.cn == 2 ? 8 : 4;        // (a lane's four pixels in one store)
    c.dst_aligned = ((uintptr_t)j.dst % galign == 0) && (j.dstride % galign == 0);
    c.border = j.border;
    if constexpr (RGB) {
        c.dst_aligned = (((uintptr_t)j.dst | j.dstride) & (j.cn == 4 ? 15 : 3)) == 0;      // (a lane's four pixels: 16 bytes, or three dwords)
        if (j.cn == 4) emit_rows<4, false>(c, j.src, j.dst, nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
        else emit_rows<3, false>(c, j.src, j.dst, nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
        return;
    }
    if (j.cn == 1) emit_rows<1, false, SB>(c, j.src, j.dst, nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
    else if (j.cn == 2 || SB == 2) emit_rows<2, false, SB>(c, j.src, j.dst, nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
    else if constexpr (SB == 1) emit_rows<3, false>(c, j.src, j.dst, nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid);
}

__global__ __launch_bounds__(NT) void warp_jobs_kernel(WarpJobsArg a) { warp_jobs_tile<1>(a); }
__global__ __launch_bounds__(NT) void warp_jobs16_kernel(WarpJobsArg a) { warp_jobs_tile<2>(a); }
__global__ __launch_bounds__(NT) void warp_jobs_rgb_kernel(WarpJobsArg a) { warp_jobs_tile<1, true>(a); }

// ---- the staged form of a scale job ------------------------------------------------------------------------------------------
// A zoom stage that does not shrink (AutoZoomCrop at the surface's own size, k_azc.hip) turns the jobs above inside out: the source
// box of an output tile is smaller than the tile, and every source sample is a tap of several output samples.  A scale map is
// diagonal (m[1] = m[3] = 0): the source column sx(x) = (coord_term(m0, 0, x) + X0) >> 10 depends on the output column alone, the
// source row on the output row alone, both monotone, so the box of a tile is [sx(x0), sx(x1) + 1] x [sy(y0), sy(y1) + 1] and
//   sx(x1) - sx(x0) <= floor((a(x1) - a(x0)) / 1024) + 1,   a(x1) - a(x0) <= m0 (x1 - x0) 1024 + 1   (two roundings of 1/2; + 1 more
// below for the rounding of the products), whatever X0 is: a bound from the inverse scale factor and the tile size alone
// (scale_span).  Whether a job can be staged is therefore decided per job on the host (scale_job_staged): every tile of a staged
// job fits the staging area, the kernel has no other path.
// The box is staged as one dword per pixel, emit_rows' `tile` (load_px_checked's form of a pixel), a lane taking four pixels: ONE
// aligned load of 4 (8-bit, cn 1), 8 (8-bit cn 2; 16-bit cn 1) or 16 bytes (16-bit cn 2) where the four lie inside the crop and the
// job's rows keep that alignment; sample by sample, each checked, elsewhere.  The columns are counted from an origin bx0a <= sx(x0)
// at which the loads are aligned; a group that reaches in front of the crop (or behind it, above, below) is of the second kind, so
// NOTHING outside the crop rectangle is ever read - its neighbours in the plane are the border, 0, and are staged as 0.
// Terms, taps, blend and stores are emit_rows' (USE_LDS).  8-bit and 16-bit samples are kernels of their own, as above.
constexpr int SBW = 160;     // staged pixels of a row (a multiple of 4): an identity tile needs 130 + 3 (origin) + 3 (rounded up)
constexpr int SBH = 24;      // staged rows: an identity tile needs 18.  160 x 24 dwords = 15 KiB: eight workgroups per CU

template <int CN, int SB>
__device__ __forceinline__ void scale_stage(const WarpJob& j, uint32_t* tile, int bx0a, int by0, int bw, int bh, int aligned, int tid) {
    const int groups = bw >> 2, n = groups * bh;
    for (int g = tid; g < n; g += NT) {
        const int r = g / groups, gx = g - r * groups;
        const int sx = bx0a + 4 * gx, sy = by0 + r;
        uint4 px = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)sy < (unsigned)j.sh) {
            if (aligned && sx >= 0 && sx + 3 < j.sw) {
                const uint8_t* p = j.src + (size_t)sy * j.sstride + (size_t)sx * (CN * SB);
                if (CN * SB == 1) {
                    const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
                    px.x = d & 255u; px.y = (d >> 8) & 255u; px.z = (d >> 16) & 255u; px.w = d >> 24;
                } else if (CN * SB == 3) {      // (three bytes per pixel: the four pixels are three dwords, stage_group's split)
                    const U3 d = *reinterpret_cast<const U3*>(p);
                    px.x = d.a & 0xFFFFFFu;
                    px.y = (d.a >> 24) | ((d.b & 0xFFFFu) << 8);
                    px.z = (d.b >> 16) | ((d.c & 0xFFu) << 16);
                    px.w = d.c >> 8;
                } else if (CN * SB == 2) {      // (two bytes per pixel: U, V of 8 bits or one 16-bit sample - the same halves of a dword)
                    const uint2 d = *reinterpret_cast<const uint2*>(p);
                    px.x = d.x & 0xFFFFu; px.y = d.x >> 16; px.z = d.y & 0xFFFFu; px.w = d.y >> 16;
                } else {
                    px = *reinterpret_cast<const uint4*>(p);
                }
            } else {
                px.x = load_px_checked<CN, SB>(j.src, j.sstride, j.sw, j.sh, sx, sy);
                px.y = load_px_checked<CN, SB>(j.src, j.sstride, j.sw, j.sh, sx + 1, sy);
                px.z = load_px_checked<CN, SB>(j.src, j.sstride, j.sw, j.sh, sx + 2, sy);
                px.w = load_px_checked<CN, SB>(j.src, j.sstride, j.sw, j.sh, sx + 3, sy);
            }
        }
        *reinterpret_cast<uint4*>(tile + r * bw + 4 * gx) = px;
    }
}

// RGB: interleaved colour jobs (8-bit, cn 3 or 4), a kernel of its own.  cn 4: ONE aligned 16-byte load as above.  cn 3: four
// pixels are 12 bytes, three dwords, and the loads ask for dword alignment only: the rows keep it when the stride is a multiple of 4,
// and since 3 = -1 (mod 4) the columns x with x = address of the crop's first sample (mod 4) are the aligned ones.  Every staged dword
// is written as part of a lane's 16 bytes (ds_write_b128, consecutive lanes consecutive 16 bytes), whatever the pixel size.
template <int SB, bool RGB = false>
__device__ __forceinline__ void scale_jobs_tile(const WarpJobsArg& a) {
    __shared__ int s_ad[TW], s_bd[TW], s_x0[TH], s_y0[TH];
    __shared__ __attribute__((aligned(16))) uint32_t tile[SBW * SBH];
    const WarpJob& j = a.j[blockIdx.z];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    if (x0 >= j.dw || y0 >= j.dh) return;                 // (workgroup-uniform)
    const int x1 = min(x0 + TW, j.dw) - 1, y1 = min(y0 + TH, j.dh) - 1;
    map_terms(j.m, x0, y0, x1, y1, tid, s_ad, s_bd, s_x0, s_y0);
    __syncthreads();
    // the tile's box from its corner terms, by emit_rows' expressions (m[1] = m[3] = 0: s_x0 is one value, s_bd is 0)
    const int bx0 = sat_s16(((s_x0[0] + s_ad[0]) >> 5) >> 5), bx1 = sat_s16(((s_x0[0] + s_ad[x1 - x0]) >> 5) >> 5);
    const int by0 = sat_s16(((s_y0[0] + s_bd[0]) >> 5) >> 5), by1 = sat_s16(((s_y0[y1 - y0] + s_bd[0]) >> 5) >> 5);
    // a lane's four pixels are one aligned load where the job's rows keep that alignment; k = the pixels between the aligned address
    // at or in front of the crop's first sample and that sample: the columns x with (x + k) % 4 == 0 are aligned
    const int pxb = j.cn * SB, lb = 4 * pxb;
    const bool rgb3 = RGB && j.cn == 3;
    const int aligned = rgb3 ? j.sstride % 4 == 0 : (uintptr_t)j.src % pxb == 0 && j.sstride % lb == 0;
    const int k = !aligned ? 0 : rgb3 ? (int)(-(uintptr_t)j.src & 3) : (int)((uintptr_t)j.src % lb) / pxb;
    const int bx0a = ((bx0 + k) & ~3) - k;
    const int bw = (bx1 + 2 - bx0a + 3) & ~3, bh = by1 + 2 - by0;
    WarpCore c;
    c.sstride = j.sstride; c.dstride = j.dstride;
    c.sw = j.sw; c.sh = j.sh; c.dw = j.dw; c.dh = j.dh;
    c.src_aligned = aligned;
    const int galign = SB == 2 ? 8 * j.cn : j.cn == 2 ? 8 : RGB && j.cn == 4 ? 16 : 4;        // (a lane's four pixels in one store; cn 3: three dwords)
    c.dst_aligned = ((uintptr_t)j.dst % galign == 0) && (j.dstride % galign == 0);
    c.border = j.border;
    if constexpr (RGB) {
        if (j.cn == 4) {
            scale_stage<4, 1>(j, tile, bx0a, by0, bw, bh, aligned, tid);
            __syncthreads();
            emit_rows<4, true>(c, j.src, j.dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
        } else {
            scale_stage<3, 1>(j, tile, bx0a, by0, bw, bh, aligned, tid);
            __syncthreads();
            emit_rows<3, true>(c, j.src, j.dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
        }
        return;
    }
    if (j.cn == 1) {
        scale_stage<1, SB>(j, tile, bx0a, by0, bw, bh, aligned, tid);
        __syncthreads();
        emit_rows<1, true, SB>(c, j.src, j.dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
    } else {
        scale_stage<2, SB>(j, tile, bx0a, by0, bw, bh, aligned, tid);
        __syncthreads();
        emit_rows<2, true, SB>(c, j.src, j.dst, tile, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, bx0a, by0, bw, tid);
    }
}

__global__ __launch_bounds__(NT) void scale_jobs_kernel(WarpJobsArg a) { scale_jobs_tile<1>(a); }
__global__ __launch_bounds__(NT) void scale_jobs16_kernel(WarpJobsArg a) { scale_jobs_tile<2>(a); }
__global__ __launch_bounds__(NT) void scale_jobs_rgb_kernel(WarpJobsArg a) { scale_jobs_tile<1, true>(a); }

// ---- tile building blocks shared by the table kernels ------------------------------------------------------------
constexpr int TABN = 2 * TW + 2 * TH;     // ints of coordinate terms per tile: ad[128] bd[128] x0[16] y0[16]

// Launch constants of a table kernel.
typedef const __attribute__((address_space(1))) int32_t* gtab_t;     // the tables are global memory (not generic: flat loads)
struct TabK {
    WarpCore c;
    gtab_t tabs;
    int tab_stride, tab_row, tab_ad;
    int gx, gy;
};

// swh / dwh: width | height << 16 of source and destination; flags: bit 0 / 1 source / destination aligned, bits 2 .. 4 the border
__device__ __forceinline__ WarpCore unpack_core(uint32_t sstride, uint32_t dstride, uint32_t swh, uint32_t dwh, uint32_t flags) {
    WarpCore c;
    c.sstride = sstride; c.dstride = dstride;
    c.sw = swh & 0xFFFFu; c.sh = swh >> 16; c.dw = dwh & 0xFFFFu; c.dh = dwh >> 16;
    c.src_aligned = flags & 1u; c.dst_aligned = (flags >> 1) & 1u; c.border = (flags >> 2) & 7u;
    return c;
}

struct TileIn {            // wave-uniform inputs of a tile
    const uint8_t* src;
    uint8_t* dst;
    int bz, x0, y0, x1, y1;
    int ad0, ad1, bd0, bd1, Xa, Xb, Ya, Yb;
};

struct TileBox { int bx0a, by0, bw, bh; bool fast, use_lds, interior, pre, slowcols; };

__device__ __forceinline__ TileBox tile_box(const WarpCore& c, const TileIn& t) {
    TileBox b;
    const int sx00 = (t.Xa + t.ad0) >> 10, sx01 = (t.Xa + t.ad1) >> 10, sx10 = (t.Xb + t.ad0) >> 10, sx11 = (t.Xb + t.ad1) >> 10;
    const int sy00 = (t.Ya + t.bd0) >> 10, sy01 = (t.Ya + t.bd1) >> 10, sy10 = (t.Yb + t.bd0) >> 10, sy11 = (t.Yb + t.bd1) >> 10;
    const int rx0 = min(min(sx00, sx01), min(sx10, sx11)), rx1 = max(max(sx00, sx01), max(sx10, sx11));
    const int ry0 = min(min(sy00, sy01), min(sy10, sy11)), ry1 = max(max(sy00, sy01), max(sy10, sy11));
    const bool saturated = rx0 < -32768 || ry0 < -32768 || rx1 > 32767 || ry1 > 32767;
    const int bx0 = max(rx0, -32768), bx1 = min(rx1, 32767) + 1;
    b.by0 = max(ry0, -32768);
    const int by1 = min(ry1, 32767) + 1;
    b.bx0a = bx0 & ~3;
    b.bw = (bx1 - b.bx0a + 1 + 3) & ~3;
    b.bh = by1 - b.by0 + 1;
    b.fast = !saturated && b.bw <= FDATA && b.bh <= FROWS;
    b.use_lds = b.fast || (!saturated && (long long)b.bw * b.bh <= LDS_PX);
    b.interior = b.fast && c.src_aligned && b.bx0a >= 0 && b.bx0a + b.bw <= c.sw && b.by0 >= 0 && b.by0 + b.bh <= c.sh &&
                 (b.bx0a + b.bw + 2 <= c.sw || b.by0 + b.bh < c.sh);
    // a box that leaves the image is staged with the same 16-byte loads (issue_tile); only its groups that straddle the
    // left / right image edge (when sw is no multiple of 4, or under BORDER_REPLICATE) are fetched pixel by pixel
    b.pre = b.fast && c.src_aligned && c.sw >= 8;
    b.slowcols = !b.interior && (b.bx0a < 0 || b.bx0a + b.bw + 2 > c.sw) && ((c.sw & 3) != 0 || c.border == VS_BORDER_REPLICATE);
    return b;
}

struct TilePre { U4 d[SPASS]; int tv0, tv1; };     // staging loads of a tile and its share of the tables, in flight

// This lane's share of the tile's coordinate terms: (ad, bd) of a column for the first 128 lanes, (X0, Y0) of a row for
// the next 16.  Columns and rows past the image repeat the last one.
__device__ __forceinline__ void load_terms(const TabK& k, const TileIn& t, int tid, int& tv0, int& tv1) {
    gtab_t Tg = k.tabs + (size_t)t.bz * k.tab_stride + k.tab_ad;
    if (tid < TW) {
        const int c = min(t.x0 + tid, t.x1);
        tv0 = Tg[c]; tv1 = Tg[k.c.dw + c];
    } else if (tid < TW + TH) {
        const int r = min(t.y0 + (tid - TW), t.y1);
        tv0 = Tg[2 * k.c.dw + r]; tv1 = Tg[2 * k.c.dw + k.c.dh + r];
    }
}

// (subx, suby): the origin of the staged box in 1/1024 px, taken off the row terms of a fast tile so that the blend's tap
// address is relative to the staged tile.
__device__ __forceinline__ void store_terms(int* tab, int tid, int tv0, int tv1, int subx = 0, int suby = 0) {
    if (tid < TW) { tab[tid] = tv0; tab[TW + tid] = tv1; }
    else if (tid < TW + TH) { tab[2 * TW + (tid - TW)] = tv0 - subx; tab[2 * TW + TH + (tid - TW)] = tv1 - suby; }
}

// Staging loads of a fast tile.  ONE load instruction per pass for every kind of tile (interior tiles and tiles that
// leave the image run the same straight code, no per-pixel checked loads at the image border): 16 bytes per lane,
// from an address that depends on the lane's group class at the image border
//   0  inside the row                 its own 16 bytes: four pixels and the B of the next one
//   1  the row's last four pixels     the 16 bytes that END with the row: the pixels are dwords b, c, d
//   4  the group left of the image    the row's first 16 bytes: the staged dword of pixel -1 carries the B of pixel 0
//   2  outside (BORDER_CONSTANT)      the row's first 16 bytes (not used)
//   3  straddles the edge             the row's first 16 bytes (not used): fetched pixel by pixel when stored
// and store_tile shifts the registers into place once they have landed.  Interior tiles are class 0 throughout.
__device__ __forceinline__ int edge_class(const WarpCore& c, int cg, bool row_ok) {
    if (!row_ok) return 2;
    if (cg >= 0 && cg + 6 <= c.sw) return 0;
    if (cg >= 0 && cg + 4 == c.sw) return 1;
    if (c.border != VS_BORDER_REPLICATE) {
        if (cg == -4) return 4;
        if (cg + 3 < 0 || cg >= c.sw) return 2;
    }
    return 3;
}

__device__ __forceinline__ void issue_tile(const TabK& k, const TileIn& t, const TileBox& b, int tid, TilePre& pf) {
    const int ly = tid / SG, lx = tid - ly * SG;
    if (tid < SG * SR && 4 * lx < b.bw) {
        const int cg = b.bx0a + 4 * lx;
        const uint32_t stride32 = (uint32_t)k.c.sstride;
        uint32_t off[SPASS];
        if (b.interior) {
            const uint32_t col = 3u * (uint32_t)cg;
#pragma unroll
            for (int q = 0; q < SPASS; q++) off[q] = __umul24((uint32_t)(b.by0 + min(ly + SR * q, b.bh - 1)), stride32) + col;
        } else {
#pragma unroll
            for (int q = 0; q < SPASS; q++) {
                const int r = b.by0 + min(ly + SR * q, b.bh - 1);
                const int rc = min(max(r, 0), k.c.sh - 1);                       // BORDER_REPLICATE: the nearest row
                const int cls = edge_class(k.c, cg, r == rc || k.c.border == VS_BORDER_REPLICATE);
                off[q] = __umul24((uint32_t)rc, stride32) + (cls == 0 ? 3u * (uint32_t)cg : (cls == 1 ? 3u * (uint32_t)cg - 4u : 0u));
            }
        }
#pragma unroll
        for (int q = 0; q < SPASS; q++)
            if (SR * q < b.bh) pf.d[q] = *reinterpret_cast<const U4*>(t.src + off[q]);
    }
}

__device__ __forceinline__ void store_tile(const TabK& k, const TileIn& t, const TileBox& b, int tid, const TilePre& pf, uint32_t* tile, int* tab) {
    const int ly = tid / SG, lx = tid - ly * SG;
    if (tid < SG * SR && 4 * lx < b.bw) {
        const int cg = b.bx0a + 4 * lx;
#pragma unroll
        for (int q = 0; q < SPASS; q++) {
            if (SR * q < b.bh && (SR * (q + 1) <= FROWS || ly + SR * q < FROWS)) {
                U4 d = pf.d[q];
                int cls = 0, r = 0;
                if (!b.interior) {
                    r = b.by0 + min(ly + SR * q, b.bh - 1);
                    const int rc = min(max(r, 0), k.c.sh - 1);
                    cls = edge_class(k.c, cg, r == rc || k.c.border == VS_BORDER_REPLICATE);
                    if (cls == 1) {                  // loaded 4 bytes early: the pixels are b, c, d; right of the last one is the border
                        d.a = d.b; d.b = d.c; d.c = d.d;
                        d.d = k.c.border == VS_BORDER_REPLICATE ? (d.c >> 8) & 0xFFu : 0u;
                    } else if (cls == 4) {           // pixels -4 .. -1: zeros, and the B of pixel 0
                        d.d = d.a; d.a = 0u; d.b = 0u; d.c = 0u;
                    } else if (cls != 0) { d.a = 0u; d.b = 0u; d.c = 0u; d.d = 0u; }
                }
                uint4 e = make_uint4(__builtin_amdgcn_perm(d.a, d.a, 0x02010300u), __builtin_amdgcn_perm(d.b, d.a, 0x05040603u),
                                     __builtin_amdgcn_perm(d.c, d.b, 0x04030502u), __builtin_amdgcn_perm(d.d, d.c, 0x03020401u));
                if (b.slowcols && cls == 3) {
                    uint32_t px[5];
#pragma unroll
                    for (int i = 0; i < 5; i++) px[i] = load_px_checked<3>(t.src, k.c.sstride, k.c.sw, k.c.sh, cg + i, r, k.c.border);
                    e = make_uint4(pair_b(px[0], px[1]), pair_b(px[1], px[2]), pair_b(px[2], px[3]), pair_b(px[3], px[4]));
                }
                *reinterpret_cast<uint4*>(&tile[(ly + SR * q) * FPITCH + 4 * lx]) = e;
            }
        }
    }
    store_terms(tab, tid, pf.tv0, pf.tv1, b.bx0a << 10, b.by0 << 10);
}

// XCD-aware tile order (xcd_seq, vs_common.h).  The hardware hands consecutive workgroups to the 8 XCDs in turn (linear id mod 8), and every XCD has
// an L2 of its own: with the plain (x, y, frame) order the eight neighbours of a tile row sit on eight different XCDs, and every
// 128-byte line that two tiles share (the box of a tile is 144 / 408 bytes wide at an arbitrary 4- / 12-byte offset, plus the halo
// rows above and below) is fetched once per XCD - read traffic of 2.28 x (planes) and 1.60 x (BGR) the algorithmic bytes at the
// L2's memory side (FETCH_SIZE, profiles/r03_a).  Here XCD c takes the c-th contiguous eighth of the launch's tiles in
// (frame, tile row, tile column) order instead: neighbours in x and y meet in one L2.  flags bit 8 selects it.
struct TileId { int x, y, z; };
// (gx, gy follow from the frame size, the frame count travels in flags bits 16.. - gridDim would be one more scalar load in
// front of the table loads - and the two divisions are multiplications by reciprocals the host provides: mgx = ceil(2^32 / gx),
// exact while seq * gx < 2^32, which the launcher checks before it sets the flag)
__device__ __forceinline__ TileId tile_id(uint32_t flags, uint32_t gx, uint32_t gy, uint32_t mgx, uint32_t mgy) {
    TileId t;
    if (!(flags & 0x100u)) { t.x = blockIdx.x; t.y = blockIdx.y; t.z = blockIdx.z; return t; }
    const uint32_t n = gx * gy * (flags >> 16);
    const uint32_t lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const uint32_t seq = xcd_seq(lin, n);
    const uint32_t row = gx == 1 ? seq : __umulhi(seq, mgx);       // (ceil(2^32 / 1) does not fit 32 bits)
    t.x = (int)(seq - row * gx);
    t.z = (int)(gy == 1 ? row : __umulhi(row, mgy));
    t.y = (int)(row - (uint32_t)t.z * gy);
    return t;
}

// ---- one tile per workgroup, everything the prologue needs in 10 dwords of kernel arguments -------------------
// gfx950 preloads the leading kernel arguments (up to 14 dwords) into scalar registers when the wave is launched
// (k_warp.hip is built with -mllvm -amdgpu-kernarg-preload-count=16), so the two scalar loads of the tile's inputs
// (frame pointers + column terms, row terms) go out with the first instructions: ONE round trip in front of the staging
// loads.  (Measured with s_memtime stamps: an argument that is not preloaded, or an input that is fetched by a third
// load later on, each cost another ~1000 cycles of a workgroup's ~9000.)  Staging through issue_tile / store_tile: tiles that leave the image take the same
// 16-byte loads as interior ones.
__global__ __launch_bounds__(NT, 8) void warp_tab_kernel(gtab_t tabs, int tab_stride, int tab_row, int tab_ad, uint32_t sstride, uint32_t dstride,
                                                      uint32_t swh, uint32_t dwh, uint32_t flags, uint32_t mgx, uint32_t mgy) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[LDS_PX];
    __shared__ __attribute__((aligned(16))) uint32_t obuf[OBUF];
    __shared__ int s_tab[TABN];
    __shared__ __attribute__((aligned(16))) uint8_t lut[32 * LUT_STRIDE];
    typedef const __attribute__((address_space(4))) int32_t* cptr;
    typedef __attribute__((address_space(1))) uint8_t* gptr;
    const int tid = threadIdx.x;
    TabK k;
    k.c = unpack_core(sstride, dstride, swh, dwh, flags);
    k.tabs = tabs; k.tab_stride = tab_stride; k.tab_row = tab_row; k.tab_ad = tab_ad;
    k.gx = (k.c.dw + TW - 1) / TW; k.gy = (k.c.dh + TH - 1) / TH;
    TileIn cur;
    const TileId tq = tile_id(flags, (uint32_t)(k.c.dw + TW - 1) / TW, (uint32_t)(k.c.dh + TH - 1) / TH, mgx, mgy);
    {
        cptr Ts = (cptr)(const int32_t*)(tabs + (size_t)tq.z * tab_stride);
        // one 32-byte and one 16-byte scalar load, issued together (as separate loads the compiler moves the frame
        // pointers down to their first use: a third round trip in front of the staging loads)
        typedef int32_t i32x8 __attribute__((ext_vector_type(8)));
        typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
        const i32x8 cc = *(const __attribute__((address_space(4))) i32x8*)(Ts + TAB_COL * tq.x);
        const i32x4 cr = *(const __attribute__((address_space(4))) i32x4*)(Ts + tab_row + 4 * tq.y);
        cur.src = (const uint8_t*)(gptr)((unsigned long long)(uint32_t)cc[0] | (unsigned long long)(uint32_t)cc[1] << 32);
        cur.dst = (uint8_t*)(gptr)((unsigned long long)(uint32_t)cc[2] | (unsigned long long)(uint32_t)cc[3] << 32);
        cur.ad0 = cc[4]; cur.ad1 = cc[5]; cur.bd0 = cc[6]; cur.bd1 = cc[7];
        cur.Xa = cr[0]; cur.Xb = cr[1]; cur.Ya = cr[2]; cur.Yb = cr[3];
        cur.bz = tq.z; cur.x0 = tq.x * TW; cur.y0 = tq.y * TH;
        cur.x1 = min(cur.x0 + TW, k.c.dw) - 1; cur.y1 = min(cur.y0 + TH, k.c.dh) - 1;
    }
    if (tid >= NT - 32) {      // weight table of the fast path (see blend3_fast)
        const uint32_t f = tid - (NT - 32);
        const uint32_t wlo = (32u - f) | (f << 8);
        *reinterpret_cast<uint4*>(lut + f * LUT_STRIDE) =
            make_uint4(wlo, wlo << 16, __float_as_uint((float)(32u - f) * 0x1p121f), __float_as_uint((float)f * 0x1p121f));
    }
    // this lane's share of the tile's coordinate terms does not depend on the box: requested while the scalar loads travel
    TilePre pf;
    pf.tv0 = 0; pf.tv1 = 0;
    load_terms(k, cur, tid, pf.tv0, pf.tv1);
    const TileBox cb = tile_box(k.c, cur);
    if (cb.pre) {
        issue_tile(k, cur, cb, tid, pf);
        store_tile(k, cur, cb, tid, pf, tile, s_tab);
    } else {
        const int tv0 = pf.tv0, tv1 = pf.tv1;
        if (cb.use_lds) {
            const int pitch = cb.fast ? FPITCH : cb.bw;
            const int gpr = cb.bw >> 2;
            const int total = gpr * cb.bh;
            for (int g = tid; g < total; g += NT) {
                const int row = g / gpr, gxx = g - row * gpr;
                uint4 px = stage_group<3>(k.c, cur.src, cb.bx0a + 4 * gxx, cb.by0 + row);
                if (cb.fast) {
                    const uint32_t nx = load_px_checked<3>(cur.src, k.c.sstride, k.c.sw, k.c.sh, cb.bx0a + 4 * gxx + 4, cb.by0 + row, k.c.border);
                    px = make_uint4(pair_b(px.x, px.y), pair_b(px.y, px.z), pair_b(px.z, px.w), pair_b(px.w, nx));
                }
                *reinterpret_cast<uint4*>(&tile[row * pitch + 4 * gxx]) = px;
            }
        }
        store_terms(s_tab, tid, tv0, tv1, cb.fast ? cb.bx0a << 10 : 0, cb.fast ? cb.by0 << 10 : 0);
    }
    __syncthreads();
    if (cb.fast) emit_fast(k.c, cur.dst, tile, obuf, lut, s_tab, s_tab + TW, s_tab + 2 * TW, s_tab + 2 * TW + TH, cur.x0, cur.y0, cur.x1, cur.y1, 0, tid);
    else if (cb.use_lds) emit_rows<3, true>(k.c, cur.src, cur.dst, tile, s_tab, s_tab + TW, s_tab + 2 * TW, s_tab + 2 * TW + TH, cur.x0, cur.y0, cur.x1,
                                            cur.y1, cb.bx0a, cb.by0, cb.bw, tid);
    else emit_rows<3, false>(k.c, cur.src, cur.dst, tile, s_tab, s_tab + TW, s_tab + 2 * TW, s_tab + 2 * TW + TH, cur.x0, cur.y0, cur.x1, cur.y1,
                             cb.bx0a, cb.by0, cb.bw, tid);
}

// ---- one- and two-channel planes of batched launches (NV12: Y and interleaved UV) ------------------------------------
// The BGR table kernel above owes its rate to what a workgroup carries through its latency chain (scalar prologue ->
// staging loads -> barrier -> blend): 6 KB of output.  A 128 x 16 tile of a Y plane is 2 KB, of a UV plane 4 KB, and the general
// kernel stages them as one dword per pixel with per-group checks: 0.22 of the HBM peak at 3840 x 2160.  This kernel gives a
// plane workgroup 8 KB of output - 128 x 64 pixels of one channel, 128 x 32 of two - and stages the source box as BYTES
// (row pitch 144 / 288, at most 73 / 41 rows: 10.5 / 11.8 KB, eight workgroups per CU):
//   staging   16-byte chunks, vector loads for chunks inside the frame, per-byte checked loads (zeros outside:
//             BORDER_CONSTANT) for the few that cross its edge;
//   taps      the two horizontal taps of a pixel are adjacent in the staged row: an 8-byte LDS read at the 4-byte
//             aligned address below them and one v_alignbyte put [p(x), p(x+1)] (or [U0 V0 U1 V1]) into the low bytes of a
//             dword, for the upper and the lower tap row;
//   blend     v_dot4 against ((32-f) | f << 8) (one channel) or ((32-f) | f << 16, and << 8 for V) = the weights as one
//             multiply-add of f; vertical lerp in fp32 on denormals as in the BGR kernel;
//   output    lane L of a 32-lane row takes the consecutive pixels 4L .. 4L+3 (with a byte-wide box neighbouring lanes then
//             read neighbouring LDS dwords) and stores its 4 / 8 bytes.
// It shares the per-frame coordinate tables with the other kernels (the tables know tiles of 16 rows: the corner terms of
// a taller tile come from the records of its first and last 16 rows).  A box that does not fit the staging area (large
// rotations or zooms) takes emit_rows' direct path, 16 rows at a time.
// A 16-byte chunk of a source row that straddles the row's left or right end (byte column xb .. xb + 15, row of `rowbytes`
// bytes at rowp): zeros outside.  All loads unconditional, from clamped addresses, so that they travel together (under
// conditions the compiler waits for each of sixteen byte loads in turn: 16 round trips for a tile at the frame's edge).
__device__ __forceinline__ uint4 load_chunk_straddling(const uint8_t* rowp, int xb, int rowbytes, bool dwords) {
    uint32_t w[4];
    if (dwords) {            // row start and row length multiples of 4: a dword is inside or outside as a whole
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int xq = xb + 4 * q;
            const bool in = xq >= 0 && xq + 4 <= rowbytes;
            const uint32_t v = *reinterpret_cast<const uint32_t*>(rowp + (in ? xq : 0));
            w[q] = in ? v : 0u;
        }
    } else {                 // four bytes at a time (a rolled loop: sixteen loads in flight would cost the callers their registers)
        uint32_t wq[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int xx = xb + 4 * q + k;
                const uint32_t v = rowp[min(max(xx, 0), rowbytes - 1)];
                wq[q] |= (xx >= 0 && xx < rowbytes ? v : 0u) << (8 * k);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = wq[q];
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The same chunk under VS_BORDER_FILL: the row's bytes inside, the bytes of `pat` outside.  pat: the plane's fill as one dword (F x 4,
// (U, V) x 2, F16 x 2 or (U16, V16)); a chunk starts at a multiple of 4 pixels, so byte k of a chunk's dword is byte k of the pattern.
__device__ __forceinline__ uint4 load_chunk_straddling_fill(const uint8_t* rowp, int xb, int rowbytes, bool dwords, uint32_t pat) {
    uint32_t w[4];
    if (dwords) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int xq = xb + 4 * q;
            const bool in = xq >= 0 && xq + 4 <= rowbytes;
            const uint32_t v = *reinterpret_cast<const uint32_t*>(rowp + (in ? xq : 0));
            w[q] = in ? v : pat;
        }
    } else {                 // unaligned rows, or a row length that is no multiple of 4: byte by byte (rolled, as above)
        uint32_t wq[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const uint32_t fb = (pat >> (8 * k)) & 0xFFu;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int xx = xb + 4 * q + k;
                const uint32_t v = rowp[min(max(xx, 0), rowbytes - 1)];
                wq[q] |= (xx >= 0 && xx < rowbytes ? v : fb) << (8 * k);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = wq[q];
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The same chunk under BORDER_REPLICATE (remapBilinear's clip()): a byte outside the row is the byte of the same channel of the
// row's first / last pixel.  (Chunks of tiles at the picture's edge only.)
// CN: the BYTES of a pixel (1, 2 or 4) - the channels of an 8-bit plane, or one / two 16-bit samples (P010 luma / chroma: a byte outside the
// row is the byte of the same sample at the same place in the edge pixel).
template <int CN>
__device__ __forceinline__ uint4 load_chunk_replicate(const uint8_t* rowp, int xb, int sw) {
    uint32_t wq[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int xx = xb + 4 * q + k;
            const int px = min(max(CN == 1 ? xx : CN == 2 ? xx >> 1 : xx >> 2, 0), sw - 1);     // (CN = 1, 2 or 4)
            wq[q] |= (uint32_t)rowp[CN == 1 ? px : CN * px + (xx & (CN - 1))] << (8 * k);
        }
    }
    return make_uint4(wq[0], wq[1], wq[2], wq[3]);
}

// SB = 2: planes of 16-bit samples (P010).  The tables and the box stay in pixels; a pixel is PXB = CN * SB bytes, and the tile shape,
// the staged box and the LDS budget follow from PXB alone: 16-bit luma (2 bytes) as the 8-bit two-channel plane - 128 x 32 pixels,
// rows of 384 bytes, 41 of them, 15.4 KiB -, 16-bit chroma (4 bytes) as the four-channel plane - 128 x 16, 640 x 25, 15.6 KiB: eight
// workgroups per CU as before.
template <int CN, int SB = 1> struct PlaneCfg {
    static constexpr int PXB = CN * SB;                  // bytes of a pixel
    static constexpr int THP = 64 / PXB;                 // rows of a tile (four bytes per pixel: 16, the rows of a table record)
    static constexpr int DB = 136 * PXB + 8 * PXB;       // staged bytes of a row (136 pixels + slack for the 8-byte tap read)
    // Row pitch of the staged box: a multiple of 128 bytes = of the 32 LDS banks.  The lanes of a tap read sit on consecutive dwords
    // of a row until the map's rotation moves them a source row down (or up), once per tile row for anything but a pure
    // translation; with a pitch of 144 bytes those lanes land 4 banks to the side, on banks their neighbours use, and every tap
    // read pays a second pass.  With this pitch a lane's bank does not depend on its row.  (scratch/blend_lab.sh: the tap reads
    // were 66 of the kernel's 209 us per 32 4K frames.)
    static constexpr int PB = (DB + 127) / 128 * 128;    // 256 / 384 / 640
    static constexpr int ROWS = THP + 9;                 // staged rows (rotations up to ~3.5 degrees)
    static constexpr int CPR = DB / 16;                  // 16-byte chunks per staged row
};

// Output of a staged plane tile: lane L of a 32-lane row takes the four CONSECUTIVE pixels 4L .. 4L+3 of rows ty, ty + 8, ...: with
// the box staged as bytes that puts neighbouring lanes on neighbouring LDS dwords, and the lane's four results are its 4 / 8
// output bytes.  tl: the staged box (row pitch PB), the terms relative to it: ad / bd of the lane's columns, s_x0 / s_y0 of the
// tile's rows.  Written for few instructions: the taps are dword reads (the address is a multiple of 4, not of 8, and an 8-byte LDS
// read off its alignment is some 20 x slower) shifted into place by v_alignbyte, which takes its byte count from the low two
// bits of the tap address as it is; the weights of both lerps come from the table; and for the common tile - whole, aligned -
// the rows are unrolled and the store address is a lane offset computed once plus a base that moves from row to row.
// What the measurements of round 3 say about it (same-box pairs, scratch/ab_lib.sh): with the row pitch
// of PlaneCfg the LDS reads no longer show (a build without them is no faster), the kernel's time does not move between 4
// and 8 waves per SIMD, and the staging loads plus the stores alone take 105 of the luma kernel's 133 us - a copy of the
// same bytes takes 95.
// One output pixel of a staged plane tile -> its value(s) in bytes 0 (Y) / 0, 1 (U, V) of the result.  Vertical lerp as in the BGR
// kernel (vlerp: three float operations of the 2-cycle class on the integer sums read as denormals).  (Measured against it on one
// box, scratch/ab_lib.sh: the integer form - t | b << 16 against (64 (32 - f), 64 f) in one v_dot2_u32_u16 preset to 2^15, result
// in byte 2: one instruction and 4 bytes of LDS weights less per pixel, bit-identical - 204 us against 198: its two
// instructions are of the 4-cycle class, scratch/valu_rate.hip.)
// Four channels (BGRA8 / RGBA8): a pixel is a dword of the staged row, so the four taps are aligned dword reads; the horizontal
// lerps pair the same channel of the two taps of a row with v_perm - (c0, c0', c1, c1') and (c2, c2', c3, c3') - and take v_dot4
// against the table's wlo (channels 0, 2) and whi (1, 3); the vertical lerp is vlerp's, and the four results' low bytes are
// packed into one dword.
__device__ __forceinline__ uint32_t plane_blend_px4(const uint8_t* tl, const uint8_t* lut, int SX, int SY) {
    typedef PlaneCfg<4> P;
    const int addr = __mul24(SY >> 10, P::PB) + ((SX >> 10) << 2);
    const uint32_t* tp = reinterpret_cast<const uint32_t*>(tl + addr);
    const uint32_t p00 = tp[0], p01 = tp[1], p10 = tp[P::PB / 4], p11 = tp[P::PB / 4 + 1];
    const LutX wx = *reinterpret_cast<const LutX*>(lut + (SX & 0x3E0));
    const LutY wy = *reinterpret_cast<const LutY*>(lut + 8 + (SY & 0x3E0));
    const uint32_t t01 = __builtin_amdgcn_perm(p01, p00, 0x05010400u), b01 = __builtin_amdgcn_perm(p11, p10, 0x05010400u);
    const uint32_t t23 = __builtin_amdgcn_perm(p01, p00, 0x07030602u), b23 = __builtin_amdgcn_perm(p11, p10, 0x07030602u);
    float m0 = vlerp(__builtin_amdgcn_udot4(t01, wx.wlo, 0u, false), __builtin_amdgcn_udot4(b01, wx.wlo, 0u, false), wy);
    float m1 = vlerp(__builtin_amdgcn_udot4(t01, wx.whi, 0u, false), __builtin_amdgcn_udot4(b01, wx.whi, 0u, false), wy);
    float m2 = vlerp(__builtin_amdgcn_udot4(t23, wx.wlo, 0u, false), __builtin_amdgcn_udot4(b23, wx.wlo, 0u, false), wy);
    float m3 = vlerp(__builtin_amdgcn_udot4(t23, wx.whi, 0u, false), __builtin_amdgcn_udot4(b23, wx.whi, 0u, false), wy);
    asm("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3));
    const uint32_t lo = __builtin_amdgcn_perm(__float_as_uint(m1), __float_as_uint(m0), 0x0C0C0400u);    // (c0, c1, 0, 0)
    const uint32_t hi = __builtin_amdgcn_perm(__float_as_uint(m3), __float_as_uint(m2), 0x0C0C0400u);    // (c2, c3, 0, 0)
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

template <int CN>
__device__ __forceinline__ uint32_t plane_blend_px(const uint8_t* tl, const uint8_t* lut, int SX, int SY) {
    typedef PlaneCfg<CN> P;
    if (CN == 4) return plane_blend_px4(tl, lut, SX, SY);
    int addr;                                                     // byte of the upper-left tap: row * PB + column * CN
    if (P::PB == 256 && CN == 1) {          // (one shift-add; left to itself the compiler makes shift, mask, add of it)
        const int sy = SY >> 10, sx = SX >> 10;
        asm("v_lshl_add_u32 %0, %1, 8, %2" : "=v"(addr) : "v"(sy), "v"(sx));
    } else {
        addr = __mul24(SY >> 10, P::PB) + (SX >> 10) * CN;
    }
    const uint32_t* tp = reinterpret_cast<const uint32_t*>(tl + (addr & ~3));
    const uint32_t top = __builtin_amdgcn_alignbyte(tp[1], tp[0], (uint32_t)addr), bot = __builtin_amdgcn_alignbyte(tp[P::PB / 4 + 1], tp[P::PB / 4], (uint32_t)addr);
    const LutY wy = *reinterpret_cast<const LutY*>(lut + 8 + (SY & 0x3E0));
    const uint32_t wx = *reinterpret_cast<const uint32_t*>(lut + (CN == 1 ? 0 : 16) + (SX & 0x3E0));   // (32 - fx) | fx << 8  /  (32 - fx) | fx << 16
    if (CN == 1) {
        float m = vlerp(__builtin_amdgcn_udot4(top, wx, 0u, false), __builtin_amdgcn_udot4(bot, wx, 0u, false), wy);
        asm("" : "+v"(m));            // (keeps the pixels' float operations apart: the packed f32 forms need moves and are no faster)
        return __float_as_uint(m);
    }
    const uint32_t wv = wx << 8;                                  // wx against bytes 0 and 2 (U0, U1), wv against bytes 1 and 3 (V0, V1)
    float mu = vlerp(__builtin_amdgcn_udot4(top, wx, 0u, false), __builtin_amdgcn_udot4(bot, wx, 0u, false), wy);
    float mv = vlerp(__builtin_amdgcn_udot4(top, wv, 0u, false), __builtin_amdgcn_udot4(bot, wv, 0u, false), wy);
    asm("" : "+v"(mu), "+v"(mv));
    return __builtin_amdgcn_perm(__float_as_uint(mv), __float_as_uint(mu), 0x0C0C0400u);     // (U, V, 0, 0)
}

// 16-bit samples.  Luma: the two horizontal taps are four adjacent bytes at a 2-byte aligned address: two dword reads and one
// v_alignbyte give [p(x), p(x+1)] as the halves of a dword.  Chroma: a pixel (U, V) is an aligned dword; v_perm pairs the U halves and the
// V halves of the two taps.  Horizontal lerp: v_dot2_u32_u16 against (32 - fx) | fx << 16 from the weight table; vertical lerp and
// rounding in integers (vlerp16).  Result: the sample in the low half (luma) / (U, V) as the halves (chroma).
template <int CN>
__device__ __forceinline__ uint32_t plane_blend_px16(const uint8_t* tl, const uint8_t* lut, int SX, int SY) {
    typedef PlaneCfg<CN, 2> P;
    const int addr = __mul24(SY >> 10, P::PB) + (SX >> 10) * P::PXB;
    const uint32_t* tp = reinterpret_cast<const uint32_t*>(tl + (addr & ~3));
    const uint32_t wx = *reinterpret_cast<const uint32_t*>(lut + 16 + (SX & 0x3E0));   // (32 - fx) | fx << 16
    const uint32_t fy = ((uint32_t)SY >> 5) & 31u;
    if (CN == 1) {
        const uint32_t top = __builtin_amdgcn_alignbyte(tp[1], tp[0], (uint32_t)addr), bot = __builtin_amdgcn_alignbyte(tp[P::PB / 4 + 1], tp[P::PB / 4], (uint32_t)addr);
        return vlerp16(hlerp16(top, wx), hlerp16(bot, wx), fy);
    }
    const uint32_t p00 = tp[0], p01 = tp[1], p10 = tp[P::PB / 4], p11 = tp[P::PB / 4 + 1];
    const uint32_t u = vlerp16(hlerp16(__builtin_amdgcn_perm(p01, p00, 0x05040100u), wx), hlerp16(__builtin_amdgcn_perm(p11, p10, 0x05040100u), wx), fy);
    const uint32_t v = vlerp16(hlerp16(__builtin_amdgcn_perm(p01, p00, 0x07060302u), wx), hlerp16(__builtin_amdgcn_perm(p11, p10, 0x07060302u), wx), fy);
    return u | (v << 16);
}

template <int CN, int SB = 1>
__device__ __forceinline__ void plane_store4(uint8_t* dq, const uint32_t (&res)[4]) {       // four pixels = 4 / 8 / 16 aligned bytes
    if (SB == 2) {
        if (CN == 1) {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            __builtin_nontemporal_store(u32x2{res[0] | (res[1] << 16), res[2] | (res[3] << 16)}, reinterpret_cast<u32x2*>(dq));
        } else {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(u32x4{res[0], res[1], res[2], res[3]}, reinterpret_cast<u32x4*>(dq));
        }
    } else if (CN == 1) {
        const uint32_t lo = __builtin_amdgcn_perm(res[1], res[0], 0x0C0C0400u), hi = __builtin_amdgcn_perm(res[3], res[2], 0x0C0C0400u);   // low bytes
        __builtin_nontemporal_store(__builtin_amdgcn_perm(hi, lo, 0x05040100u), reinterpret_cast<uint32_t*>(dq));
    } else if (CN == 4) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(u32x4{res[0], res[1], res[2], res[3]}, reinterpret_cast<u32x4*>(dq));
    } else {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(u32x2{res[0] | (res[1] << 16), res[2] | (res[3] << 16)}, reinterpret_cast<u32x2*>(dq));
    }
}

template <int CN, int SB>
__device__ __forceinline__ uint32_t plane_px(const uint8_t* tl, const uint8_t* lut, int SX, int SY) {
    if constexpr (SB == 2) return plane_blend_px16<CN>(tl, lut, SX, SY);
    else return plane_blend_px<CN>(tl, lut, SX, SY);
}

template <int CN, int SB = 1>
__device__ __forceinline__ void plane_blend_rows(const WarpCore& c, const uint8_t* tl, const uint8_t* lut, const int2* s_row,
                                                 const int (&ad)[4], const int (&bd)[4], int L, int ty, uint8_t* dst, uint32_t dstride,
                                                 int x0, int y0, int x1, int y1) {
    typedef PlaneCfg<CN, SB> P;
    constexpr int NR = P::THP / TYN;
    uint8_t* const dtile = dst + (size_t)y0 * dstride + (size_t)x0 * P::PXB;      // wave-uniform base, 32-bit lane offsets
    if (c.dst_aligned && x1 - x0 == TW - 1 && y1 - y0 == P::THP - 1) {         // (tile-uniform)
        const uint32_t voff = __umul24((uint32_t)ty, dstride) + (uint32_t)(4 * P::PXB) * L;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int2 XY = s_row[ty + TYN * r];
            uint32_t res[4];
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = plane_px<CN, SB>(tl, lut, XY.x + ad[i], XY.y + bd[i]);
            plane_store4<CN, SB>(dtile + (size_t)(TYN * r) * dstride + voff, res);
        }
        return;
    }
    const int x = x0 + 4 * L;
    for (int r = 0; r < NR; r++) {
        const int yl = ty + TYN * r;
        const int2 XY = s_row[ty + TYN * r];
        const int X0 = XY.x, Y0 = XY.y;
        uint32_t res[4];
#pragma unroll
        for (int i = 0; i < 4; i++) res[i] = plane_px<CN, SB>(tl, lut, X0 + ad[i], Y0 + bd[i]);
        const int y = y0 + yl;
        if (y > y1 || x > x1) continue;
        uint8_t* dp = dst + (size_t)y * c.dstride + (size_t)x * P::PXB;
        if (c.dst_aligned && x + 3 <= x1) { plane_store4<CN, SB>(dp, res); continue; }
        for (int i = 0; i < 4; i++) {
            if (x + i > x1) break;
            for (int k = 0; k < CN; k++) {
                if (SB == 2) reinterpret_cast<uint16_t*>(dp)[i * CN + k] = (uint16_t)(res[i] >> (16 * k));
                else dp[i * CN + k] = (uint8_t)(res[i] >> (8 * k));     // (one channel: the low byte of the float's bits)
            }
        }
    }
}

// The terms of a tile of ROWS rows from the plane's table Tg into s_tab - ad[128] bd[128] x0[ROWS] y0[ROWS] -, for the direct paths
// below.  Columns and rows past the plane repeat the last one.
template <int ROWS>
__device__ __forceinline__ void stage_terms(const WarpCore& c, gtab_t Tg, int* s_tab, int x0, int y0, int x1, int y1, int tid) {
    if (tid < TW) {
        const int cx = min(x0 + tid, x1);
        s_tab[tid] = Tg[cx]; s_tab[TW + tid] = Tg[c.dw + cx];
    } else if (tid < TW + ROWS) {
        const int r = min(y0 + (tid - TW), y1);
        s_tab[2 * TW + (tid - TW)] = Tg[2 * c.dw + r]; s_tab[2 * TW + ROWS + (tid - TW)] = Tg[2 * c.dw + c.dh + r];
    }
}

// A plane tile whose source box does not fit the staging area (large rotations, zooms, saturated coordinates, BORDER_REPLICATE): the
// general path without staging (emit_rows works on 16 rows, terms as arrays: they go where the box would be).  Not inlined: as
// part of the kernel body it costs the common path its eighth wave per SIMD or register spills.
// (OWN: a copy of its own for the kernel that names it.  A noinline callee that two kernels share changes the register allocation of
// both, so the instances that came later - 16-bit BORDER_REPLICATE per subsampling: copies 1 .. 4, the taller 4:2:2 box: copy 8 - each
// call their own, and the earlier kernels keep their code.)
template <int CN, int SB = 1, int OWN = 0>
__device__ __attribute__((noinline)) void plane_direct_tile(WarpCore c, const uint8_t* src, uint8_t* dst, gtab_t Tg, int* s_tab, int x0, int y0, int x1, int y1,
                                                            int bx0a, int by0, int bw, int tid) {
    typedef PlaneCfg<CN, SB> P;
    stage_terms<P::THP>(c, Tg, s_tab, x0, y0, x1, y1, tid);
    __syncthreads();
    for (int j = 0; y0 + TH * j <= y1; j++)
        emit_rows<CN, false, SB>(c, src, dst, nullptr, s_tab, s_tab + TW, s_tab + 2 * TW + TH * j, s_tab + 2 * TW + P::THP + TH * j, x0, y0 + TH * j, x1,
                             min(y0 + TH * j + TH - 1, y1), bx0a, by0, bw, tid);
}

// The direct path of the VS_BORDER_FILL kernels: plane_direct_tile with the fill pixel (one copy per kernel: OWN).
template <int CN, int SB, int OWN>
__device__ __attribute__((noinline)) void plane_direct_tile_fill(WarpCore c, const uint8_t* src, uint8_t* dst, gtab_t Tg, int* s_tab, int x0, int y0, int x1, int y1,
                                                                 int tid, uint32_t fillpx) {
    typedef PlaneCfg<CN, SB> P;
    stage_terms<P::THP>(c, Tg, s_tab, x0, y0, x1, y1, tid);
    __syncthreads();
    for (int j = 0; y0 + TH * j <= y1; j++)
        emit_rows<CN, false, SB, true>(c, src, dst, nullptr, s_tab, s_tab + TW, s_tab + 2 * TW + TH * j, s_tab + 2 * TW + P::THP + TH * j, x0, y0 + TH * j, x1,
                                       min(y0 + TH * j + TH - 1, y1), 0, 0, 0, tid, fillpx);
}

// Four channels: the tile is ONE 16-row pass of emit_rows, and inlined - the call's saved registers would be the kernel's only
// scratch.
__device__ __forceinline__ void plane_direct_tile4(const WarpCore& c, const uint8_t* src, uint8_t* dst, gtab_t Tg, int* s_tab, int x0, int y0, int x1, int y1,
                                                int bx0a, int by0, int bw, int tid) {
    static_assert(PlaneCfg<4>::THP == TH, "one pass of emit_rows per tile");
    stage_terms<TH>(c, Tg, s_tab, x0, y0, x1, y1, tid);
    __syncthreads();
    emit_rows<4, false>(c, src, dst, nullptr, s_tab, s_tab + TW, s_tab + 2 * TW, s_tab + 2 * TW + TH, x0, y0, x1, y1, bx0a, by0, bw, tid);
}

// One tile of a plane: tile (tx, ty) of the frame whose plane table starts at Ts (column records) / Tg (the per-column and
// per-row terms).  tile / lut / s_row: the workgroup's LDS.  src_add / dst_add: bytes from the plane the records name to the plane
// this tile belongs to (wave-uniform).
// BORDER: what the staged box holds where it leaves the picture - zeros (cv::warpAffine BORDER_CONSTANT: the stabilizer's warp) or the
// nearest picture pixel (BORDER_REPLICATE: the roll stage's rotation); a launch whose border is the other one takes the direct path.
// OWN: the plane_direct_tile / plane_direct_tile_fill copy of the kernel that says so (see plane_direct_tile).
// XR: extra staged rows - 0, or 8 for the taller box of the 4:2:2 instances (warp_i422_tall_kernel): the box may have ROWS + XR rows, the
// caller's `tile` holds them, and the direct path is copy 8.
// BORDER = VS_BORDER_FILL (edge fill on YUV surfaces): the VS_BORDER_BLACK instance with `fill` - the plane's fill as one dword pattern, in
// phase with every staged chunk (they start at a multiple of 4 pixels) - wherever that one holds zeros: rows and chunks outside the
// picture, the outside bytes of a chunk that straddles its left or right edge (load_chunk_straddling_fill), and, on the direct path
// (plane_direct_tile_fill, copy OWN), the taps outside.
template <int CN, int BORDER = VS_BORDER_BLACK, int SB = 1, int OWN = 0, int XR = 0>
__device__ __forceinline__ void plane_tile(const WarpCore& c, const __attribute__((address_space(4))) int32_t* Ts, gtab_t Tg, int tab_row, int tx, int tyl,
                                           uint8_t* tile, uint8_t* lut, int2* s_row, int tid, int src_add = 0, int dst_add = 0, uint32_t fill = 0u) {
    typedef PlaneCfg<CN, SB> P;
    constexpr int ROWS = P::ROWS + XR;
    static_assert(SB == 1 || (SB == 2 && CN <= 2), "16-bit planes: one or two channels");
    static_assert(XR == 0 || (CN == 1 && BORDER == VS_BORDER_REPLICATE), "the taller box: one-channel planes under BORDER_REPLICATE");
    typedef __attribute__((address_space(1))) uint8_t* gptr;
    const int L = tid & 31, ty = tid >> 5;
    int ad[4], bd[4];
    const int x0 = tx * TW, y0 = tyl * P::THP;
    const int x1 = min(x0 + TW, c.dw) - 1, y1 = min(y0 + P::THP, c.dh) - 1;
    const uint8_t* src;
    uint8_t* dst;
    int ad0, ad1, bd0, bd1, Xa, Xb, Ya, Yb;
    {
        typedef int32_t i32x8 __attribute__((ext_vector_type(8)));
        typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
        const i32x8 cc = *(const __attribute__((address_space(4))) i32x8*)(Ts + TAB_COL * tx);
        const i32x4 r0 = *(const __attribute__((address_space(4))) i32x4*)(Ts + tab_row + 4 * (y0 / TH));
        const i32x4 r1 = *(const __attribute__((address_space(4))) i32x4*)(Ts + tab_row + 4 * (y1 / TH));
        src = (const uint8_t*)(gptr)((unsigned long long)(uint32_t)cc[0] | (unsigned long long)(uint32_t)cc[1] << 32);
        dst = (uint8_t*)(gptr)((unsigned long long)(uint32_t)cc[2] | (unsigned long long)(uint32_t)cc[3] << 32);
        ad0 = cc[4]; ad1 = cc[5]; bd0 = cc[6]; bd1 = cc[7];
        Xa = r0[0]; Ya = r0[2]; Xb = r1[1]; Yb = r1[3];
    }
    // (I420: the table's records name the U plane; a V tile is given the byte distances V - U.  Zero for every other caller.)
    src += src_add; dst += dst_add;
    if (tid >= NT - 32) {      // vertical weights (the table of the BGR kernel: only W0 / W1 are read here)
        const uint32_t f = tid - (NT - 32);
        const uint32_t wlo = (32u - f) | (f << 8);
        *reinterpret_cast<uint4*>(lut + f * LUT_STRIDE) =
            make_uint4(wlo, wlo << 16, __float_as_uint((float)(32u - f) * 0x1p121f), __float_as_uint((float)f * 0x1p121f));
        *reinterpret_cast<uint32_t*>(lut + f * LUT_STRIDE + 16) = (32u - f) | (f << 16);
    }
    // source box of the tile (the maps are monotone in x and in y separately)
    int bx0a, by0, bw, bh;
    bool fit;
    {
        const int sx00 = (Xa + ad0) >> 10, sx01 = (Xa + ad1) >> 10, sx10 = (Xb + ad0) >> 10, sx11 = (Xb + ad1) >> 10;
        const int sy00 = (Ya + bd0) >> 10, sy01 = (Ya + bd1) >> 10, sy10 = (Yb + bd0) >> 10, sy11 = (Yb + bd1) >> 10;
        const int rx0 = min(min(sx00, sx01), min(sx10, sx11)), rx1 = max(max(sx00, sx01), max(sx10, sx11));
        const int ry0 = min(min(sy00, sy01), min(sy10, sy11)), ry1 = max(max(sy00, sy01), max(sy10, sy11));
        const bool saturated = rx0 < -32768 || ry0 < -32768 || rx1 > 32767 || ry1 > 32767;
        const int bx0 = max(rx0, -32768), bx1 = min(rx1, 32767) + 1;
        by0 = max(ry0, -32768);
        const int by1 = min(ry1, 32767) + 1;
        bx0a = bx0 & ~3;
        bw = bx1 - bx0a + 1;
        bh = by1 - by0 + 1;
        fit = !saturated && bw <= 136 && bh <= ROWS && c.border == BORDER;       // (bh <= ROWS: every staged row lies inside `tile`)
    }
    if (fit) {
        // ---- staging: chunks of 16 bytes, (row, chunk) = (i / CPR, i % CPR); all loads of a lane first, then its stores
        constexpr int NCH = (ROWS * P::CPR + NT - 1) / NT;
        const int total = bh * P::CPR;
        const long long rowbytes = (long long)c.sw * P::PXB;
        uint4 d[NCH];
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const int i = tid + NT * k;
            if constexpr (BORDER == VS_BORDER_FILL) d[k] = make_uint4(fill, fill, fill, fill);
            else d[k] = make_uint4(0u, 0u, 0u, 0u);
            if (i < total) {
                const int r = i / P::CPR, ch = i - r * P::CPR;
                const int y = by0 + r;
                const long long xb = (long long)bx0a * P::PXB + 16 * ch;      // byte column of the chunk in the source row
                if constexpr (BORDER == VS_BORDER_REPLICATE) {
                    const uint8_t* row = src + (size_t)min(max(y, 0), c.sh - 1) * c.sstride;
                    if (xb >= 0 && xb + 16 <= rowbytes && c.src_aligned) d[k] = *reinterpret_cast<const uint4*>(row + xb);
                    else d[k] = load_chunk_replicate<P::PXB>(row, (int)max(min(xb, (long long)rowbytes + 64), -64ll), c.sw);
                } else if ((unsigned)y < (unsigned)c.sh) {
                    const uint8_t* row = src + (size_t)y * c.sstride;
                    if (xb >= 0 && xb + 16 <= rowbytes && c.src_aligned) {
                        d[k] = *reinterpret_cast<const uint4*>(row + xb);       // 4-byte aligned: bx0a is a multiple of 4 pixels
                    } else if (xb + 16 > 0 && xb < rowbytes) {
                        if constexpr (BORDER == VS_BORDER_FILL) d[k] = load_chunk_straddling_fill(row, (int)xb, (int)rowbytes, c.src_aligned && (rowbytes & 3) == 0, fill);
                        else d[k] = load_chunk_straddling(row, (int)xb, (int)rowbytes, c.src_aligned && (rowbytes & 3) == 0);
                    }
                }
            }
        }
        // the terms (behind the box's loads): (ad, bd) of the lane's four columns straight into its registers, (X0, Y0) of the tile's
        // rows, relative to the box, into a small array (broadcast reads).  (Kept in the free bytes of the staged rows instead - one
        // LDS array less - the lanes of a read sit 256 bytes apart on ONE bank: 217 us instead of 192.)
        const int x = x0 + 4 * L;
        if (x1 - x0 == TW - 1 && (c.dw & 3) == 0) {
            typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
            typedef const __attribute__((address_space(1))) i32x4* g4;
            const i32x4 a4 = *(g4)(Tg + x), b4 = *(g4)(Tg + c.dw + x);
            ad[0] = a4.x; ad[1] = a4.y; ad[2] = a4.z; ad[3] = a4.w;
            bd[0] = b4.x; bd[1] = b4.y; bd[2] = b4.z; bd[3] = b4.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int cx = min(x + i, x1);
                ad[i] = Tg[cx]; bd[i] = Tg[c.dw + cx];
            }
        }
        if (tid >= TW && tid < TW + P::THP) {
            const int r = min(y0 + (tid - TW), y1);
            s_row[tid - TW] = make_int2(Tg[2 * c.dw + r] - (bx0a << 10), Tg[2 * c.dw + c.dh + r] - (by0 << 10));
        }
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const int i = tid + NT * k;
            if (i < total) {
                const int r = i / P::CPR;
                *reinterpret_cast<uint4*>(tile + r * P::PB + 16 * (i - r * P::CPR)) = d[k];
            }
        }
    }
    if (!fit) {
        if constexpr (CN == 4) plane_direct_tile4(c, src, dst, Tg, reinterpret_cast<int*>(tile), x0, y0, x1, y1, bx0a, by0, bw, tid);
        else if constexpr (BORDER == VS_BORDER_FILL)      // (the fill pixel: the pattern's first sample, or its (U, V) pair)
            plane_direct_tile_fill<CN, SB, OWN>(c, src, dst, Tg, reinterpret_cast<int*>(tile), x0, y0, x1, y1, tid, P::PXB == 1 ? fill & 0xFFu : P::PXB == 2 ? fill & 0xFFFFu : fill);
        else plane_direct_tile<CN, SB, (XR ? 8 : SB == 2 && BORDER == VS_BORDER_REPLICATE ? 1 + OWN : 0)>(c, src, dst, Tg, reinterpret_cast<int*>(tile), x0, y0, x1, y1, bx0a, by0, bw, tid);
        return;
    }
    __syncthreads();
    // ---- output
    plane_blend_rows<CN, SB>(c, tile, lut, s_row, ad, bd, L, ty, dst, (uint32_t)c.dstride, x0, y0, x1, y1);
}

template <int CN>
__global__ __launch_bounds__(NT, 8) void warp_plane_kernel(gtab_t tabs, int tab_stride, int tab_row, int tab_ad, uint32_t sstride, uint32_t dstride,
                                                        uint32_t swh, uint32_t dwh, uint32_t flags, uint32_t mgx, uint32_t mgy) {
    typedef PlaneCfg<CN> P;
    __shared__ __attribute__((aligned(16))) uint8_t tile[P::ROWS * P::PB];
    __shared__ __attribute__((aligned(16))) uint8_t lut[32 * LUT_STRIDE];
    __shared__ __attribute__((aligned(16))) int2 s_row[P::THP];                 // (X0, Y0) of the tile's rows
    typedef const __attribute__((address_space(4))) int32_t* cptr;
    const WarpCore c = unpack_core(sstride, dstride, swh, dwh, flags);
    const TileId tq = tile_id(flags, (uint32_t)(c.dw + TW - 1) / TW, (uint32_t)(c.dh + P::THP - 1) / P::THP, mgx, mgy);
    plane_tile<CN>(c, (cptr)(const int32_t*)(tabs + (size_t)tq.z * tab_stride), tabs + (size_t)tq.z * tab_stride + tab_ad, tab_row, tq.x, tq.y,
                   tile, lut, s_row, threadIdx.x);
}

// ---- YUV surfaces: the tiles of all planes of all frames in ONE launch ---------------------------------------------------------
// NV12 as two launches per 32 surfaces (warp_plane_kernel<1>, then <2>) had two launch tails and two table walks, and the luma
// launch - bound by its blend's instruction count - never shared a CU with the chroma launch, which is bound by its memory phase.
// Here the launch is a sequence of tiles (frame, plane, tile row, tile column): a frame's luma tiles, then its chroma tiles;
// workgroup `lin` takes tile seq(lin) of that sequence, the XCD-aware order as in tile_id.  A frame's tables lie in one block
// (warp_tab.h): luma table, then chroma table, `tab_stride` ints from frame to frame.  flags as in the plane kernels, plus bits 5 / 6:
// chroma source / destination aligned, and the frame count in bits 16...  mtpf = ceil(2^32 / tiles per frame), mgx1 / mgx2 likewise
// for the tile columns of the luma and the chroma planes.
//
// Two bodies: interleaved chroma (NV12, P010) and planar chroma (I420 and its kin).  Each declares the workgroup's LDS, finds the
// workgroup's frame, plane and tile, and calls plane_tile.  The __global__ templates below them are one call each: their names, launch
// bounds and argument lists are what the kernarg preload and the launchers see.
// VS_BORDER_FILL (edge fill on YUV surfaces): cv::warpAffine(..., INTER_LINEAR, BORDER_CONSTANT, borderValue = fill) per plane - the
// VS_BORDER_BLACK instances with the plane's fill sample where those read zeros (plane_tile<CN, VS_BORDER_FILL, SB>).  The fill travels
// as two more kernel arguments - Y | U << 16 and V, samples as they lie in memory - behind the others (13 and 16 dwords: still preloaded
// into scalar registers); only the fill kernels have them, so that the others keep their argument lists and their scalar registers, and
// only the VS_BORDER_FILL instances of a body read them.
// A plane's pattern: an 8-bit sample four times, the (U, V) byte pair twice, a 16-bit sample twice, or the (U, V) pair of P010.
// (Instances of another border have no fill: they read neither argument.)
template <int BORDER, int SB>
__device__ __forceinline__ uint32_t fill_pattern(uint32_t f) {
    if constexpr (BORDER != VS_BORDER_FILL) return 0u;
    else return SB == 2 ? (f & 0xFFFFu) | f << 16 : (f & 0xFFu) * 0x01010101u;
}
template <int BORDER, int SB>
__device__ __forceinline__ uint32_t fill_pattern_uv(uint32_t fill_yu, uint32_t fill_v) {
    if constexpr (BORDER != VS_BORDER_FILL) return 0u;
    else {
        const uint32_t u = fill_yu >> 16;
        return SB == 2 ? u | fill_v << 16 : ((u & 0xFFu) | (fill_v & 0xFFu) << 8) * 0x00010001u;
    }
}

// Frame f and tile t inside it of this workgroup, in a launch of (flags >> 16) frames of tpf tiles each
struct SurfTile { uint32_t f, t; };
__device__ __forceinline__ SurfTile surf_tile(uint32_t flags, uint32_t tpf, uint32_t mtpf) {
    const uint32_t n = tpf * (flags >> 16);
    const uint32_t lin = blockIdx.x;
    uint32_t seq = lin;
    if (flags & 0x100u) seq = xcd_seq(lin, n);
    const uint32_t f = __umulhi(seq, mtpf);
    return {f, seq - f * tpf};
}

// NV12 (SB = 1) and P010 (SB = 2: planes of 16-bit samples, PlaneCfg<CN, 2>).  The chroma plane's geometry is the luma plane's halved;
// the surfaces share one pitch.
template <int BORDER, int SB>
__device__ __forceinline__ void nv12_surface_tile(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t swh, uint32_t dwh, uint32_t flags,
                                                  uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, uint32_t fill_yu = 0u, uint32_t fill_v = 0u) {
    typedef PlaneCfg<1, SB> P1;
    typedef PlaneCfg<2, SB> P2;
    constexpr int TILE_BYTES = P1::ROWS * P1::PB > P2::ROWS * P2::PB ? P1::ROWS * P1::PB : P2::ROWS * P2::PB;
    __shared__ __attribute__((aligned(16))) uint8_t tile[TILE_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t lut[32 * LUT_STRIDE];
    __shared__ __attribute__((aligned(16))) int2 s_row[P1::THP];
    typedef const __attribute__((address_space(4))) int32_t* cptr;
    WarpCore c = unpack_core(sstride, dstride, swh, dwh, flags);
    const uint32_t gx1 = (uint32_t)(c.dw + TW - 1) / TW, gy1 = (uint32_t)(c.dh + P1::THP - 1) / P1::THP;
    const uint32_t dw2 = (uint32_t)c.dw >> 1, dh2 = (uint32_t)c.dh >> 1;
    const uint32_t gx2 = (dw2 + TW - 1) / TW, gy2 = (dh2 + P2::THP - 1) / P2::THP;
    const uint32_t n1 = gx1 * gy1, tpf = n1 + gx2 * gy2;
    const SurfTile q = surf_tile(flags, tpf, mtpf);
    uint32_t t = q.t;
    gtab_t T = tabs + (size_t)q.f * tab_stride;
    if (t < n1) {
        const TabLayout L = tab_layout(c.dw, c.dh);
        const uint32_t row = gx1 == 1 ? t : __umulhi(t, mgx1);
        plane_tile<1, BORDER, SB>(c, (cptr)(const int32_t*)T, T + L.ad, L.row, (int)(t - row * gx1), (int)row, tile, lut, s_row, threadIdx.x, 0, 0,
                                  fill_pattern<BORDER, SB>(fill_yu));
    } else {
        t -= n1;
        T += tab_layout(c.dw, c.dh).stride;
        c.sw >>= 1; c.sh >>= 1; c.dw = (int)dw2; c.dh = (int)dh2;
        c.src_aligned = (flags >> 5) & 1u; c.dst_aligned = (flags >> 6) & 1u;
        const TabLayout L = tab_layout(c.dw, c.dh);
        const uint32_t row = gx2 == 1 ? t : __umulhi(t, mgx2);
        plane_tile<2, BORDER, SB>(c, (cptr)(const int32_t*)T, T + L.ad, L.row, (int)(t - row * gx2), (int)row, tile, lut, s_row, threadIdx.x, 0, 0,
                                  fill_pattern_uv<BORDER, SB>(fill_yu, fill_v));
    }
}

// Planar surfaces: a frame's Y tiles, then its U tiles, then its V tiles.  All three planes are one-channel planes (PlaneCfg<1, SB>:
// tiles of 128 x 64 pixels, of 128 x 32 for the 16-bit formats I010 / I012 and their kin); U and V have (w >> CSX) x (h >> CSY) samples,
// a pitch of their own (scpitch / dcpitch) and alignment flags of their own (flags bits 5, 6).  A frame keeps the two table blocks of
// an NV12 surface (warp_tab.h): the luma table and ONE chroma table, in pixels; the chroma table's pointer records name the U plane, and
// a V tile adds the byte distances V - U (svu / dvu: all surfaces of a launch share one layout; negative for YV12).  The release
// workgroups of the batch schedule therefore build I420 tables exactly as they build NV12 tables.
// Arguments: 14 dwords - what gfx950 preloads into scalar registers at wave launch - with source and destination geometry in one
// dword (they are equal) and the plane distances as 32-bit values (the launcher sends surfaces whose V - U does not fit to the
// per-plane kernels).  Pitches, V - U and the alignment flags are in bytes for either sample size.
// (CSX, CSY) = (1, 1) is planar 4:2:0, (1, 0) is 4:2:2 (I422, I210, I212), (0, 0) is 4:4:4 (I444, I410, I412).  Nothing else differs: the
// chroma table is sized for that plane and built from the chroma map Mc = S^-1 M S, which for 4:2:2 is not a rotation - its 2 m3 term
// makes the source box of a chroma tile about 2 sin(angle) x 128 rows taller, so such tiles leave the staging area for
// plane_direct_tile at a smaller angle than luma tiles do (DESIGN.md section 4 has the figure).
// XR: plane_tile's extra staged rows (warp_i422_tall_kernel).
template <int BORDER, int SB, int CSX, int CSY, int XR>
__device__ __forceinline__ void planar_surface_tile(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t scpitch, uint32_t dcpitch, uint32_t wh,
                                                    uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, int32_t svu, int32_t dvu, uint32_t fill_yu = 0u,
                                                    uint32_t fill_v = 0u) {
    typedef PlaneCfg<1, SB> P;
    __shared__ __attribute__((aligned(16))) uint8_t tile[(P::ROWS + XR) * P::PB];
    __shared__ __attribute__((aligned(16))) uint8_t lut[32 * LUT_STRIDE];
    __shared__ __attribute__((aligned(16))) int2 s_row[P::THP];
    typedef const __attribute__((address_space(4))) int32_t* cptr;
    const int w = wh & 0xFFFFu, h = wh >> 16;
    const uint32_t gx1 = (uint32_t)(w + TW - 1) / TW, gy1 = (uint32_t)(h + P::THP - 1) / P::THP;
    const uint32_t w2 = (uint32_t)w >> CSX, h2 = (uint32_t)h >> CSY;
    const uint32_t gx2 = (w2 + TW - 1) / TW, gy2 = (h2 + P::THP - 1) / P::THP;
    const uint32_t n1 = gx1 * gy1, n2 = gx2 * gy2, tpf = n1 + 2 * n2;
    const SurfTile q = surf_tile(flags, tpf, mtpf);
    uint32_t t = q.t;
    gtab_t T = tabs + (size_t)q.f * tab_stride;
    // the tile's plane (workgroup-uniform): its geometry, pitches, alignment, table, tile columns, fill sample, and for V the plane distances
    WarpCore c;
    c.border = (flags >> 2) & 7u;
    uint32_t gx, mgx, fs = 0u;
    int sadd = 0, dadd = 0;
    if (t < n1) {
        c.sstride = sstride; c.dstride = dstride;
        c.sw = c.dw = w; c.sh = c.dh = h;
        c.src_aligned = flags & 1u; c.dst_aligned = (flags >> 1) & 1u;
        gx = gx1; mgx = mgx1;
        if constexpr (BORDER == VS_BORDER_FILL) fs = fill_yu;
    } else {
        t -= n1;
        if constexpr (BORDER == VS_BORDER_FILL) fs = fill_yu >> 16;
        if (t >= n2) {
            t -= n2; sadd = svu; dadd = dvu;
            if constexpr (BORDER == VS_BORDER_FILL) fs = fill_v;
        }
        T += tab_layout(w, h).stride;
        c.sstride = scpitch; c.dstride = dcpitch;
        c.sw = c.dw = (int)w2; c.sh = c.dh = (int)h2;
        c.src_aligned = (flags >> 5) & 1u; c.dst_aligned = (flags >> 6) & 1u;
        gx = gx2; mgx = mgx2;
    }
    const TabLayout L = tab_layout(c.dw, c.dh);
    const uint32_t row = gx == 1 ? t : __umulhi(t, mgx);
    // (the direct-path callee: the 16-bit BORDER_REPLICATE and the VS_BORDER_FILL instances have one per subsampling, see plane_direct_tile)
    constexpr int OWN = BORDER == VS_BORDER_FILL || (SB == 2 && BORDER == VS_BORDER_REPLICATE) ? (CSY == 1 ? 1 : CSX == 1 ? 2 : 3) : 0;
    plane_tile<1, BORDER, SB, OWN, XR>(c, (cptr)(const int32_t*)T, T + L.ad, L.row, (int)(t - row * gx), (int)row, tile, lut, s_row, threadIdx.x, sadd, dadd,
                                       fill_pattern<BORDER, SB>(fs));
}

template <int BORDER, int SB = 1>
__global__ __launch_bounds__(NT, 8) void warp_nv12_kernel(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t swh, uint32_t dwh,
                                                       uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2) {
    nv12_surface_tile<BORDER, SB>(tabs, tab_stride, sstride, dstride, swh, dwh, flags, mtpf, mgx1, mgx2);
}

template <int BORDER, int SB = 1, int CSX = 1, int CSY = 1>
__global__ __launch_bounds__(NT, 8) void warp_i420_kernel(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t scpitch, uint32_t dcpitch,
                                                       uint32_t wh, uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, int32_t svu, int32_t dvu) {
    planar_surface_tile<BORDER, SB, CSX, CSY, 0>(tabs, tab_stride, sstride, dstride, scpitch, dcpitch, wh, flags, mtpf, mgx1, mgx2, svu, dvu);
}

// Planar 4:2:2 surfaces under host maps of a few degrees: a taller staged box.  The roll stage and vs_op_warp_affine_planar rotate by
// degrees, and the 4:2:2 chroma map S^-1 M S has 2 sin(angle) where a rotation has sin(angle): a full-width chroma tile's source box
// outgrows the THP + 9 rows of PlaneCfg at 1.80 - 2.04 degrees, where luma tiles (and the tiles of a 4:2:0 surface) stay staged up to
// 3.61 - 4.07.  These instances stage THP + 17 rows: 254 sin(angle) < 16 keeps every full-width 4:2:2 chroma tile staged up to 3.61
// degrees (and luma tiles up to 7.2).  BORDER_REPLICATE only, (CSX, CSY) = (1, 0) only; the launcher picks them only where the maps are
// host doubles and some surface's chroma box needs the rows (i420_needs_tall_box) - the stabilizer's launches, whose maps are on the
// device, keep the instances they have.
// LDS: 8-bit 81 rows x 256 B + 1536 B = 22 272 B, seven workgroups per CU where the THP + 9 box allows eight; 16-bit 49 x 384 B + 1280 B
// = 20 096 B, eight.
template <int SB>
__global__ __launch_bounds__(NT, 7) void warp_i422_tall_kernel(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t scpitch, uint32_t dcpitch,
                                                            uint32_t wh, uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, int32_t svu, int32_t dvu) {
    planar_surface_tile<VS_BORDER_REPLICATE, SB, 1, 0, 8>(tabs, tab_stride, sstride, dstride, scpitch, dcpitch, wh, flags, mtpf, mgx1, mgx2, svu, dvu);
}

template <int SB>
__global__ __launch_bounds__(NT, 8) void warp_nv12_fill_kernel(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t swh, uint32_t dwh,
                                                            uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, uint32_t fill_yu, uint32_t fill_v) {
    nv12_surface_tile<VS_BORDER_FILL, SB>(tabs, tab_stride, sstride, dstride, swh, dwh, flags, mtpf, mgx1, mgx2, fill_yu, fill_v);
}

template <int SB, int CSX, int CSY>
__global__ __launch_bounds__(NT, 8) void warp_i420_fill_kernel(gtab_t tabs, int tab_stride, uint32_t sstride, uint32_t dstride, uint32_t scpitch, uint32_t dcpitch,
                                                            uint32_t wh, uint32_t flags, uint32_t mtpf, uint32_t mgx1, uint32_t mgx2, int32_t svu, int32_t dvu,
                                                            uint32_t fill_yu, uint32_t fill_v) {
    planar_surface_tile<VS_BORDER_FILL, SB, CSX, CSY, 0>(tabs, tab_stride, sstride, dstride, scpitch, dcpitch, wh, flags, mtpf, mgx1, mgx2, svu, dvu, fill_yu, fill_v);
}

// Launches without tables (a caller's tables exist for launches of WARP_TAB_MIN surfaces and more only), chroma planes that do not lie
// one offset behind their luma planes, geometry outside what the two kernels above pack: one plane of 8- or 16-bit samples (CN = 1, or
// 2: interleaved chroma) under VS_BORDER_FILL, terms from the frame's inverse map, taps read directly - warp_affine16_kernel with the
// fill pixel.  (The general kernels take their border from WarpCore, which keeps its fields.)
template <int CN, int SB>
__global__ __launch_bounds__(NT) void warp_plane_fill_kernel(WarpArgs a, uint32_t fillpx) {
    __shared__ int s_ad[TW], s_bd[TW], s_x0[TH], s_y0[TH];
    const int bz = blockIdx.z;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int x1 = min(x0 + TW, a.c.dw) - 1, y1 = min(y0 + TH, a.c.dh) - 1;
    double m[6];
    load_map(a, bz, m);
    map_terms(m, x0, y0, x1, y1, tid, s_ad, s_bd, s_x0, s_y0);
    __syncthreads();
    emit_rows<CN, false, SB, true>(a.c, a.srcs[bz], a.dsts[bz], nullptr, s_ad, s_bd, s_x0, s_y0, x0, y0, x1, y1, 0, 0, 0, tid, fillpx);
}

// Ints of table workspace per frame of dw x dh (see warp_tables_kernel).
inline int tab_stride_of(int dw, int dh) { return tab_layout(dw, dh).stride; }

// what: VS_WARP_ALL = tables (when d_tabs is given) and warp; VS_WARP_TABLES_ONLY / VS_WARP_ONLY = the two halves apart, so
// that a caller whose maps are ready long before it warps (the batch tail of the stabilizer) builds the tables then.
// tab_stride: ints from one frame's table to the next (0: the tables are packed; NV12 blocks hold two planes' tables per frame)
// sb = 2: a plane of 16-bit samples (cn = 1 or 2).  Its tables are built like any plane's (they are in pixels); the warp itself
// is the general 16-bit kernel, which takes its terms from the maps.
template <int CN>
void launch_one(WarpArgs& a, dim3 grid, int32_t* d_tabs, int what, hipStream_t st, int tab_stride, int sb) {
    a.tabs = d_tabs;
    const TabLayout tl = tab_layout(a.c.dw, a.c.dh);
    a.tab_stride = tab_stride > 0 ? tab_stride : tl.stride; a.tab_row = tl.row; a.tab_ad = tl.ad;
    if (sb == 2) {
        if (d_tabs && what != VS_WARP_ONLY)
            hipLaunchKernelGGL(warp_tables_kernel, dim3((a.c.dw + a.c.dh + grid.x + grid.y + NT - 1) / NT, grid.z), dim3(NT), 0, st, a);
        if (d_tabs && what == VS_WARP_TABLES_ONLY) return;
        if constexpr (CN <= 2) hipLaunchKernelGGL((warp_affine16_kernel<CN>), grid, dim3(NT), 0, st, a);
        return;
    }
    if (d_tabs) {
        if (what != VS_WARP_ONLY)
            hipLaunchKernelGGL(warp_tables_kernel, dim3((a.c.dw + a.c.dh + grid.x + grid.y + NT - 1) / NT, grid.z), dim3(NT), 0, st, a);
        if (what == VS_WARP_TABLES_ONLY) return;
        // (the table kernels pack sizes into 16 bits and form row offsets with 24-bit multiplies: larger frames or pitches of
        // 16 MiB and more take the general kernel)
        const bool packs = a.c.sw < 65536 && a.c.sh < 65536 && a.c.dw < 65536 && a.c.dh < 65536 && a.c.sstride < (1ull << 24) && a.c.dstride < (1ull << 24);
        // XCD-aware tile order (tile_id): the reciprocals of the grid's x and y extents, and the flag only where they are exact
        auto order = [](const dim3& g, uint32_t* mgx, uint32_t* mgy) -> uint32_t {
            *mgx = (uint32_t)((0x100000000ull + g.x - 1) / g.x); *mgy = (uint32_t)((0x100000000ull + g.y - 1) / g.y);
            const unsigned long long n = (unsigned long long)g.x * g.y * g.z;
            return (g.x > 1 || g.y > 1) && n * std::max(g.x, g.y) < (1ull << 31) && g.z < 65536 ? (0x100u | (uint32_t)g.z << 16) : 0u;
        };
        uint32_t mgx = 0, mgy = 0;
        if (CN == 3 && packs) {
            // 12 dwords of arguments: all of them among the 14 the hardware preloads into scalar registers
            const uint32_t of = order(grid, &mgx, &mgy);
            hipLaunchKernelGGL(warp_tab_kernel, grid, dim3(NT), 0, st, (gtab_t)a.tabs, a.tab_stride, a.tab_row, a.tab_ad, (uint32_t)a.c.sstride,
                               (uint32_t)a.c.dstride, (uint32_t)a.c.sw | (uint32_t)a.c.sh << 16, (uint32_t)a.c.dw | (uint32_t)a.c.dh << 16,
                               (uint32_t)(a.c.src_aligned ? 1 : 0) | (uint32_t)(a.c.dst_aligned ? 2 : 0) | (uint32_t)a.c.border << 2 | of, mgx, mgy);
        } else if (CN != 3 && packs && a.c.border == VS_BORDER_BLACK) {
            const dim3 pg(grid.x, (a.c.dh + PlaneCfg<CN>::THP - 1) / PlaneCfg<CN>::THP, grid.z);
            const uint32_t of = order(pg, &mgx, &mgy);
            hipLaunchKernelGGL((warp_plane_kernel<(CN == 3 ? 1 : CN)>), pg, dim3(NT), 0, st, (gtab_t)a.tabs, a.tab_stride, a.tab_row, a.tab_ad, (uint32_t)a.c.sstride,
                               (uint32_t)a.c.dstride, (uint32_t)a.c.sw | (uint32_t)a.c.sh << 16, (uint32_t)a.c.dw | (uint32_t)a.c.dh << 16,
                               (uint32_t)(a.c.src_aligned ? 1 : 0) | (uint32_t)(a.c.dst_aligned ? 2 : 0) | (uint32_t)a.c.border << 2 | of, mgx, mgy);
        } else {
            hipLaunchKernelGGL((warp_affine_kernel<CN, true>), grid, dim3(NT), 0, st, a);
        }
    } else {
        hipLaunchKernelGGL((warp_affine_kernel<CN, false>), grid, dim3(NT), 0, st, a);
    }
}

void launch_cn(WarpArgs& a, dim3 grid, int cn, int32_t* d_tabs, hipStream_t st, int what = VS_WARP_ALL, int tab_stride = 0, int sb = 1) {
    if (cn == 3) launch_one<3>(a, grid, d_tabs, what, st, tab_stride, sb);
    else if (cn == 4) launch_one<4>(a, grid, d_tabs, what, st, tab_stride, sb);
    else if (cn == 1) launch_one<1>(a, grid, d_tabs, what, st, tab_stride, sb);
    else launch_one<2>(a, grid, d_tabs, what, st, tab_stride, sb);
}

// (cn: the bytes of a pixel - channels x bytes per sample)
bool bad_args(const void* d_src, const void* d_dst, const void* M, size_t sstride, int sw, int sh, size_t dstride,
              int dw, int dh, int cn, int batch) {
    return !d_src || !d_dst || !M || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || batch <= 0 ||
           (cn < 1 || cn > 4) || sstride < (size_t)sw * cn || dstride < (size_t)dw * cn ||
           dh > 65535 * TH;
}

// 16-bit samples sit on even addresses: pointers, pitches (and with them the plane offsets).
bool odd16(const uint8_t* const* srcs, uint8_t* const* dsts, int n, size_t sstride, size_t dstride) {
    if ((sstride | dstride) & 1) return true;
    for (int i = 0; i < n; i++)
        if (((uintptr_t)srcs[i] | (uintptr_t)dsts[i]) & 1) return true;
    return false;
}

// Validation shared by the launchers: the border, the table choice, and no null frame in the lists.
// fill_ok: the YUV launchers, which also take VS_BORDER_FILL
bool bad_call(const uint8_t* const* srcs, uint8_t* const* dsts, int n, int border, const WarpTabs& tabs, bool fill_ok = false) {
    if ((border != VS_BORDER_BLACK && border != VS_BORDER_REPLICATE && !(fill_ok && border == VS_BORDER_FILL)) || (tabs.kind == WarpTabs::CALLER && !tabs.tabs) ||
        (tabs.kind != WarpTabs::CALLER && tabs.what != VS_WARP_ALL))
        return true;
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return true;
    return false;
}

// Table scratch of the standalone operators (vs_op_warp_affine*, the roll correction): one grow-only device buffer per stream.
// Launches on a stream run in order, so the tables of a call are consumed before the next call on that stream rewrites them.
// (hipMallocAsync memory is not used: with it, in-flight builds of round 2 read zeroed tables for the later frames of a launch
// and faulted on the null source pointers; the cause was not established - DESIGN.md section 8 has the evidence.)
struct OpScratch { int32_t* p = nullptr; size_t bytes = 0; };
std::mutex g_op_mutex;
std::map<std::pair<int, hipStream_t>, OpScratch> g_op_scratch;

int op_tabs(hipStream_t st, size_t bytes, int32_t** out) {
    int dev = 0;
    VS_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_op_mutex);
    OpScratch& sc = g_op_scratch[std::make_pair(dev, st)];
    if (sc.bytes < bytes) {
        if (sc.p) {                       // queued launches may still read the old block
            VS_HIP_TRY(hipStreamSynchronize(st));
            (void)hipFree(sc.p);
            sc.p = nullptr; sc.bytes = 0;
        }
        VS_HIP_TRY(hipMalloc((void**)&sc.p, bytes));
        sc.bytes = bytes;
    }
    *out = sc.p;
    return VS_OK;
}

// The maps of the frames from the k-th on.
WarpMaps maps_from(WarpMaps m, int k) { m.m += (size_t)m.stride * k; return m; }

// ONE launch over n <= MAXB frames of one plane.  d_tabs: the launch's tables (tab_stride ints apart, 0 = packed), or nullptr.
// border VS_BORDER_FILL (cn 1 or 2): fillpx is the plane's fill pixel - the sample, or the (U, V) pair as load_px_checked forms it -, the
// tables are built as for any border, and the warp is warp_plane_fill_kernel's.
int plane_launch(const uint8_t* const* srcs, uint8_t* const* dsts, int n, size_t sstride, int sw, int sh, size_t dstride, int dw, int dh,
                 int cn, WarpMaps maps, int border, int32_t* d_tabs, int tab_stride, int what, hipStream_t st, int sb = 1, uint32_t fillpx = 0u) {
    WarpArgs a;
    a.c.sstride = sstride; a.c.dstride = dstride;
    a.c.sw = sw; a.c.sh = sh; a.c.dw = dw; a.c.dh = dh;
    a.c.border = border;
    const int galign = cn * sb == 2 ? 8 : 4;
    const int dalign = cn * sb == 4 ? 16 : sb == 2 ? 8 : galign;      // (four bytes per pixel: a lane's four pixels are one aligned 16-byte store)
    a.c.src_aligned = sstride % galign == 0;
    a.c.dst_aligned = dstride % dalign == 0;
    for (int i = 0; i < MAXB; i++) {
        a.srcs[i] = srcs[i < n ? i : 0]; a.dsts[i] = dsts[i < n ? i : 0];
        if ((uintptr_t)a.srcs[i] % galign) a.c.src_aligned = 0;
        if ((uintptr_t)a.dsts[i] % dalign) a.c.dst_aligned = 0;
    }
    a.Minv_dev = maps.host ? nullptr : maps.m;
    a.minv_stride = maps.stride;
    for (int b = 0; b < MAXB; b++)
        for (int i = 0; i < 6; i++) a.Minv_val[6 * b + i] = maps.host && b < n ? maps.m[(size_t)maps.stride * b + i] : 0.;
    dim3 grid((dw + TW - 1) / TW, (dh + TH - 1) / TH, n);
    if (border == VS_BORDER_FILL) {
        if (cn > 2) { set_last_error("warp: VS_BORDER_FILL takes planes of one or two channels"); return VS_ERR_INVALID_ARG; }
        a.tabs = d_tabs;
        const TabLayout tl = tab_layout(dw, dh);
        a.tab_stride = tab_stride > 0 ? tab_stride : tl.stride; a.tab_row = tl.row; a.tab_ad = tl.ad;
        if (d_tabs && what != VS_WARP_ONLY)
            hipLaunchKernelGGL(warp_tables_kernel, dim3((dw + dh + grid.x + grid.y + NT - 1) / NT, grid.z), dim3(NT), 0, st, a);
        if (!(d_tabs && what == VS_WARP_TABLES_ONLY)) {
            if (sb == 2 && cn == 2) hipLaunchKernelGGL((warp_plane_fill_kernel<2, 2>), grid, dim3(NT), 0, st, a, fillpx);
            else if (sb == 2) hipLaunchKernelGGL((warp_plane_fill_kernel<1, 2>), grid, dim3(NT), 0, st, a, fillpx);
            else if (cn == 2) hipLaunchKernelGGL((warp_plane_fill_kernel<2, 1>), grid, dim3(NT), 0, st, a, fillpx);
            else hipLaunchKernelGGL((warp_plane_fill_kernel<1, 1>), grid, dim3(NT), 0, st, a, fillpx);
        }
        VS_HIP_TRY(hipGetLastError());
        return VS_OK;
    }
    launch_cn(a, grid, cn, d_tabs, st, what, tab_stride, sb);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

// The fill of a VS_BORDER_FILL launch as the kernels take it: Y | U << 16 and V; 8-bit formats hold 8-bit samples.
bool bad_fill(const WarpFill& f, int sb) { const uint32_t top = sb == 2 ? 0xFFFFu : 0xFFu; return f.y > top || f.u > top || f.v > top; }

// NV12 surfaces of one geometry and pitch, luma and chroma planes in ONE launch (warp_nv12_kernel), from the frames' table blocks
// (warp_tab.h: luma table, then chroma table; nv12_tab_ints(w, h) ints per frame), ALREADY BUILT.  The chroma planes lie src_uv /
// dst_uv bytes behind the luma planes.  Returns VS_ERR_UNSUPPORTED when the geometry is outside what the kernel packs.
int nv12_launch(const uint8_t* const* ys, uint8_t* const* yd, int n, size_t sstride, size_t dstride, int w, int h, size_t src_uv,
                size_t dst_uv, const int32_t* d_tabs, int border, hipStream_t st, int sb = 1, WarpFill fill = WarpFill()) {
    // (sb = 2, P010: tiles of half the rows; BORDER_REPLICATE: the roll stage's rotation of P010 surfaces)
    const int thp1 = sb == 2 ? PlaneCfg<1, 2>::THP : PlaneCfg<1>::THP, thp2 = sb == 2 ? PlaneCfg<2, 2>::THP : PlaneCfg<2>::THP;
    const unsigned long long gx1 = (w + TW - 1) / TW, gy1 = (h + thp1 - 1) / thp1, gx2 = (w / 2 + TW - 1) / TW, gy2 = (h / 2 + thp2 - 1) / thp2;
    const unsigned long long tpf = gx1 * gy1 + gx2 * gy2, total = tpf * (unsigned long long)n;
    if (w >= 65536 || h >= 65536 || sstride >= (1ull << 24) || dstride >= (1ull << 24) || n >= 65536 || total * std::max(tpf, std::max(gx1, gx2)) >= (1ull << 31))
        return VS_ERR_UNSUPPORTED;
    uint32_t al = 0xFu;          // bit 0 / 1: luma source / destination 4-byte aligned; bit 2 / 3: chroma 8-byte aligned
    // (P010: a lane's four pixels are 8 bytes of luma, 16 of chroma; the staging loads ask for 4-byte alignment on either plane)
    const size_t a_ys = 4, a_yd = sb == 2 ? 8 : 4, a_us = sb == 2 ? 4 : 8, a_ud = sb == 2 ? 16 : 8;
    if (sstride % a_ys) al &= ~1u;
    if (dstride % a_yd) al &= ~2u;
    if (sstride % a_us || src_uv % a_us) al &= ~4u;
    if (dstride % a_ud || dst_uv % a_ud) al &= ~8u;
    for (int i = 0; i < n; i++) {
        if ((uintptr_t)ys[i] % a_ys) al &= ~1u;
        if ((uintptr_t)yd[i] % a_yd) al &= ~2u;
        if ((uintptr_t)ys[i] % a_us) al &= ~4u;
        if ((uintptr_t)yd[i] % a_ud) al &= ~8u;
    }
    const uint32_t flags = (al & 1u) | (al & 2u) | (uint32_t)border << 2 | ((al >> 2) & 1u) << 5 | ((al >> 3) & 1u) << 6 | 0x100u | (uint32_t)n << 16;
    const uint32_t mtpf = (uint32_t)((0x100000000ull + tpf - 1) / tpf), mgx1 = (uint32_t)((0x100000000ull + gx1 - 1) / gx1),
                   mgx2 = (uint32_t)((0x100000000ull + gx2 - 1) / gx2);
    const uint32_t wh = (uint32_t)w | (uint32_t)h << 16;
    auto go = [&](auto kernel, auto... fills) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(NT), 0, st, (gtab_t)d_tabs, nv12_tab_ints(w, h), (uint32_t)sstride, (uint32_t)dstride, wh, wh, flags,
                           mtpf, mgx1, mgx2, fills...);
    };
    if (border == VS_BORDER_FILL && sb == 2) go(warp_nv12_fill_kernel<2>, fill.y | fill.u << 16, fill.v);
    else if (border == VS_BORDER_FILL) go(warp_nv12_fill_kernel<1>, fill.y | fill.u << 16, fill.v);
    else if (sb == 2 && border == VS_BORDER_REPLICATE) go(warp_nv12_kernel<VS_BORDER_REPLICATE, 2>);
    else if (sb == 2) go(warp_nv12_kernel<VS_BORDER_BLACK, 2>);
    else if (border == VS_BORDER_REPLICATE) go(warp_nv12_kernel<VS_BORDER_REPLICATE>);
    else go(warp_nv12_kernel<VS_BORDER_BLACK>);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

// I420 surfaces of one geometry and layout, all three planes in ONE launch (warp_i420_kernel), from the frames' table blocks (luma
// table, then the chroma table whose records name the U planes; nv12_tab_ints(w, h) ints per frame), ALREADY BUILT.  Returns
// VS_ERR_UNSUPPORTED when the geometry is outside what the kernel packs.
int i420_launch(const uint8_t* const* ys, uint8_t* const* yd, int n, const I420Layout& sl, const I420Layout& dl, int w, int h, const int32_t* d_tabs,
                int border, hipStream_t st, int sb = 1, int sx = 1, int sy = 1, bool tall = false, WarpFill fill = WarpFill()) {
    // (sb = 2, I010 / I012: tiles of half the rows; BORDER_REPLICATE: the roll stage's rotation of I010 / I012 surfaces)
    const int thp = sb == 2 ? PlaneCfg<1, 2>::THP : PlaneCfg<1>::THP;
    const unsigned long long gx1 = (w + TW - 1) / TW, gy1 = (h + thp - 1) / thp, gx2 = ((w >> sx) + TW - 1) / TW, gy2 = ((h >> sy) + thp - 1) / thp;
    const unsigned long long tpf = gx1 * gy1 + 2 * gx2 * gy2, total = tpf * (unsigned long long)n;
    const long long svu = (long long)sl.v - (long long)sl.u, dvu = (long long)dl.v - (long long)dl.u;
    if (w >= 65536 || h >= 65536 || sl.pitch >= (1ull << 24) || dl.pitch >= (1ull << 24) || sl.cpitch >= (1ull << 24) || dl.cpitch >= (1ull << 24) ||
        (sx != 0 && sx != 1) || (sy != 0 && sy != 1) || sy > sx || n >= 65536 || total * std::max(tpf, std::max(gx1, gx2)) >= (1ull << 31) || svu != (int32_t)svu || dvu != (int32_t)dvu)
        return VS_ERR_UNSUPPORTED;
    // bit 0 / 1: luma source / destination aligned - 4 bytes for the staging loads, a lane's four pixels (4 bytes; 16-bit samples: 8)
    // for the stores; bit 2 / 3: both chroma planes (pointers and pitch)
    const size_t a_s = 4, a_d = sb == 2 ? 8 : 4;
    uint32_t al = 0xFu;
    if (sl.pitch % a_s) al &= ~1u;
    if (dl.pitch % a_d) al &= ~2u;
    if (sl.cpitch % a_s || sl.u % a_s || sl.v % a_s) al &= ~4u;
    if (dl.cpitch % a_d || dl.u % a_d || dl.v % a_d) al &= ~8u;
    for (int i = 0; i < n; i++) {
        if ((uintptr_t)ys[i] % a_s) al &= ~5u;
        if ((uintptr_t)yd[i] % a_d) al &= ~10u;
    }
    const uint32_t flags = (al & 3u) | (uint32_t)border << 2 | ((al >> 2) & 1u) << 5 | ((al >> 3) & 1u) << 6 | 0x100u | (uint32_t)n << 16;
    const uint32_t mtpf = (uint32_t)((0x100000000ull + tpf - 1) / tpf), mgx1 = (uint32_t)((0x100000000ull + gx1 - 1) / gx1),
                   mgx2 = (uint32_t)((0x100000000ull + gx2 - 1) / gx2);
    auto go = [&](auto kernel, auto... fills) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(NT), 0, st, (gtab_t)d_tabs, planar_tab_ints(w, h, sx, sy), (uint32_t)sl.pitch, (uint32_t)dl.pitch,
                           (uint32_t)sl.cpitch, (uint32_t)dl.cpitch, (uint32_t)w | (uint32_t)h << 16, flags, mtpf, mgx1, mgx2, (int32_t)svu, (int32_t)dvu, fills...);
    };
    // a kernel's instance for this launch's subsampling, of its three: 4:2:0, 4:2:2, 4:4:4
    auto sub = [&](auto k420, auto k422, auto k444) { return sx == 1 && sy == 1 ? k420 : sx == 1 ? k422 : k444; };
    // (tall: 4:2:2, BORDER_REPLICATE, host maps that need the taller staged box - launch_warp_i420 decides)
    const bool use_tall = tall && sx == 1 && sy == 0 && border == VS_BORDER_REPLICATE;
    const bool use_fill = border == VS_BORDER_FILL;
    // (the instances are named in the order in which they came: a later one is placed behind the earlier ones in the code object, which
    // keep their place)
    if (use_tall || use_fill) ;
    else if (sb == 2 && border == VS_BORDER_REPLICATE)
        go(sub(warp_i420_kernel<VS_BORDER_REPLICATE, 2, 1, 1>, warp_i420_kernel<VS_BORDER_REPLICATE, 2, 1, 0>, warp_i420_kernel<VS_BORDER_REPLICATE, 2, 0, 0>));
    else if (sb == 2) go(sub(warp_i420_kernel<VS_BORDER_BLACK, 2, 1, 1>, warp_i420_kernel<VS_BORDER_BLACK, 2, 1, 0>, warp_i420_kernel<VS_BORDER_BLACK, 2, 0, 0>));
    else if (border == VS_BORDER_REPLICATE)
        go(sub(warp_i420_kernel<VS_BORDER_REPLICATE, 1, 1, 1>, warp_i420_kernel<VS_BORDER_REPLICATE, 1, 1, 0>, warp_i420_kernel<VS_BORDER_REPLICATE, 1, 0, 0>));
    else go(sub(warp_i420_kernel<VS_BORDER_BLACK, 1, 1, 1>, warp_i420_kernel<VS_BORDER_BLACK, 1, 1, 0>, warp_i420_kernel<VS_BORDER_BLACK, 1, 0, 0>));
    if (use_tall && sb == 2) go(warp_i422_tall_kernel<2>);
    else if (use_tall) go(warp_i422_tall_kernel<1>);
    else if (use_fill && sb == 2) go(sub(warp_i420_fill_kernel<2, 1, 1>, warp_i420_fill_kernel<2, 1, 0>, warp_i420_fill_kernel<2, 0, 0>), fill.y | fill.u << 16, fill.v);
    else if (use_fill) go(sub(warp_i420_fill_kernel<1, 1, 1>, warp_i420_fill_kernel<1, 1, 0>, warp_i420_fill_kernel<1, 0, 0>), fill.y | fill.u << 16, fill.v);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace

// Ints of workspace the table form of a launch over `frames` frames of dw x dh needs (d_tabs of the launchers).
size_t warp_tabs_ints(int dw, int dh, int frames) { return (size_t)tab_stride_of(dw, dh) * (size_t)(frames > 0 ? frames : 1); }

int launch_warp_plane(const uint8_t* const* srcs, uint8_t* const* dsts, int n, size_t sstride, int sw, int sh, size_t dstride, int dw,
                      int dh, int cn, WarpMaps maps, int border, WarpTabs tabs, hipStream_t st, int sb) {
    if (n < 1 || !srcs || !dsts || (sb != 1 && sb != 2) || (sb == 2 && (cn < 1 || cn > 2 || tabs.kind != WarpTabs::NONE)) ||
        bad_args(srcs[0], dsts[0], maps.m, sstride, sw, sh, dstride, dw, dh, cn * sb, n) || bad_call(srcs, dsts, n, border, tabs)) {
        set_last_error(sb == 2 ? "warp_affine16: invalid argument (planes of 16-bit samples, as those of P010: cn 1 or 2)" : "warp_affine: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    if (sb == 2 && odd16(srcs, dsts, n, sstride, dstride)) {
        set_last_error("warp_affine16: pointers and strides of 16-bit planes (P010's) must be even");
        return VS_ERR_INVALID_ARG;
    }
    if (tabs.kind == WarpTabs::SCRATCH && n >= WARP_TAB_MIN)
        VS_TRY(op_tabs(st, warp_tabs_ints(dw, dh, std::min(n, MAXB)) * sizeof(int32_t), &tabs.tabs));
    // the caller's buffer holds the tables of all frames, the scratch those of one launch
    const size_t tab_step = tabs.kind != WarpTabs::CALLER ? 0 : tabs.stride > 0 ? (size_t)tabs.stride : (size_t)tab_stride_of(dw, dh);
    for (int b0 = 0; b0 < n; b0 += MAXB) {
        const int nb = std::min(MAXB, n - b0);
        int32_t* T = tabs.kind != WarpTabs::NONE && nb >= WARP_TAB_MIN ? tabs.tabs + b0 * tab_step : nullptr;
        if (!T && tabs.what == VS_WARP_TABLES_ONLY) continue;
        VS_TRY(plane_launch(srcs + b0, dsts + b0, nb, sstride, sw, sh, dstride, dw, dh, cn, maps_from(maps, b0), border, T, tabs.stride,
                            T ? tabs.what : VS_WARP_ALL, st, sb));
    }
    return VS_OK;
}

// Per launch: the tables of both planes (host maps: one launch for up to NVT_MAX surfaces; else one per plane), then both planes in
// ONE grid; plane by plane when the launch has no tables, when the chroma planes do not all lie one offset behind the luma planes
// (the one-launch kernel and the table launch take one offset), or when the geometry is outside what the one-launch kernel packs.
int launch_warp_nv12(const uint8_t* const* ys, uint8_t* const* yd, const uint8_t* const* us, uint8_t* const* ud, int n, size_t sstride,
                     size_t dstride, int w, int h, WarpMaps maps, int border, WarpTabs tabs, hipStream_t st, int sb, WarpFill fill) {
    if (n < 1 || !ys || !yd || !us || !ud || w < 2 || h < 2 || (w & 1) || (h & 1) || (sb != 1 && sb != 2) ||
        bad_args(ys[0], yd[0], maps.m, sstride, w, h, dstride, w, h, sb, n) || bad_call(ys, yd, n, border, tabs, true) ||
        bad_call(us, ud, n, border, tabs, true) || (border == VS_BORDER_FILL && bad_fill(fill, sb))) {
        set_last_error(sb == 2 ? "warp_p010: invalid argument (w and h must be even)" : "warp_nv12: invalid argument (w and h must be even)");
        return VS_ERR_INVALID_ARG;
    }
    if (sb == 2 && (odd16(ys, yd, n, sstride, dstride) || odd16(us, ud, n, sstride, dstride))) {
        set_last_error("warp_p010: P010 pointers, pitches and plane offsets must be even");
        return VS_ERR_INVALID_ARG;
    }
    // (P010 with the scratch tables: every launch builds them - one kernel serves single surfaces and batches alike.  A caller's
    // tables exist for launches of WARP_TAB_MIN frames and more only, whatever the format.)
    // (VS_BORDER_FILL likewise: a single surface goes through the one-launch kernel and its staged box)
    const int tab_min = (sb == 2 || border == VS_BORDER_FILL) && tabs.kind == WarpTabs::SCRATCH ? 1 : WARP_TAB_MIN;
    const uint32_t fpx_y = fill.y, fpx_uv = sb == 2 ? fill.u | fill.v << 16 : fill.u | fill.v << 8;      // (the planes' fill pixels: plane_launch)
    const int block = nv12_tab_ints(w, h), sy = tab_layout(w, h).stride;
    if (tabs.kind == WarpTabs::SCRATCH && n >= tab_min)
        VS_TRY(op_tabs(st, (size_t)block * std::min(n, MAXB) * sizeof(int32_t), &tabs.tabs));
    const WarpMaps muv = {maps.m + 6, maps.stride, maps.host};
    const size_t tab_step = tabs.kind == WarpTabs::CALLER ? block : 0;
    for (int b0 = 0; b0 < n; b0 += MAXB) {
        const int nb = std::min(MAXB, n - b0);
        int32_t* T = tabs.kind != WarpTabs::NONE && nb >= tab_min ? tabs.tabs + b0 * tab_step : nullptr;
        if (!T && tabs.what == VS_WARP_TABLES_ONLY) continue;
        const WarpMaps my = maps_from(maps, b0), mu = maps_from(muv, b0);
        const size_t src_uv = (uintptr_t)us[b0] - (uintptr_t)ys[b0], dst_uv = (uintptr_t)ud[b0] - (uintptr_t)yd[b0];
        bool one_uv = true;
        for (int i = b0; i < b0 + nb; i++)
            one_uv &= (uintptr_t)us[i] - (uintptr_t)ys[i] == src_uv && (uintptr_t)ud[i] - (uintptr_t)yd[i] == dst_uv;
        if (T && tabs.what != VS_WARP_ONLY) {
            if (maps.host && nb <= NVT_MAX && one_uv) {      // (the tables are in pixels: the same for either sample size)
                NvTabArgs t;
                t.tabs = T; t.block = block; t.chroma = sy; t.w = w; t.h = h; t.src_uv = src_uv; t.dst_uv = dst_uv;
                for (int i = 0; i < NVT_MAX; i++) { t.ys[i] = ys[b0 + (i < nb ? i : 0)]; t.yd[i] = yd[b0 + (i < nb ? i : 0)]; }
                for (int i = 0; i < NVT_MAX * 6; i++) {
                    t.my[i] = i < 6 * nb ? my.m[(size_t)my.stride * (i / 6) + i % 6] : 0.;
                    t.muv[i] = i < 6 * nb ? mu.m[(size_t)mu.stride * (i / 6) + i % 6] : 0.;
                }
                const int entries = w + h + (w + TW - 1) / TW + (h + TH - 1) / TH;
                hipLaunchKernelGGL(warp_tables_nv12_kernel, dim3((entries + NT - 1) / NT, nb, 2), dim3(NT), 0, st, t);
            } else {
                VS_TRY(plane_launch(ys + b0, yd + b0, nb, sstride, w, h, dstride, w, h, 1, my, border, T, block, VS_WARP_TABLES_ONLY, st, sb, fpx_y));
                VS_TRY(plane_launch(us + b0, ud + b0, nb, sstride, w / 2, h / 2, dstride, w / 2, h / 2, 2, mu, border, T + sy, block,
                                    VS_WARP_TABLES_ONLY, st, sb, fpx_uv));
            }
        }
        if (tabs.what == VS_WARP_TABLES_ONLY) continue;
        const int one = T && one_uv ? nv12_launch(ys + b0, yd + b0, nb, sstride, dstride, w, h, src_uv, dst_uv, T, border, st, sb, fill) : VS_ERR_UNSUPPORTED;
        if (one != VS_ERR_UNSUPPORTED) {
            VS_TRY(one);
            continue;
        }
        const int what = T ? VS_WARP_ONLY : VS_WARP_ALL;
        VS_TRY(plane_launch(ys + b0, yd + b0, nb, sstride, w, h, dstride, w, h, 1, my, border, T, block, what, st, sb, fpx_y));
        VS_TRY(plane_launch(us + b0, ud + b0, nb, sstride, w / 2, h / 2, dstride, w / 2, h / 2, 2, mu, border, T ? T + sy : nullptr, block, what, st, sb, fpx_uv));
    }
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

// Whether a launch of 4:2:2 surfaces under host maps goes to the instances with the taller staged box (warp_i422_tall_kernel): some
// surface's full-width chroma tile - min(cw, 128) columns, THP rows - has a source box of floor(D) + 2 or + 3 rows, D = (THP - 1) |d| +
// (columns - 1) |c| under its inverse chroma map [a b; c d], that may outgrow the THP + 9 rows of PlaneCfg and can lie inside THP + 17.
// Below that (every tile staged as it is) and above it (direct either way) the launch keeps the instance it has always had.
static bool i420_needs_tall_box(const WarpMaps& mu, int nb, int cw, int sb) {
    const int thp = sb == 2 ? PlaneCfg<1, 2>::THP : PlaneCfg<1>::THP;
    const int cols = std::min(cw, TW);
    for (int i = 0; i < nb; i++) {
        const double* m = mu.m + (size_t)mu.stride * i;
        const double D = (thp - 1) * std::fabs(m[4]) + (cols - 1) * std::fabs(m[3]);
        if (!(D >= 0) || D > 1e6) continue;
        const int rows = (int)std::floor(D);
        if (rows + 3 > thp + 9 && rows + 2 <= thp + 17) return true;
    }
    return false;
}

// Per launch of up to 32 surfaces: the luma table and the chroma table (pointer records: the U planes) of every surface - host maps:
// the NV12 table launch; else one table launch per plane -, then all three planes in ONE grid.  A launch without tables (a caller's
// tables exist for launches of WARP_TAB_MIN surfaces and more only; the scratch tables serve any number), or one whose geometry is
// outside what warp_i420_kernel packs, goes plane by plane through the general kernels: V from the maps, without a table.
// sb = 2: I010 / I012 surfaces - the layouts stay in bytes.
int launch_warp_i420(const uint8_t* const* ys, uint8_t* const* yd, int n, I420Layout sl, I420Layout dl, int w, int h, WarpMaps maps, int border,
                     WarpTabs tabs, hipStream_t st, int sb, int sx, int sy, WarpFill fill) {
    const int cw = w >> sx, ch = h >> sy;             // a chroma plane's samples per row, and its rows
    const char* const kind = sx == 0 ? "planar 4:4:4" : sy == 0 ? "planar 4:2:2" : sb == 2 ? "warp_i010" : "warp_i420";
    if ((sx != 0 && sx != 1) || (sy != 0 && sy != 1) || sy > sx) { set_last_error("warp_planar: chroma shifts must be (1, 1), (1, 0) or (0, 0)"); return VS_ERR_INVALID_ARG; }
    if (n < 1 || !ys || !yd || w < 1 || h < 1 || cw < 1 || ch < 1 || (w & ((1 << sx) - 1)) || (h & ((1 << sy) - 1)) || (sb != 1 && sb != 2) ||
        bad_args(ys[0], yd[0], maps.m, sl.pitch, w, h, dl.pitch, w, h, sb, n) ||
        sl.cpitch < (size_t)cw * sb || dl.cpitch < (size_t)cw * sb || !sl.u || !sl.v || !dl.u || !dl.v || sl.u == sl.v || dl.u == dl.v ||
        bad_call(ys, yd, n, border, tabs, true) || (border == VS_BORDER_FILL && bad_fill(fill, sb))) {
        if (sy == 0) set_last_error(std::string("warp_planar: ") + kind + ": invalid argument (4:2:2 needs an even w; chroma pitches must hold a chroma row)");
        else set_last_error(sb == 2 ? "warp_i010: invalid argument (w and h must be even, chroma pitches at least w bytes)"
                                    : "warp_i420: invalid argument (w and h must be even, chroma pitches at least w / 2)");
        return VS_ERR_INVALID_ARG;
    }
    if (sb == 2 && (odd16(ys, yd, n, sl.pitch, dl.pitch) || ((sl.cpitch | sl.u | sl.v | dl.cpitch | dl.u | dl.v) & 1))) {
        set_last_error(sy == 0 ? "warp_planar: pointers, pitches and plane offsets of 16-bit planar surfaces must be even"
                               : "warp_i010: I010 / I012 pointers, pitches and plane offsets must be even");
        return VS_ERR_INVALID_ARG;
    }
    const int tab_min = tabs.kind == WarpTabs::SCRATCH ? 1 : WARP_TAB_MIN;
    const int block = planar_tab_ints(w, h, sx, sy), ty = tab_layout(w, h).stride;
    if (tabs.kind == WarpTabs::SCRATCH)
        VS_TRY(op_tabs(st, (size_t)block * std::min(n, MAXB) * sizeof(int32_t), &tabs.tabs));
    const WarpMaps muv = {maps.m + 6, maps.stride, maps.host};
    const size_t tab_step = tabs.kind == WarpTabs::CALLER ? block : 0;
    const uint8_t* ps[MAXB];
    uint8_t* pd[MAXB];
    for (int b0 = 0; b0 < n; b0 += MAXB) {
        const int nb = std::min(MAXB, n - b0);
        int32_t* T = tabs.kind != WarpTabs::NONE && nb >= tab_min ? tabs.tabs + b0 * tab_step : nullptr;
        if (!T && tabs.what == VS_WARP_TABLES_ONLY) continue;
        const WarpMaps my = maps_from(maps, b0), mu = maps_from(muv, b0);
        auto plane = [&](size_t so, size_t d_o, size_t sp, size_t dp, int pw, int ph, WarpMaps m, int32_t* tab, int what, uint32_t fillpx) -> int {
            for (int i = 0; i < nb; i++) { ps[i] = ys[b0 + i] + so; pd[i] = yd[b0 + i] + d_o; }
            return plane_launch(ps, pd, nb, sp, pw, ph, dp, pw, ph, 1, m, border, tab, block, what, st, sb, fillpx);
        };
        if (T && tabs.what != VS_WARP_ONLY) {
            if (maps.host && nb <= NVT_MAX && sx == 1 && sy == 1) {     // (the NV12 table launch halves both sizes)
                NvTabArgs t;
                t.tabs = T; t.block = block; t.chroma = ty; t.w = w; t.h = h; t.src_uv = sl.u; t.dst_uv = dl.u;
                for (int i = 0; i < NVT_MAX; i++) { t.ys[i] = ys[b0 + (i < nb ? i : 0)]; t.yd[i] = yd[b0 + (i < nb ? i : 0)]; }
                for (int i = 0; i < NVT_MAX * 6; i++) {
                    t.my[i] = i < 6 * nb ? my.m[(size_t)my.stride * (i / 6) + i % 6] : 0.;
                    t.muv[i] = i < 6 * nb ? mu.m[(size_t)mu.stride * (i / 6) + i % 6] : 0.;
                }
                const int entries = w + h + (w + TW - 1) / TW + (h + TH - 1) / TH;
                hipLaunchKernelGGL(warp_tables_nv12_kernel, dim3((entries + NT - 1) / NT, nb, 2), dim3(NT), 0, st, t);
            } else {
                VS_TRY(plane(0, 0, sl.pitch, dl.pitch, w, h, my, T, VS_WARP_TABLES_ONLY, fill.y));
                VS_TRY(plane(sl.u, dl.u, sl.cpitch, dl.cpitch, cw, ch, mu, T + ty, VS_WARP_TABLES_ONLY, fill.u));
            }
        }
        if (tabs.what == VS_WARP_TABLES_ONLY) continue;
        const bool tall = maps.host && sx == 1 && sy == 0 && border == VS_BORDER_REPLICATE && i420_needs_tall_box(mu, nb, cw, sb);
        const int one = T ? i420_launch(ys + b0, yd + b0, nb, sl, dl, w, h, T, border, st, sb, sx, sy, tall, fill) : VS_ERR_UNSUPPORTED;
        if (one != VS_ERR_UNSUPPORTED) {
            VS_TRY(one);
            continue;
        }
        const int what = T ? VS_WARP_ONLY : VS_WARP_ALL;
        VS_TRY(plane(0, 0, sl.pitch, dl.pitch, w, h, my, T, what, fill.y));
        VS_TRY(plane(sl.u, dl.u, sl.cpitch, dl.cpitch, cw, ch, mu, T ? T + ty : nullptr, what, fill.u));
        VS_TRY(plane(sl.v, dl.v, sl.cpitch, dl.cpitch, cw, ch, mu, nullptr, VS_WARP_ALL, fill.v));
    }
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

// What the job launchers refuse about a job (first: the launch's first job - one sample size per launch).  rgb: the launchers of
// interleaved colour jobs, 8-bit samples, cn 3 or 4.
static bool bad_job(const WarpJob& j, const WarpJob& first, bool rgb) {
    const bool bad_cn = rgb ? j.sb != 1 || (j.cn != 3 && j.cn != 4) : j.cn < 1 || j.cn > (j.sb == 2 ? 2 : 3);
    return (j.sb != 1 && j.sb != 2) || j.sb != first.sb || bad_cn ||
           bad_args(j.src, j.dst, j.m, j.sstride, j.sw, j.sh, j.dstride, j.dw, j.dh, j.cn * j.sb, 1) ||
           (j.border != VS_BORDER_BLACK && j.border != VS_BORDER_REPLICATE) ||
           (j.sb == 2 && (((uintptr_t)j.src | (uintptr_t)j.dst | j.sstride | j.dstride) & 1));
}

// n <= WARP_JOBS_MAX warps of any geometry (inverse maps in double on the host) as one launch; one sample size for all of them.
static int warp_jobs_go(const WarpJob* jobs, int n, hipStream_t st, bool rgb) {
    if (!jobs || n < 1 || n > WARP_JOBS_MAX) { set_last_error("warp_jobs: invalid argument"); return VS_ERR_INVALID_ARG; }
    WarpJobsArg a;
    int gw = 1, gh = 1;
    for (int i = 0; i < WARP_JOBS_MAX; i++) {
        a.j[i] = jobs[i < n ? i : 0];
        if (i >= n) continue;
        const WarpJob& j = jobs[i];
        if (bad_job(j, jobs[0], rgb)) {
            set_last_error("warp_jobs: invalid argument");
            return VS_ERR_INVALID_ARG;
        }
        gw = std::max(gw, (j.dw + TW - 1) / TW);
        gh = std::max(gh, (j.dh + TH - 1) / TH);
    }
    if (rgb) hipLaunchKernelGGL(warp_jobs_rgb_kernel, dim3(gw, gh, n), dim3(NT), 0, st, a);
    else if (jobs[0].sb == 2) hipLaunchKernelGGL(warp_jobs16_kernel, dim3(gw, gh, n), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(warp_jobs_kernel, dim3(gw, gh, n), dim3(NT), 0, st, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

int launch_warp_jobs(const WarpJob* jobs, int n, hipStream_t st) { return warp_jobs_go(jobs, n, st, false); }

// Samples of a source row or column that a full tile of n output samples touches at most, taps included, under the inverse scale
// factor inv (the bound in front of scale_jobs_tile).
static int scale_span(double inv, int n) { return (int)std::floor((inv * (n - 1) * 1024 + 2) / 1024) + 3; }

// Whether launch_scale_jobs sends a job to the staged kernel: a diagonal map that does not mirror, border 0, cn 1 or 2, and the box of
// a full tile - widened by the 3 + 3 samples of the aligned origin and the rounded-up pitch - inside the staging area.  That is an
// inverse factor below (SBW - 9) / (TW - 1) = 1.19 across and (SBH - 3) / (TH - 1) = 1.4 down: every zoom-in, and mild downscales.
// (the staging area is one dword per pixel whatever the pixel's size: the colour jobs, cn 3 and 4, are staged under the same bound)
static bool scale_map_staged(const WarpJob& j) {
    if (j.border != VS_BORDER_BLACK || j.m[1] != 0 || j.m[3] != 0 || !(j.m[0] > 0) || !(j.m[4] > 0)) return false;
    if (j.m[0] > 2 || j.m[4] > 2 || j.sw > 32767 || j.sh > 32767) return false;      // (far outside; sat_s16 never acts on a staged job)
    return scale_span(j.m[0], TW) + 6 <= SBW && scale_span(j.m[4], TH) <= SBH;
}
bool scale_job_staged(const WarpJob& j) { return j.cn >= 1 && j.cn <= 2 && scale_map_staged(j); }
bool scale_job_staged_rgb(const WarpJob& j) { return j.sb == 1 && (j.cn == 3 || j.cn == 4) && scale_map_staged(j); }

// The crop-and-scale jobs of a batch: those that can be staged as ONE launch of the staged kernel, the others as ONE launch of
// launch_warp_jobs - a batch of one class is one launch.  path 1: all of them through launch_warp_jobs.
// rgb: interleaved colour jobs (cn 3 or 4, 8-bit) through the colour instances of both kernels.
static int scale_jobs_go(const WarpJob* jobs, int n, int path, hipStream_t st, bool rgb) {
    if (!jobs || n < 1 || n > WARP_JOBS_MAX || (path != 0 && path != 1)) { set_last_error("scale_jobs: invalid argument"); return VS_ERR_INVALID_ARG; }
    WarpJob direct[WARP_JOBS_MAX];
    WarpJobsArg a;
    int ns = 0, nd = 0, gw = 1, gh = 1;
    for (int i = 0; i < n; i++) {
        const WarpJob& j = jobs[i];
        if (bad_job(j, jobs[0], rgb)) {
            set_last_error("scale_jobs: invalid argument");
            return VS_ERR_INVALID_ARG;
        }
        if (path == 1 || !(rgb ? scale_job_staged_rgb(j) : scale_job_staged(j))) { direct[nd++] = j; continue; }
        a.j[ns++] = j;
        gw = std::max(gw, (j.dw + TW - 1) / TW);
        gh = std::max(gh, (j.dh + TH - 1) / TH);
    }
    if (ns) {
        for (int i = ns; i < WARP_JOBS_MAX; i++) a.j[i] = a.j[0];
        if (rgb) hipLaunchKernelGGL(scale_jobs_rgb_kernel, dim3(gw, gh, ns), dim3(NT), 0, st, a);
        else if (jobs[0].sb == 2) hipLaunchKernelGGL(scale_jobs16_kernel, dim3(gw, gh, ns), dim3(NT), 0, st, a);
        else hipLaunchKernelGGL(scale_jobs_kernel, dim3(gw, gh, ns), dim3(NT), 0, st, a);
        VS_HIP_TRY(hipGetLastError());
    }
    return nd ? warp_jobs_go(direct, nd, st, rgb) : VS_OK;
}

int launch_scale_jobs(const WarpJob* jobs, int n, int path, hipStream_t st) { return scale_jobs_go(jobs, n, path, st, false); }
int launch_scale_jobs_rgb(const WarpJob* jobs, int n, int path, hipStream_t st) { return scale_jobs_go(jobs, n, path, st, true); }

}  // namespace vsd
