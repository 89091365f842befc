// Image enhancer for gfx950: counterpart of vs::Enhancer::enhanceImage
// (/root/reference/src/Enhancer.cpp:138-239; stage helpers :19-69).
//
// The reference runs every stage as its own OpenCV call over the whole frame (7 passes for its
// shipped config).  Here the stage list is compiled into as few passes over HBM as the data
// dependencies allow:
//   * per-sample stages (convertTo, white-balance scaling, gamma) are 256-entry tables;
//   * enh_unsharp_kernel<R> reads a tile + halo once, applies the tables in front of the blur,
//     runs the separable 8.8 fixed-point Gaussian (bit-exact with cv::GaussianBlur on CV_8U:
//     v_dot4 on bytes along x, v_dot2 on row pairs of 16-bit sums along y), cv::addWeighted, the
//     tables behind it, and writes the tile: 3 B/px read + 3 B/px written for
//     brightness/contrast + unsharp + gamma (the reference's config.yaml);
//   * stages that need a whole-frame statistic (white balance: channel sums; CLAHE: tile
//     histograms) get one extra read-only pass that evaluates the pending per-pixel stages on the fly;
//   * vibrance (HSV round trip) and CLAHE (Lab round trip + tile-table interpolation) are per-pixel
//     stages of enh_point_kernel;
//   * both frame kernels also exist in a form that reads and writes YUV surfaces (IO = YuvIo, or YuvIoCs under a colorimetry
//     descriptor; the conversion arithmetic of cvt_px.h on the way into the pass and out of it): a stage list that is ONE pass
//     runs on up to 32 decoder surfaces in one launch, without a BGR8 frame in between (vs_enh_apply_yuv_batch_dev).
// Nothing is computed on the host except 256-entry tables that depend on parameters only (the gamma
// table needs libm's powf, as in the reference) and the colour-conversion tables built once per object.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "cvt_px.h"
#include "launchers.h"
#include "vs_common.h"

namespace vsd {
namespace {

constexpr int E_TW = 64, E_TH = 32, E_NT = 256;   // unsharp tile: 64 x 32 px, one 4-px group x 2 rows per thread
constexpr int MAX_R = 16;                          // up to 33 taps
constexpr int CHAIN_MAX = 4, LUT_SLOTS = 4, SLOT_BYTES = 768;
enum { OP_LUT = 1, OP_VIB = 2, OP_CLAHE = 3 };
enum { SLOT_CB = 0, SLOT_GAMMA = 1, SLOT_WB = 2, SLOT_IDENT = 3 };
constexpr int MAX_TILES = 16;

// color_lab.cpp / color_hsv.simd.hpp tables (built on the host once, see build_tables)
constexpr int kLabShift = 12, kGammaShift = 3, kLabShift2 = kLabShift + kGammaShift;
constexpr int kCbrtTabSize = 256 * 3 / 2 * (1 << kGammaShift);
constexpr int kBaseShift = 14, kBase = 1 << kBaseShift;
constexpr int kInvGammaShift = 12, kInvGammaTabSize = 1 << kInvGammaShift;

struct EnhTables {
    int32_t sdiv[256], hdiv[256];
    uint16_t gamma[256];
    uint16_t cbrt_[kCbrtTabSize];
    uint16_t l2yf[512];
    uint16_t inv_gamma[kInvGammaTabSize];
    uint16_t lin_inv_gamma[kInvGammaTabSize];   // linearInvGammaTab_b (COLOR_Lab2LBGR)
    int32_t fwd[9], inv[9];
};

struct Chain { int32_t n; int32_t op[CHAIN_MAX]; int32_t slot[CHAIN_MAX]; };

struct PointCtx {
    const EnhTables* tabs;
    const uint8_t* clahe_lut;    // tiles*tiles*256
    float vib_alpha;
    int32_t tiles;
    float inv_tw, inv_th;
};

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// ---- cvtColor 8U restatements (one pixel) ------------------------------------------------------
__device__ __forceinline__ void bgr2hsv_px(const EnhTables* T, int b, int g, int r, int& ho, int& so, int& vo) {
    const int hsv_shift = 12;
    const int v = max(b, max(g, r)), vmin = min(b, min(g, r));
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    so = (diff * T->sdiv[v] + (1 << (hsv_shift - 1))) >> hsv_shift;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * T->hdiv[diff] + (1 << (hsv_shift - 1))) >> hsv_shift;
    h += h < 0 ? 180 : 0;
    ho = clamp255(h);
    vo = v;
}

__device__ __forceinline__ void hsv2bgr_px(int hb, int sb, int vb, int& bo, int& go, int& ro) {
    float h = __fmul_rn((float)hb, 6.f / 180.f);
    const float s = __fmul_rn((float)sb, 1.f / 255.f), v = __fmul_rn((float)vb, 1.f / 255.f);
    const float pre = (float)(int)h;
    h = __fsub_rn(h, pre);
    const float vs = __fmul_rn(v, s);
    const float t1 = __fsub_rn(v, vs);
    const float t2 = __fsub_rn(v, __fmul_rn(vs, h));
    const float t3 = __fadd_rn(__fsub_rn(v, vs), __fmul_rn(vs, h));
    const int sector = (int)pre % 6;
    float b, g, r;
    switch (sector) {
        case 0: b = t1; g = t3; r = v; break;
        case 1: b = t1; g = v; r = t2; break;
        case 2: b = t3; g = v; r = t1; break;
        case 3: b = v; g = t2; r = t1; break;
        case 4: b = v; g = t1; r = t3; break;
        default: b = t2; g = t1; r = v; break;
    }
    bo = clamp255(f_round(__fmul_rn(b, 255.f)));
    go = clamp255(f_round(__fmul_rn(g, 255.f)));
    ro = clamp255(f_round(__fmul_rn(r, 255.f)));
}

__device__ __forceinline__ int bgr2L(const EnhTables* T, int b, int g, int r) {
    const int Lscale = (116 * 255 + 50) / 100;
    const int Lshift = -((16 * 255 * (1 << kLabShift2) + 50) / 100);
    const int B = T->gamma[b], G = T->gamma[g], R = T->gamma[r];
    const int fY = T->cbrt_[descale(B * T->fwd[3] + G * T->fwd[4] + R * T->fwd[5], kLabShift)];
    return clamp255(descale(Lscale * fY + Lshift, kLabShift2));
}

template <bool SRGB = true>
__device__ __forceinline__ void bgr2lab_px(const EnhTables* T, int b, int g, int r, int& Lo, int& ao, int& bo) {
    const int Lscale = (116 * 255 + 50) / 100;
    const int Lshift = -((16 * 255 * (1 << kLabShift2) + 50) / 100);
    // COLOR_LBGR2Lab: linearGammaTab_b[i] = i << gamma_shift
    const int B = SRGB ? T->gamma[b] : b << kGammaShift, G = SRGB ? T->gamma[g] : g << kGammaShift, R = SRGB ? T->gamma[r] : r << kGammaShift;
    const int fX = T->cbrt_[descale(B * T->fwd[0] + G * T->fwd[1] + R * T->fwd[2], kLabShift)];
    const int fY = T->cbrt_[descale(B * T->fwd[3] + G * T->fwd[4] + R * T->fwd[5], kLabShift)];
    const int fZ = T->cbrt_[descale(B * T->fwd[6] + G * T->fwd[7] + R * T->fwd[8], kLabShift)];
    Lo = clamp255(descale(Lscale * fY + Lshift, kLabShift2));
    ao = clamp255(descale(500 * (fX - fY) + 128 * (1 << kLabShift2), kLabShift2));
    bo = clamp255(descale(200 * (fY - fZ) + 128 * (1 << kLabShift2), kLabShift2));
}

// abToXZ_b entry computed instead of tabulated (147 KB table in OpenCV)
__device__ __forceinline__ int ab2xz(int i) {
    if (i <= 3390) return i * 108 / 841 - kBase * 16 / 116 * 108 / 841;
    return i * i / kBase * i / kBase;
}

template <bool SRGB = true>
__device__ __forceinline__ void lab2bgr_px(const EnhTables* T, int LL, int aa, int bb, int& bo, int& go, int& ro) {
    const uint16_t* igt = SRGB ? T->inv_gamma : T->lin_inv_gamma;
    const int y = T->l2yf[LL * 2], ify = T->l2yf[LL * 2 + 1];
    const int adiv = ((5 * aa * 53687 + (1 << 7)) >> 13) - 128 * kBase / 500;
    const int bdiv = ((bb * 41943 + (1 << 4)) >> 9) - 128 * kBase / 200 + 1;
    const int x = ab2xz(ify + adiv), z = ab2xz(ify - bdiv);
    const int shift = kLabShift + (kBaseShift - kInvGammaShift);
    int r0 = descale(T->inv[0] * x + T->inv[1] * y + T->inv[2] * z, shift);
    int g0 = descale(T->inv[3] * x + T->inv[4] * y + T->inv[5] * z, shift);
    int b0 = descale(T->inv[6] * x + T->inv[7] * y + T->inv[8] * z, shift);
    r0 = max(0, min(kInvGammaTabSize - 1, r0));
    g0 = max(0, min(kInvGammaTabSize - 1, g0));
    b0 = max(0, min(kInvGammaTabSize - 1, b0));
    bo = clamp255(igt[b0]); go = clamp255(igt[g0]); ro = clamp255(igt[r0]);
}

// vibranceCPU, Enhancer.cpp:41-57
__device__ __forceinline__ void vib_px(const PointCtx& pc, int& b, int& g, int& r) {
    int h, s, v;
    bgr2hsv_px(pc.tabs, b, g, r, h, s, v);
    float sv = (float)s;
    sv = __fadd_rn(sv, __fmul_rn(pc.vib_alpha, __fsub_rn(255.f, sv)));
    s = clamp255(f_round(sv));
    hsv2bgr_px(h, s, v, b, g, r);
}

// CLAHE_Interpolation_Body (clahe.cpp) on the L plane, between BGR2Lab and Lab2BGR (Enhancer.cpp:59-69)
__device__ __forceinline__ void clahe_px(const PointCtx& pc, int x, int y, int& b, int& g, int& r) {
    int L, A, Bq;
    bgr2lab_px(pc.tabs, b, g, r, L, A, Bq);
    const float tyf = __fsub_rn(__fmul_rn((float)y, pc.inv_th), 0.5f);
    int ty1 = f_floor(tyf), ty2 = ty1 + 1;
    const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.0f, ya);
    ty1 = max(ty1, 0); ty2 = min(ty2, pc.tiles - 1);
    const float txf = __fsub_rn(__fmul_rn((float)x, pc.inv_tw), 0.5f);
    int tx1 = f_floor(txf), tx2 = tx1 + 1;
    const float xa = __fsub_rn(txf, (float)tx1), xa1 = __fsub_rn(1.0f, xa);
    tx1 = max(tx1, 0); tx2 = min(tx2, pc.tiles - 1);
    const uint8_t* p1 = pc.clahe_lut + (size_t)ty1 * pc.tiles * 256;
    const uint8_t* p2 = pc.clahe_lut + (size_t)ty2 * pc.tiles * 256;
    const int i1 = tx1 * 256 + L, i2 = tx2 * 256 + L;
    const float top = __fadd_rn(__fmul_rn((float)p1[i1], xa1), __fmul_rn((float)p1[i2], xa));
    const float bot = __fadd_rn(__fmul_rn((float)p2[i1], xa1), __fmul_rn((float)p2[i2], xa));
    const float res = __fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya));
    L = clamp255(f_round(res));
    lab2bgr_px(pc.tabs, L, A, Bq, b, g, r);
}

// LUT-only chain (tables in LDS)
__device__ __forceinline__ void apply_luts(const Chain& ch, const uint8_t* lut, int& b, int& g, int& r) {
#pragma unroll
    for (int k = 0; k < CHAIN_MAX; k++) {
        if (k < ch.n) {
            const uint8_t* l = lut + ch.slot[k] * SLOT_BYTES;
            b = l[b]; g = l[256 + g]; r = l[512 + r];
        }
    }
}

// general chain of per-pixel stages; (x, y) = position of the pixel in the frame (CLAHE tiles)
__device__ __forceinline__ void apply_chain(const Chain& ch, const uint8_t* lut, const PointCtx& pc, int x, int y, int& b,
                                            int& g, int& r) {
#pragma unroll
    for (int k = 0; k < CHAIN_MAX; k++) {
        if (k < ch.n) {
            const int op = ch.op[k];
            if (op == OP_LUT) {
                const uint8_t* l = lut + ch.slot[k] * SLOT_BYTES;
                b = l[b]; g = l[256 + g]; r = l[512 + r];
            } else if (op == OP_VIB) {
                vib_px(pc, b, g, r);
            } else {
                clahe_px(pc, x, y, b, g, r);
            }
        }
    }
}

__device__ __forceinline__ void load_luts(uint8_t* s_lut, const uint8_t* g_lut, int tid, int nthreads) {
    const uint32_t* s = (const uint32_t*)g_lut;
    uint32_t* d = (uint32_t*)s_lut;
    for (int i = tid; i < LUT_SLOTS * SLOT_BYTES / 4; i += nthreads) d[i] = s[i];
}

// 4 interleaved BGR pixels <-> three dwords
__device__ __forceinline__ void unpack12(uint32_t d0, uint32_t d1, uint32_t d2, int* b, int* g, int* r) {
    b[0] = d0 & 255; g[0] = (d0 >> 8) & 255; r[0] = (d0 >> 16) & 255;
    b[1] = d0 >> 24; g[1] = d1 & 255; r[1] = (d1 >> 8) & 255;
    b[2] = (d1 >> 16) & 255; g[2] = d1 >> 24; r[2] = d2 & 255;
    b[3] = (d2 >> 8) & 255; g[3] = (d2 >> 16) & 255; r[3] = d2 >> 24;
}
__device__ __forceinline__ void pack12(const int* b, const int* g, const int* r, uint32_t& d0, uint32_t& d1, uint32_t& d2) {
    d0 = (uint32_t)b[0] | ((uint32_t)g[0] << 8) | ((uint32_t)r[0] << 16) | ((uint32_t)b[1] << 24);
    d1 = (uint32_t)g[1] | ((uint32_t)r[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)g[2] << 24);
    d2 = (uint32_t)r[2] | ((uint32_t)b[3] << 8) | ((uint32_t)g[3] << 16) | ((uint32_t)r[3] << 24);
}

typedef const uint8_t __attribute__((address_space(1)))* gptr_c;   // global address space: global_load/store, not flat
typedef uint8_t __attribute__((address_space(1)))* gptr;

// ---- YUV surfaces as the source and the destination of the two frame kernels (vs_enh_apply_yuv_batch_dev) -----------------------
// n surfaces of one format and geometry; the layouts are those cvt_check_yuv resolved (NV12 / P010: u = the interleaved plane).
// Everything here is wave-uniform: the format's layout travels as kernel arguments, not as template parameters (the unsharp
// kernel already has sixteen instances).  Row offsets inside a plane are 32-bit; the host sends larger surfaces the other way.
struct YuvIo {
    const uint8_t* src[CVT_MAX_SURFACES];
    uint8_t* dst[CVT_MAX_SURFACES];
    size_t su, sv, du, dv;                // plane offsets behind the surface pointer
    uint32_t spitch, scpitch, dpitch, dcpitch;
    int32_t sb, il, sx, sy, shift;        // bytes per sample; (U, V) interleaved; chroma plane (w >> sx) x (h >> sy); 16-bit: byte = min(sample >> shift, 255)
};
// ... with a colour space of its own (vs_enh_set_yuv_colorimetry).  The default - BT.601 limited, top-left chroma - keeps YuvIo and
// with it the literal constants and the code without block sums: reading the integers from the arguments cost the two kernels
// 4 % and 10 % (DESIGN section 8 "Colorimetry"), which the surfaces that need no descriptor do not pay.
struct YuvIoCs : YuvIo {
    CvtCoef k;
};
// the integers an IO converts with, and whether chroma is the mean of a block
template <class IO>
__device__ __forceinline__ CvtCoef yuv_coef(const IO& io) {
    if constexpr (std::is_same<IO, YuvIoCs>::value) return io.k;
    else return cvt_coef_default();
}
template <class IO>
__device__ __forceinline__ bool yuv_mean(const IO& io) {
    if constexpr (std::is_same<IO, YuvIoCs>::value) return io.k.mean != 0;
    else return false;
}

typedef const uint16_t __attribute__((address_space(1)))* gptr16_c;
typedef uint16_t __attribute__((address_space(1)))* gptr16;
typedef const uint32_t __attribute__((address_space(1)))* gptr32_c;
typedef uint32_t __attribute__((address_space(1)))* gptr32;

// one sample, and runs of two and of four consecutive samples, as bytes (sample i in byte i of the result).  A run whose address
// is aligned moves as dwords (16-bit words for two 8-bit samples); any other goes sample by sample, as in k_cvt.hip.
template <int SB>
__device__ __forceinline__ uint32_t yuv_ld1(gptr_c p, int shift) {
    if constexpr (SB == 1) return *p;
    else return (uint32_t)cvt_sample_to_byte((int)*(gptr16_c)p, shift);
}
template <int SB>
__device__ __forceinline__ uint32_t yuv_ld2(gptr_c p, int shift) {
    if constexpr (SB == 1) {
        if (((uintptr_t)p & 1) == 0) return *(gptr16_c)p;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    } else {
        uint32_t a;
        if (((uintptr_t)p & 3) == 0) a = *(gptr32_c)p;
        else a = (uint32_t)((gptr16_c)p)[0] | ((uint32_t)((gptr16_c)p)[1] << 16);
        return (uint32_t)cvt_sample_to_byte((int)(a & 0xffffu), shift) | ((uint32_t)cvt_sample_to_byte((int)(a >> 16), shift) << 8);
    }
}
template <int SB>
__device__ __forceinline__ uint32_t yuv_ld4(gptr_c p, int shift) {
    if constexpr (SB == 1) {
        if (((uintptr_t)p & 3) == 0) return *(gptr32_c)p;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    } else {
        uint32_t a, b;
        if (((uintptr_t)p & 3) == 0) { a = ((gptr32_c)p)[0]; b = ((gptr32_c)p)[1]; }
        else {
            gptr16_c q = (gptr16_c)p;
            a = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
            b = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
        }
        return (uint32_t)cvt_sample_to_byte((int)(a & 0xffffu), shift) | ((uint32_t)cvt_sample_to_byte((int)(a >> 16), shift) << 8) |
               ((uint32_t)cvt_sample_to_byte((int)(b & 0xffffu), shift) << 16) | ((uint32_t)cvt_sample_to_byte((int)(b >> 16), shift) << 24);
    }
}
// N = 2 or 4 samples from the bytes of v, the first `valid` of them inside the row: nothing beyond them is written
template <int SB, int N>
__device__ __forceinline__ void yuv_st(gptr p, int valid, int shift, uint32_t v) {
    static_assert(N == 2 || N == 4, "runs of two or four samples");
    if (valid == N && ((uintptr_t)p & (SB * N == 2 ? 1 : 3)) == 0) {
        if constexpr (SB == 1 && N == 2) *(gptr16)p = (uint16_t)v;
        else if constexpr (SB == 1) *(gptr32)p = v;
        else {
            ((gptr32)p)[0] = cvt_byte_to_sample(v & 255u, shift) | (cvt_byte_to_sample((v >> 8) & 255u, shift) << 16);
            if constexpr (N == 4) ((gptr32)p)[1] = cvt_byte_to_sample((v >> 16) & 255u, shift) | (cvt_byte_to_sample(v >> 24, shift) << 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (i < valid) {
                const uint32_t b = (v >> (8 * i)) & 255u;
                if constexpr (SB == 1) p[i] = (uint8_t)b;
                else ((gptr16)p)[i] = (uint16_t)cvt_byte_to_sample(b, shift);
            }
        }
    }
}

// how the chroma of a format lies: one plane of interleaved (U, V) pairs, or two planes with a sample per two / per one pixel
enum { YL_UV = 0, YL_HALF = 1, YL_FULL = 2 };
template <int SB_, int LAY_> struct YuvLay { static constexpr int SB = SB_, LAY = LAY_; };
// calls f with the layout of y as a type: six straight-line variants behind one wave-uniform branch
template <class F>
__device__ __forceinline__ void yuv_dispatch(const YuvIo& y, F&& f) {
    if (y.sb == 1) {
        if (y.il) f(YuvLay<1, YL_UV>{});
        else if (y.sx) f(YuvLay<1, YL_HALF>{});
        else f(YuvLay<1, YL_FULL>{});
    } else {
        if (y.il) f(YuvLay<2, YL_UV>{});
        else if (y.sx) f(YuvLay<2, YL_HALF>{});
        else f(YuvLay<2, YL_FULL>{});
    }
}

struct YuvPlanes { gptr_c y, u, v; };          // v of an interleaved plane: the sample behind u
struct YuvPlanesOut { gptr y, u, v; };

// The unit of both kernels - pixels px .. px + 3 of luma row `row`, px a multiple of 4 - as three dwords: the four luma bytes and,
// per pixel, the bytes of the chroma sample at (x >> sx, row >> sy) (CHROMA = false: the luma dword alone).  Inside the row the
// samples move as runs; a unit that crosses an edge takes the pixels at reflect101(x, w), one by one.
template <class L, bool CHROMA = true>
__device__ __forceinline__ void yuv_load_unit(const YuvIo& io, const YuvPlanes& s, int row, int px, int w, uint32_t (&raw)[3]) {
    constexpr int SB = L::SB;
    const uint32_t yoff = (uint32_t)row * io.spitch, coff = (uint32_t)(row >> io.sy) * io.scpitch;
    if (px >= 0 && px + 3 < w) {
        raw[0] = yuv_ld4<SB>(s.y + (yoff + (uint32_t)px * SB), io.shift);
        if constexpr (!CHROMA) {
        } else if constexpr (L::LAY == YL_UV) {
            const uint32_t t = yuv_ld4<SB>(s.u + (coff + (uint32_t)px * SB), io.shift);       // U0 V0 U1 V1
            raw[1] = (t & 255u) * 0x0101u | ((t >> 16) & 255u) * 0x01010000u;
            raw[2] = ((t >> 8) & 255u) * 0x0101u | (t >> 24) * 0x01010000u;
        } else if constexpr (L::LAY == YL_HALF) {
            const uint32_t cb = coff + (uint32_t)(px >> 1) * SB;
            const uint32_t tu = yuv_ld2<SB>(s.u + cb, io.shift), tv = yuv_ld2<SB>(s.v + cb, io.shift);
            raw[1] = (tu & 255u) * 0x0101u | (tu >> 8) * 0x01010000u;
            raw[2] = (tv & 255u) * 0x0101u | (tv >> 8) * 0x01010000u;
        } else {
            raw[1] = yuv_ld4<SB>(s.u + (coff + (uint32_t)px * SB), io.shift);
            raw[2] = yuv_ld4<SB>(s.v + (coff + (uint32_t)px * SB), io.shift);
        }
    } else {
        constexpr int CSTEP = L::LAY == YL_UV ? 2 * SB : SB;
        raw[0] = 0;
        if constexpr (CHROMA) raw[1] = raw[2] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int xi = reflect101(px + i, w);
            raw[0] |= yuv_ld1<SB>(s.y + (yoff + (uint32_t)xi * SB), io.shift) << (8 * i);
            if constexpr (CHROMA) {
                const uint32_t cb = coff + (uint32_t)(L::LAY == YL_FULL ? xi : xi >> 1) * CSTEP;
                raw[1] |= yuv_ld1<SB>(s.u + cb, io.shift) << (8 * i);
                raw[2] |= yuv_ld1<SB>(s.v + cb, io.shift) << (8 * i);
            }
        }
    }
}

// ... and as four B, G, R pixels (the YUV -> BGR formulas of the header)
__device__ __forceinline__ void yuv_unit_to_bgr(const CvtCoef& k, const uint32_t (&raw)[3], int* b, int* g, int* r) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int ru, gu, bu;
        cvt_chroma_terms(k, (int)((raw[1] >> (8 * i)) & 255u), (int)((raw[2] >> (8 * i)) & 255u), ru, gu, bu);
        cvt_yuv_px(k, (int)((raw[0] >> (8 * i)) & 255u), ru, gu, bu, r[i], g[i], b[i]);
    }
}

// Four results of luma row `row` at pixels px .. px + 3 (px a multiple of 4) through the RGB -> YUV formulas: Y of every pixel, and
// the chroma of the blocks these pixels lie in.  top / last: `row` is the first / the last row of its chroma blocks (both with
// sy = 0).  Top-left rule: U and V of the pixel at the left of each block, stored with the top row.  Mean rule (yuv_mean(io)): `sum`
// carries the R, G, B sums of the two blocks from the top row to the last, where U and V are stored; the caller keeps it across
// the rows of a block and reads nothing from it.
template <class L, class IO>
__device__ __forceinline__ void yuv_store_unit(const IO& io, const YuvPlanesOut& d, int row, int px, int w, const int* b, const int* g,
                                               const int* r, bool top, bool last, int (&sum)[2][3]) {
    constexpr int SB = L::SB;
    const CvtCoef k = yuv_coef(io);
    const int valid = min(4, w - px);
    uint32_t y4 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) y4 |= (uint32_t)cvt_luma(k, r[i], g[i], b[i]) << (8 * i);
    yuv_st<SB, 4>(d.y + ((uint32_t)row * io.dpitch + (uint32_t)px * SB), valid, io.shift, y4);
    const bool mean = yuv_mean(io);
    if (!mean && !top) return;
    const uint32_t coff = (uint32_t)(row >> io.sy) * io.dcpitch;
    if constexpr (L::LAY == YL_FULL) {                 // one pixel per block: the two rules are one
        uint32_t u4 = 0, v4 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int u, v;
            cvt_chroma(k, r[i], g[i], b[i], 0, u, v);
            u4 |= (uint32_t)u << (8 * i); v4 |= (uint32_t)v << (8 * i);
        }
        yuv_st<SB, 4>(d.u + (coff + (uint32_t)px * SB), valid, io.shift, u4);
        yuv_st<SB, 4>(d.v + (coff + (uint32_t)px * SB), valid, io.shift, v4);
    } else {
        if (mean) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int tr = r[2 * j] + r[2 * j + 1], tg = g[2 * j] + g[2 * j + 1], tb = b[2 * j] + b[2 * j + 1];
                sum[j][0] = top ? tr : sum[j][0] + tr;
                sum[j][1] = top ? tg : sum[j][1] + tg;
                sum[j][2] = top ? tb : sum[j][2] + tb;
            }
            if (!last) return;
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) { sum[j][0] = r[2 * j]; sum[j][1] = g[2 * j]; sum[j][2] = b[2 * j]; }
        }
        const int sh = mean ? 1 + io.sy : 0;
        int u0, v0, u1, v1;
        cvt_chroma(k, sum[0][0], sum[0][1], sum[0][2], sh, u0, v0);
        cvt_chroma(k, sum[1][0], sum[1][1], sum[1][2], sh, u1, v1);
        if constexpr (L::LAY == YL_UV) {
            yuv_st<SB, 4>(d.u + (coff + (uint32_t)px * SB), 2 * (valid >> 1), io.shift,
                          (uint32_t)u0 | ((uint32_t)v0 << 8) | ((uint32_t)u1 << 16) | ((uint32_t)v1 << 24));
        } else {
            const uint32_t cb = coff + (uint32_t)(px >> 1) * SB;
            yuv_st<SB, 2>(d.u + cb, valid >> 1, io.shift, (uint32_t)u0 | ((uint32_t)u1 << 8));
            yuv_st<SB, 2>(d.v + cb, valid >> 1, io.shift, (uint32_t)v0 | ((uint32_t)v1 << 8));
        }
    }
}

__device__ __forceinline__ YuvPlanes yuv_src_planes(const YuvIo& io, int k) {
    gptr_c p = (gptr_c)io.src[k];
    return YuvPlanes{p, p + io.su, io.il ? p + io.su + io.sb : p + io.sv};
}
__device__ __forceinline__ YuvPlanesOut yuv_dst_planes(const YuvIo& io, int k) {
    gptr p = (gptr)io.dst[k];
    return YuvPlanesOut{p, p + io.du, io.il ? p + io.du + io.sb : p + io.dv};
}

// ---- unsharp tile kernel ------------------------------------------------------------------------
struct UnsharpArgs {
    const uint8_t* src; uint8_t* dst;
    const ImgPair* table;                 // optional: (src, dst) of frame blockIdx.z
    size_t sstride, dstride;
    int32_t w, h;
    const uint8_t* luts;
    Chain pre, post;                      // OP_LUT only
    uint32_t wq[(2 * MAX_R + 1 + 3) / 4];  // taps packed 4 per dword, first tap in byte 0
    uint32_t we[MAX_R + 1], wo[MAX_R + 1]; // (k[2j], k[2j+1]) and (k[2j-1], k[2j]) as 16-bit halves
    float alpha, beta;                    // addWeighted(src, alpha, blurred, beta, 0)
    int32_t src_aligned, dst_aligned, ident;
};

__device__ __forceinline__ uint32_t udot2(uint32_t a, uint32_t b, uint32_t c) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b), c, false);
}

// One composed table per side of the blur at fixed LDS addresses: lookups need no address arithmetic.
__device__ __forceinline__ void compose_luts(const Chain& ch, const uint8_t* g_lut, uint8_t* s_tab, int tid) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int v = tid;
#pragma unroll
        for (int k = 0; k < CHAIN_MAX; k++)
            if (k < ch.n) v = g_lut[ch.slot[k] * SLOT_BYTES + c * 256 + v];
        s_tab[c * 256 + tid] = (uint8_t)v;
    }
}

struct NoYuv {};     // the BGR8 form: samples come from and go to a.src / a.dst (or a.table)

// One tile of either form.  IO = NoYuv: interleaved BGR8 frames.  IO = YuvIo: blockIdx.z = surface (a.src, a.dst, a.table, the strides
// and the alignment flags are not read); the staging converts the samples of a YUV surface on their way into the planes (which
// hold B, G, R bytes as before: LDS does not grow), the store side converts the results back.
template <int R, class IO>
__global__ __launch_bounds__(E_NT) void enh_unsharp_kernel(const UnsharpArgs a, const IO io) {
    constexpr bool YUV = !std::is_same<IO, NoYuv>::value;
    constexpr int RA = (R + 3) / 4 * 4;             // halo along x rounded up to whole 4-px groups
    constexpr int SW = E_TW + 2 * RA, SH = E_TH + 2 * R, GW = SW / 4;
    constexpr int N = 2 * R + 1, NQ = (N + 3) / 4;
    constexpr int NDW = ((RA + R + 3) >> 2) + 1;    // dwords of a staged row one output group reads
    constexpr int NU = SH * GW, NRND = (NU + E_NT - 1) / E_NT;
    constexpr int HP = SH / 2;                      // row pairs
    __shared__ uint32_t s_plane[3 * SH][GW];        // staged samples behind the front table, 4 px per dword; row c*SH + y
    __shared__ uint32_t s_h2[3 * HP][E_TW];         // horizontal sums of rows (2p, 2p+1) as (lo, hi) halves; row c*HP + p
    __shared__ uint8_t s_pre[SLOT_BYTES], s_post[SLOT_BYTES];

    const int tid = threadIdx.x;
    gptr_c src = nullptr;
    gptr dst = nullptr;
    if constexpr (!YUV) {
        src = (gptr_c)a.src;
        dst = (gptr)a.dst;
        if (a.table) { src = (gptr_c)a.table[blockIdx.z].src; dst = (gptr)a.table[blockIdx.z].dst; }
    }
    const int x0 = blockIdx.x * E_TW, y0 = blockIdx.y * E_TH;
    const bool has_pre = a.pre.n > 0, has_post = a.post.n > 0;

    // 1a. raw loads of tile + halo (all rounds in flight), table composition meanwhile
    uint32_t raw[NRND][3];
    if constexpr (YUV) {
        const YuvPlanes sp = yuv_src_planes(io, blockIdx.z);
        yuv_dispatch(io, [&](auto lay) {
#pragma unroll
            for (int k = 0; k < NRND; k++) {
                const int u = tid + k * E_NT;
                raw[k][0] = raw[k][1] = raw[k][2] = 0;
                if (NU % E_NT == 0 || u < NU) {
                    const int ry = u / GW, gx = u - ry * GW;
                    int sy = y0 - R + ry;
                    if ((unsigned)sy >= (unsigned)a.h) sy = reflect101(sy, a.h);
                    yuv_load_unit<decltype(lay)>(io, sp, sy, x0 - RA + 4 * gx, a.w, raw[k]);
                }
            }
        });
    } else {
#pragma unroll
        for (int k = 0; k < NRND; k++) {
            const int u = tid + k * E_NT;
            raw[k][0] = raw[k][1] = raw[k][2] = 0;
            if (NU % E_NT == 0 || u < NU) {
                const int ry = u / GW, gx = u - ry * GW;
                int sy = y0 - R + ry;
                if ((unsigned)sy >= (unsigned)a.h) sy = reflect101(sy, a.h);
                const int px = x0 - RA + 4 * gx;
                const uint32_t roff = (uint32_t)sy * (uint32_t)a.sstride;
                if (a.src_aligned && px >= 0 && px + 3 < a.w) {
                    const uint32_t __attribute__((address_space(1)))* p =
                        (const uint32_t __attribute__((address_space(1)))*)(src + (roff + (uint32_t)px * 3u));
                    raw[k][0] = p[0]; raw[k][1] = p[1]; raw[k][2] = p[2];
                } else {
                    uint32_t by[12];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        gptr_c q = src + (roff + (uint32_t)reflect101(px + i, a.w) * 3u);
                        by[3 * i] = q[0]; by[3 * i + 1] = q[1]; by[3 * i + 2] = q[2];
                    }
                    raw[k][0] = by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24);
                    raw[k][1] = by[4] | (by[5] << 8) | (by[6] << 16) | (by[7] << 24);
                    raw[k][2] = by[8] | (by[9] << 8) | (by[10] << 16) | (by[11] << 24);
                }
            }
        }
    }
    if (has_pre) compose_luts(a.pre, a.luts, s_pre, tid);
    if (has_post) compose_luts(a.post, a.luts, s_post, tid);
    __syncthreads();

    // 1b. front table, interleaved -> planar
#pragma unroll
    for (int k = 0; k < NRND; k++) {
        const int u = tid + k * E_NT;
        if (NU % E_NT == 0 || u < NU) {
            const int ry = u / GW, gx = u - ry * GW;
            int b[4], g[4], r[4];
            if constexpr (YUV) yuv_unit_to_bgr(yuv_coef(io), raw[k], b, g, r);
            else unpack12(raw[k][0], raw[k][1], raw[k][2], b, g, r);
            if (has_pre) {
#pragma unroll
                for (int i = 0; i < 4; i++) { b[i] = s_pre[b[i]]; g[i] = s_pre[256 + g[i]]; r[i] = s_pre[512 + r[i]]; }
            }
            s_plane[ry][gx] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
            s_plane[SH + ry][gx] = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16) | ((uint32_t)g[3] << 24);
            s_plane[2 * SH + ry][gx] = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
        }
    }
    __syncthreads();

    // 2. horizontal pass: exact 16-bit sums (kernel sums to 256); item = (row pair of one channel, 4-px group)
    if (!a.ident) {
        const int g = tid & 15;
        for (int pr = tid >> 4; pr < 3 * HP; pr += E_NT / 16) {
            uint32_t hsum[2][4];
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                uint32_t D[NDW];
#pragma unroll
                for (int k = 0; k < NDW; k++) D[k] = s_plane[2 * pr + rr][g + k];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const int s = RA - R + o + 4 * q;
                        const int idx = s >> 2, sh = s & 3;
                        const uint32_t lo = D[idx];
                        const uint32_t hi = (idx + 1 < NDW) ? D[(idx + 1 < NDW) ? idx + 1 : idx] : 0u;
                        const uint32_t win = sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
                        acc = __builtin_amdgcn_udot4(win, a.wq[q], acc, false);
                    }
                    hsum[rr][o] = acc;
                }
            }
            uint4 v;
            v.x = hsum[0][0] | (hsum[1][0] << 16);
            v.y = hsum[0][1] | (hsum[1][1] << 16);
            v.z = hsum[0][2] | (hsum[1][2] << 16);
            v.w = hsum[0][3] | (hsum[1][3] << 16);
            *(uint4*)&s_h2[pr][4 * g] = v;
        }
        __syncthreads();
    }

    // 3. vertical pass on row pairs + addWeighted + back table + store: thread = (4-px group, row pair)
    const int g = tid & 15, P = tid >> 4;
    const int xg = x0 + 4 * g, yA = y0 + 2 * P;
    if (xg >= a.w || yA >= a.h) return;
    uint32_t idx[2][3][4];                         // results as integers 0..255
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t sA = s_plane[c * SH + 2 * P + R][RA / 4 + g], sB = s_plane[c * SH + 2 * P + R + 1][RA / 4 + g];
        float fa[4], fb[4], ba[4], bb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { fa[i] = (float)((sA >> (8 * i)) & 255u); fb[i] = (float)((sB >> (8 * i)) & 255u); }
        if (a.ident) {
#pragma unroll
            for (int i = 0; i < 4; i++) { ba[i] = fa[i]; bb[i] = fb[i]; }
        } else {
            uint32_t accE[4] = {32768u, 32768u, 32768u, 32768u}, accO[4] = {32768u, 32768u, 32768u, 32768u};
#pragma unroll
            for (int j = 0; j <= R; j++) {
                const uint4 v = *(const uint4*)&s_h2[c * HP + P + j][4 * g];
                const uint32_t e = a.we[j], o = a.wo[j];
                accE[0] = udot2(v.x, e, accE[0]); accO[0] = udot2(v.x, o, accO[0]);
                accE[1] = udot2(v.y, e, accE[1]); accO[1] = udot2(v.y, o, accO[1]);
                accE[2] = udot2(v.z, e, accE[2]); accO[2] = udot2(v.z, o, accO[2]);
                accE[3] = udot2(v.w, e, accE[3]); accO[3] = udot2(v.w, o, accO[3]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { ba[i] = (float)((accE[i] >> 16) & 255u); bb[i] = (float)((accO[i] >> 16) & 255u); }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // v_cvt_pk_u8_f32: round to nearest even and saturate to 0..255 = saturate_cast<uchar>(cvRound(x))
            idx[0][c][i] = __builtin_amdgcn_cvt_pk_u8_f32(__fmaf_rn(fa[i], a.alpha, __fmul_rn(ba[i], a.beta)), 0, 0);
            idx[1][c][i] = __builtin_amdgcn_cvt_pk_u8_f32(__fmaf_rn(fb[i], a.alpha, __fmul_rn(bb[i], a.beta)), 0, 0);
        }
    }
    int csum[2][3] = {};                           // YUV, mean chroma: the block sums, carried from the top row to the last
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        if (yA + rr >= a.h) break;
        int ob[4], og[4], orr[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ob[i] = has_post ? s_post[idx[rr][0][i]] : idx[rr][0][i];
            og[i] = has_post ? s_post[256 + idx[rr][1][i]] : idx[rr][1][i];
            orr[i] = has_post ? s_post[512 + idx[rr][2][i]] : idx[rr][2][i];
        }
        if constexpr (YUV) {
            const YuvPlanesOut dp = yuv_dst_planes(io, blockIdx.z);
            yuv_dispatch(io, [&](auto lay) { yuv_store_unit<decltype(lay)>(io, dp, yA + rr, xg, a.w, ob, og, orr, rr == 0 || !io.sy, rr == 1 || !io.sy, csum); });
        } else {
            gptr drow = dst + ((uint32_t)(yA + rr) * (uint32_t)a.dstride + (uint32_t)xg * 3u);
            if (a.dst_aligned && xg + 3 < a.w) {
                uint32_t d0, d1, d2;
                pack12(ob, og, orr, d0, d1, d2);
                uint32_t __attribute__((address_space(1)))* q = (uint32_t __attribute__((address_space(1)))*)drow;
                q[0] = d0; q[1] = d1; q[2] = d2;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (xg + i < a.w) { drow[3 * i] = (uint8_t)ob[i]; drow[3 * i + 1] = (uint8_t)og[i]; drow[3 * i + 2] = (uint8_t)orr[i]; }
            }
        }
    }
}

// ---- per-pixel kernel, channel sums, CLAHE histograms ---------------------------------------------
// rows per workgroup (256 threads = 64 groups of 4 px x 4 rows per step): few for one frame (more workgroups in flight),
// many when the launch is large anyway or ends in atomics
constexpr int P_ROWS_SMALL = 8, P_ROWS_LARGE = 32;

struct PointArgs {
    const uint8_t* src; uint8_t* dst;
    const ImgPair* table;
    size_t sstride, dstride;
    int32_t w, h;
    const uint8_t* luts;
    Chain chain;
    PointCtx pc;
    int32_t src_aligned, dst_aligned;
    int32_t heavy;                  // chain has a non-table stage
    int32_t rows;                   // rows per workgroup (multiple of 4)
    unsigned long long* sums;       // sums kernel: 3 accumulators
};

// IO = NoYuv: interleaved BGR8 frames.  IO = YuvIo: blockIdx.z = surface (a.src, a.dst, a.table, the strides and the alignment flags
// are not read); a thread covers its four pixels in the 1 << sy rows that share a chroma row (a.rows
// and blockIdx.y count chroma rows) and holds every sample of that block in registers before it stores the first, so a surface
// may be converted in place.
template <bool SUMS, class IO>
__global__ __launch_bounds__(256) void enh_point_kernel(const PointArgs a, const IO io) {
    constexpr bool YUV = !std::is_same<IO, NoYuv>::value;
    static_assert(!(SUMS && YUV), "the channel sums are taken on BGR8 frames");
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[LUT_SLOTS * SLOT_BYTES];   // heavy chains: every slot; else [0,768): the composed table
    __shared__ unsigned long long s_sum[3];
    const int tid = threadIdx.x;
    const uint8_t* src = nullptr;
    uint8_t* dst = nullptr;
    if constexpr (!YUV) {
        src = a.src;
        dst = a.dst;
        if (a.table) { src = (const uint8_t*)a.table[blockIdx.z].src; dst = (uint8_t*)a.table[blockIdx.z].dst; }
    }
    if (a.heavy) load_luts(s_lut, a.luts, tid, 256);
    else compose_luts(a.chain, a.luts, s_lut, tid);
    if (SUMS && tid < 3) s_sum[tid] = 0;
    __syncthreads();
    const int gx = tid & 63, ry = tid >> 6;
    const int px = (blockIdx.x * 64 + gx) * 4;
    unsigned int acc[3] = {0, 0, 0};
    if constexpr (YUV) {
        if (px < a.w) {
            const YuvPlanes sp = yuv_src_planes(io, blockIdx.z);
            const YuvPlanesOut dp = yuv_dst_planes(io, blockIdx.z);
            const int crows = a.h >> io.sy;
            for (int k = 0; k < a.rows / 4; k++) {
                const int cy = blockIdx.y * a.rows + k * 4 + ry;
                if (cy >= crows) break;
                const int y0 = cy << io.sy;
                uint32_t raw0[3], raw1[3] = {0, 0, 0};
                yuv_dispatch(io, [&](auto lay) {
                    yuv_load_unit<decltype(lay)>(io, sp, y0, px, a.w, raw0);
                    if (io.sy) yuv_load_unit<decltype(lay), false>(io, sp, y0 + 1, px, a.w, raw1);
                });
                raw1[1] = raw0[1]; raw1[2] = raw0[2];
                int csum[2][3] = {};                // mean chroma: the block sums, carried from the top row to the last
                auto row = [&](const uint32_t (&raw)[3], int y, bool top, bool last) {
                    int b[4], g[4], r[4];
                    yuv_unit_to_bgr(yuv_coef(io), raw, b, g, r);
                    if (a.heavy) {
#pragma unroll
                        for (int i = 0; i < 4; i++) apply_chain(a.chain, s_lut, a.pc, px + i, y, b[i], g[i], r[i]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; i++) { b[i] = s_lut[b[i]]; g[i] = s_lut[256 + g[i]]; r[i] = s_lut[512 + r[i]]; }
                    }
                    yuv_dispatch(io, [&](auto lay) { yuv_store_unit<decltype(lay)>(io, dp, y, px, a.w, b, g, r, top, last, csum); });
                };
                row(raw0, y0, true, !io.sy);
                if (io.sy) row(raw1, y0 + 1, false, true);
            }
        }
        return;
    }
    if (px < a.w) {
        for (int k = 0; k < a.rows / 4; k++) {
            const int y = blockIdx.y * a.rows + k * 4 + ry;
            if (y >= a.h) break;
            const uint8_t* row = src + (size_t)y * a.sstride + (size_t)px * 3;
            int b[4], g[4], r[4];
            const bool full = px + 3 < a.w;
            if (a.src_aligned && full) {
                const uint32_t* p = (const uint32_t*)row;
                unpack12(p[0], p[1], p[2], b, g, r);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int xi = min(px + i, a.w - 1);
                    const uint8_t* q = src + (size_t)y * a.sstride + (size_t)xi * 3;
                    b[i] = q[0]; g[i] = q[1]; r[i] = q[2];
                }
            }
            if (a.heavy) {
#pragma unroll
                for (int i = 0; i < 4; i++) apply_chain(a.chain, s_lut, a.pc, px + i, y, b[i], g[i], r[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) { b[i] = s_lut[b[i]]; g[i] = s_lut[256 + g[i]]; r[i] = s_lut[512 + r[i]]; }
            }
            if (SUMS) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (px + i < a.w) { acc[0] += b[i]; acc[1] += g[i]; acc[2] += r[i]; }
            } else {
                uint8_t* drow = dst + (size_t)y * a.dstride + (size_t)px * 3;
                if (a.dst_aligned && full) {
                    uint32_t d0, d1, d2;
                    pack12(b, g, r, d0, d1, d2);
                    uint32_t* q = (uint32_t*)drow;
                    q[0] = d0; q[1] = d1; q[2] = d2;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (px + i < a.w) { drow[3 * i] = (uint8_t)b[i]; drow[3 * i + 1] = (uint8_t)g[i]; drow[3 * i + 2] = (uint8_t)r[i]; }
                }
            }
        }
    }
    if (SUMS) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            unsigned int v = acc[c];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((tid & 63) == 0) atomicAdd(&s_sum[c], (unsigned long long)v);
        }
        __syncthreads();
        if (tid < 3) atomicAdd(&a.sums[tid], s_sum[tid]);
    }
}


// whiteBalanceCPU (Enhancer.cpp:22-39): table of `ch *= scale` from the channel sums
__global__ void enh_wb_lut_kernel(const unsigned long long* sums, unsigned long long npix, float alpha, uint8_t* lut) {
    const int i = threadIdx.x;
    double m[3];
    for (int c = 0; c < 3; c++) m[c] = (double)sums[c] / (double)npix;
    const double gray = (m[0] + m[1] + m[2]) / 3.0;
    for (int c = 0; c < 3; c++) {
        double s = gray / (m[c] + 1e-6);
        s = 1.0 + (double)alpha * (s - 1.0);
        const float af = (float)s;
        lut[c * 256 + i] = (uint8_t)clamp255(f_round(__fmaf_rn((float)i, af, 0.f)));
    }
}

struct HistArgs {
    const uint8_t* src;
    size_t sstride;
    int32_t w, h;
    const uint8_t* luts;
    Chain chain;
    PointCtx pc;
    int32_t heavy;
    int32_t tiles, tw, th, rows_per_block;
    unsigned int* hist;     // tiles*tiles*256
};

// CLAHE_CalcLut_Body histogram part: L of the (reflect-101 padded) tile, clahe.cpp
__global__ __launch_bounds__(256) void enh_hist_kernel(const HistArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[LUT_SLOTS * SLOT_BYTES];
    __shared__ unsigned int s_hist[256];
    const int tid = threadIdx.x;
    load_luts(s_lut, a.luts, tid, 256);
    s_hist[tid] = 0;
    __syncthreads();
    const int k = blockIdx.x, ty = k / a.tiles, tx = k - ty * a.tiles;
    const int r0 = blockIdx.y * a.rows_per_block, r1 = min(r0 + a.rows_per_block, a.th);
    const int npx = (r1 - r0) * a.tw;
    for (int i = tid; i < npx; i += 256) {
        const int yy = r0 + i / a.tw, xx = i - (i / a.tw) * a.tw;
        const int x = reflect101(tx * a.tw + xx, a.w), y = reflect101(ty * a.th + yy, a.h);
        const uint8_t* q = a.src + (size_t)y * a.sstride + (size_t)x * 3;
        int b = q[0], g = q[1], r = q[2];
        if (a.heavy) apply_chain(a.chain, s_lut, a.pc, x, y, b, g, r);
        else apply_luts(a.chain, s_lut, b, g, r);
        atomicAdd(&s_hist[bgr2L(a.pc.tabs, b, g, r)], 1u);
    }
    __syncthreads();
    if (s_hist[tid]) atomicAdd(&a.hist[(size_t)k * 256 + tid], s_hist[tid]);
}

// clip + redistribute + cumulative table of one tile (clahe.cpp CLAHE_CalcLut_Body), one block per tile
__global__ __launch_bounds__(256) void enh_clahe_lut_kernel(const unsigned int* hist, int clip, float lut_scale, uint8_t* lut) {
    __shared__ int s[256];
    const int i = threadIdx.x, k = blockIdx.x;
    int v = (int)hist[(size_t)k * 256 + i];
    if (clip > 0) {
        int over = v > clip ? v - clip : 0;
        if (v > clip) v = clip;
        s[i] = over;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (i < off) s[i] += s[i + off];
            __syncthreads();
        }
        const int clipped = s[0];
        __syncthreads();
        const int batch = clipped / 256, residual = clipped - batch * 256;
        v += batch;
        if (residual != 0) {
            const int step = max(256 / residual, 1);
            if (i % step == 0 && i / step < residual) v++;
        }
    }
    s[i] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {      // inclusive scan
        const int t = i >= off ? s[i - off] : 0;
        __syncthreads();
        s[i] += t;
        __syncthreads();
    }
    lut[(size_t)k * 256 + i] = (uint8_t)clamp255(f_round(__fmul_rn((float)s[i], lut_scale)));
}

__global__ void enh_cvt_color_kernel(const EnhTables* T, const uint8_t* src, uint8_t* dst, size_t n, int code) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int a = src[3 * i], b = src[3 * i + 1], c = src[3 * i + 2], o0, o1, o2;
    switch (code) {
        case VS_CVT_BGR2HSV: bgr2hsv_px(T, a, b, c, o0, o1, o2); break;
        case VS_CVT_HSV2BGR: hsv2bgr_px(a, b, c, o0, o1, o2); break;
        case VS_CVT_BGR2LAB: bgr2lab_px(T, a, b, c, o0, o1, o2); break;
        default: lab2bgr_px(T, a, b, c, o0, o1, o2); break;
    }
    dst[3 * i] = (uint8_t)o0; dst[3 * i + 1] = (uint8_t)o1; dst[3 * i + 2] = (uint8_t)o2;
}

// ---- cv::fastNlMeansDenoisingColored (Enhancer.cpp:165-169) -------------------------------------------------------------
// BGR -> Lab without the sRGB curve (COLOR_LBGR2Lab), L and (a,b) as separate planes (photo/src/denoising.cpp)
__global__ void enh_split_lab_kernel(const EnhTables* T, const uint8_t* src, size_t stride, int w, int h, uint8_t* L, uint8_t* ab) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* p = src + (size_t)y * stride + (size_t)x * 3;
    int l, a, b;
    bgr2lab_px<false>(T, p[0], p[1], p[2], l, a, b);
    const size_t i = (size_t)y * w + x;
    L[i] = (uint8_t)l; ab[2 * i] = (uint8_t)a; ab[2 * i + 1] = (uint8_t)b;
}
__global__ void enh_merge_lab_kernel(const EnhTables* T, const uint8_t* L, const uint8_t* ab, int w, int h, uint8_t* dst, size_t dstride) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const size_t i = (size_t)y * w + x;
    int b, g, r;
    lab2bgr_px<false>(T, L[i], ab[2 * i], ab[2 * i + 1], b, g, r);
    uint8_t* p = dst + (size_t)y * dstride + (size_t)x * 3;
    p[0] = (uint8_t)b; p[1] = (uint8_t)g; p[2] = (uint8_t)r;
}

// cv::fastNlMeansDenoising(src, dst, h, 7, 21) on a CN-channel 8-bit plane (FastNlMeansDenoisingInvoker, DistSquared,
// fixed-point weights).  One workgroup = 32x32 output pixels.  For each of the 21x21 search offsets the squared
// differences of the two shifted copies of the staged tile are box-filtered 7x7 (rows, then columns, through LDS), which
// gives the patch distance of every output pixel at that offset at once; every step is exact integer arithmetic, so the
// result equals OpenCV's sliding-sum evaluation.
constexpr int N_TW = 32, N_TH = 32, N_T = 3, N_S = 10, N_B = N_T + N_S;
constexpr int N_SW = N_TW + 2 * N_B, N_SH = N_TH + 2 * N_B;      // staged tile: 58 x 58 pixels
constexpr int N_DW = N_TW + 2 * N_T, N_DH = N_TH + 2 * N_T;      // squared differences: 38 x 38
constexpr int N_DP = N_DW + 1;                                   // pitch of s_D
constexpr int N_EL = (N_DW * N_DH + 255) / 256;                  // difference elements per thread
constexpr int NLM_TAB_LDS = 4096;

struct NlmArgs {
    const uint8_t* src; uint8_t* dst;
    size_t stride, dstride;
    int32_t w, h;
    const int32_t* wtab;       // almost_dist2weight_ (device), entries >= tabn are 0
    int32_t tabn, shift;
};

template <int CN>
__global__ __launch_bounds__(256) void nlm_kernel(const NlmArgs a) {
    constexpr int PITCH = (N_SW * CN + 3) & ~3;
    __shared__ uint8_t s_px[N_SH * PITCH];
    __shared__ uint32_t s_D[N_DH * N_DP];
    __shared__ uint32_t s_H[N_DH * N_TW];
    __shared__ int32_t s_w[NLM_TAB_LDS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * N_TW, y0 = blockIdx.y * N_TH;
    for (int i = tid; i < NLM_TAB_LDS; i += 256) s_w[i] = i < a.tabn ? a.wtab[i] : 0;
    for (int i = tid; i < N_SH * N_SW; i += 256) {                 // copyMakeBorder(BORDER_DEFAULT) on the fly
        const int sy = i / N_SW, sx = i - sy * N_SW;
        const uint8_t* p = a.src + (size_t)reflect101(y0 - N_B + sy, a.h) * a.stride + (size_t)reflect101(x0 - N_B + sx, a.w) * CN;
#pragma unroll
        for (int c = 0; c < CN; c++) s_px[sy * PITCH + sx * CN + c] = p[c];
    }
    // this thread's share of the difference image: LDS offset of the centre pixel, s_D offset (-1: none)
    int e_px[N_EL], e_d[N_EL];
#pragma unroll
    for (int k = 0; k < N_EL; k++) {
        const int e = tid + 256 * k;
        const int ry = e / N_DW, rx = e - ry * N_DW;
        e_px[k] = (ry + N_S) * PITCH + (rx + N_S) * CN;
        e_d[k] = e < N_DW * N_DH ? ry * N_DP + rx : -1;
    }
    // row pass: item = (row of s_D, group of 4 outputs); column pass + accumulation: thread = (column, block of 4 rows)
    const int cx = tid & 31, cy = (tid >> 5) * 4;
    unsigned int est[4][CN], wsum[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        wsum[r] = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) est[r][c] = 0;
    }
    __syncthreads();
    for (int dy = -N_S; dy <= N_S; dy++) {
        for (int dx = -N_S; dx <= N_S; dx++) {
            const int sh_off = dy * PITCH + dx * CN;
            // A: squared differences between the tile and its copy shifted by (dx, dy)
#pragma unroll
            for (int k = 0; k < N_EL; k++) {
                if (e_d[k] >= 0) {
                    unsigned int d2 = 0;
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const int d = (int)s_px[e_px[k] + c] - (int)s_px[e_px[k] + sh_off + c];
                        d2 += (unsigned)(d * d);
                    }
                    s_D[e_d[k]] = d2;
                }
            }
            __syncthreads();
            // B: sums of 7 along x, four outputs per item with a sliding window
            for (int it = tid; it < N_DH * (N_TW / 4); it += 256) {
                const int ry = it >> 3, g4 = (it & 7) * 4;
                const uint32_t* dr = &s_D[ry * N_DP + g4];
                uint32_t v[10];
#pragma unroll
                for (int j = 0; j < 10; j++) v[j] = dr[j];
                uint32_t s0 = v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6];
                const uint32_t s1 = s0 - v[0] + v[7], s2 = s1 - v[1] + v[8], s3 = s2 - v[2] + v[9];
                uint32_t* hr = &s_H[ry * N_TW + g4];
                hr[0] = s0; hr[1] = s1; hr[2] = s2; hr[3] = s3;
            }
            __syncthreads();
            // C: sums of 7 along y -> patch distance -> weight -> weighted accumulation of the shifted pixel
            {
                uint32_t hv[10];
#pragma unroll
                for (int j = 0; j < 10; j++) hv[j] = s_H[(cy + j) * N_TW + cx];
                uint32_t dist = hv[0] + hv[1] + hv[2] + hv[3] + hv[4] + hv[5] + hv[6];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (r > 0) dist = dist - hv[r - 1] + hv[r + 6];
                    const uint32_t idx = dist >> a.shift;
                    const int wgt = idx < (uint32_t)NLM_TAB_LDS ? s_w[idx] : (idx < (uint32_t)a.tabn ? a.wtab[idx] : 0);
                    const uint8_t* p = &s_px[(cy + r + N_B + dy) * PITCH + (cx + N_B + dx) * CN];
#pragma unroll
                    for (int c = 0; c < CN; c++) est[r][c] += (unsigned)wgt * p[c];
                    wsum[r] += (unsigned)wgt;
                }
            }
            // the next A writes s_D while C may still read s_H: distinct buffers; the barrier after A orders C before the next B
        }
    }
    const int x = x0 + cx;
    if (x < a.w) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + cy + r;
            if (y < a.h) {
#pragma unroll
                for (int c = 0; c < CN; c++)
                    a.dst[(size_t)y * a.dstride + (size_t)x * CN + c] = (uint8_t)min((est[r][c] + wsum[r] / 2) / wsum[r], 255u);   // divByWeightsSum
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------
inline int h_rne(float v) { return (int)lrintf(v); }
inline int h_rne(double v) { return (int)lrint(v); }
inline uint8_t h_sat(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// color_lab.cpp initLabTabs / color_hsv tables (float arithmetic where OpenCV uses softfloat)
void build_tables(EnhTables& T) {
    static const double D65[3] = {0.950456, 1.0, 1.088754};
    static const double rgb2xyz[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    static const double xyz2rgb[9] = {3.240479, -1.53715, -0.498535, -0.969256, 1.875991, 0.041556, 0.055648, -0.204043, 1.057311};
    T.sdiv[0] = T.hdiv[0] = 0;
    for (int i = 1; i < 256; i++) {
        T.sdiv[i] = h_rne((255 << 12) / (1. * i));
        T.hdiv[i] = h_rne((180 << 12) / (6. * i));
    }
    for (int i = 0; i < 256; i++) {
        const float x = (float)i / 255.f;
        const float gm = x <= 0.04045f ? x * (1.f / 12.92f) : powf((x + 0.055f) * (1.f / 1.055f), 2.4f);
        T.gamma[i] = (uint16_t)h_rne((float)(255 * (1 << kGammaShift)) * gm);
    }
    for (int i = 0; i < kCbrtTabSize; i++) {
        const float x = (float)i / (float)(255 * (1 << kGammaShift));
        const float f = x < 0.008856f ? x * 7.787f + 0.13793103448275862f : (float)cbrt((double)x);
        T.cbrt_[i] = (uint16_t)h_rne((float)(1 << kLabShift2) * f);
    }
    for (int i = 0; i < 3; i++) {
        T.fwd[i * 3 + 2] = h_rne((double)(1 << kLabShift) * rgb2xyz[i * 3 + 0] / D65[i]);
        T.fwd[i * 3 + 1] = h_rne((double)(1 << kLabShift) * rgb2xyz[i * 3 + 1] / D65[i]);
        T.fwd[i * 3 + 0] = h_rne((double)(1 << kLabShift) * rgb2xyz[i * 3 + 2] / D65[i]);
        T.inv[i + 0] = h_rne((double)(1 << kLabShift) * xyz2rgb[0 * 3 + i] * D65[i]);
        T.inv[i + 3] = h_rne((double)(1 << kLabShift) * xyz2rgb[1 * 3 + i] * D65[i]);
        T.inv[i + 6] = h_rne((double)(1 << kLabShift) * xyz2rgb[2 * 3 + i] * D65[i]);
    }
    for (int i = 0; i < 256; i++) {
        int y, ify;
        if (i <= 20) {
            y = h_rne((float)(i * kBase * 20 * 9) / (float)(17 * 29 * 29 * 29));
            ify = h_rne((float)kBase * ((float)16 / (float)116 + (float)(i * 5) / (float)(3 * 17 * 29)));
        } else {
            const float fy = (float)(i * 100 * kBase) / (float)(255 * 116) + (float)(16 * kBase) / (float)116;
            ify = h_rne(fy);
            y = h_rne(fy * fy * fy / (float)(kBase * kBase));
        }
        T.l2yf[i * 2] = (uint16_t)y;
        T.l2yf[i * 2 + 1] = (uint16_t)ify;
    }
    for (int i = 0; i < kInvGammaTabSize; i++) {
        const float x = (float)i / (float)(kInvGammaTabSize - 1);
        const float gm = x <= 0.0031308f ? x * 12.92f : 1.055f * powf(x, 1.f / 2.4f) - 0.055f;
        T.inv_gamma[i] = (uint16_t)h_rne(255.f * gm);
        T.lin_inv_gamma[i] = (uint16_t)(int)(255.f * x);      // cvTrunc
    }
}

// getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (smooth.dispatch.cpp), 8 fractional bits
void gaussian_kernel_q8(int n, double sigma, uint16_t* q) {
    const int n2 = (n - 1) / 2;
    std::vector<double> vals(n2 + 1), k(n);
    const double scale2x = -0.125 / (sigma * sigma);
    double sum = 0;
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
        vals[i] = std::exp((double)(x * x) * scale2x);
        sum += vals[i];
    }
    sum = sum * 2 + 1.0;
    const double mul1 = 1.0 / sum;
    for (int i = 0; i < n2; i++) k[i] = k[n - 1 - i] = vals[i] * mul1;
    k[n2] = mul1;
    double err = 0;
    int64_t isum = 0;
    for (int i = 0; i < n2; i++) {
        const double adj = k[i] * 256.0 + err;
        const int64_t v0 = (int64_t)lrint(adj);
        err = adj - (double)v0;
        const int64_t v = std::max<int64_t>(0, std::min<int64_t>(65535, v0));
        isum += v;
        q[i] = q[n - 1 - i] = (uint16_t)v;
    }
    q[n2] = (uint16_t)(256 - 2 * isum);
}

// io: the YUV form on its surfaces (nullptr: the BGR8 form on a.src / a.dst / a.table)
// io: YUV surfaces; the default colour space takes the instance with the literal constants
bool yuv_is_default(const YuvIoCs& io) {
    const CvtCoef d = cvt_coef_default();
    return memcmp(&io.k, &d, sizeof d) == 0;
}
template <int R>
void launch_unsharp_r(const UnsharpArgs& a, const YuvIoCs* io, dim3 grid, hipStream_t st) {
    if (io && yuv_is_default(*io)) hipLaunchKernelGGL((enh_unsharp_kernel<R, YuvIo>), grid, dim3(E_NT), 0, st, a, static_cast<const YuvIo&>(*io));
    else if (io) hipLaunchKernelGGL((enh_unsharp_kernel<R, YuvIoCs>), grid, dim3(E_NT), 0, st, a, *io);
    else hipLaunchKernelGGL((enh_unsharp_kernel<R, NoYuv>), grid, dim3(E_NT), 0, st, a, NoYuv{});
}

void launch_unsharp(int R, const UnsharpArgs& a, const YuvIoCs* io, dim3 grid, hipStream_t st) {
    switch (R) {
        case 1: launch_unsharp_r<1>(a, io, grid, st); break;
        case 2: launch_unsharp_r<2>(a, io, grid, st); break;
        case 3: launch_unsharp_r<3>(a, io, grid, st); break;
        case 4: launch_unsharp_r<4>(a, io, grid, st); break;
        case 5: launch_unsharp_r<5>(a, io, grid, st); break;
        case 6: launch_unsharp_r<6>(a, io, grid, st); break;
        case 7: launch_unsharp_r<7>(a, io, grid, st); break;
        case 8: launch_unsharp_r<8>(a, io, grid, st); break;
        case 9: launch_unsharp_r<9>(a, io, grid, st); break;
        case 10: launch_unsharp_r<10>(a, io, grid, st); break;
        case 11: launch_unsharp_r<11>(a, io, grid, st); break;
        case 12: launch_unsharp_r<12>(a, io, grid, st); break;
        case 13: launch_unsharp_r<13>(a, io, grid, st); break;
        case 14: launch_unsharp_r<14>(a, io, grid, st); break;
        case 15: launch_unsharp_r<15>(a, io, grid, st); break;
        default: launch_unsharp_r<16>(a, io, grid, st); break;
    }
}

}  // namespace
}  // namespace vsd

using namespace vsd;

struct vs_enh {
    int device = 0;
    hipStream_t st = nullptr;
    std::string err;
    EnhTables* d_tabs = nullptr;
    uint8_t* d_luts = nullptr;          // LUT_SLOTS x 768
    uint8_t* h_luts = nullptr;          // pinned copy of the parameter-only tables
    float cb_alpha = NAN, cb_beta = NAN, gamma = NAN;
    unsigned long long* d_sums = nullptr;
    unsigned int* d_hist = nullptr;     // MAX_TILES^2 x 256
    uint8_t* d_clahe_lut = nullptr;     // MAX_TILES^2 x 256
    uint8_t* d_tmp[2] = {nullptr, nullptr};  size_t tmp_bytes[2] = {0, 0};   // intermediate frames (ping-pong)
    uint8_t* d_planes = nullptr; size_t planes_bytes = 0;                    // denoise: L, ab, L', ab' planes
    int32_t* d_nlm_tab[2] = {nullptr, nullptr}; int nlm_tabn[2] = {0, 0}; int nlm_cap[2] = {0, 0}; float nlm_h[2] = {NAN, NAN};
    int nlm_shift = 6;
    uint8_t* d_in = nullptr;   uint8_t* d_out = nullptr; size_t io_bytes = 0;
    ImgPair* d_table = nullptr; int table_cap = 0;
    int passes = 0;                     // frame passes of the last apply (for tests / docs)
    int fused = 0;                      // surfaces of the last vs_enh_apply_yuv_batch_dev that went through the fused launch
    CvtCoef yuv_k = cvt_coef_default(); // the colour space of the YUV calls (vs_enh_set_yuv_colorimetry), resolved
};

namespace {

struct Pending {
    Chain pre{}, post{};
    bool unsharp = false;
    bool pre_heavy = false;
};

// The walk over the stage list (enh_walk) either runs on an object - it launches every pass but the last, which it leaves to the
// caller as a Pending - or, with e == nullptr, only plans: no device call, no object; it counts the passes and notes of which kind
// they are (vs_enh_yuv_plan, the decision of vs_enh_apply_yuv_batch_dev).
struct PlanCtx {
    vs_enh* e;                                   // nullptr: plan only
    std::string msg;                             // the refusal of a plan
    int passes = 0;                              // frame passes so far
    bool stats = false, denoise = false, mid = false;   // a per-frame statistic, the denoiser, an intermediate frame were needed
    const vs_enh_params_c* p;
    int w, h;
    const uint8_t* cur; size_t cur_stride;       // single-frame mode
    const ImgPair* table; int frames;            // batch mode (table on the device)
    uint8_t* dst; size_t dst_stride;
    PointCtx pc;
    // unsharp weights
    int R = 0, ident = 0;
    uint32_t wq[(2 * MAX_R + 1 + 3) / 4];
    uint32_t we[MAX_R + 1], wo[MAX_R + 1];
    float alpha = 1.f, beta = 0.f;
};

bool aligned4(const void* p, size_t stride) { return ((uintptr_t)p & 3) == 0 && (stride & 3) == 0; }

int plan_fail(PlanCtx& c, int code, const char* msg) {
    if (c.e) return vs_obj_fail(c.e, code, msg);
    c.msg = msg;
    return code;
}
void count_passes(PlanCtx& c, int k) {
    c.passes += k;
    if (c.e) c.e->passes += k;
}

// io: the pass reads and writes YUV surfaces (the fused launch; out and out_stride are not used)
int run_pass(PlanCtx& c, Pending& pd, uint8_t* out, size_t out_stride, const YuvIoCs* io = nullptr) {
    vs_enh* e = c.e;
    if (!e) { count_passes(c, 1); return VS_OK; }
    // batch mode: geometry alignment was checked by the caller for all frames
    const bool sal = c.table ? true : aligned4(c.cur, c.cur_stride);
    const bool dal = c.table ? true : aligned4(out, out_stride);
    if (pd.unsharp) {
        UnsharpArgs a{};
        a.src = c.cur; a.dst = out; a.table = c.table; a.sstride = c.cur_stride; a.dstride = out_stride;
        a.w = c.w; a.h = c.h; a.luts = e->d_luts; a.pre = pd.pre; a.post = pd.post;
        memcpy(a.wq, c.wq, sizeof a.wq); memcpy(a.we, c.we, sizeof a.we); memcpy(a.wo, c.wo, sizeof a.wo);
        a.alpha = c.alpha; a.beta = c.beta; a.src_aligned = sal; a.dst_aligned = dal; a.ident = c.ident;
        dim3 grid((c.w + E_TW - 1) / E_TW, (c.h + E_TH - 1) / E_TH, c.table || io ? c.frames : 1);
        launch_unsharp(c.R, a, io, grid, e->st);
    } else {
        PointArgs a{};
        a.src = c.cur; a.dst = out; a.table = c.table; a.sstride = c.cur_stride; a.dstride = out_stride;
        a.w = c.w; a.h = c.h; a.luts = e->d_luts; a.chain = pd.pre; a.pc = c.pc; a.src_aligned = sal; a.dst_aligned = dal;
        a.heavy = pd.pre_heavy; a.sums = nullptr;
        a.rows = ((c.table || io) && c.frames >= 4) ? P_ROWS_LARGE : P_ROWS_SMALL;
        const int rows = io ? c.h >> io->sy : c.h;         // the YUV form counts chroma rows
        dim3 grid((c.w + 255) / 256, (rows + a.rows - 1) / a.rows, c.table || io ? c.frames : 1);
        if (io && yuv_is_default(*io)) hipLaunchKernelGGL((enh_point_kernel<false, YuvIo>), grid, dim3(256), 0, e->st, a, static_cast<const YuvIo&>(*io));
        else if (io) hipLaunchKernelGGL((enh_point_kernel<false, YuvIoCs>), grid, dim3(256), 0, e->st, a, *io);
        else hipLaunchKernelGGL((enh_point_kernel<false, NoYuv>), grid, dim3(256), 0, e->st, a, NoYuv{});
    }
    VS_OBJ_HIP(e, hipGetLastError());
    count_passes(c, 1);
    return VS_OK;
}

// one of the two intermediate frames, the one the current data does not live in
int other_tmp(PlanCtx& c, size_t bytes, int* which) {
    vs_enh* e = c.e;
    const int k = c.cur == e->d_tmp[0] ? 1 : 0;
    if (e->tmp_bytes[k] < bytes) {
        if (e->d_tmp[k]) { VS_OBJ_HIP(e, hipStreamSynchronize(e->st)); (void)hipFree(e->d_tmp[k]); e->d_tmp[k] = nullptr; e->tmp_bytes[k] = 0; }
        VS_OBJ_HIP(e, hipMalloc((void**)&e->d_tmp[k], bytes));
        e->tmp_bytes[k] = bytes;
    }
    *which = k;
    return VS_OK;
}

// materialise the pending stages into an intermediate frame (single-frame mode only)
int flush_mid(PlanCtx& c, Pending& pd) {
    if (c.table) return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: this stage list needs an intermediate frame (single-frame entry point only)");
    c.mid = true;
    if (!c.e) { count_passes(c, 1); pd = Pending{}; return VS_OK; }
    const size_t pitch = ((size_t)c.w * 3 + 3) & ~(size_t)3;
    int k;
    int rc = other_tmp(c, pitch * c.h, &k);
    if (rc != VS_OK) return rc;
    rc = run_pass(c, pd, c.e->d_tmp[k], pitch);
    if (rc != VS_OK) return rc;
    c.cur = c.e->d_tmp[k]; c.cur_stride = pitch;
    pd = Pending{};
    return VS_OK;
}

int add_point(PlanCtx& c, Pending& pd, int op, int slot) {
    const bool heavy = op != OP_LUT;
    if (pd.unsharp && heavy) { int rc = flush_mid(c, pd); if (rc != VS_OK) return rc; }
    Chain* ch = pd.unsharp ? &pd.post : &pd.pre;
    if (ch->n == CHAIN_MAX) { int rc = flush_mid(c, pd); if (rc != VS_OK) return rc; ch = &pd.pre; }
    ch->op[ch->n] = op; ch->slot[ch->n] = slot; ch->n++;
    if (heavy) pd.pre_heavy = true;
    return VS_OK;
}

// upload the parameter-only tables when the parameters changed
int refresh_luts(vs_enh* e, const vs_enh_params_c* p) {
    const bool cb_changed = !(e->cb_alpha == p->contrast && e->cb_beta == p->brightness);
    const bool g_changed = !(e->gamma == p->gamma);
    if (!cb_changed && !g_changed) return VS_OK;
    VS_OBJ_HIP(e, hipStreamSynchronize(e->st));       // a previous upload may still read h_luts
    if (cb_changed) {
        const float a = (float)(double)p->contrast, b = (float)(double)p->brightness;   // convertTo(img, -1, contrast, brightness), :150
        for (int c = 0; c < 3; c++)
            for (int i = 0; i < 256; i++) e->h_luts[SLOT_CB * SLOT_BYTES + c * 256 + i] = h_sat(h_rne(fmaf((float)i, a, b)));
        e->cb_alpha = p->contrast; e->cb_beta = p->brightness;
    }
    if (g_changed) {
        for (int c = 0; c < 3; c++)
            for (int i = 0; i < 256; i++) {                                              // :171-178
                const float norm = i / 255.f;
                const float corrected = std::pow(norm, p->gamma);
                e->h_luts[SLOT_GAMMA * SLOT_BYTES + c * 256 + i] = h_sat(h_rne(corrected * 255.f));
            }
        e->gamma = p->gamma;
    }
    VS_OBJ_HIP(e, hipMemcpyAsync(e->d_luts, e->h_luts, 2 * SLOT_BYTES, hipMemcpyHostToDevice, e->st));
    return VS_OK;
}

int setup_unsharp(PlanCtx& c) {
    const vs_enh_params_c* p = c.p;
    const double sigma = (double)p->blur_sigma;
    if (!(sigma > 0)) return plan_fail(c, VS_ERR_INVALID_ARG, "enhancer: blur_sigma must be > 0 (cv::GaussianBlur asserts)");
    const int n = h_rne(sigma * 3 * 2 + 1) | 1;      // GaussianBlur(Size(0,0), sigma) on CV_8U
    const int R = n / 2;
    if (R > MAX_R) return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: blur_sigma needs more than 33 taps");
    uint16_t k[2 * MAX_R + 1];
    gaussian_kernel_q8(n, sigma, k);
    c.ident = k[R] >= 256;                            // all weight on the centre tap: blurred == source
    c.R = std::max(R, 1);
    memset(c.wq, 0, sizeof c.wq); memset(c.we, 0, sizeof c.we); memset(c.wo, 0, sizeof c.wo);
    if (!c.ident) {
        if (R < 1) return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: degenerate kernel");
        for (int j = 0; j < n; j++) c.wq[j >> 2] |= (uint32_t)(k[j] & 255u) << (8 * (j & 3));
        for (int j = 0; j <= R; j++) {
            const uint32_t e0 = k[2 * j], e1 = (2 * j + 1 < n) ? k[2 * j + 1] : 0;
            const uint32_t o0 = (2 * j - 1 >= 0) ? k[2 * j - 1] : 0, o1 = k[2 * j];
            c.we[j] = e0 | (e1 << 16);
            c.wo[j] = o0 | (o1 << 16);
        }
    }
    c.alpha = (float)(1.0 + p->sharpness);            // addWeighted(img, 1.0 + sharpness, blurred, -sharpness, 0), :162
    c.beta = (float)(-(double)p->sharpness);
    return VS_OK;
}

int stats_wb(PlanCtx& c, Pending& pd) {
    vs_enh* e = c.e;
    c.stats = true;
    if (!e) { count_passes(c, 1); return VS_OK; }
    VS_OBJ_HIP(e, hipMemsetAsync(e->d_sums, 0, 3 * sizeof(unsigned long long), e->st));
    PointArgs a{};
    a.src = c.cur; a.dst = nullptr; a.table = nullptr; a.sstride = c.cur_stride; a.w = c.w; a.h = c.h; a.luts = e->d_luts;
    a.chain = pd.pre; a.pc = c.pc; a.src_aligned = aligned4(c.cur, c.cur_stride); a.heavy = pd.pre_heavy; a.sums = e->d_sums;
    a.rows = P_ROWS_LARGE;
    dim3 grid((c.w + 255) / 256, (c.h + a.rows - 1) / a.rows, 1);
    hipLaunchKernelGGL((enh_point_kernel<true, NoYuv>), grid, dim3(256), 0, e->st, a, NoYuv{});
    hipLaunchKernelGGL(enh_wb_lut_kernel, dim3(1), dim3(256), 0, e->st, e->d_sums, (unsigned long long)c.w * c.h, c.p->wb_strength,
                       e->d_luts + SLOT_WB * SLOT_BYTES);
    VS_OBJ_HIP(e, hipGetLastError());
    count_passes(c, 1);
    return VS_OK;
}

int stats_clahe(PlanCtx& c, Pending& pd) {
    vs_enh* e = c.e;
    c.stats = true;
    if (!e) { count_passes(c, 1); return VS_OK; }
    const int tiles = c.p->clahe_tile_grid_size;
    int ew = c.w, eh = c.h;
    if (c.w % tiles != 0 || c.h % tiles != 0) { ew = c.w + (tiles - c.w % tiles); eh = c.h + (tiles - c.h % tiles); }
    const int tw = ew / tiles, th = eh / tiles;
    const int tile_total = tw * th;
    const float lut_scale = (float)255 / tile_total;
    int clip = 0;
    if ((double)c.p->clahe_clip_limit > 0.0) {
        clip = (int)((double)c.p->clahe_clip_limit * tile_total / 256);
        clip = std::max(clip, 1);
    }
    VS_OBJ_HIP(e, hipMemsetAsync(e->d_hist, 0, (size_t)tiles * tiles * 256 * sizeof(unsigned int), e->st));
    HistArgs a{};
    a.src = c.cur; a.sstride = c.cur_stride; a.w = c.w; a.h = c.h; a.luts = e->d_luts; a.chain = pd.pre; a.pc = c.pc;
    a.heavy = pd.pre_heavy; a.tiles = tiles; a.tw = tw; a.th = th;
    a.rows_per_block = std::max(1, 4096 / tw);
    a.hist = e->d_hist;
    dim3 grid(tiles * tiles, (th + a.rows_per_block - 1) / a.rows_per_block, 1);
    hipLaunchKernelGGL(enh_hist_kernel, grid, dim3(256), 0, e->st, a);
    hipLaunchKernelGGL(enh_clahe_lut_kernel, dim3(tiles * tiles), dim3(256), 0, e->st, e->d_hist, clip, lut_scale, e->d_clahe_lut);
    VS_OBJ_HIP(e, hipGetLastError());
    c.pc.tiles = tiles; c.pc.inv_tw = 1.0f / tw; c.pc.inv_th = 1.0f / th; c.pc.clahe_lut = e->d_clahe_lut;
    count_passes(c, 1);
    return VS_OK;
}

// almost_dist2weight_ of cv::fastNlMeansDenoising for 8-bit data (fast_nlmeans_denoising_invoker.hpp, DistSquared, int weights):
// host libm exp in double like the reference; uploaded when h changes.  k = 0: L plane (1 channel), k = 1: ab plane (2).
int refresh_nlm_table(vs_enh* e, int k, float h) {
    if (e->nlm_h[k] == h && e->d_nlm_tab[k]) return VS_OK;
    const int cn = k + 1, tsq = 49, search = 21;
    int shift = 0;
    while ((1 << shift) < tsq) shift++;
    const double mult = (double)(1 << shift) / tsq;
    const int almost_max = (int)(255 * 255 * cn / mult + 1);
    const int fixed_point_mult = (int)(2147483647LL / (search * search * 255));
    std::vector<int32_t> tab(almost_max);
    int tabn = 0;
    for (int a = 0; a < almost_max; a++) {
        const double dist = a * mult;
        double w = std::exp(-dist / (h * h * cn));
        if (std::isnan(w)) w = 1.0;
        int weight = (int)lrint(fixed_point_mult * w);
        if (weight < 0.001 * fixed_point_mult) weight = 0;
        tab[a] = weight;
        if (weight) tabn = a + 1;
    }
    if (e->nlm_cap[k] < std::max(tabn, 1)) {
        VS_OBJ_HIP(e, hipStreamSynchronize(e->st));
        if (e->d_nlm_tab[k]) (void)hipFree(e->d_nlm_tab[k]);
        e->d_nlm_tab[k] = nullptr; e->nlm_cap[k] = 0;
        VS_OBJ_HIP(e, hipMalloc((void**)&e->d_nlm_tab[k], sizeof(int32_t) * std::max(tabn, 1)));
        e->nlm_cap[k] = std::max(tabn, 1);
    }
    VS_OBJ_HIP(e, hipStreamSynchronize(e->st));       // kernels of an earlier call may still read the table
    VS_OBJ_HIP(e, hipMemcpy(e->d_nlm_tab[k], tab.data(), sizeof(int32_t) * std::max(tabn, 1), hipMemcpyHostToDevice));
    e->nlm_tabn[k] = tabn; e->nlm_h[k] = h; e->nlm_shift = shift;
    return VS_OK;
}

// cv::fastNlMeansDenoisingColored(img, img, h, h, 7, 21), Enhancer.cpp:165-169: LBGR2Lab, NLM on L and on (a,b), Lab2LBGR
int run_denoise(PlanCtx& c, Pending& pd) {
    vs_enh* e = c.e;
    int rc = VS_OK;
    if (pd.pre.n > 0 || pd.unsharp) { rc = flush_mid(c, pd); if (rc != VS_OK) return rc; }
    else if (c.table) return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: denoise runs frame by frame");
    c.denoise = true;
    if (!e) { count_passes(c, 4); return VS_OK; }
    const size_t n = (size_t)c.w * c.h;
    if (e->planes_bytes < 6 * n) {
        VS_OBJ_HIP(e, hipStreamSynchronize(e->st));
        if (e->d_planes) (void)hipFree(e->d_planes);
        e->d_planes = nullptr; e->planes_bytes = 0;
        VS_OBJ_HIP(e, hipMalloc((void**)&e->d_planes, 6 * n));
        e->planes_bytes = 6 * n;
    }
    uint8_t *L = e->d_planes, *ab = L + n, *L2 = ab + 2 * n, *ab2 = L2 + n;
    if ((rc = refresh_nlm_table(e, 0, c.p->denoise_strength)) != VS_OK) return rc;
    if ((rc = refresh_nlm_table(e, 1, c.p->denoise_strength)) != VS_OK) return rc;
    const size_t pitch = ((size_t)c.w * 3 + 3) & ~(size_t)3;
    int k;
    if ((rc = other_tmp(c, pitch * c.h, &k)) != VS_OK) return rc;
    const dim3 pgrid((c.w + 255) / 256, c.h), tgrid((c.w + N_TW - 1) / N_TW, (c.h + N_TH - 1) / N_TH);
    hipLaunchKernelGGL(enh_split_lab_kernel, pgrid, dim3(256), 0, e->st, e->d_tabs, c.cur, c.cur_stride, c.w, c.h, L, ab);
    NlmArgs a{};
    a.w = c.w; a.h = c.h; a.shift = e->nlm_shift;
    a.src = L; a.dst = L2; a.stride = a.dstride = (size_t)c.w; a.wtab = e->d_nlm_tab[0]; a.tabn = e->nlm_tabn[0];
    hipLaunchKernelGGL(nlm_kernel<1>, tgrid, dim3(256), 0, e->st, a);
    a.src = ab; a.dst = ab2; a.stride = a.dstride = (size_t)c.w * 2; a.wtab = e->d_nlm_tab[1]; a.tabn = e->nlm_tabn[1];
    hipLaunchKernelGGL(nlm_kernel<2>, tgrid, dim3(256), 0, e->st, a);
    hipLaunchKernelGGL(enh_merge_lab_kernel, pgrid, dim3(256), 0, e->st, e->d_tabs, L2, ab2, c.w, c.h, e->d_tmp[k], pitch);
    VS_OBJ_HIP(e, hipGetLastError());
    c.cur = e->d_tmp[k]; c.cur_stride = pitch;
    count_passes(c, 4);
    return VS_OK;
}

enum { ST_WB, ST_CB, ST_CLAHE, ST_VIB, ST_UNSHARP, ST_GAMMA, ST_DENOISE };

// The stage list of Enhancer::enhanceImage, :138-239, compiled into passes.  c: the object (or none: plan only), the parameters and, on
// an object, the source.  Every pass but the last has run (or is counted) on return; the last is left in pd.
int enh_walk(PlanCtx& c, Pending& pd) {
    vs_enh* e = c.e;
    const vs_enh_params_c* p = c.p;
    const bool do_denoise = p->enable_denoise && p->denoise_strength > 0.f;
    const bool do_unsharp = p->enable_unsharp && p->sharpness > 0.f;
    const bool do_gamma = std::fabs(p->gamma - 1.f) > 1e-3;
    if (p->enable_clahe && (p->clahe_tile_grid_size < 1 || p->clahe_tile_grid_size > MAX_TILES))
        return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: clahe_tile_grid_size must be 1..16");
    if (c.table && (p->enable_white_balance || p->enable_clahe || do_denoise))
        return plan_fail(c, VS_ERR_UNSUPPORTED, "enhancer: batch entry point supports table stages, vibrance and unsharp only");
    int rc = e ? refresh_luts(e, p) : VS_OK;
    if (rc != VS_OK) return rc;
    c.pc.tabs = e ? e->d_tabs : nullptr; c.pc.clahe_lut = e ? e->d_clahe_lut : nullptr; c.pc.vib_alpha = p->vibrance_strength; c.pc.tiles = 1;
    c.pc.inv_tw = c.pc.inv_th = 1.f;
    if (do_unsharp) { rc = setup_unsharp(c); if (rc != VS_OK) return rc; }
    int stages[8], ns = 0;
    if (!p->use_cuda) {                                    // :142-181
        if (p->enable_white_balance) stages[ns++] = ST_WB;
        stages[ns++] = ST_CB;
        if (p->enable_clahe) stages[ns++] = ST_CLAHE;
        if (p->enable_vibrance) stages[ns++] = ST_VIB;
        if (do_unsharp) stages[ns++] = ST_UNSHARP;
        if (do_denoise) stages[ns++] = ST_DENOISE;
        if (do_gamma) stages[ns++] = ST_GAMMA;
    } else {                                               // :183-233
        stages[ns++] = ST_CB;
        if (do_unsharp) stages[ns++] = ST_UNSHARP;
        if (do_denoise) stages[ns++] = ST_DENOISE;
        if (p->enable_white_balance) stages[ns++] = ST_WB;
        if (p->enable_vibrance) stages[ns++] = ST_VIB;
        if (p->enable_clahe) stages[ns++] = ST_CLAHE;
        if (do_gamma) stages[ns++] = ST_GAMMA;
    }
    if (e) e->passes = 0;
    pd = Pending{};
    for (int i = 0; i < ns; i++) {
        switch (stages[i]) {
            case ST_CB: rc = add_point(c, pd, OP_LUT, SLOT_CB); break;
            case ST_GAMMA: rc = add_point(c, pd, OP_LUT, SLOT_GAMMA); break;
            case ST_VIB: rc = add_point(c, pd, OP_VIB, 0); break;
            case ST_DENOISE: rc = run_denoise(c, pd); break;
            case ST_UNSHARP:
                if (pd.unsharp || pd.pre_heavy) rc = flush_mid(c, pd);
                if (rc == VS_OK) pd.unsharp = true;
                break;
            case ST_WB:
                if (pd.unsharp) rc = flush_mid(c, pd);
                if (rc == VS_OK) rc = stats_wb(c, pd);
                if (rc == VS_OK) rc = add_point(c, pd, OP_LUT, SLOT_WB);
                break;
            case ST_CLAHE:
                if (pd.unsharp) rc = flush_mid(c, pd);
                if (rc == VS_OK) rc = stats_clahe(c, pd);
                if (rc == VS_OK) rc = add_point(c, pd, OP_CLAHE, 0);
                break;
        }
        if (rc != VS_OK) return rc;
    }
    return VS_OK;
}

// Enhancer::enhanceImage, :138-239.  Frames in HBM; everything is left in flight on e->st.
int enh_run(vs_enh* e, const vs_enh_params_c* p, const uint8_t* d_src, size_t sstride, const ImgPair* table, int frames, int w, int h,
            uint8_t* d_dst, size_t dstride) {
    if ((unsigned long long)h * sstride >= (1ull << 32) || (unsigned long long)h * dstride >= (1ull << 32))
        return vs_obj_fail(e, VS_ERR_UNSUPPORTED, "enhancer: frames of 4 GiB and more are not supported (32-bit row offsets)");
    PlanCtx c{};
    c.e = e; c.p = p; c.w = w; c.h = h; c.cur = d_src; c.cur_stride = sstride; c.table = table; c.frames = frames;
    c.dst = d_dst; c.dst_stride = dstride;
    Pending pd{};
    const int rc = enh_walk(c, pd);
    if (rc != VS_OK) return rc;
    return run_pass(c, pd, d_dst, dstride);
}

// What a stage list comes to, without an object or a device: rc != VS_OK is the refusal enh_run would give (text in c.msg).  The fused
// YUV launch takes a plan of ONE pass that needs no per-frame statistic, no denoiser and no intermediate frame - its stages then
// fit the pre / post chains of pd - and, where that pass is the unsharp pass, no surface in place: a tile reads its neighbours'
// samples, which another workgroup may already have overwritten.  (The point pass owns whole chroma blocks per thread.)
int enh_plan(const vs_enh_params_c* p, PlanCtx& c, Pending& pd) {
    c = PlanCtx{};
    c.p = p;
    const int rc = enh_walk(c, pd);
    if (rc != VS_OK) return rc;
    return run_pass(c, pd, nullptr, 0);
}
bool plan_is_fused(const PlanCtx& c, const Pending& pd, bool in_place) {
    return c.passes == 1 && !c.stats && !c.denoise && !c.mid && !(pd.unsharp && in_place);
}

// d_in / d_out: the object's own BGR8 frames (vs_enh_apply's staging, vs_enh_apply_yuv_dev's conversions), grown on demand
int enh_grow_io(vs_enh* e, size_t bytes) {
    if (e->io_bytes >= bytes) return VS_OK;
    VS_OBJ_HIP(e, hipStreamSynchronize(e->st));
    if (e->d_in) (void)hipFree(e->d_in);
    if (e->d_out) (void)hipFree(e->d_out);
    e->d_in = e->d_out = nullptr; e->io_bytes = 0;
    VS_OBJ_HIP(e, hipMalloc((void**)&e->d_in, bytes));
    VS_OBJ_HIP(e, hipMalloc((void**)&e->d_out, bytes));
    e->io_bytes = bytes;
    return VS_OK;
}

// vs_enh_apply_yuv_dev behind its checks - the definition of the enhancer on a YUV surface: conversion into the object's scratch,
// the stages, conversion back
int enh_yuv_three_calls(vs_enh* e, const vs_enh_params_c* p, const PixFmt& yf, const void* d_surface, const I420Layout& li, void* d_out,
                        const I420Layout& lo, int w, int h) {
    const PixFmt& bgr = *pixfmt(VS_FMT_BGR8);
    const size_t pitch = ((size_t)w * 3 + 3) & ~(size_t)3;
    VS_TRY(enh_grow_io(e, pitch * h));
    const void* const src[1] = {d_surface};
    void* const dst[1] = {d_out};
    void* const bgr_in[1] = {e->d_in};
    void* const bgr_out[1] = {e->d_out};
    VS_OBJ_TRY(e, launch_cvt_yuv_to_rgb(yf, src, li, bgr, bgr_in, pitch, 1, w, h, e->yuv_k, e->st));
    VS_OBJ_TRY(e, enh_run(e, p, e->d_in, pitch, nullptr, 1, w, h, e->d_out, pitch));
    VS_OBJ_TRY(e, launch_cvt_rgb_to_yuv(bgr, bgr_out, pitch, yf, dst, lo, 1, w, h, e->yuv_k, e->st));
    return VS_OK;
}

}  // namespace

extern "C" {

void vs_enh_params_default(vs_enh_params_c* p) {   // Enhancer.h:12-43
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (int32_t)sizeof *p;
    p->brightness = 0.f; p->contrast = 1.f;
    p->enable_white_balance = 0; p->wb_strength = 1.f;
    p->enable_vibrance = 0; p->vibrance_strength = 0.3f;
    p->enable_unsharp = 0; p->sharpness = 0.f; p->blur_sigma = 1.f;
    p->enable_clahe = 0; p->clahe_clip_limit = 2.f; p->clahe_tile_grid_size = 8;
    p->enable_denoise = 0; p->denoise_strength = 10.f;
    p->gamma = 1.f;
    p->use_cuda = 0;
}

int vs_enh_create(int device, vs_enh** out) {
    if (!out) return VS_ERR_INVALID_ARG;
    *out = nullptr;
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipSetDevice(device));
    vs_enh* e = new (std::nothrow) vs_enh();
    if (!e) return VS_ERR_HIP;
    e->device = device;
    auto fail = [&](hipError_t err) { set_last_error(hipGetErrorString(err)); vs_enh_destroy(e); return VS_ERR_HIP; };
    hipError_t err;
    if ((err = hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking)) != hipSuccess) return fail(err);
    if ((err = hipMalloc((void**)&e->d_tabs, sizeof(EnhTables))) != hipSuccess) return fail(err);
    if ((err = hipMalloc((void**)&e->d_luts, LUT_SLOTS * SLOT_BYTES)) != hipSuccess) return fail(err);
    if ((err = hipHostMalloc((void**)&e->h_luts, LUT_SLOTS * SLOT_BYTES, hipHostMallocDefault)) != hipSuccess) return fail(err);
    if ((err = hipMalloc((void**)&e->d_sums, 3 * sizeof(unsigned long long))) != hipSuccess) return fail(err);
    if ((err = hipMalloc((void**)&e->d_hist, (size_t)MAX_TILES * MAX_TILES * 256 * sizeof(unsigned int))) != hipSuccess) return fail(err);
    if ((err = hipMalloc((void**)&e->d_clahe_lut, (size_t)MAX_TILES * MAX_TILES * 256)) != hipSuccess) return fail(err);
    {
        std::vector<EnhTables> T(1);
        build_tables(T[0]);
        if ((err = hipMemcpy(e->d_tabs, T.data(), sizeof(EnhTables), hipMemcpyHostToDevice)) != hipSuccess) return fail(err);
    }
    for (int s = 0; s < LUT_SLOTS; s++)
        for (int c = 0; c < 3; c++)
            for (int i = 0; i < 256; i++) e->h_luts[s * SLOT_BYTES + c * 256 + i] = (uint8_t)i;
    if ((err = hipMemcpy(e->d_luts, e->h_luts, LUT_SLOTS * SLOT_BYTES, hipMemcpyHostToDevice)) != hipSuccess) return fail(err);
    *out = e;
    return VS_OK;
}

void vs_enh_destroy(vs_enh* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->st) (void)hipStreamSynchronize(e->st);
    if (e->d_tabs) (void)hipFree(e->d_tabs);
    if (e->d_luts) (void)hipFree(e->d_luts);
    if (e->h_luts) (void)hipHostFree(e->h_luts);
    if (e->d_sums) (void)hipFree(e->d_sums);
    if (e->d_hist) (void)hipFree(e->d_hist);
    if (e->d_clahe_lut) (void)hipFree(e->d_clahe_lut);
    for (int k = 0; k < 2; k++) {
        if (e->d_tmp[k]) (void)hipFree(e->d_tmp[k]);
        if (e->d_nlm_tab[k]) (void)hipFree(e->d_nlm_tab[k]);
    }
    if (e->d_planes) (void)hipFree(e->d_planes);
    if (e->d_in) (void)hipFree(e->d_in);
    if (e->d_out) (void)hipFree(e->d_out);
    if (e->d_table) (void)hipFree(e->d_table);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e;
}

const char* vs_enh_last_error(const vs_enh* e) { return e ? e->err.c_str() : ""; }

int vs_enh_sync(vs_enh* e) {
    if (!e) return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    VS_OBJ_HIP(e, hipStreamSynchronize(e->st));
    return VS_OK;
}

int vs_enh_last_passes(const vs_enh* e) { return e ? e->passes : 0; }

int vs_enh_apply_dev(vs_enh* e, const vs_enh_params_c* p, const void* d_data, int w, int h, size_t stride, void* d_out,
                     size_t out_stride) {
    if (!e || !p || !d_data || !d_out || w <= 0 || h <= 0 || stride < (size_t)w * 3 || out_stride < (size_t)w * 3 || d_data == d_out)
        return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    return enh_run(e, p, (const uint8_t*)d_data, stride, nullptr, 1, w, h, (uint8_t*)d_out, out_stride);
}

int vs_enh_apply_batch_dev(vs_enh* e, const vs_enh_params_c* p, const void* const* d_frames, void* const* d_outs, int n, int w,
                           int h, size_t stride, size_t out_stride) {
    if (!e || !p || !d_frames || !d_outs || n <= 0 || w <= 0 || h <= 0 || stride < (size_t)w * 3 || out_stride < (size_t)w * 3)
        return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    bool al = (stride & 3) == 0 && (out_stride & 3) == 0;
    for (int i = 0; i < n; i++) {
        if (!d_frames[i] || !d_outs[i] || d_frames[i] == d_outs[i]) return VS_ERR_INVALID_ARG;
        al = al && ((uintptr_t)d_frames[i] & 3) == 0 && ((uintptr_t)d_outs[i] & 3) == 0;
    }
    if (!al || p->enable_white_balance || p->enable_clahe || (p->enable_denoise && p->denoise_strength > 0.f)) {      // per-frame statistics or odd alignment: frame by frame
        for (int i = 0; i < n; i++) {
            int rc = enh_run(e, p, (const uint8_t*)d_frames[i], stride, nullptr, 1, w, h, (uint8_t*)d_outs[i], out_stride);
            if (rc != VS_OK) return rc;
        }
        return VS_OK;
    }
    if (e->table_cap < n) {
        if (e->d_table) { VS_OBJ_HIP(e, hipStreamSynchronize(e->st)); (void)hipFree(e->d_table); e->d_table = nullptr; e->table_cap = 0; }
        VS_OBJ_HIP(e, hipMalloc((void**)&e->d_table, (size_t)n * sizeof(ImgPair)));
        e->table_cap = n;
    }
    std::vector<ImgPair> hp(n);
    for (int i = 0; i < n; i++) { hp[i].src = d_frames[i]; hp[i].dst = d_outs[i]; }
    VS_OBJ_HIP(e, hipMemcpyAsync(e->d_table, hp.data(), (size_t)n * sizeof(ImgPair), hipMemcpyHostToDevice, e->st));   // pageable: staged before return
    int rc = enh_run(e, p, nullptr, stride, e->d_table, n, w, h, nullptr, out_stride);
    if (rc == VS_ERR_UNSUPPORTED) {                                // stage list with an intermediate frame
        for (int i = 0; i < n; i++) {
            rc = enh_run(e, p, (const uint8_t*)d_frames[i], stride, nullptr, 1, w, h, (uint8_t*)d_outs[i], out_stride);
            if (rc != VS_OK) return rc;
        }
    }
    return rc;
}

int vs_enh_apply(vs_enh* e, const vs_enh_params_c* p, const uint8_t* data, int w, int h, size_t stride, uint8_t* out,
                 size_t out_stride) {
    if (!e || !p || !data || !out || w <= 0 || h <= 0 || stride < (size_t)w * 3 || out_stride < (size_t)w * 3) return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    const size_t pitch = ((size_t)w * 3 + 3) & ~(size_t)3;
    VS_TRY(enh_grow_io(e, pitch * h));
    VS_OBJ_HIP(e, hipMemcpy2DAsync(e->d_in, pitch, data, stride, (size_t)w * 3, h, hipMemcpyHostToDevice, e->st));
    int rc = enh_run(e, p, e->d_in, pitch, nullptr, 1, w, h, e->d_out, pitch);
    if (rc != VS_OK) return rc;
    VS_OBJ_HIP(e, hipMemcpy2DAsync(out, out_stride, e->d_out, pitch, (size_t)w * 3, h, hipMemcpyDeviceToHost, e->st));
    VS_OBJ_HIP(e, hipStreamSynchronize(e->st));
    return VS_OK;
}

int vs_enh_apply_yuv_dev(vs_enh* e, const vs_enh_params_c* p, int yuv_fmt, const void* d_surface, const vs_i420_layout* in, void* d_out,
                         const vs_i420_layout* out, int w, int h) {
    if (!e) return VS_ERR_INVALID_ARG;
    if (!p) return vs_obj_fail(e, VS_ERR_INVALID_ARG, "vs_enh_apply_yuv_dev: null pointer");
    I420Layout li, lo;
    std::string msg;
    const void* const src[1] = {d_surface};
    void* const dst[1] = {d_out};
    if (cvt_check_yuv("vs_enh_apply_yuv_dev", yuv_fmt, src, 1, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv("vs_enh_apply_yuv_dev", yuv_fmt, dst, 1, out, w, h, &lo, &msg) != VS_OK)
        return vs_obj_fail(e, VS_ERR_INVALID_ARG, msg);
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    return enh_yuv_three_calls(e, p, *pixfmt(yuv_fmt), d_surface, li, d_out, lo, w, h);
}

int vs_enh_yuv_plan(const vs_enh_params_c* p, int yuv_fmt, int in_place) {
    const PixFmt* f = pixfmt(yuv_fmt);
    if (!p || !f || f->kind == PIX_INTERLEAVED) return -VS_ERR_INVALID_ARG;
    PlanCtx c;
    Pending pd;
    const int rc = enh_plan(p, c, pd);
    if (rc != VS_OK) return -rc;
    return plan_is_fused(c, pd, in_place != 0) ? 1 : 0;
}

int vs_enh_last_fused(const vs_enh* e) { return e ? e->fused : 0; }

int vs_enh_set_yuv_colorimetry(vs_enh* e, const vs_cvt_colorimetry* cs) {
    CvtCoef k;
    std::string msg;
    if (cvt_resolve("vs_enh_set_yuv_colorimetry", cs, &k, &msg) != VS_OK) {          // before the object: the text reaches vs_last_error without one
        if (e) return vs_obj_fail(e, VS_ERR_INVALID_ARG, msg);
        set_last_error(msg);
        return VS_ERR_INVALID_ARG;
    }
    if (!e) { set_last_error("vs_enh_set_yuv_colorimetry: null object"); return VS_ERR_INVALID_ARG; }
    e->yuv_k = k;
    return VS_OK;
}

int vs_enh_apply_yuv_batch_dev(vs_enh* e, const vs_enh_params_c* p, int yuv_fmt, const void* const* d_surfaces, const vs_i420_layout* in,
                               void* const* d_outs, const vs_i420_layout* out, int n, int w, int h) {
    static const char call[] = "vs_enh_apply_yuv_batch_dev";
    if (!e) return VS_ERR_INVALID_ARG;
    e->fused = 0;
    if (!p) return vs_obj_fail(e, VS_ERR_INVALID_ARG, std::string(call) + ": null pointer");
    I420Layout li, lo;
    std::string msg;
    if (cvt_check_yuv(call, yuv_fmt, d_surfaces, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv(call, yuv_fmt, d_outs, n, out, w, h, &lo, &msg) != VS_OK)
        return vs_obj_fail(e, VS_ERR_INVALID_ARG, msg);
    const PixFmt& yf = *pixfmt(yuv_fmt);
    bool in_place = false;
    for (int k = 0; k < n; k++) in_place = in_place || d_outs[k] == d_surfaces[k];
    PlanCtx c;
    Pending pd;
    const int rc = enh_plan(p, c, pd);                      // what the stage list refuses, before any device call
    if (rc != VS_OK) return vs_obj_fail(e, rc, std::string(call) + ": " + yf.name + ": " + c.msg);
    // 32-bit row offsets inside a plane
    const unsigned long long span = (unsigned long long)h * std::max(std::max(li.pitch, li.cpitch), std::max(lo.pitch, lo.cpitch));
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    if (!plan_is_fused(c, pd, in_place) || span >= (1ull << 32)) {
        for (int k = 0; k < n; k++) VS_TRY(enh_yuv_three_calls(e, p, yf, d_surfaces[k], li, d_outs[k], lo, w, h));
        return VS_OK;
    }
    VS_TRY(refresh_luts(e, p));
    YuvIoCs io{};
    for (int k = 0; k < n; k++) { io.src[k] = (const uint8_t*)d_surfaces[k]; io.dst[k] = (uint8_t*)d_outs[k]; }
    io.su = li.u; io.sv = li.v; io.du = lo.u; io.dv = lo.v;
    io.spitch = (uint32_t)li.pitch; io.scpitch = (uint32_t)li.cpitch; io.dpitch = (uint32_t)lo.pitch; io.dcpitch = (uint32_t)lo.cpitch;
    io.sb = yf.sample_bytes; io.il = yf.luma_uv(); io.sx = yf.sx; io.sy = yf.sy;
    io.shift = yf.sample_bytes == 2 ? (yf.luma_uv() ? 8 : yf.bits - 8) : 0;
    io.k = e->yuv_k;
    c.e = e; c.w = w; c.h = h; c.frames = n;
    c.pc.tabs = e->d_tabs; c.pc.clahe_lut = e->d_clahe_lut;
    e->passes = 0;
    VS_TRY(run_pass(c, pd, nullptr, 0, &io));
    e->fused = n;
    return VS_OK;
}

int vs_enh_cvt_color(vs_enh* e, int code, const void* d_src, void* d_dst, size_t npix) {
    if (!e || !d_src || !d_dst || code < VS_CVT_BGR2HSV || code > VS_CVT_LAB2BGR) return VS_ERR_INVALID_ARG;
    if (npix == 0) return VS_OK;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    hipLaunchKernelGGL(enh_cvt_color_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, e->st, e->d_tabs, (const uint8_t*)d_src,
                       (uint8_t*)d_dst, npix, code);
    VS_OBJ_HIP(e, hipGetLastError());
    return VS_OK;
}

int vs_enh_gaussian_blur(vs_enh* e, const void* d_src, size_t stride, int w, int h, double sigma, void* d_dst, size_t dstride) {
    if (!e || !d_src || !d_dst || w <= 0 || h <= 0 || stride < (size_t)w * 3 || dstride < (size_t)w * 3 || d_src == d_dst)
        return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(e, hipSetDevice(e->device));
    vs_enh_params_c p;
    vs_enh_params_default(&p);
    p.blur_sigma = (float)sigma; p.enable_unsharp = 1; p.sharpness = 1.f;
    PlanCtx c{};
    c.e = e; c.p = &p; c.w = w; c.h = h; c.cur = (const uint8_t*)d_src; c.cur_stride = stride;
    int rc = setup_unsharp(c);
    if (rc != VS_OK) return rc;
    c.alpha = 0.f; c.beta = 1.f;                     // addWeighted(src, 0, blurred, 1) == blurred
    Pending pd{};
    pd.unsharp = true;
    return run_pass(c, pd, (uint8_t*)d_dst, dstride);
}

}  // extern "C"
