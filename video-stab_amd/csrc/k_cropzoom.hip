// The zoom half of crop-and-zoom on YUV surfaces: vs_op_resize_jobs, and the launch a stream with vs_stab_set_yuv_crop_zoom queues
// behind its warps.  A job resizes one crop (sw x sh samples of cn channels, src = its first sample) to one plane (dw x dh, dw >= sw,
// dh >= sh); the definition is in include/vs_stab.h (cv::resize INTER_LINEAR as oracle/vso_resize_linear_u8 states it for 8-bit
// samples, the same coordinates and coefficients with ONE exact rounding for 16-bit samples; tests/cropzoomref.py in numpy).
//
// One launch takes up to CZ_MAX_JOBS jobs in the scheme of plane_jobs.h (40 bytes of kernel arguments each); the order of the
// sequence lets the tiles that share source lines meet in one L2.
//
// A tile is CZ_TB bytes of CZ_TR destination rows.  A lane owns the CZ_LB bytes at one place of CZ_R consecutive rows (a wave: 64
// lanes side by side, so a row of a wave is one 256-byte run).  What belongs to its columns - source columns, the coefficient
// pairs a0 / a1, the edge rule - is computed once per tile and kept in registers; what belongs to the tile's rows (source rows,
// b0 / b1) is computed by the first CZ_TR threads and read from LDS.
//
// The upscale's reuse: a destination row blends the horizontal sums h0 / h1 of source rows y0 and y1, and the next destination row
// needs y0 again or moves on by one, so a lane keeps the sums of the last two source rows it has built (ha of row ca, hb of row cb)
// and builds a row's sums only when neither holds them: CZ_R rows cost about CZ_R * sh / dh + 1 source rows instead of 2 CZ_R.  The
// sums kept are the integers a fresh evaluation gives - v0 * a0 + v1 * a1 of the same samples and coefficients - so the reuse is
// bit-exact by construction.
//
// Loads: the source bytes of a lane's columns (at most CZ_LB + one pixel, the upscale's steps being 0 or 1 source pixel per
// destination pixel) come as up to three aligned dwords when those dwords lie inside the crop's row; a lane at the crop's left or
// right edge whose dwords would reach outside [x, x + cw), and a lane whose steps are irregular (float rounding at coordinates in
// the ten thousands), load tap by tap.  No load touches a byte outside the crop, no store a byte outside dw x dh.  Stores are
// aligned non-temporal dwords where the lane's four bytes are all inside the row and aligned, else sample by sample.
#include <hip/hip_runtime.h>

#include "plane_jobs.h"

namespace vsd {
namespace {

constexpr int CZ_LB = 4;                     // destination bytes per lane and row
constexpr int CZ_R = 16;                     // consecutive rows per lane (16 against 8: 5 - 7 % less time at 3840 x 2160)
constexpr int CZ_WAVES = 4;
constexpr int CZ_TB = 64 * CZ_LB;            // tile: bytes ...
constexpr int CZ_TR = CZ_WAVES * CZ_R;       // ... and rows
static_assert(CZ_TR <= 64, "the lanes of the first wave fill the tile's row table: one row each");
constexpr int CZ_COEF = 2048;                // INTER_RESIZE_COEF_SCALE

struct CzJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sstride, dstride;
    uint32_t swh, dwh;                       // w | h << 16
    uint32_t tile0;                          // the job's first tile in the launch's sequence
    uint32_t cn;
};
struct CzArgs {
    CzJob j[CZ_MAX_JOBS];
    uint32_t n, tiles;
};
static_assert(sizeof(CzArgs) <= 4096, "the jobs travel as kernel arguments");

// The 16-bit blend S = sum of v * a * b over the four taps stays far inside 64 bits: a sample is at most 65535 and a coefficient
// pair sums to at most 2049 (each of (1 - f) * 2048 and f * 2048 is rounded on its own).
constexpr uint64_t CZ_S_MAX = 65535ull * (CZ_COEF + 1) * (CZ_COEF + 1);
static_assert(CZ_S_MAX + (1ull << 21) < (1ull << 40), "the 16-bit blend fits 64-bit arithmetic");
static_assert(65535ull * (CZ_COEF + 1) < (1ull << 32), "a horizontal sum of 16-bit samples fits 32 bits");

// cv::resize's source coordinate of destination index d: the sample index, and f in [0, 1) (oracle/vso_resize_linear_u8)
__device__ __forceinline__ int cz_coord(int d, double scale, float* f) {
    float v = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = f_floor(v);
    *f = v - (float)s;
    return s;
}
__device__ __forceinline__ double cz_scale(int s, int d) { return 1. / ((double)d / (double)s); }

template <int SB, int CN>
__device__ __forceinline__ void cz_tile(const CzJob& J, int tx, int ty, uint32_t* s_y, uint32_t* s_b) {
    constexpr int NEL = CZ_LB / SB;                   // samples of a lane per row
    constexpr int NPX = NEL / CN;                     // pixels
    constexpr int PB = SB * CN;                       // bytes of a pixel
    constexpr uint32_t SM = SB == 1 ? 0xffu : 0xffffu;
    static_assert(NPX >= 1 && NPX * PB == CZ_LB, "a lane holds whole pixels");
    const int sw = J.swh & 0xffffu, sh = J.swh >> 16, dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int lane = threadIdx.x, wave = threadIdx.y;

    // the tile's rows: source rows (clamped to the crop) and coefficients
    if (wave == 0 && lane < CZ_TR) {
        const int dy = min(ty * CZ_TR + lane, dh - 1);
        float fy;
        const int sy = cz_coord(dy, cz_scale(sh, dh), &fy);
        const int b0 = sat_s16(f_round((1.f - fy) * (float)CZ_COEF)), b1 = sat_s16(f_round(fy * (float)CZ_COEF));
        const int y0 = min(max(sy, 0), sh - 1), y1 = min(max(sy + 1, 0), sh - 1);
        s_y[lane] = (uint32_t)y0 | (uint32_t)y1 << 16;
        s_b[lane] = (uint32_t)b0 | (uint32_t)b1 << 16;
    }
    __syncthreads();

    const int eb = (tx * 64 + lane) * NEL;            // first sample of the lane in the destination row
    const int nv = min(NEL, dw * CN - eb);            // its samples inside the row (a multiple of CN)
    if (nv <= 0) return;

    // the lane's columns
    int sx[NPX];
    uint32_t a0[NPX], a1[NPX];
    bool edge_last = false, regular = true;
    uint32_t steps = 0;
    const double scale_x = cz_scale(sw, dw);
#pragma unroll
    for (int k = 0; k < NPX; k++) {
        const int dx = min(eb / CN + k, dw - 1);      // (pixels past the row repeat its last one; they are not stored)
        float fx;
        int s = cz_coord(dx, scale_x, &fx);
        if (s < 0) { fx = 0; s = 0; }
        bool edge = false;
        if (s + 1 >= sw) {
            edge = true;
            if (s >= sw - 1) { fx = 0; s = sw - 1; }
        }
        sx[k] = s;
        // the edge rule: the sample itself, times 2048 (HResizeLinear from xmax on)
        a0[k] = edge ? (uint32_t)CZ_COEF : (uint32_t)sat_s16(f_round((1.f - fx) * (float)CZ_COEF));
        a1[k] = edge ? 0u : (uint32_t)sat_s16(f_round(fx * (float)CZ_COEF));
        edge_last = edge;
        if (k > 0) {
            const int st = s - sx[k - 1];
            if (st == 1) steps |= 1u << k;
            else if (st != 0) regular = false;
        }
    }
    const uint32_t lo = (uint32_t)sx[0] * PB, hi = (uint32_t)(sx[NPX - 1] + (edge_last ? 1 : 2)) * PB;     // the bytes of a crop row the lane reads
    const uint32_t row_bytes = (uint32_t)sw * PB;

    // horizontal sums of the lane's samples in source row y
    auto hrow = [&](int y, uint32_t (&H)[NEL]) {
        const uint8_t* __restrict__ rp = J.src + (size_t)y * J.sstride;
        const uintptr_t r0 = (uintptr_t)rp, alo = (r0 + lo) & ~(uintptr_t)3, ahi = (r0 + hi + 3) & ~(uintptr_t)3;
        if (regular && alo >= r0 && ahi <= r0 + row_bytes) {
            // hi - lo <= CZ_LB + PB <= 8 bytes, from byte m <= 3 of the first dword: at most three dwords
            const uint32_t* q = reinterpret_cast<const uint32_t*>(alo);
            const uint32_t nd = (uint32_t)(ahi - alo) >> 2, m = (uint32_t)(r0 + lo) & 3u;
            const uint32_t w0 = q[0], w1 = nd > 1 ? q[1] : 0u, w2 = nd > 2 ? q[2] : 0u;
            uint64_t win = (uint64_t)w1 << 32 | w0;
            if (m) win = win >> (8 * m) | (uint64_t)w2 << (64 - 8 * m);
#pragma unroll
            for (int k = 0; k < NPX; k++) {
                if (k > 0 && (steps >> k & 1u)) win >>= 8 * PB;
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const uint32_t v0 = (uint32_t)(win >> (8 * SB * c)) & SM, v1 = (uint32_t)(win >> (8 * (PB + SB * c))) & SM;
                    H[k * CN + c] = v0 * a0[k] + v1 * a1[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NPX; k++) {
                const uint8_t* p = rp + (size_t)sx[k] * PB;
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const uint32_t v0 = pj_ld<SB>(p + SB * c);
                    const uint32_t v1 = a1[k] ? pj_ld<SB>(p + PB + SB * c) : 0u;       // (a1 == 0: at the edge, or a weight of nothing)
                    H[k * CN + c] = v0 * a0[k] + v1 * a1[k];
                }
            }
        }
    };

    uint32_t ha[NEL], hb[NEL];
    int ca = -1, cb = -1;                              // the source rows ha and hb hold
#pragma unroll
    for (int e = 0; e < NEL; e++) ha[e] = hb[e] = 0;
#pragma unroll
    for (int r = 0; r < CZ_R; r++) {
        const int dy = ty * CZ_TR + wave * CZ_R + r;   // (wave-uniform, as are the branches on rows below)
        if (dy >= dh) break;
        const uint32_t yy = s_y[wave * CZ_R + r], bb = s_b[wave * CZ_R + r];
        const int y0 = yy & 0xffffu, y1 = yy >> 16;
        const uint32_t b0 = bb & 0xffffu, b1 = bb >> 16;
        if (y0 != ca) {
            if (y0 == cb) {
#pragma unroll
                for (int e = 0; e < NEL; e++) ha[e] = hb[e];
            } else hrow(y0, ha);
            ca = y0;
        }
        if (y1 == ca) {
#pragma unroll
            for (int e = 0; e < NEL; e++) hb[e] = ha[e];
            cb = ca;
        } else if (y1 != cb) {
            hrow(y1, hb);
            cb = y1;
        }
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) {
            if constexpr (SB == 1) {
                // VResizeLinear 8u
                o[e] = (uint32_t)(((((int)b0 * (int)(ha[e] >> 4)) >> 16) + (((int)b1 * (int)(hb[e] >> 4)) >> 16) + 2) >> 2) & 0xffu;
            } else {
                // the exact sum over the four taps, one rounding half to even at bit 22
                const uint64_t S = (uint64_t)ha[e] * b0 + (uint64_t)hb[e] * b1;
                const uint64_t v = (S + ((1ull << 21) - 1) + ((S >> 22) & 1ull)) >> 22;
                o[e] = (uint32_t)(v < 65535ull ? v : 65535ull);
            }
        }
        uint8_t* __restrict__ dp = J.dst + (size_t)dy * J.dstride + (size_t)eb * SB;
        if (nv == NEL && ((uintptr_t)dp & 3) == 0) {
            uint32_t q = 0;
#pragma unroll
            for (int e = 0; e < NEL; e++) q |= o[e] << (8 * SB * e);
            __builtin_nontemporal_store(q, reinterpret_cast<uint32_t*>(dp));
        } else {
#pragma unroll
            for (int e = 0; e < NEL; e++) {
                if (e < nv) {
                    if constexpr (SB == 1) dp[e] = (uint8_t)o[e];
                    else reinterpret_cast<uint16_t*>(dp)[e] = (uint16_t)o[e];
                }
            }
        }
    }
}

template <int SB>
__global__ __launch_bounds__(64 * CZ_WAVES) void cropzoom_kernel(const CzArgs a) {
    __shared__ uint32_t s_y[CZ_TR], s_b[CZ_TR];
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const CzJob J = a.j[pj_find(a, seq, [](const CzJob& j) { return j.tile0; })];
    const PjTile t = pj_split(seq - J.tile0, (J.dwh & 0xffffu) * J.cn * SB, CZ_TB);
    if (J.cn == 1) cz_tile<SB, 1>(J, t.tx, t.ty, s_y, s_b);
    else cz_tile<SB, 2>(J, t.tx, t.ty, s_y, s_b);
}

// What the operator refuses about a job, decided before any device call; nullptr = accepted.
const char* cz_job_refusal(const vs_scale_job& s, int sample_bytes, int* rc) {
    if (!s.src || !s.dst) return "a null src or dst";
    if (const char* why = pj_bad_sizes({s.sw, s.sh, s.dw, s.dh})) return why;
    if (const char* why = pj_bad_cn(s.cn, s.reserved)) return why;
    if (const char* why = pj_bad_strides({{s.src_stride, (size_t)s.sw * s.cn * sample_bytes}, {s.dst_stride, (size_t)s.dw * s.cn * sample_bytes}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.src | (uintptr_t)s.dst | s.src_stride | s.dst_stride)) return why;
    if (s.dw < s.sw || s.dh < s.sh) {
        *rc = VS_ERR_UNSUPPORTED;
        return "dw >= sw and dh >= sh (this operator is the zoom-in of crop-and-zoom, not a general resize)";
    }
    return nullptr;
}

}  // namespace

int launch_cropzoom(const vs_scale_job* jobs, int n, int sample_bytes, hipStream_t st) {
    CzArgs a{};
    return pj_launch(
        "vs_op_resize_jobs", jobs, n, CZ_MAX_JOBS, sample_bytes, a, cz_job_refusal,
        [&](const vs_scale_job& s, CzJob& j, uint32_t tile0) {      // (96 jobs of at most 512 x 1024 tiles)
            j.src = (const uint8_t*)s.src; j.dst = (uint8_t*)s.dst;
            j.sstride = (uint32_t)s.src_stride; j.dstride = (uint32_t)s.dst_stride;
            j.swh = (uint32_t)s.sw | (uint32_t)s.sh << 16; j.dwh = (uint32_t)s.dw | (uint32_t)s.dh << 16;
            j.tile0 = tile0; j.cn = (uint32_t)s.cn;
            return pj_tiles((size_t)s.dw * s.cn * sample_bytes, s.dh, CZ_TB, CZ_TR);
        },
        [&](auto sb, const CzArgs& args, unsigned tiles) { hipLaunchKernelGGL(cropzoom_kernel<decltype(sb)::value>, dim3(tiles), dim3(64, CZ_WAVES), 0, st, args); });
}

}  // namespace vsd

extern "C" int vs_op_resize_jobs(const vs_scale_job* jobs, int n, int sample_bytes, void* stream) {
    return vsd::launch_cropzoom(jobs, n, sample_bytes, (hipStream_t)stream);
}
