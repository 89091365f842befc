// Resize to an output size on the device: vs_op_resample_jobs with its plan, vs_op_resize_yuv, vs_op_resize_rgb and
// vs_resize_axis_table.  A job resizes one plane (sw x sh samples of cn channels) to dw x dh in any ratio, INTER_LINEAR or
// INTER_LANCZOS4; the definition is in include/vs_stab.h, tests/resizeref.py states it in numpy.
//
// Where the arithmetic comes from.  Everything that belongs to an axis - the source index of every tap, already clamped into the
// source, and its 11-bit coefficient - is a table built on the host (resize_tables.h: the host's double sin / cos, never a device
// libm) and read here from device memory: an entry is K uint16 indices and K int16 coefficients, K = 2 or 8.  The kernels only
// gather, multiply and round, in integers, so the staged and the direct kernel give the same bytes by construction.  The tables of
// a device live in ONE arena (RsArena below); a job record holds their offsets, which keeps it at 40 bytes: 96 jobs travel as
// kernel arguments in the scheme of plane_jobs.h (tile sequence, bisection, split).
//
// A tile is RS_TB bytes of RS_TR destination rows, a workgroup four waves.  In the vertical pass a lane owns the RS_LB bytes at one
// place of RS_R consecutive rows (a wave: 64 lanes side by side, one 256-byte run per row).
//   staged: the tile's source box - the columns idx[first] .. idx[last] of its destination columns, the rows likewise - comes
//           into LDS as aligned dwords (a dword that would reach outside the row's sw samples is put together from the bytes
//           inside); one horizontal pass makes int32 sums of every box row for the tile's destination samples, once per box row
//           and not once per destination row; the vertical pass reads those sums.  LDS is dynamic: the launch asks for the rows
//           its jobs need (rs_lds_bytes).
//   direct: a lane gathers the taps of its samples from global memory: the jobs whose boxes exceed the staging area (strong
//           downscales), and every job with path 1.  A tile of the staged kernel whose box does not fit falls back to this body.
//   mean:   INTER_LINEAR at exactly 2 : 1 on both axes is the 2 x 2 mean (cv::resize reroutes it to INTER_AREA): a short path of
//           its own in both kernels, without tables.
// No load touches a byte outside a job's sw x sh samples, no store a byte outside dw x dh.  Stores are aligned non-temporal dwords
// where the lane's four bytes are all inside the row and aligned, else sample by sample (k_cropzoom.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>
#include <vector>

#include "plane_jobs.h"
#include "resize_tables.h"

namespace vsd {
namespace {

static_assert(RS_LINEAR == VS_INTERP_LINEAR && RS_LANCZOS4 == VS_INTERP_LANCZOS4, "resize_tables.h restates enum vs_interp");

constexpr int RS_LB = 4;                      // destination bytes per lane and row
constexpr int RS_R = 4;                       // consecutive rows per lane
constexpr int RS_WAVES = 4;
constexpr int RS_TB = 64 * RS_LB;             // tile: bytes ...
constexpr int RS_TR = RS_WAVES * RS_R;        // ... and rows
constexpr int RS_THREADS = 64 * RS_WAVES;
// The staging area: at most RS_BOX_ROWS box rows of RS_RAW_PITCH bytes (a row's aligned dwords: its span and up to 3 bytes on
// either side) and, per box row, the int32 sums of the tile's RS_TB / sample_bytes destination samples.  40 rows x 550 bytes hold
// the box of a 2 : 1 Lanczos tile (2 x 16 + 7 rows; 2 x 256 + 7 pixels of 4 bytes).
constexpr int RS_BOX_ROWS = 40;
constexpr int RS_RAW_PITCH = 576;
constexpr int RS_SPAN_MAX = RS_RAW_PITCH - 6;
constexpr int RS_LDS_LIMIT = 64 * 1024;       // of a workgroup
constexpr int rs_h_pitch(int sb) { return RS_TB / sb * 4; }
constexpr int rs_lds_bytes(int sb, int rows) { return rows * (rs_h_pitch(sb) + RS_RAW_PITCH); }
static_assert(rs_lds_bytes(1, RS_BOX_ROWS) <= RS_LDS_LIMIT && rs_lds_bytes(2, RS_BOX_ROWS) <= RS_LDS_LIMIT, "the staging area fits a workgroup's LDS");
static_assert(RS_RAW_PITCH % 16 == 0 && rs_h_pitch(1) % 16 == 0 && rs_h_pitch(2) % 16 == 0, "every carve of the dynamic LDS is 16-byte aligned");
static_assert(RS_THREADS % (RS_TB / 1) == 0 && RS_THREADS % (RS_TB / 2) == 0, "the horizontal pass: a thread per destination sample, row groups side by side");

// 8-bit planes sum in 32 bits (include/vs_stab.h: over a dense scan of f the positive coefficients of an axis sum to at most 2780)
static_assert(255ll * 2780 * 2780 + (1ll << 21) < (1ll << 31), "the 8-bit Lanczos sum fits 32-bit arithmetic");
static_assert(65535ll * 2780 < (1ll << 31), "a horizontal sum of 16-bit samples fits 32 bits");

// A table of the arena: RS_TAB_HEAD dwords (the source size, the destination size, K, 0), then K dwords per destination index:
// K / 2 dwords of uint16 tap indices, K / 2 dwords of int16 coefficients.
constexpr int RS_TAB_HEAD = 4;

struct RsJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sstride, dstride;
    uint32_t dwh;                             // dw | dh << 16
    uint32_t tile0;                           // the job's first tile in the launch's sequence
    uint32_t xtab, ytab;                      // its column and row table: dwords behind the arena's base (24 bits); xtab: | cn << 24 | mean << 28
};
struct RsArgs {
    RsJob j[RS_MAX_JOBS];
    const uint32_t* arena;
    uint32_t n, tiles;
    int32_t max_value;
    int32_t box_rows;                         // the box rows the launch's LDS holds (staged kernel)
};
static_assert(sizeof(RsJob) == 40 && sizeof(RsArgs) <= 4096, "the jobs travel as kernel arguments");
constexpr uint32_t RS_AT_MASK = 0xffffffu;
constexpr char AREA_UPSCALE[] = "dw > sw or dh > sh: area averaging only downscales (the upscale emulation of INTER_AREA is not built)";

// One entry of a table: the K tap indices and coefficients of destination index d
template <int K>
__device__ __forceinline__ void rs_entry(const uint32_t* __restrict__ tab, int d, int (&ix)[K], int (&cf)[K]) {
    const uint32_t* e = tab + RS_TAB_HEAD + (size_t)d * K;
#pragma unroll
    for (int j = 0; j < K / 2; j++) {
        const uint32_t wi = e[j], wc = e[K / 2 + j];
        ix[2 * j] = (int)(wi & 0xffffu); ix[2 * j + 1] = (int)(wi >> 16);
        cf[2 * j] = (int)(int16_t)(wc & 0xffffu); cf[2 * j + 1] = (int)wc >> 16;
    }
}

// The rounding of a destination sample: h[k] = the horizontal sums of its K tap rows, b[k] their coefficients
template <int SB, int K>
__device__ __forceinline__ uint32_t rs_finish(const int (&h)[K], const int (&b)[K], int max_value) {
    if constexpr (K == 8) {
        // INTER_LANCZOS4: clamp((S + 2^21) >> 22, 0, max_value), arithmetic shift
        if constexpr (SB == 1) {
            int S = 0;
#pragma unroll
            for (int k = 0; k < K; k++) S += h[k] * b[k];
            return (uint32_t)min(max((S + (1 << 21)) >> 22, 0), max_value);
        } else {
            int64_t S = 0;
#pragma unroll
            for (int k = 0; k < K; k++) S += (int64_t)h[k] * b[k];
            const int64_t v = (S + (1ll << 21)) >> 22;
            return (uint32_t)(v < 0 ? 0 : v > max_value ? max_value : v);
        }
    } else if constexpr (SB == 1) {
        // VResizeLinear 8u
        const int v = (((((b[0] * (h[0] >> 4)) >> 16) + ((b[1] * (h[1] >> 4)) >> 16) + 2) >> 2) & 0xff);
        return (uint32_t)min(v, max_value);
    } else {
        // the exact sum over the four taps, one rounding half to even at bit 22 (k_cropzoom.hip)
        const uint64_t S = (uint64_t)(uint32_t)h[0] * (uint32_t)b[0] + (uint64_t)(uint32_t)h[1] * (uint32_t)b[1];
        const uint64_t v = (S + ((1ull << 21) - 1) + ((S >> 22) & 1ull)) >> 22;
        return (uint32_t)(v < (uint64_t)max_value ? v : (uint64_t)max_value);
    }
}

// A lane's RS_LB bytes of destination row dy: o[e] = sample e
template <int SB>
__device__ __forceinline__ void rs_store(const RsJob& J, int dy, int eb, int nv, const uint32_t (&o)[RS_LB / SB]) {
    constexpr int NEL = RS_LB / SB;
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

// INTER_LINEAR at 2 : 1: (s00 + s01 + s10 + s11 + 2) >> 2.  Destination sample (dx, c) of row dy reads source pixels 2 dx and
// 2 dx + 1 of rows 2 dy and 2 dy + 1: sw = 2 dw and sh = 2 dh, so every read is inside the source.
template <int SB, int CN>
__device__ __forceinline__ void rs_mean_tile(const RsJob& J, int tx, int ty, int lane, int wave, int max_value) {
    constexpr int NEL = RS_LB / SB, PB = SB * CN;
    const int dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int eb = (tx * 64 + lane) * NEL;
    const int nv = min(NEL, dw * CN - eb);
    if (nv <= 0) return;
#pragma unroll
    for (int r = 0; r < RS_R; r++) {
        const int dy = ty * RS_TR + wave * RS_R + r;
        if (dy >= dh) break;
        const uint8_t* __restrict__ r0 = J.src + (size_t)(2 * dy) * J.sstride;
        const uint8_t* __restrict__ r1 = r0 + J.sstride;
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) {
            o[e] = 0;
            if (e < nv) {
                const int s = eb + e, dx = s / CN, c = s - dx * CN;
                const size_t at = (size_t)(2 * dx) * PB + (size_t)c * SB;
                const uint32_t v = (pj_ld<SB>(r0 + at) + pj_ld<SB>(r0 + at + PB) + pj_ld<SB>(r1 + at) + pj_ld<SB>(r1 + at + PB) + 2u) >> 2;
                o[e] = min(v, (uint32_t)max_value);
            }
        }
        rs_store<SB>(J, dy, eb, nv, o);
    }
}

// The direct body: every tap from global memory
template <int SB, int CN, int K>
__device__ __forceinline__ void rs_direct_tile(const RsJob& J, const uint32_t* __restrict__ xt, const uint32_t* __restrict__ yt, int tx, int ty, int lane,
                                               int wave, int max_value) {
    constexpr int NEL = RS_LB / SB, PB = SB * CN;
    const int dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int eb = (tx * 64 + lane) * NEL;
    const int nv = min(NEL, dw * CN - eb);
    if (nv <= 0) return;
    // the lane's columns: the byte of every tap in a source row, and its coefficient
    int xi[NEL][K], xc[NEL][K];
#pragma unroll
    for (int e = 0; e < NEL; e++) {
        const int s = min(eb + e, dw * CN - 1), dx = s / CN, c = s - dx * CN;      // (samples past the row repeat its last one; they are not stored)
        rs_entry<K>(xt, dx, xi[e], xc[e]);
#pragma unroll
        for (int k = 0; k < K; k++) xi[e][k] = xi[e][k] * PB + c * SB;
    }
#pragma unroll 1
    for (int r = 0; r < RS_R; r++) {
        const int dy = ty * RS_TR + wave * RS_R + r;              // (wave-uniform)
        if (dy >= dh) break;
        int yi[K], yc[K];
        rs_entry<K>(yt, dy, yi, yc);
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) {
            int h[K];
#pragma unroll
            for (int ky = 0; ky < K; ky++) {
                const uint8_t* __restrict__ rp = J.src + (size_t)yi[ky] * J.sstride;
                int acc = 0;
#pragma unroll
                for (int kx = 0; kx < K; kx++) acc += xc[e][kx] * (int)pj_ld<SB>(rp + xi[e][kx]);
                h[ky] = acc;
            }
            o[e] = rs_finish<SB, K>(h, yc, max_value);
        }
        rs_store<SB>(J, dy, eb, nv, o);
    }
}

// The staged body.  lds: box_rows rows of int32 sums (rs_h_pitch bytes each), then box_rows rows of RS_RAW_PITCH source bytes.
template <int SB, int CN, int K>
__device__ __forceinline__ void rs_staged_tile(const RsJob& J, const uint32_t* __restrict__ xt, const uint32_t* __restrict__ yt, int tx, int ty, int lane,
                                               int wave, int max_value, int box_rows, uint8_t* lds) {
    constexpr int NEL = RS_LB / SB, PB = SB * CN, TS = RS_TB / SB, HP = rs_h_pitch(SB);
    const int dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int sw = (int)xt[0];
    // the tile's box: pixels px0 .. px1, rows ry0 .. ry1 (the tables' indices are monotonic and clamped into the source)
    const int s_first = tx * TS, s_last = min((tx + 1) * TS, dw * CN) - 1;
    const int d_first = s_first / CN, d_last = s_last / CN;
    const int r_first = ty * RS_TR, r_last = min(r_first + RS_TR, dh) - 1;
    int t0[K], t1[K], tc[K];
    rs_entry<K>(xt, d_first, t0, tc);
    rs_entry<K>(xt, d_last, t1, tc);
    const int px0 = t0[0], px1 = t1[K - 1];
    rs_entry<K>(yt, r_first, t0, tc);
    rs_entry<K>(yt, r_last, t1, tc);
    const int ry0 = t0[0], ry1 = t1[K - 1];
    const int nr = ry1 - ry0 + 1, lo = px0 * PB, span = (px1 + 1 - px0) * PB;
    if (nr > box_rows || span > RS_SPAN_MAX) {                    // (uniform over the workgroup; the plan sends no such job here)
        rs_direct_tile<SB, CN, K>(J, xt, yt, tx, ty, lane, wave, max_value);
        return;
    }
    int* __restrict__ H = reinterpret_cast<int*>(lds);
    uint8_t* __restrict__ raw = lds + (size_t)box_rows * HP;
    const int tid = wave * 64 + lane;
    const uintptr_t row_bytes = (uintptr_t)sw * PB;

    // 1. the box, row by row as aligned dwords: byte b of box row r lies at raw[r * RS_RAW_PITCH + m_r + b], m_r = its address mod 4
    constexpr int QW = RS_RAW_PITCH / 4;
    for (int i = tid; i < nr * QW; i += RS_THREADS) {
        const int r = i / QW, q = i - r * QW;
        const uintptr_t r0 = (uintptr_t)(J.src + (size_t)(ry0 + r) * J.sstride);
        const uintptr_t a0 = (r0 + lo) & ~(uintptr_t)3, a = a0 + 4 * (uintptr_t)q;
        if (a >= r0 + lo + span) continue;                        // behind the box
        uint32_t v = 0;
        if (a >= r0 && a + 4 <= r0 + row_bytes) v = *reinterpret_cast<const uint32_t*>(a);
        else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (a + b >= r0 && a + b < r0 + row_bytes) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + b) << (8 * b);
        }
        reinterpret_cast<uint32_t*>(raw)[r * QW + q] = v;
    }
    __syncthreads();

    // 2. horizontal sums: a thread owns one destination sample of the tile and walks the box rows of its row group
    {
        constexpr int RG = RS_THREADS / TS;
        const int e = tid % TS, g = tid / TS;
        const int s = min(s_first + e, dw * CN - 1), dx = s / CN, c = s - dx * CN;
        int xi[K], xc[K];
        rs_entry<K>(xt, dx, xi, xc);
#pragma unroll
        for (int k = 0; k < K; k++) xi[k] = (xi[k] - px0) * PB + c * SB;
        for (int r = g; r < nr; r += RG) {
            const uint32_t m = (uint32_t)((uintptr_t)(J.src + (size_t)(ry0 + r) * J.sstride) + lo) & 3u;
            const uint8_t* __restrict__ rp = raw + r * RS_RAW_PITCH + m;
            int acc = 0;
#pragma unroll
            for (int k = 0; k < K; k++) acc += xc[k] * (int)pj_ld<SB>(rp + xi[k]);
            H[r * TS + e] = acc;
        }
    }
    __syncthreads();

    // 3. the vertical pass
    const int eb = (tx * 64 + lane) * NEL;
    const int nv = min(NEL, dw * CN - eb);
    if (nv <= 0) return;
#pragma unroll
    for (int r = 0; r < RS_R; r++) {
        const int dy = ty * RS_TR + wave * RS_R + r;              // (wave-uniform)
        if (dy >= dh) break;
        int yi[K], yc[K];
        rs_entry<K>(yt, dy, yi, yc);
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) {
            int h[K];
#pragma unroll
            for (int k = 0; k < K; k++) h[k] = H[(yi[k] - ry0) * TS + lane * NEL + e];
            o[e] = rs_finish<SB, K>(h, yc, max_value);
        }
        rs_store<SB>(J, dy, eb, nv, o);
    }
}

template <int SB, int CN, int K, bool STAGED>
__device__ __forceinline__ void rs_tile(const RsArgs& a, const RsJob& J, int tx, int ty, int lane, int wave, uint8_t* lds) {
    if (J.xtab >> 28 & 1u) {
        rs_mean_tile<SB, CN>(J, tx, ty, lane, wave, a.max_value);
        return;
    }
    const uint32_t* __restrict__ xt = a.arena + (J.xtab & RS_AT_MASK);
    const uint32_t* __restrict__ yt = a.arena + J.ytab;
    if constexpr (STAGED) rs_staged_tile<SB, CN, K>(J, xt, yt, tx, ty, lane, wave, a.max_value, a.box_rows, lds);
    else rs_direct_tile<SB, CN, K>(J, xt, yt, tx, ty, lane, wave, a.max_value);
}

template <int SB, int K, bool STAGED>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const RsJob J = a.j[pj_find(a, seq, [](const RsJob& j) { return j.tile0; })];
    const uint32_t cn = J.xtab >> 24 & 7u;
    const PjTile t = pj_split(seq - J.tile0, (J.dwh & 0xffffu) * cn * SB, RS_TB);
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (cn == 1) rs_tile<SB, 1, K, STAGED>(a, J, t.tx, t.ty, lane, wave, rs_lds);
    else if (cn == 2) rs_tile<SB, 2, K, STAGED>(a, J, t.tx, t.ty, lane, wave, rs_lds);
    else if constexpr (SB == 1) {
        if (cn == 3) rs_tile<SB, 3, K, STAGED>(a, J, t.tx, t.ty, lane, wave, rs_lds);
        else rs_tile<SB, 4, K, STAGED>(a, J, t.tx, t.ty, lane, wave, rs_lds);
    }
}

// ---- area-averaging downscale (vs_op_area_jobs): cv::resize(INTER_AREA), dw <= sw and dh <= sh -----------------------------------
// The same job record, tile, lane shape and store path.  A job is general (class 0: both axes through an area table of the arena,
// float32 sums in OpenCV's order, every product and sum rounded on its own), an integer box (class 1: the exact integer sum of
// ix x iy samples, one float32 product) or the 2 x 2 mean (class 2: rs_mean_tile above); the three ride in ONE launch.  J.xtab: | cn << 24 | class
// << 28; J.ytab of classes 1 and 2: ix | iy << 16 (then sw = ix dw and sh = iy dh exactly).
// An area table: RS_TAB_HEAD dwords, then 4 dwords per destination index: first | count << 16, w_first, w_mid, w_last (float bits).
// The taps of a sample in a source row lie PB bytes apart; a lane walks them through the aligned dwords that hold them, one load
// per dword (a 3 : 1 luma row: three or four taps from one or two dwords); a dword that would reach outside the row's bytes is put
// together from the bytes inside.
struct ArEntry { int first, count; float wf, wm, wl; };
__device__ __forceinline__ ArEntry ar_entry(const uint32_t* __restrict__ tab, int d) {
    const pj_u4 q = *reinterpret_cast<const pj_u4*>(tab + RS_TAB_HEAD + (size_t)d * 4);      // (a table's place is 16-byte aligned)
    return {(int)(q.x & 0xffffu), (int)(q.x >> 16), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)};
}
// (the weights by value: a choice between fields of a record in memory becomes a load through a chosen address, which keeps the
// record out of registers)
__device__ __forceinline__ float ar_weight(int count, float wf, float wm, float wl, int k) { return k == 0 ? wf : k == count - 1 ? wl : wm; }

// n samples of the row at r0 (row_bytes bytes), PB bytes apart from byte b0 on, in ascending order: f(k, sample)
template <int SB, int PB, class F>
__device__ __forceinline__ void ar_row(uintptr_t r0, uint32_t row_bytes, uint32_t b0, int n, F f) {
    uintptr_t p = r0 + b0;
    int k = 0;
    while (k < n) {
        const uintptr_t a = p & ~(uintptr_t)3;
        uint32_t q = 0;
        if (a >= r0 && a + 4 <= r0 + row_bytes) q = *reinterpret_cast<const uint32_t*>(a);
        else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (a + b >= r0 && a + b < r0 + row_bytes) q |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + b) << (8 * b);
        }
        do {
            f(k, (q >> (8 * (uint32_t)(p & 3))) & (SB == 1 ? 0xffu : 0xffffu));
            k++;
            p += PB;
        } while (k < n && (p & ~(uintptr_t)3) == a);
    }
}

template <int SB, int CN>
__device__ __forceinline__ void ar_general_tile(const RsJob& J, const uint32_t* __restrict__ xt, const uint32_t* __restrict__ yt, int tx, int ty, int lane,
                                                int wave, int max_value) {
    constexpr int NEL = RS_LB / SB, PB = SB * CN;
    const int dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int eb = (tx * 64 + lane) * NEL;
    const int nv = min(NEL, dw * CN - eb);
    if (nv <= 0) return;
    const uint32_t row_bytes = xt[0] * PB;
    ArEntry X[NEL];
    uint32_t b0[NEL];
#pragma unroll
    for (int e = 0; e < NEL; e++) {
        const int s = min(eb + e, dw * CN - 1), dx = s / CN, c = s - dx * CN;      // (samples past the row repeat its last one; they are not stored)
        X[e] = ar_entry(xt, dx);
        b0[e] = (uint32_t)X[e].first * PB + c * SB;
    }
#pragma unroll 1
    for (int r = 0; r < RS_R; r++) {
        const int dy = ty * RS_TR + wave * RS_R + r;              // (wave-uniform)
        if (dy >= dh) break;
        const ArEntry Y = ar_entry(yt, dy);
        float sum[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) sum[e] = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < Y.count; ky++) {
            const uintptr_t r0 = (uintptr_t)(J.src + (size_t)(Y.first + ky) * J.sstride);
            const float beta = ar_weight(Y.count, Y.wf, Y.wm, Y.wl, ky);
#pragma unroll
            for (int e = 0; e < NEL; e++) {
                const int nx = X[e].count;
                const float wf = X[e].wf, wm = X[e].wm, wl = X[e].wl;
                float buf = 0.f;
                ar_row<SB, PB>(r0, row_bytes, b0[e], nx, [&](int k, uint32_t v) { buf = __fadd_rn(buf, __fmul_rn((float)v, ar_weight(nx, wf, wm, wl, k))); });
                const float t = __fmul_rn(beta, buf);
                sum[e] = ky == 0 ? t : __fadd_rn(sum[e], t);
            }
        }
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) o[e] = (uint32_t)min(max(__float2int_rn(sum[e]), 0), max_value);
        rs_store<SB>(J, dy, eb, nv, o);
    }
}

template <int SB, int CN>
__device__ __forceinline__ void ar_box_tile(const RsJob& J, int tx, int ty, int lane, int wave, int max_value) {
    constexpr int NEL = RS_LB / SB, PB = SB * CN;
    const int dw = J.dwh & 0xffffu, dh = J.dwh >> 16;
    const int ix = J.ytab & 0xffffu, iy = J.ytab >> 16;
    const int eb = (tx * 64 + lane) * NEL;
    const int nv = min(NEL, dw * CN - eb);
    if (nv <= 0) return;
    const uint32_t row_bytes = (uint32_t)(dw * ix) * PB;
    // 1.f / (ix * iy) as OpenCV computes it, from a division in double: a float quotient rounded from 53 bits is the correctly
    // rounded one (2 x 24 + 2 <= 53), whatever the device's float division does
    const float inv = (float)(1.0 / (double)(float)(ix * iy));
    uint32_t b0[NEL];
#pragma unroll
    for (int e = 0; e < NEL; e++) {
        const int s = min(eb + e, dw * CN - 1), dx = s / CN, c = s - dx * CN;
        b0[e] = (uint32_t)(dx * ix) * PB + c * SB;
    }
#pragma unroll 1
    for (int r = 0; r < RS_R; r++) {
        const int dy = ty * RS_TR + wave * RS_R + r;              // (wave-uniform)
        if (dy >= dh) break;
        uint64_t S[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) S[e] = 0;
#pragma unroll 1
        for (int ky = 0; ky < iy; ky++) {
            const uintptr_t r0 = (uintptr_t)(J.src + (size_t)(dy * iy + ky) * J.sstride);
#pragma unroll
            for (int e = 0; e < NEL; e++) {
                uint32_t rs = 0;                                  // (65535 x 32767 < 2^31)
                ar_row<SB, PB>(r0, row_bytes, b0[e], ix, [&](int, uint32_t v) { rs += v; });
                S[e] += rs;
            }
        }
        uint32_t o[NEL];
#pragma unroll
        for (int e = 0; e < NEL; e++) o[e] = min((uint32_t)__float2int_rn(__fmul_rn((float)S[e], inv)), (uint32_t)max_value);
        rs_store<SB>(J, dy, eb, nv, o);
    }
}

template <int SB, int CN>
__device__ __forceinline__ void ar_tile(const RsArgs& a, const RsJob& J, int tx, int ty, int lane, int wave) {
    const uint32_t cls = J.xtab >> 28 & 3u;
    if (cls == 2) rs_mean_tile<SB, CN>(J, tx, ty, lane, wave, a.max_value);          // the resize's own 2 x 2 mean: the same bytes, the same time
    else if (cls) ar_box_tile<SB, CN>(J, tx, ty, lane, wave, a.max_value);
    else ar_general_tile<SB, CN>(J, a.arena + (J.xtab & RS_AT_MASK), a.arena + J.ytab, tx, ty, lane, wave, a.max_value);
}

template <int SB>
__global__ __launch_bounds__(RS_THREADS) void area_kernel(const RsArgs a) {
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const RsJob J = a.j[pj_find(a, seq, [](const RsJob& j) { return j.tile0; })];
    const uint32_t cn = J.xtab >> 24 & 7u;
    const PjTile t = pj_split(seq - J.tile0, (J.dwh & 0xffffu) * cn * SB, RS_TB);
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (cn == 1) ar_tile<SB, 1>(a, J, t.tx, t.ty, lane, wave);
    else if (cn == 2) ar_tile<SB, 2>(a, J, t.tx, t.ty, lane, wave);
    else if constexpr (SB == 1) {
        if (cn == 3) ar_tile<SB, 3>(a, J, t.tx, t.ty, lane, wave);
        else ar_tile<SB, 4>(a, J, t.tx, t.ty, lane, wave);
    }
}

// ---- host: the tables ------------------------------------------------------------------------------------------------------
// The table of one axis as the arena holds it
typedef std::tuple<int, int, int, int> RsKey;              // src, dst, interp (or RS_AREA), axis (LINEAR only: the others have one table for both axes)
RsKey rs_key(int src, int dst, int interp, int axis) { return RsKey(src, dst, interp, interp == RS_LINEAR ? axis : 0); }

struct RsTable {
    int k = 0, dst = 0;
    std::vector<uint32_t> words;
    int idx(int d, int t) const { const uint32_t w = words[RS_TAB_HEAD + (size_t)d * k + t / 2]; return (int)(t & 1 ? w >> 16 : w & 0xffffu); }
};

std::shared_ptr<const RsTable> rs_build_table(const RsKey& key) {
    const int src = std::get<0>(key), dst = std::get<1>(key), interp = std::get<2>(key), axis = std::get<3>(key);
    if (interp == RS_AREA) {                               // 4 dwords per destination index (ar_entry)
        std::vector<int32_t> first(dst), count(dst);
        std::vector<float> wf(dst), wm(dst), wl(dst);
        rs_area_axis_table(src, dst, first.data(), count.data(), wf.data(), wm.data(), wl.data());
        auto t = std::make_shared<RsTable>();
        t->k = 4; t->dst = dst;
        t->words.assign(RS_TAB_HEAD + (size_t)dst * 4, 0u);
        t->words[0] = (uint32_t)src; t->words[1] = (uint32_t)dst; t->words[2] = 4u;
        for (int d = 0; d < dst; d++) {
            uint32_t* e = &t->words[RS_TAB_HEAD + (size_t)d * 4];
            e[0] = (uint32_t)first[d] | (uint32_t)count[d] << 16;
            std::memcpy(e + 1, &wf[d], 4); std::memcpy(e + 2, &wm[d], 4); std::memcpy(e + 3, &wl[d], 4);
        }
        return t;
    }
    const int k = rs_taps(interp);
    std::vector<int32_t> idx((size_t)dst * k);
    std::vector<int16_t> coef((size_t)dst * k);
    rs_axis_table(src, dst, interp, axis, idx.data(), coef.data());
    auto t = std::make_shared<RsTable>();
    t->k = k; t->dst = dst;
    t->words.assign(RS_TAB_HEAD + (size_t)dst * k, 0u);
    t->words[0] = (uint32_t)src; t->words[1] = (uint32_t)dst; t->words[2] = (uint32_t)k;
    for (int d = 0; d < dst; d++)
        for (int j = 0; j < k / 2; j++) {
            const size_t at = (size_t)d * k + 2 * j;
            t->words[RS_TAB_HEAD + (size_t)d * k + j] = (uint32_t)idx[at] | (uint32_t)idx[at + 1] << 16;
            t->words[RS_TAB_HEAD + (size_t)d * k + k / 2 + j] = (uint32_t)(uint16_t)coef[at] | (uint32_t)(uint16_t)coef[at + 1] << 16;
        }
    return t;
}

// The tables a process has built (host side; needs no device) and, per device, the arena that holds their copies.  A table's place
// in an arena is written once, by a blocking copy into bytes no launch has been given, and then only read; when an arena is full
// the device is drained (no launch that reads a table is in flight any more) before its places are given out anew.  rs_mutex is
// held from the look-up to the launch, so no other call can recycle the arena between the two.
constexpr size_t RS_ARENA_BYTES = 64u << 20;
static_assert(RS_ARENA_BYTES / 4 <= RS_AT_MASK + 1, "a table's place fits the 24 bits of a job record");
constexpr size_t RS_HOST_TABLES_MAX = 512;
struct RsArena {
    uint32_t* base = nullptr;
    size_t used = 0;                                       // dwords
    std::map<RsKey, uint32_t> at;
};
std::mutex rs_mutex;
std::map<RsKey, std::shared_ptr<const RsTable>> rs_host_tables;
std::map<int, RsArena> rs_arenas;

std::shared_ptr<const RsTable> rs_host_table(const RsKey& key) {          // rs_mutex held
    auto it = rs_host_tables.find(key);
    if (it != rs_host_tables.end()) return it->second;
    if (rs_host_tables.size() >= RS_HOST_TABLES_MAX) rs_host_tables.clear();
    return rs_host_tables[key] = rs_build_table(key);
}
size_t rs_table_dwords(const RsTable& t) { return (t.words.size() + 3) & ~(size_t)3; }      // 16-byte places

// What a job needs of the tables
struct RsPlan {
    bool mean = false, staged = false;
    int box_rows = 0;                                      // the most box rows of a tile
    std::shared_ptr<const RsTable> x, y;
};

RsPlan rs_plan_job(const vs_scale_job& s, int sample_bytes, int interp) {                   // rs_mutex held
    RsPlan p;
    if (interp == RS_LINEAR && s.sw == 2 * s.dw && s.sh == 2 * s.dh) {
        p.mean = p.staged = true;                          // (it rides in the staged launch and needs no staging)
        return p;
    }
    p.x = rs_host_table(rs_key(s.sw, s.dw, interp, 0));
    p.y = rs_host_table(rs_key(s.sh, s.dh, interp, 1));
    const int k = p.x->k, pb = sample_bytes * s.cn, ts = RS_TB / sample_bytes, row = s.dw * s.cn;
    p.staged = true;
    for (int s0 = 0; s0 < row && p.staged; s0 += ts) {
        const int d0 = s0 / s.cn, d1 = (std::min(s0 + ts, row) - 1) / s.cn;
        if ((p.x->idx(d1, k - 1) + 1 - p.x->idx(d0, 0)) * pb > RS_SPAN_MAX) p.staged = false;
    }
    for (int r0 = 0; r0 < s.dh && p.staged; r0 += RS_TR) {
        const int nr = p.y->idx(std::min(r0 + RS_TR, (int)s.dh) - 1, k - 1) - p.y->idx(r0, 0) + 1;
        p.box_rows = std::max(p.box_rows, nr);
        if (nr > RS_BOX_ROWS) p.staged = false;
    }
    return p;
}

// What the operator refuses about the launch and about a job, decided before any device call; nullptr = accepted.
std::string rs_launch_refusal(int sample_bytes, int interp, int max_value, int path) {
    if (interp != VS_INTERP_LINEAR && interp != VS_INTERP_LANCZOS4) return "interp = " + std::to_string(interp) + " is not a vs_interp (0, 1)";
    if (path != 0 && path != 1) return "path = " + std::to_string(path) + " must be 0 or 1";
    const int top = sample_bytes == 1 ? 255 : 65535;
    if (max_value < 0 || max_value > top) return "max_value = " + std::to_string(max_value) + " must be 0 .. " + std::to_string(top);
    return std::string();
}
const char* rs_job_refusal(const vs_scale_job& s, int sample_bytes) {
    if (!s.src || !s.dst) return "a null src or dst";
    if (const char* why = pj_bad_sizes({s.sw, s.sh, s.dw, s.dh})) return why;
    if (s.reserved != 0) return "reserved must be 0";
    if (s.cn < 1 || s.cn > (sample_bytes == 1 ? 4 : 2)) return sample_bytes == 1 ? "cn must be 1 .. 4 with 8-bit samples" : "cn must be 1 or 2 with 16-bit samples";
    const size_t srow = (size_t)s.sw * s.cn * sample_bytes, drow = (size_t)s.dw * s.cn * sample_bytes;
    if (const char* why = pj_bad_strides({{s.src_stride, srow}, {s.dst_stride, drow}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.src | (uintptr_t)s.dst | s.src_stride | s.dst_stride)) return why;
    if (pj_overlap((uintptr_t)s.src, pj_end(s.src, s.src_stride, s.sh, srow), (uintptr_t)s.dst, pj_end(s.dst, s.dst_stride, s.dh, drow)))
        return "the destination must not overlap the source";
    return nullptr;
}

// Launch check, then every job, with the job's index in the text
int rs_check(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int interp, int max_value, int path) {
    if (!pj_launch_ok(jobs, n, RS_MAX_JOBS, sample_bytes)) {
        set_last_error(std::string(name) + ": invalid argument (1 .. " + std::to_string(RS_MAX_JOBS) + " jobs of one sample size, 1 or 2 bytes)");
        return VS_ERR_INVALID_ARG;
    }
    const std::string why = rs_launch_refusal(sample_bytes, interp, max_value, path);
    if (!why.empty()) {
        set_last_error(std::string(name) + ": " + why);
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; i++)
        if (const char* bad = rs_job_refusal(jobs[i], sample_bytes)) {
            set_last_error(std::string(name) + ": job " + std::to_string(i) + ": " + bad);
            return VS_ERR_INVALID_ARG;
        }
    return VS_OK;
}

// The place of a table in the device's arena; *full: it did not fit
uint32_t rs_place(RsArena& A, const RsKey& key, const RsTable& t, bool* full) {
    auto it = A.at.find(key);
    if (it != A.at.end()) return it->second;
    const size_t need = rs_table_dwords(t);
    if (A.used + need > RS_ARENA_BYTES / 4) { *full = true; return 0; }
    const uint32_t at = (uint32_t)A.used;
    A.used += need;
    A.at[key] = at;
    return at;
}

// A table a call needs, and its place in the device's arena
struct RsNeed {
    RsKey key;
    std::shared_ptr<const RsTable> t;
    uint32_t at = 0;
};

// The arena of the current device with the call's tables in place, uploaded where they are new (rs_mutex held)
int rs_place_tables(const char* name, std::vector<RsNeed>& needs, const uint32_t** arena) {
    size_t need = 0;
    {
        std::map<RsKey, size_t> distinct;
        for (const RsNeed& q : needs) distinct[q.key] = rs_table_dwords(*q.t);
        for (const auto& d : distinct) need += d.second;
    }
    if (need > RS_ARENA_BYTES / 4) {
        set_last_error(std::string(name) + ": the axis tables of one call exceed the table arena (" + std::to_string(RS_ARENA_BYTES >> 20) + " MiB)");
        return VS_ERR_CAPACITY;
    }
    VS_TRY(ensure_device());
    int dev = 0;
    VS_HIP_TRY(hipGetDevice(&dev));
    RsArena& A = rs_arenas[dev];
    if (!A.base) VS_HIP_TRY(hipMalloc((void**)&A.base, RS_ARENA_BYTES));
    // the places of the call's tables; a full arena: drain the device, then give every place out anew (the call's tables fit: `need`)
    for (int attempt = 0; attempt < 2; attempt++) {
        bool full = false;
        const size_t used0 = A.used;
        for (size_t i = 0; i < needs.size() && !full; i++) needs[i].at = rs_place(A, needs[i].key, *needs[i].t, &full);
        if (!full) {
            // upload what is new: places at or behind used0, each written once by a copy that has finished when it returns
            std::set<uint32_t> done;
            for (const RsNeed& q : needs)
                if (q.at >= used0 && done.insert(q.at).second) VS_HIP_TRY(hipMemcpy(A.base + q.at, q.t->words.data(), q.t->words.size() * 4, hipMemcpyHostToDevice));
            break;
        }
        VS_HIP_TRY(hipDeviceSynchronize());
        A.at.clear();
        A.used = 0;
    }
    *arena = A.base;
    return VS_OK;
}

template <int SB, bool STAGED>
void rs_launch_kernel(int interp, const RsArgs& a, unsigned tiles, hipStream_t st) {
    const size_t lds = STAGED ? (size_t)rs_lds_bytes(SB, a.box_rows) : 0;
    if (interp == RS_LANCZOS4) hipLaunchKernelGGL((resize_kernel<SB, 8, STAGED>), dim3(tiles), dim3(64, RS_WAVES), lds, st, a);
    else hipLaunchKernelGGL((resize_kernel<SB, 2, STAGED>), dim3(tiles), dim3(64, RS_WAVES), lds, st, a);
}

}  // namespace

int launch_resample(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int interp, int max_value, int path, hipStream_t st) {
    VS_TRY(rs_check(name, jobs, n, sample_bytes, interp, max_value, path));
    if (!max_value) max_value = sample_bytes == 1 ? 255 : 65535;
    std::lock_guard<std::mutex> lock(rs_mutex);
    std::vector<RsPlan> plans(n);
    std::vector<RsNeed> needs;                             // of job i: needs[at[i]] (columns), needs[at[i] + 1] (rows)
    std::vector<int> at(n, -1);
    for (int i = 0; i < n; i++) {
        plans[i] = rs_plan_job(jobs[i], sample_bytes, interp);
        if (plans[i].mean) continue;
        at[i] = (int)needs.size();
        needs.push_back({rs_key(jobs[i].sw, jobs[i].dw, interp, 0), plans[i].x});
        needs.push_back({rs_key(jobs[i].sh, jobs[i].dh, interp, 1), plans[i].y});
    }
    const uint32_t* arena = nullptr;
    VS_TRY(rs_place_tables(name, needs, &arena));
    std::vector<uint32_t> xat(n, 0u), yat(n, 0u);
    for (int i = 0; i < n; i++)
        if (at[i] >= 0) { xat[i] = needs[at[i]].at; yat[i] = needs[at[i] + 1].at; }
    // one launch per class
    for (int cls = 0; cls < 2; cls++) {
        const bool staged = cls == 0;
        std::vector<vs_scale_job> sel;
        std::vector<int> which;
        int box_rows = 1;
        for (int i = 0; i < n; i++)
            if ((path == 0 && plans[i].staged) == staged) {
                sel.push_back(jobs[i]);
                which.push_back(i);
                if (staged) box_rows = std::max(box_rows, plans[i].box_rows);
            }
        if (sel.empty()) continue;
        RsArgs a{};
        a.arena = arena; a.max_value = max_value; a.box_rows = box_rows;
        int k = 0;
        VS_TRY(pj_launch(
            name, sel.data(), (int)sel.size(), RS_MAX_JOBS, sample_bytes, a, [](const vs_scale_job&, int, int*) -> const char* { return nullptr; },
            [&](const vs_scale_job& s, RsJob& j, uint32_t tile0) {      // (96 jobs of at most 512 x 2048 tiles)
                const int i = which[k++];
                j.src = (const uint8_t*)s.src; j.dst = (uint8_t*)s.dst;
                j.sstride = (uint32_t)s.src_stride; j.dstride = (uint32_t)s.dst_stride;
                j.dwh = (uint32_t)s.dw | (uint32_t)s.dh << 16;
                j.tile0 = tile0;
                j.xtab = xat[i] | (uint32_t)s.cn << 24 | (plans[i].mean ? 1u << 28 : 0u); j.ytab = yat[i];
                return pj_tiles((size_t)s.dw * s.cn * sample_bytes, s.dh, RS_TB, RS_TR);
            },
            [&](auto sb, const RsArgs& args, unsigned tiles) {
                if (staged) rs_launch_kernel<decltype(sb)::value, true>(interp, args, tiles, st);
                else rs_launch_kernel<decltype(sb)::value, false>(interp, args, tiles, st);
            }));
    }
    return VS_OK;
}

int resample_plan(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int interp, int32_t* staged) {
    VS_TRY(rs_check(name, jobs, n, sample_bytes, interp, 0, 0));
    if (!staged) {
        set_last_error(std::string(name) + ": null pointer");
        return VS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lock(rs_mutex);
    for (int i = 0; i < n; i++) staged[i] = rs_plan_job(jobs[i], sample_bytes, interp).staged ? 1 : 0;
    return VS_OK;
}

// ---- area-averaging downscale --------------------------------------------------------------------------------------------------
// Everything the resize refuses about the launch and its jobs (VS_ERR_INVALID_ARG), then an upscale on either axis of a job
static int area_check(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int max_value) {
    VS_TRY(rs_check(name, jobs, n, sample_bytes, VS_INTERP_LINEAR, max_value, 0));
    for (int i = 0; i < n; i++)
        if (jobs[i].dw > jobs[i].sw || jobs[i].dh > jobs[i].sh) {
            set_last_error(std::string(name) + ": job " + std::to_string(i) + ": " + AREA_UPSCALE);
            return VS_ERR_UNSUPPORTED;
        }
    return VS_OK;
}

int launch_area(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int max_value, hipStream_t st) {
    VS_TRY(area_check(name, jobs, n, sample_bytes, max_value));
    if (!max_value) max_value = sample_bytes == 1 ? 255 : 65535;
    std::lock_guard<std::mutex> lock(rs_mutex);
    std::vector<RsNeed> needs;                             // of a general job i: needs[at[i]] (columns), needs[at[i] + 1] (rows)
    std::vector<int> at(n, -1), cls(n), ix(n), iy(n);
    for (int i = 0; i < n; i++) {
        const vs_scale_job& s = jobs[i];
        cls[i] = rs_area_class(s.sw, s.sh, s.dw, s.dh, &ix[i], &iy[i]);
        if (cls[i]) continue;
        at[i] = (int)needs.size();
        const RsKey kx = rs_key(s.sw, s.dw, RS_AREA, 0), ky = rs_key(s.sh, s.dh, RS_AREA, 1);
        needs.push_back({kx, rs_host_table(kx)});
        needs.push_back({ky, rs_host_table(ky)});
    }
    RsArgs a{};
    VS_TRY(rs_place_tables(name, needs, &a.arena));
    a.max_value = max_value;
    int i = 0;
    return pj_launch(
        name, jobs, n, RS_MAX_JOBS, sample_bytes, a, [](const vs_scale_job&, int, int*) -> const char* { return nullptr; },
        [&](const vs_scale_job& s, RsJob& j, uint32_t tile0) {
            j.src = (const uint8_t*)s.src; j.dst = (uint8_t*)s.dst;
            j.sstride = (uint32_t)s.src_stride; j.dstride = (uint32_t)s.dst_stride;
            j.dwh = (uint32_t)s.dw | (uint32_t)s.dh << 16;
            j.tile0 = tile0;
            j.xtab = (cls[i] ? 0u : needs[at[i]].at) | (uint32_t)s.cn << 24 | (uint32_t)cls[i] << 28;
            j.ytab = cls[i] ? (uint32_t)ix[i] | (uint32_t)iy[i] << 16 : needs[at[i] + 1].at;
            i++;
            return pj_tiles((size_t)s.dw * s.cn * sample_bytes, s.dh, RS_TB, RS_TR);
        },
        [&](auto sb, const RsArgs& args, unsigned tiles) { hipLaunchKernelGGL((area_kernel<decltype(sb)::value>), dim3(tiles), dim3(64, RS_WAVES), 0, st, args); });
}

int area_plan(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int32_t* cls) {
    VS_TRY(area_check(name, jobs, n, sample_bytes, 0));
    if (!cls) {
        set_last_error(std::string(name) + ": null pointer");
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; i++) {
        int ix, iy;
        cls[i] = rs_area_class(jobs[i].sw, jobs[i].sh, jobs[i].dw, jobs[i].dh, &ix, &iy);
    }
    return VS_OK;
}

}  // namespace vsd

// ---- the C entry points (include/vs_stab.h) -------------------------------------------------------------------------------
namespace {

using namespace vsd;

int rs_refuse(const std::string& why) {
    set_last_error(why);
    return VS_ERR_INVALID_ARG;
}

// What the surface calls refuse beyond a side's own rules: sizes above 32767, interp, a source that is a destination
int rs_check_surfaces(const std::string& head, int sw, int sh, int dw, int dh, int interp, const void* const* d_src, void* const* d_dst, int n, std::string* msg) {
    if (pj_bad_sizes({sw, sh, dw, dh})) { *msg = head + "sizes must be 1 .. 32767"; return VS_ERR_INVALID_ARG; }
    if (interp != VS_INTERP_LINEAR && interp != VS_INTERP_LANCZOS4) { *msg = head + "interp = " + std::to_string(interp) + " is not a vs_interp (0, 1)"; return VS_ERR_INVALID_ARG; }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
            if (d_src[i] == d_dst[j]) {
                *msg = head + "source surface " + std::to_string(i) + " is destination surface " + std::to_string(j) + " (surfaces may not overlap)";
                return VS_ERR_INVALID_ARG;
            }
    return VS_OK;
}

// The surface calls of the resize (area = false) and of the area-averaging downscale (area = true: no interp; an upscale is
// VS_ERR_UNSUPPORTED, after everything that is VS_ERR_INVALID_ARG)
int rs_unsupported(const std::string& why) {
    set_last_error(why);
    return VS_ERR_UNSUPPORTED;
}

int rs_yuv_call(const char* call, bool area, int fmt, const void* const* d_src, const vs_i420_layout* in, int sw, int sh, void* const* d_dst,
                const vs_i420_layout* out, int dw, int dh, int n, int interp, void* stream) {
    I420Layout li, lo;
    std::string msg;
    if (cvt_check_yuv((std::string(call) + ": source").c_str(), fmt, d_src, n, in, sw, sh, &li, &msg) != VS_OK ||
        cvt_check_yuv((std::string(call) + ": destination").c_str(), fmt, d_dst, n, out, dw, dh, &lo, &msg) != VS_OK)
        return rs_refuse(msg);
    const PixFmt& f = *pixfmt(fmt);
    const std::string head = std::string(call) + ": " + f.name + ": ";
    if (rs_check_surfaces(head, sw, sh, dw, dh, interp, d_src, d_dst, n, &msg) != VS_OK) return rs_refuse(msg);
    if (area && (dw > sw || dh > sh)) return rs_unsupported(head + AREA_UPSCALE);
    // the planes of a surface: luma; the interleaved (U, V) plane as cn 2, or U and V as planes of their own
    struct P { size_t soff, spitch, doff, dpitch; int sx, sy, cn; } planes[3] = {{0, li.pitch, 0, lo.pitch, 0, 0, 1}};
    int np = 1;
    if (f.luma_uv()) planes[np++] = P{li.u, li.cpitch, lo.u, lo.cpitch, f.sx, f.sy, 2};
    else {
        planes[np++] = P{li.u, li.cpitch, lo.u, lo.cpitch, f.sx, f.sy, 1};
        planes[np++] = P{li.v, li.cpitch, lo.v, lo.cpitch, f.sx, f.sy, 1};
    }
    std::vector<vs_scale_job> jobs;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < np; k++) {
            const P& p = planes[k];
            jobs.push_back(vs_scale_job{(const uint8_t*)d_src[i] + p.soff, p.spitch, sw >> p.sx, sh >> p.sy, (uint8_t*)d_dst[i] + p.doff, p.dpitch,
                                        dw >> p.sx, dh >> p.sy, p.cn, 0});
        }
    const std::string name = std::string(call) + ": " + f.name;
    const int max_value = (area || interp == VS_INTERP_LANCZOS4) && yuv_low_bit(f) ? (1 << f.bits) - 1 : 0;
    if (area) return launch_area(name.c_str(), jobs.data(), (int)jobs.size(), f.sample_bytes, max_value, (hipStream_t)stream);
    return launch_resample(name.c_str(), jobs.data(), (int)jobs.size(), f.sample_bytes, interp, max_value, 0, (hipStream_t)stream);
}

int rs_rgb_call(const char* call, bool area, int fmt, const void* const* d_src, size_t src_stride, int sw, int sh, void* const* d_dst, size_t dst_stride,
                int dw, int dh, int n, int interp, void* stream) {
    const PixFmt* f = pixfmt(fmt);
    if (!f || f->kind != PIX_INTERLEAVED)
        return rs_refuse(std::string(call) + ": " + (f ? std::string(f->name) : "format " + std::to_string(fmt)) +
                         " is not an interleaved 8-bit format (BGR8, RGB8, BGRA8, RGBA8, GRAY8)");
    const std::string head = std::string(call) + ": " + f->name + ": ";
    if (n < 1 || n > CVT_MAX_SURFACES) return rs_refuse(head + "n must be 1 .. 32 surfaces");
    if (!d_src || !d_dst) return rs_refuse(head + "null pointer");
    for (int i = 0; i < n; i++)
        if (!d_src[i] || !d_dst[i]) return rs_refuse(head + "null pointer");
    std::string msg;
    if (rs_check_surfaces(head, sw, sh, dw, dh, interp, d_src, d_dst, n, &msg) != VS_OK) return rs_refuse(msg);
    if (src_stride < (size_t)sw * f->cn) return rs_refuse(head + "source: the pitch must hold a row of the picture");
    if (dst_stride < (size_t)dw * f->cn) return rs_refuse(head + "destination: the pitch must hold a row of the picture");
    if (area && (dw > sw || dh > sh)) return rs_unsupported(head + AREA_UPSCALE);
    std::vector<vs_scale_job> jobs;
    for (int i = 0; i < n; i++) jobs.push_back(vs_scale_job{d_src[i], src_stride, sw, sh, d_dst[i], dst_stride, dw, dh, f->cn, 0});
    const std::string name = std::string(call) + ": " + f->name;
    if (area) return launch_area(name.c_str(), jobs.data(), n, 1, 0, (hipStream_t)stream);
    return launch_resample(name.c_str(), jobs.data(), n, 1, interp, 0, 0, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int vs_op_resample_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int interp, int max_value, int path, void* stream) {
    return vsd::launch_resample("vs_op_resample_jobs", jobs, n, sample_bytes, interp, max_value, path, (hipStream_t)stream);
}

int vs_op_resample_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int interp, int32_t* staged) {
    return vsd::resample_plan("vs_op_resample_jobs_plan", jobs, n, sample_bytes, interp, staged);
}

int vs_op_resize_yuv(int fmt, const void* const* d_src, const vs_i420_layout* in, int sw, int sh, void* const* d_dst, const vs_i420_layout* out, int dw,
                     int dh, int n, int interp, void* stream) {
    return rs_yuv_call("vs_op_resize_yuv", false, fmt, d_src, in, sw, sh, d_dst, out, dw, dh, n, interp, stream);
}

int vs_op_resize_rgb(int fmt, const void* const* d_src, size_t src_stride, int sw, int sh, void* const* d_dst, size_t dst_stride, int dw, int dh, int n,
                     int interp, void* stream) {
    return rs_rgb_call("vs_op_resize_rgb", false, fmt, d_src, src_stride, sw, sh, d_dst, dst_stride, dw, dh, n, interp, stream);
}

int vs_resize_axis_table(int src, int dst, int interp, int axis, int32_t* idx, int16_t* coef) {
    static const char call[] = "vs_resize_axis_table: ";
    if (pj_bad_sizes({src, dst})) return rs_refuse(std::string(call) + "sizes must be 1 .. 32767");
    if (interp != VS_INTERP_LINEAR && interp != VS_INTERP_LANCZOS4) return rs_refuse(std::string(call) + "interp = " + std::to_string(interp) + " is not a vs_interp (0, 1)");
    if (axis != 0 && axis != 1) return rs_refuse(std::string(call) + "axis = " + std::to_string(axis) + " must be 0 (columns) or 1 (rows)");
    if (!idx || !coef) return rs_refuse(std::string(call) + "null pointer");
    rs_axis_table(src, dst, interp, axis, idx, coef);
    return VS_OK;
}

// ---- area-averaging downscale ------------------------------------------------------------------------------------------------
int vs_op_area_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int max_value, void* stream) {
    return vsd::launch_area("vs_op_area_jobs", jobs, n, sample_bytes, max_value, (hipStream_t)stream);
}

int vs_op_area_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int32_t* cls) {
    return vsd::area_plan("vs_op_area_jobs_plan", jobs, n, sample_bytes, cls);
}

int vs_op_area_yuv(int fmt, const void* const* d_src, const vs_i420_layout* in, int sw, int sh, void* const* d_dst, const vs_i420_layout* out, int dw, int dh,
                   int n, void* stream) {
    return rs_yuv_call("vs_op_area_yuv", true, fmt, d_src, in, sw, sh, d_dst, out, dw, dh, n, VS_INTERP_LINEAR, stream);
}

int vs_op_area_rgb(int fmt, const void* const* d_src, size_t src_stride, int sw, int sh, void* const* d_dst, size_t dst_stride, int dw, int dh, int n,
                   void* stream) {
    return rs_rgb_call("vs_op_area_rgb", true, fmt, d_src, src_stride, sw, sh, d_dst, dst_stride, dw, dh, n, VS_INTERP_LINEAR, stream);
}

int vs_area_axis_table(int src, int dst, int32_t* first, int32_t* count, float* w_first, float* w_mid, float* w_last) {
    static const char call[] = "vs_area_axis_table: ";
    if (pj_bad_sizes({src, dst})) return rs_refuse(std::string(call) + "sizes must be 1 .. 32767");
    if (dst > src) return rs_unsupported(std::string(call) + AREA_UPSCALE);
    if (!first || !count || !w_first || !w_mid || !w_last) return rs_refuse(std::string(call) + "null pointer");
    rs_area_axis_table(src, dst, first, count, w_first, w_mid, w_last);
    return VS_OK;
}

}  // extern "C"
