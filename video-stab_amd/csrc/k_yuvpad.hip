// The pad half of border pad on YUV surfaces: vs_op_pad_jobs, and the launch a stream with vs_stab_set_yuv_border_pad queues in
// front of its warps.  A job gives one plane (sw x sh samples of cn channels) a border of bx columns and by rows on every side:
// cv::copyMakeBorder per plane as tests/compref.py states it (border_index), with a fill sample per channel where the reference
// writes 0 (VS_BORDER_BLACK); tests/yuvpadref.py in numpy.  It is a copy with an index map: no arithmetic on the samples.
//
// One launch takes up to YP_MAX_JOBS jobs in the scheme of plane_jobs.h (40 bytes of kernel arguments each).
//
// A tile is 128 bytes x 256 destination rows (8-bit samples) or 256 bytes x 128 rows (16-bit).  A lane owns the PJ_LB = 16 bytes at
// one place of YP_R rows; a wave is 8 (16) lanes side by side times 8 (4) rows, so that the lanes that gather - those at the left and
// right border of a plane - share their waves with few others: with 64 lanes side by side half the waves of a 4K luma plane held such
// a lane and ran its sample-by-sample path for all.  The source pixel of each of a gathering lane's pixels (or -1: the fill) is computed once per
// tile and kept in registers; the source row of a destination row costs a compare inside the picture (no LDS).
//
//   interior lanes (all 16 bytes inside the copied picture): their 16 contiguous source bytes in ONE 16-byte load, aligned where
//     source and destination alignments agree (the stream's planes with a border whose bytes are a multiple of 16) and at the
//     source's own alignment otherwise (b = 30 puts an 8-bit luma plane 14 bytes off): exactly those 16 bytes either way.
//   border lanes (some byte left or right of the picture, or behind the row's end): sample by sample through the column map;
//     VS_BORDER_BLACK pixels are not loaded.
//   fill rows (VS_BORDER_BLACK above and below the picture): stores only.
//
// Stores are 16-byte non-temporal where the lane's 16 bytes are inside the row and the address is 16-byte aligned, else sample by
// sample.  No load touches a byte outside the sw x sh samples of the source plane, no store a byte outside the padded plane.
//
// The sample-by-sample store is plane_jobs.h's pj_scatter written out here: through the shared function the two instances kept their
// instructions but not their order and registers (about 260 / 100 instructions moved inside their blocks), and the 16-bit launches
// of scratch/pad_measure.py then took 0.3 - 1 % longer than the parent's in both of two alternated runs (P010 reflect 0.2847 / 0.2844
// ms against 0.2829 / 0.2814, outside the parent's own windows).  Written out, both instances are the parent's but for one commuted
// scalar add.
#include <hip/hip_runtime.h>

#include "plane_jobs.h"

namespace vsd {
namespace {

constexpr int YP_R = 8;                      // rows per lane
constexpr int YP_WAVES = 4;
// A wave is cl lanes side by side times 64 / cl rows.  8-bit samples: 8 lanes (128 bytes of a row); 16-bit samples: 16 lanes (256
// bytes).  Measured at 3840 x 2160, b = 30, 32 surfaces: NV12 1.13 - 1.20 x a copy with 8 lanes against 1.18 -
// 1.46 with 16 and 1.8 - 2.2 with 64; P010 0.95 - 1.00 with 16 against 1.07 - 1.10 with 8 (a gathering lane loads 16 bytes one by
// one, but only 8 words).
constexpr int yp_cl(int sb) { return sb == 1 ? 8 : 16; }
constexpr int yp_tb(int sb) { return pj_tb(yp_cl(sb)); }
constexpr int yp_tr(int sb) { return pj_tr(YP_WAVES, YP_R, yp_cl(sb)); }

struct YpJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sstride, dstride;
    uint32_t swh;                            // sw | sh << 16
    uint32_t bxy;                            // bx | by << 16
    uint32_t t0f;                            // the job's first tile in the launch's sequence (24 bits) | (cn - 1) << 24 | border << 25
    uint32_t fill;                           // fill[0] | fill[1] << 16
};
struct YpArgs {
    YpJob j[YP_MAX_JOBS];
    uint32_t n, tiles;
};
static_assert(sizeof(YpJob) == 40 && sizeof(YpArgs) <= 4096, "the jobs travel as kernel arguments");
constexpr uint32_t YP_T0_MASK = 0xffffffu;
// 96 jobs of at most 512 x 128 (8-bit: 32767 pixels of 2 bytes) or 512 x 256 tiles (16-bit: of 4 bytes), 32767 rows
static_assert(96ull * ((32767ull * 2 + yp_tb(1) - 1) / yp_tb(1)) * ((32767 + yp_tr(1) - 1) / yp_tr(1)) <= YP_T0_MASK &&
                  96ull * ((32767ull * 4 + yp_tb(2) - 1) / yp_tb(2)) * ((32767 + yp_tr(2) - 1) / yp_tr(2)) <= YP_T0_MASK,
              "a launch's tiles fit 24 bits");

// cv::borderInterpolate in closed form (tests/compref.py, border_index): the source index of coordinate p on an axis of n samples,
// -1 where the fill applies.  Reflections that fold more than once (an axis shorter than its border) are the same modulus.
__device__ __forceinline__ int yp_map(int p, int n, int border) {
    if ((unsigned)p < (unsigned)n) return p;
    if (border == VS_BORDER_BLACK) return -1;
    if (border == VS_BORDER_REPLICATE) return p < 0 ? 0 : n - 1;
    // one fold or one period, the common case (a border no wider than the axis), without a division
    const int q = border == VS_BORDER_WRAP ? (p < 0 ? p + n : p - n)
                : border == VS_BORDER_REFLECT ? (p < 0 ? -p - 1 : 2 * n - 1 - p)
                                              : (p < 0 ? -p : 2 * n - 2 - p);
    if ((unsigned)q < (unsigned)n) return q;
    if (border == VS_BORDER_WRAP) {
        const int m = p % n;
        return m < 0 ? m + n : m;
    }
    if (border == VS_BORDER_REFLECT) {               // ... c b a | a b c | c b a ...: period 2n
        int m = p % (2 * n);
        if (m < 0) m += 2 * n;
        return m < n ? m : 2 * n - 1 - m;
    }
    if (n == 1) return 0;                            // VS_BORDER_REFLECT_101 ... c b | a b c | b a ...: period 2n - 2
    const int period = 2 * n - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

template <int SB, int CN>
__device__ __forceinline__ void yp_tile(const YpJob& J, int tx, int ty) {
    constexpr int NEL = PJ_LB / SB;                   // samples of a lane per row
    constexpr int NPX = NEL / CN;                     // pixels
    constexpr int PB = SB * CN;                       // bytes of a pixel
    constexpr int SPD = 4 / SB;                       // samples per dword
    const int sw = J.swh & 0xffffu, sh = J.swh >> 16, bx = J.bxy & 0xffffu, by = J.bxy >> 16;
    const int dw = sw + 2 * bx, dh = sh + 2 * by;
    const int border = (int)(J.t0f >> 25);
    constexpr int YP_CL = yp_cl(SB), YP_RW = 64 / YP_CL, YP_TR = yp_tr(SB);
    const int lane = threadIdx.x & (YP_CL - 1), sub = threadIdx.x / YP_CL, wave = threadIdx.y;
    const uint32_t fills[2] = {J.fill & 0xffffu, J.fill >> 16};

    const PjLane L = pj_lane<YP_CL, PB>(tx, lane, dw);      // the lane in the destination row
    if (L.nvb <= 0) return;
    const int e0 = L.e0, px0 = L.px0(PB);
    const bool interior = px0 >= bx && px0 + NPX <= bx + sw;      // (then L.full())
    // the lane's columns, for the lanes that gather: the source pixel of each of its pixels, -1 where the fill applies (pixels past
    // the row repeat its last one; they are not stored).  Waves of interior lanes skip this.
    int cx[NPX];
#pragma unroll
    for (int k = 0; k < NPX; k++) cx[k] = 0;
    if (!interior) {
#pragma unroll
        for (int k = 0; k < NPX; k++) cx[k] = yp_map(min(px0 + k, dw - 1) - bx, sw, border);
    }

    const uint32_t fq = pj_fill_dword<SB, CN>(fills, J.fill);

#pragma unroll 1
    for (int r = 0; r < YP_R; r++) {
        const int dy = ty * YP_TR + (wave * YP_R + r) * YP_RW + sub;
        if (dy >= dh) break;
        const int sy = yp_map(dy - by, sh, border);
        uint8_t* __restrict__ dp = J.dst + (size_t)dy * J.dstride + (size_t)e0;
        uint32_t o[4];
        if (sy < 0) {
            o[0] = o[1] = o[2] = o[3] = fq;
        } else {
            const uint8_t* __restrict__ rp = J.src + (size_t)sy * J.sstride;
            if (interior) {
                // exactly the lane's 16 source bytes, wherever they start
                pj_load16<pj_q1>(rp + (size_t)(px0 - bx) * PB, o);
            } else {
                o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
                for (int k = 0; k < NPX; k++) {
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const int i = k * CN + c;
                        const uint32_t v = cx[k] < 0 ? fills[c] : pj_ld<SB>(rp + ((size_t)cx[k] * CN + c) * SB);
                        o[i / SPD] |= v << (8 * SB * (i % SPD));
                    }
                }
            }
        }
        if (L.full() && ((uintptr_t)dp & 15) == 0) {
            __builtin_nontemporal_store(pj_pack16(o), reinterpret_cast<pj_u4*>(dp));
        } else {
            // pj_scatter, written out (see the head of the file)
#pragma unroll
            for (int i = 0; i < NEL; i++) {
                if (i * SB < L.nvb) {
                    const uint32_t v = o[i / SPD] >> (8 * SB * (i % SPD));
                    if constexpr (SB == 1) dp[i] = (uint8_t)v;
                    else reinterpret_cast<uint16_t*>(dp)[i] = (uint16_t)v;
                }
            }
        }
    }
}

template <int SB>
__global__ __launch_bounds__(64 * YP_WAVES) void yuvpad_kernel(const YpArgs a) {
    const uint32_t seq = xcd_seq(blockIdx.x, a.tiles);
    const YpJob J = a.j[pj_find(a, seq, [](const YpJob& j) { return j.t0f & YP_T0_MASK; })];
    const uint32_t cn = ((J.t0f >> 24) & 1u) + 1u;
    const uint32_t dw = (J.swh & 0xffffu) + 2u * (J.bxy & 0xffffu);
    const PjTile t = pj_split(seq - (J.t0f & YP_T0_MASK), dw * cn * SB, yp_tb(SB));
    if (cn == 1) yp_tile<SB, 1>(J, t.tx, t.ty);
    else yp_tile<SB, 2>(J, t.tx, t.ty);
}

// What the operator refuses about a job, decided before any device call; nullptr = accepted.
const char* yp_job_refusal(const vs_pad_job& s, int sample_bytes, int*) {
    if (!s.src || !s.dst) return "a null src or dst";
    if (const char* why = pj_bad_padded_sizes(s.sw, s.sh, s.bx, s.by)) return why;
    if (const char* why = pj_bad_cn(s.cn, s.reserved)) return why;
    if (s.border < VS_BORDER_BLACK || s.border > VS_BORDER_WRAP) return "border must be VS_BORDER_BLACK .. VS_BORDER_WRAP";
    if (const char* why = pj_bad_fill(s.fill, sample_bytes)) return why;
    const size_t srow = (size_t)s.sw * s.cn * sample_bytes, drow = (size_t)(s.sw + 2 * s.bx) * s.cn * sample_bytes;
    if (const char* why = pj_bad_strides({{s.src_stride, srow}, {s.dst_stride, drow}})) return why;
    if (const char* why = pj_bad_parity(sample_bytes, (uintptr_t)s.src | (uintptr_t)s.dst | s.src_stride | s.dst_stride)) return why;
    if (pj_overlap((uintptr_t)s.src, pj_end(s.src, s.src_stride, s.sh, srow), (uintptr_t)s.dst, pj_end(s.dst, s.dst_stride, s.sh + 2 * s.by, drow)))
        return "source and destination overlap";
    return nullptr;
}

}  // namespace

int launch_yuvpad(const vs_pad_job* jobs, int n, int sample_bytes, hipStream_t st) {
    YpArgs a{};
    return pj_launch(
        "vs_op_pad_jobs", jobs, n, YP_MAX_JOBS, sample_bytes, a, yp_job_refusal,
        [&](const vs_pad_job& s, YpJob& j, uint32_t tile0) {
            j.src = (const uint8_t*)s.src; j.dst = (uint8_t*)s.dst;
            j.sstride = (uint32_t)s.src_stride; j.dstride = (uint32_t)s.dst_stride;
            j.swh = (uint32_t)s.sw | (uint32_t)s.sh << 16; j.bxy = (uint32_t)s.bx | (uint32_t)s.by << 16;
            j.t0f = tile0 | (uint32_t)(s.cn - 1) << 24 | (uint32_t)s.border << 25;
            j.fill = (uint32_t)s.fill[0] | (uint32_t)s.fill[1] << 16;
            return pj_tiles((size_t)(s.sw + 2 * s.bx) * s.cn * sample_bytes, s.sh + 2 * s.by, yp_tb(sample_bytes), yp_tr(sample_bytes));
        },
        [&](auto sb, const YpArgs& args, unsigned tiles) { hipLaunchKernelGGL(yuvpad_kernel<decltype(sb)::value>, dim3(tiles), dim3(64, YP_WAVES), 0, st, args); });
}

}  // namespace vsd

extern "C" int vs_op_pad_jobs(const vs_pad_job* jobs, int n, int sample_bytes, void* stream) {
    return vsd::launch_yuvpad(jobs, n, sample_bytes, (hipStream_t)stream);
}
