// Auto zoom/crop for gfx950: counterpart of vs::AutoZoomCrop::autoZoomCrop
// (/root/reference/src/AutoZoomCrop.cpp:102-283).
//
// Split of the work (the reference has the same split, AutoZoomCrop.cpp:141-147: the mask is
// downloaded for cv::findContours on the CPU):
//   device  threshold_bits_kernel: BGR2GRAY + threshold(>1) as a bit plane (3 B/px read, 1 bit/px written)
//           close5_bits_kernel   : MORPH_CLOSE(5x5 ellipse) on the bit plane, 64 pixels per register
//   host    crop_from_mask      : border following on the bit mask (pointer chasing along one
//                                 contour: serial by nature), filled interior as row spans, the
//                                 shrink loop of :189-205 on the spans
//   device  warp_affine_kernel  : crop + scale to the output size, 640x360 unless vs_azc_set_output_size says otherwise
//                                 (cv::warpAffine semantics, k_warp.hip; the batches of the asynchronous forms: launch_scale_jobs)
// Only the mask (one bit per pixel) crosses PCIe between the two device stages; the frame stays in HBM.
#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "azc_contour.h"
#include <chrono>
#include <condition_variable>
#include <deque>
#include <thread>

#include "launchers.h"

namespace vsd {

namespace {

typedef unsigned long long u64;

struct __attribute__((aligned(4))) U3 { uint32_t a, b, c; };

// gray = (B*3735 + G*19235 + R*9798 + 2^14) >> 15 (BGR2GRAY); threshold(gray, 1, 255, BINARY) keeps gray >= 2
__device__ __forceinline__ unsigned content_bgr(uint32_t b, uint32_t g, uint32_t r) {
    return b * 3735u + g * 19235u + r * 9798u + (1u << 14) >= (2u << 15) ? 1u : 0u;
}

// Pass 1: BGR2GRAY + threshold as a bit plane T (64 pixels per word, wpr words per row, bits past the width 0).
// A lane takes 4 pixels (12 bytes, three dword loads when the rows allow), a workgroup 1024 pixels of one row;
// the 4-bit results go through LDS and 16 lanes pack them into the 16 words.
// (several pictures per launch: blockIdx.z selects the picture - its source from `srcs`, a kernel argument, its bit plane tfb
// words behind T)
// (BI: the byte of B inside a colour pixel - 0 BGR8 / BGRA8, 2 RGB8 / RGBA8: the first and the third byte change places in the
// weights.  CN = 4: a lane's four pixels are ONE 16-byte load - `aligned` then says that the rows keep 16 bytes -, the fourth byte of
// a pixel is never looked at.)
constexpr int SRC_LIST_MAX = 8;
struct SrcList { const uint8_t* p[SRC_LIST_MAX]; };
template <int CN, int BI = 0>
__global__ __launch_bounds__(256) void threshold_bits_kernel(const uint8_t* __restrict__ src, size_t stride, int w,
                                                             int aligned, u64* __restrict__ T, int wpr, SrcList srcs, size_t tfb) {
    __shared__ __attribute__((aligned(16))) uint8_t nib[256];
    if (!src) { src = srcs.p[blockIdx.z]; T += (size_t)blockIdx.z * tfb; }
    const int tid = threadIdx.x, x = (blockIdx.x * 256 + tid) * 4, y = blockIdx.y;
    const uint8_t* row = src + (size_t)y * stride;
    auto content = [](uint32_t c0, uint32_t c1, uint32_t c2) { return BI ? content_bgr(c2, c1, c0) : content_bgr(c0, c1, c2); };
    unsigned n = 0;
    if (x + 3 < w && aligned) {
        if (CN == 4) {
            const uint4 d = *reinterpret_cast<const uint4*>(row + (size_t)x * 4);
            auto px = [&](uint32_t v) { return content(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u); };
            n = px(d.x) | px(d.y) << 1 | px(d.z) << 2 | px(d.w) << 3;
        } else if (CN == 3) {
            const U3 d = *reinterpret_cast<const U3*>(row + (size_t)x * 3);
            n = content(d.a & 255u, (d.a >> 8) & 255u, (d.a >> 16) & 255u) |
                content(d.a >> 24, d.b & 255u, (d.b >> 8) & 255u) << 1 |
                content((d.b >> 16) & 255u, d.b >> 24, d.c & 255u) << 2 |
                content((d.c >> 8) & 255u, (d.c >> 16) & 255u, d.c >> 24) << 3;
        } else {
            const uint32_t d = *reinterpret_cast<const uint32_t*>(row + x);
            n = ((d & 255u) > 1u) | (((d >> 8) & 255u) > 1u) << 1 | (((d >> 16) & 255u) > 1u) << 2 | ((d >> 24) > 1u) << 3;
        }
    } else {
        for (int i = 0; i < 4; i++) {
            if (x + i >= w) break;
            const uint8_t* p = row + (size_t)(x + i) * CN;
            n |= (CN >= 3 ? content(p[0], p[1], p[2]) : (p[0] > 1 ? 1u : 0u)) << i;
        }
    }
    nib[tid] = (uint8_t)n;
    __syncthreads();
    const int word = blockIdx.x * 16 + tid;
    if (tid < 16 && word < wpr) {
        const uint4 q = reinterpret_cast<const uint4*>(nib)[tid];
        auto squeeze = [](uint32_t d) {          // four nibbles, one per byte -> 16 bits
            return (d & 0xFu) | ((d >> 4) & 0xF0u) | ((d >> 8) & 0xF00u) | ((d >> 12) & 0xF000u);
        };
        const u64 lo = squeeze(q.x) | (squeeze(q.y) << 16), hi = squeeze(q.z) | (squeeze(q.w) << 16);
        T[(size_t)y * wpr + word] = lo | (hi << 32);
    }
}

// Pass 1 for one-channel pictures whose width is a multiple of 16 and whose rows are 16-byte aligned (the luma planes of the
// asynchronous NV12 path): a lane takes 16 pixels with ONE 16-byte load, a wave 1024 pixels of a row, a workgroup four rows; the
// lane's 16 bits meet their three neighbours' through two lane exchanges - no LDS, no barrier, a quarter of the workgroups.
// (Measured against the general kernel above on eight 3840 x 2160 luma planes per launch: see DESIGN.md section 5.)
__device__ __forceinline__ uint32_t above1_nibble(uint32_t d) {         // bit k = byte k of d > 1
    const uint32_t t = (d | ((d & 0x7F7F7F7Fu) + 0x7E7E7E7Eu)) & 0x80808080u;      // bit 7 of a byte: byte >= 2 (no carries between bytes)
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;                                // bits 0, 8, 16, 24 -> 21, 22, 23, 24
}
__global__ __launch_bounds__(256) void threshold_bits_gray16_kernel(size_t stride, int w, int h, u64* __restrict__ T, int wpr, SrcList srcs,
                                                                    size_t tfb) {
    const uint8_t* __restrict__ src = srcs.p[blockIdx.z];
    T += (size_t)blockIdx.z * tfb;
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int x = blockIdx.x * 1024 + lane * 16, word = blockIdx.x * 16 + (lane >> 2);
    if (y >= h) return;                                                  // (wave-uniform)
    u64 bits = 0;
    if (x < w) {                                                         // (w is a multiple of 16: the lane's pixels are all inside or all outside)
        const uint4 d = *reinterpret_cast<const uint4*>(src + (size_t)y * stride + x);
        bits = (u64)(above1_nibble(d.x) | above1_nibble(d.y) << 4 | above1_nibble(d.z) << 8 | above1_nibble(d.w) << 12) << (16 * (lane & 3));
    }
    bits |= __shfl_xor(bits, 1);
    bits |= __shfl_xor(bits, 2);
    if ((lane & 3) == 0 && word < wpr) T[(size_t)y * wpr + word] = bits;
}

// Pass 1 for the luma planes of P010 surfaces: the content mask of a P010 surface is that of the 8-bit plane of its luma samples' high
// bytes, (sample >> 8) > 1 - the low byte is never looked at.  A lane takes 8 samples - WIDE: with ONE 16-byte load (width a multiple
// of 8 samples, rows 16-byte aligned); else sample by sample, any width and any even pitch -, tests the high bytes (bytes 1 and 3 of a
// dword) with the carry-free byte trick of above1_nibble, and its 8 bits meet its seven neighbours' through three lane exchanges:
// a wave 512 samples of a row = eight of the words close5_bits_kernel reads, a workgroup four rows; no LDS, no barrier.
__device__ __forceinline__ uint32_t above1_high_bytes(uint32_t d) {     // bit k = the high byte of sample k (half k of d) > 1
    const uint32_t t = (d | ((d & 0x7F7F7F7Fu) + 0x7E7E7E7Eu)) & 0x80008000u;      // bit 7 of bytes 1 and 3: byte >= 2 (no carries between bytes)
    return ((t >> 15) & 1u) | ((t >> 30) & 2u);
}
template <bool WIDE>
__global__ __launch_bounds__(256) void threshold_bits_p010_kernel(size_t stride, int w, int h, u64* __restrict__ T, int wpr, SrcList srcs, size_t tfb) {
    const uint8_t* __restrict__ src = srcs.p[blockIdx.z];
    T += (size_t)blockIdx.z * tfb;
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int x = blockIdx.x * 512 + lane * 8, word = blockIdx.x * 8 + (lane >> 3);
    if (y >= h) return;                                                  // (wave-uniform)
    uint32_t m = 0;
    const uint8_t* row = src + (size_t)y * stride;
    if (WIDE) {
        if (x < w) {                                                     // (w is a multiple of 8: the lane's samples are all inside or all outside)
            const uint4 d = *reinterpret_cast<const uint4*>(row + (size_t)x * 2);
            m = above1_high_bytes(d.x) | above1_high_bytes(d.y) << 2 | above1_high_bytes(d.z) << 4 | above1_high_bytes(d.w) << 6;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (x + i < w) m |= ((reinterpret_cast<const uint16_t*>(row)[x + i] >> 8) > 1u ? 1u : 0u) << i;
    }
    u64 bits = (u64)m << (8 * (lane & 7));
    bits |= __shfl_xor(bits, 1);
    bits |= __shfl_xor(bits, 2);
    bits |= __shfl_xor(bits, 4);
    if ((lane & 7) == 0 && word < wpr) T[(size_t)y * wpr + word] = bits;
}

// Pass 1 for the Y planes of I010 / I012 surfaces: the content mask is that of the 8-bit analysis plane min(sample >> shift, 255) (shift =
// bits - 8: 2 or 4, a kernel argument as in k_gray.hip) - min(sample >> shift, 255) > 1, which is (sample >> shift) > 1: the saturation
// cannot undo it.  All sixteen bits of a sample are looked at: out-of-range content is content.  The lane / wave / workgroup layout of
// threshold_bits_p010_kernel: a lane takes 8 samples - WIDE: with ONE 16-byte load (width a multiple of 8 samples, rows 16-byte aligned);
// else sample by sample, any width and any even pitch.
template <bool WIDE>
__global__ __launch_bounds__(256) void threshold_bits_lo16_kernel(size_t stride, int w, int h, u64* __restrict__ T, int wpr, SrcList srcs, size_t tfb,
                                                                  int shift) {
    const uint8_t* __restrict__ src = srcs.p[blockIdx.z];
    T += (size_t)blockIdx.z * tfb;
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int x = blockIdx.x * 512 + lane * 8, word = blockIdx.x * 8 + (lane >> 3);
    if (y >= h) return;                                                  // (wave-uniform)
    uint32_t m = 0;
    const uint8_t* row = src + (size_t)y * stride;
    if (WIDE) {
        if (x < w) {                                                     // (w is a multiple of 8: the lane's samples are all inside or all outside)
            const uint4 d = *reinterpret_cast<const uint4*>(row + (size_t)x * 2);
            auto pair = [shift](uint32_t v) { return (((v & 0xFFFFu) >> shift) > 1u ? 1u : 0u) | ((v >> (16 + shift)) > 1u ? 2u : 0u); };
            m = pair(d.x) | pair(d.y) << 2 | pair(d.z) << 4 | pair(d.w) << 6;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (x + i < w) m |= (((uint32_t)reinterpret_cast<const uint16_t*>(row)[x + i] >> shift) > 1u ? 1u : 0u) << i;
    }
    u64 bits = (u64)m << (8 * (lane & 7));
    bits |= __shfl_xor(bits, 1);
    bits |= __shfl_xor(bits, 2);
    bits |= __shfl_xor(bits, 4);
    if ((lane & 7) == 0 && word < wpr) T[(size_t)y * wpr + word] = bits;
}

constexpr int MC_ROWS = 56;      // rows a wave of the morphology pass owns (lanes 4..59; halo 4 above and below)

// OR / AND of a row with itself moved by -2..2 pixels; l, r: the words left and right of it
__device__ __forceinline__ u64 spread5(u64 l, u64 t, u64 r) {
    return t | (t << 1) | (l >> 63) | (t << 2) | (l >> 62) | (t >> 1) | (r << 63) | (t >> 2) | (r << 62);
}
__device__ __forceinline__ u64 shrink5(u64 l, u64 t, u64 r) {
    return t & ((t << 1) | (l >> 63)) & ((t << 2) | (l >> 62)) & ((t >> 1) | (r << 63)) & ((t >> 2) | (r << 62));
}
__device__ __forceinline__ u64 row_from(u64 v, int d, int lane) {     // value of lane + d, zero past the wave
    const u64 t = __shfl(v, lane + d);
    return (unsigned)(lane + d) < 64u ? t : 0;
}

// Pass 2: MORPH_CLOSE with the 5x5 ellipse (rows -1..1 five wide, rows -2 and +2 the centre only) on the bit
// plane: wave = one word column, lane = row, a row of 64 pixels one register.  Dilation sees zeros outside the
// image, erosion ones (cv::morphologyEx border value).  The result goes out as a zero-framed BitFrame (host
// side below) or, for vs_op_content_mask, as a plain bit plane that expand_bits_kernel turns into bytes.
__global__ __launch_bounds__(64) void close5_bits_kernel(const u64* __restrict__ T, int wpr, int w, int h,
                                                         u64* __restrict__ out, int opitch, int oframe, size_t tfb, size_t ofb) {
    T += (size_t)blockIdx.z * tfb; out += (size_t)blockIdx.z * ofb;      // (words between the pictures of a launch)
    const int lane = threadIdx.x, k = blockIdx.x, y = blockIdx.y * MC_ROWS - 4 + lane;
    const bool row_in = y >= 0 && y < h;
    auto word_in = [&](int kk) { return kk >= 0 && kk < wpr; };
    auto ones_outside = [&](int kk) -> u64 {        // bits of word kk that lie outside the image
        if (!row_in || !word_in(kk)) return ~0ull;
        const int left = w - 64 * kk;                // pixels of this word inside the image
        return left >= 64 ? 0ull : ~0ull << left;
    };
    u64 t[5];
#pragma unroll
    for (int j = 0; j < 5; j++) t[j] = (row_in && word_in(k - 2 + j)) ? T[(size_t)y * wpr + k - 2 + j] : 0ull;
    u64 d[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {                    // dilated words k-1, k, k+1
        const u64 hrow = spread5(t[j], t[j + 1], t[j + 2]);
        d[j] = row_from(hrow, -1, lane) | hrow | row_from(hrow, 1, lane) | row_from(t[j + 1], -2, lane) |
               row_from(t[j + 1], 2, lane);
        d[j] |= ones_outside(k - 1 + j);
    }
    // rows past the wave count as outside for the lanes that look at them; those lanes' results are not stored
    const u64 erow = shrink5(d[0], d[1], d[2]);
    auto and_from = [&](u64 v, int dd) { const u64 tv = __shfl(v, lane + dd); return (unsigned)(lane + dd) < 64u ? tv : ~0ull; };
    u64 f = and_from(erow, -1) & erow & and_from(erow, 1) & and_from(d[1], -2) & and_from(d[1], 2);
    f &= ~ones_outside(k);
    if (row_in && lane >= 4 && lane < 4 + MC_ROWS) out[(size_t)(y + oframe) * opitch + k + oframe] = f;
}

__global__ __launch_bounds__(256) void expand_bits_kernel(const u64* __restrict__ F, int wpr, int w, int h,
                                                          uint8_t* __restrict__ mask, size_t mstride) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < w && y < h) mask[(size_t)y * mstride + x] = (F[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1 ? 255 : 0;
}

// The pictures a content mask is taken from: what a pixel is, and - for a batch - the table of sources.
struct MaskSources {
    int cn = 1;                  // channels of a pixel: 1, or 3 / 4 (interleaved colour pictures)
    int sb = 1;                  // bytes of a sample; 2 (a table of sources, cn 1): luma planes of 16-bit samples, stride in bytes, everything even
    int lo_shift = 0;            // 16-bit samples: 0 = the mask of their high bytes (P010), else that of min(sample >> lo_shift, 255) (I010: 2, I012: 4)
    int bi = 0;                  // the byte of B inside a colour pixel (BGR8 / BGRA8: 0, RGB8 / RGBA8: 2)
    // the table (optional, d_src == nullptr): `frames` <= SRC_LIST_MAX source pointers on the HOST, one geometry and pitch, aligned:
    // every one of them is 4-byte aligned; the pictures' bit planes / results lie tfb / ofb words apart
    const uint8_t* const* srcs = nullptr;
    int frames = 1, aligned = 0;
    size_t tfb = 0, ofb = 0;
};
// ... the sample part of it for the frames of a format (the roll / zoom stages' formats: the luma plane, or the colour picture)
MaskSources mask_sources(const PixFmt& f) {
    MaskSources m;
    m.cn = f.kind == PIX_INTERLEAVED ? f.cn : 1;
    m.sb = f.sample_bytes;
    m.lo_shift = f.lo16_shift();
    m.bi = f.fmt == VS_FMT_RGB8 || f.fmt == VS_FMT_RGBA8 ? 2 : 0;
    return m;
}

// d_T: scratch of ceil(w/64)*h words.  The closed mask goes to d_out with row pitch opitch words, shifted by
// oframe rows and words (1 for a BitFrame whose frame is already zero, 0 for a plain bit plane).
// d_src: the one picture, or nullptr: the table of m.
int launch_content_bits(const uint8_t* d_src, size_t stride, int w, int h, u64* d_T, u64* d_out, int opitch, int oframe, hipStream_t st,
                        const MaskSources& m) {
    const int cn = m.cn, sb = m.sb, lo_shift = m.lo_shift, bi = m.bi, frames = m.frames;
    const uint8_t* const* srcs = m.srcs;
    bool ok = d_T && d_out && w > 0 && h > 0 && frames >= 1;
    ok = ok && (cn == 1 || cn == 3 || cn == 4) && (sb == 1 || sb == 2);
    ok = ok && lo_shift >= 0 && lo_shift <= 8 && (!lo_shift || sb == 2);
    ok = ok && (sb == 1 || (!d_src && cn == 1));                     // 16-bit samples: a table of luma planes
    ok = ok && (d_src || (srcs && frames <= SRC_LIST_MAX));
    ok = ok && (bi == 0 || (bi == 2 && cn >= 3));
    if (!ok) { set_last_error("content_mask: invalid argument"); return VS_ERR_INVALID_ARG; }
    if (h > 65535) { set_last_error("content_mask: image too tall"); return VS_ERR_INVALID_ARG; }
    const int wpr = (w + 63) / 64;
    // (a table of sources: srcs_aligned = every one of them is 4-byte aligned; four-byte pixels: a lane's load is 16 bytes, looked up here)
    int aligned = !d_src ? (m.aligned && (stride & 3) == 0) : ((((uintptr_t)d_src | stride) & 3) == 0);
    if (cn == 4) {
        aligned = (stride & 15) == 0 && ((uintptr_t)d_src & 15) == 0;
        for (int i = 0; !d_src && aligned && i < frames; i++) aligned = ((uintptr_t)srcs[i] & 15) == 0;
    }
    SrcList sl;
    for (int i = 0; i < SRC_LIST_MAX; i++) sl.p[i] = !d_src ? srcs[i < frames ? i : 0] : nullptr;
    dim3 g1((w + 1023) / 1024, h, frames);
    bool wide = !d_src && cn == 1 && (w & (sb == 2 ? 7 : 15)) == 0 && (stride & 15) == 0;
    for (int i = 0; wide && i < frames; i++) wide = ((uintptr_t)srcs[i] & 15) == 0;
    if (sb == 2 && lo_shift) {
        const dim3 g((w + 511) / 512, (h + 3) / 4, frames);
        if (wide) hipLaunchKernelGGL(threshold_bits_lo16_kernel<true>, g, dim3(256), 0, st, stride, w, h, d_T, wpr, sl, m.tfb, lo_shift);
        else hipLaunchKernelGGL(threshold_bits_lo16_kernel<false>, g, dim3(256), 0, st, stride, w, h, d_T, wpr, sl, m.tfb, lo_shift);
    } else if (sb == 2) {
        const dim3 g((w + 511) / 512, (h + 3) / 4, frames);
        if (wide) hipLaunchKernelGGL(threshold_bits_p010_kernel<true>, g, dim3(256), 0, st, stride, w, h, d_T, wpr, sl, m.tfb);
        else hipLaunchKernelGGL(threshold_bits_p010_kernel<false>, g, dim3(256), 0, st, stride, w, h, d_T, wpr, sl, m.tfb);
    } else if (wide) hipLaunchKernelGGL(threshold_bits_gray16_kernel, dim3((w + 1023) / 1024, (h + 3) / 4, frames), dim3(256), 0, st, stride, w, h, d_T, wpr, sl, m.tfb);
    else if (cn == 4 && bi) hipLaunchKernelGGL((threshold_bits_kernel<4, 2>), g1, dim3(256), 0, st, d_src, stride, w, aligned, d_T, wpr, sl, m.tfb);
    else if (cn == 4) hipLaunchKernelGGL((threshold_bits_kernel<4, 0>), g1, dim3(256), 0, st, d_src, stride, w, aligned, d_T, wpr, sl, m.tfb);
    else if (cn == 3 && bi) hipLaunchKernelGGL((threshold_bits_kernel<3, 2>), g1, dim3(256), 0, st, d_src, stride, w, aligned, d_T, wpr, sl, m.tfb);
    else if (cn == 3) hipLaunchKernelGGL(threshold_bits_kernel<3>, g1, dim3(256), 0, st, d_src, stride, w, aligned, d_T, wpr, sl, m.tfb);
    else hipLaunchKernelGGL(threshold_bits_kernel<1>, g1, dim3(256), 0, st, d_src, stride, w, aligned, d_T, wpr, sl, m.tfb);
    dim3 g2(wpr, (h + MC_ROWS - 1) / MC_ROWS, frames);
    hipLaunchKernelGGL(close5_bits_kernel, g2, dim3(64), 0, st, d_T, wpr, w, h, d_out, opitch, oframe, m.tfb, m.ofb);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace
}  // namespace vsd

using namespace vsd;

struct vs_azc {
    int device = 0;
    hipStream_t st = nullptr;
    std::string err;
    uint8_t* d_mask = nullptr;
    uint8_t* h_mask = nullptr;        // pinned; both hold the mask as a BitFrame
    u64* d_tbits = nullptr;           // thresholded bit plane, before the closing
    uint8_t* d_in = nullptr;
    uint8_t* d_out = nullptr;
    int mask_w = 0, mask_h = 0;       // the size d_mask / h_mask (a BitFrame) are laid out for
    size_t io_bytes = 0;
    CropScratch scratch;
    int32_t info[8] = {0};
    int ow = 640, oh = 360;           // the output size (vs_azc_set_output_size): the reference's constants, or 0, 0 = the surface's own
    // ---- asynchronous NV12 path (vs_azc_apply_nv12_dev) ----
    // Eight consecutive frames form a batch: their mask kernels are ONE launch each (blockIdx.z = frame) and their bit masks come
    // to page-locked memory with one copy (a launch costs the host 6 - 7 us on this runtime: per frame they were half of the
    // chain's host time).  The contour logic - host work in the reference as well (AutoZoomCrop.cpp:141-147 downloads the mask for
    // cv::findContours) - runs on worker threads, a frame each (frames do not depend on each other; 0.3 ms per 4K frame and
    // thread); the worker that finishes a batch's last contour queues the crop-and-scale of the batch's surfaces, both planes, as
    // one launch.  NBS batches in flight.
    static constexpr int ZB = 8, NBS = 4, NRES = 1024;      // (ZB <= SRC_LIST_MAX, 3 ZB <= WARP_JOBS_MAX: three planes of a planar surface)
    int nw = 12;                         // worker threads (VS_AZC_WORKERS, 1 .. 16): 31 k frames/s alone with eight, 41 k with twelve
    // ow, oh: the output size the frame was handed over under, resolved (never 0)
    struct Frame : StageFrame { long ticket; int ow, oh; };
    struct BatchSlot {
        uint8_t* d_masks = nullptr;      // ZB BitFrames
        uint8_t* h_masks = nullptr;      // page-locked
        u64* d_tbits = nullptr;          // ZB thresholded bit planes, before the closing
        hipStream_t st = nullptr;        // the batch's mask kernels and mask copy: a stream per slot, so that the next batch's kernels
                                         // do not queue behind this batch's 8 MB on the way to the host
        hipEvent_t ev = nullptr;
        int mw = 0, mh = 0;
        int n = 0, left = 0;             // frames of the batch / n until the batch's crop-and-scale has been queued, then 0 (slot free)
        int todo = 0, nwj = 0;           // host parts not yet through / crop-and-scale jobs collected (wj)
        WarpJob wj[3 * ZB];
        int arrived = 0;                 // the masks: 0 on their way, 2 there, 3 the wait for them failed
        std::chrono::steady_clock::time_point t_issue, t_arrive;
        Frame fr[ZB];
    } bslot[NBS];
    struct Result { long ticket = -1; int out_w = 0, out_h = 0, rc = 0; int32_t info[8] = {0}; } results[NRES];
    std::vector<Frame> pending;          // handed over, not yet a batch
    long nbatches = 0;
    hipStream_t st_out = nullptr;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::deque<std::pair<int, int>> jobs;    // (batch slot, frame of the batch): the masks are there
    std::deque<int> on_the_way;              // batch slots whose masks are on their way, oldest first
    bool waiting = false;                    // a worker waits for the oldest of them
    bool quit = false;
    long issued = 0, completed = 0;
    FirstFailure failure;                // the first failed frame of the workers (reported by vs_azc_sync)
    // where the workers' time goes (vs_azc_worker_times): frames, and seconds waiting for a job / for a batch's masks / in the
    // contour logic / queueing launches and publishing
    double wt[5] = {0, 0, 0, 0, 0};
    double bt[4] = {0, 0, 0, 0};         // batches; seconds from a batch's launches to its masks' arrival / from there to its crop launch /
                                         // the caller waited for a free batch slot
};

static_assert(vs_azc::ZB <= SRC_LIST_MAX && 3 * vs_azc::ZB <= WARP_JOBS_MAX, "a batch's sources and warp jobs travel as kernel arguments");

extern "C" {

// The mask as 0 / 255 bytes (the form cv::threshold / cv::morphologyEx hand on); scratch for the two bit planes is
// kept between calls.
int vs_op_content_mask(const void* d_src, size_t stride, int w, int h, int cn, void* d_mask, size_t mask_stride,
                       void* stream) {
    VS_TRY(ensure_device());
    if (!d_mask || w <= 0 || h <= 0 || mask_stride < (size_t)w || (cn != 1 && cn != 3)) { set_last_error("content_mask: invalid argument"); return VS_ERR_INVALID_ARG; }
    static std::mutex mu;
    static u64* planes = nullptr;
    static size_t plane_words = 0;
    std::lock_guard<std::mutex> lock(mu);
    const int wpr = (w + 63) / 64;
    const size_t words = (size_t)wpr * h;
    hipStream_t st = (hipStream_t)stream;
    if (plane_words < words) {
        if (planes) { VS_HIP_TRY(hipDeviceSynchronize()); (void)hipFree(planes); planes = nullptr; plane_words = 0; }
        VS_HIP_TRY(hipMalloc((void**)&planes, 2 * words * 8));
        plane_words = words;
    }
    MaskSources m;
    m.cn = cn;
    VS_TRY(launch_content_bits((const uint8_t*)d_src, stride, w, h, planes, planes + plane_words, wpr, 0, st, m));
    dim3 grid((w + 255) / 256, h);
    hipLaunchKernelGGL(expand_bits_kernel, grid, dim3(256), 0, st, planes + plane_words, wpr, w, h, (uint8_t*)d_mask, mask_stride);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

int vs_azc_create(int device, vs_azc** out) {
    if (!out) return VS_ERR_INVALID_ARG;
    *out = nullptr;
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipSetDevice(device));
    vs_azc* a = new (std::nothrow) vs_azc();
    if (!a) return VS_ERR_HIP;
    a->device = device;
    hipError_t e = hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking);
    if (e != hipSuccess) { set_last_error(hipGetErrorString(e)); delete a; return VS_ERR_HIP; }
    *out = a;
    return VS_OK;
}

void vs_azc_destroy(vs_azc* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (!a->workers.empty()) {
        { std::lock_guard<std::mutex> g(a->mu); a->quit = true; }
        a->cv_job.notify_all();
        for (auto& t : a->workers) t.join();
    }
    if (a->st_out) { (void)hipStreamSynchronize(a->st_out); (void)hipStreamDestroy(a->st_out); }
    for (auto& q : a->bslot) {
        if (q.st) { (void)hipStreamSynchronize(q.st); (void)hipStreamDestroy(q.st); }
        if (q.d_masks) (void)hipFree(q.d_masks);
        if (q.h_masks) (void)hipHostFree(q.h_masks);
        if (q.d_tbits) (void)hipFree(q.d_tbits);
        if (q.ev) (void)hipEventDestroy(q.ev);
    }
    if (a->st) (void)hipStreamSynchronize(a->st);
    if (a->d_mask) (void)hipFree(a->d_mask);
    if (a->h_mask) (void)hipHostFree(a->h_mask);
    if (a->d_tbits) (void)hipFree(a->d_tbits);
    if (a->d_in) (void)hipFree(a->d_in);
    if (a->d_out) (void)hipFree(a->d_out);
    if (a->st) (void)hipStreamDestroy(a->st);
    delete a;
}

const char* vs_azc_last_error(const vs_azc* a) { return a ? a->err.c_str() : ""; }

int vs_azc_get_info(const vs_azc* a, int32_t* info8) {
    if (!a || !info8) return VS_ERR_INVALID_ARG;
    memcpy(info8, a->info, sizeof a->info);
    return VS_OK;
}

static int azc_flush_pending(vs_azc* a, std::unique_lock<std::mutex>& lk);

int vs_azc_sync(vs_azc* a) {
    if (!a) return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(a, hipSetDevice(a->device));
    if (!a->workers.empty()) {          // asynchronous NV12 frames: their host parts first, then what the workers queued
        std::unique_lock<std::mutex> lk(a->mu);
        const int frc = azc_flush_pending(a, lk);      // (a failed flush completes its frames with the error)
        a->cv_done.wait(lk, [&] { return a->completed == a->issued; });
        const FirstFailure wf = a->failure.take();
        lk.unlock();
        VS_OBJ_HIP(a, hipStreamSynchronize(a->st_out));
        if (frc != VS_OK) return frc;
        if (wf.rc != VS_OK) return vs_obj_fail(a, wf.rc, wf.msg);
    }
    VS_OBJ_HIP(a, hipStreamSynchronize(a->st));
    return VS_OK;
}

// Mask on the device, contour logic on the host: fills a->info (:111-228).
static int azc_plan(vs_azc* a, const void* d_data, int w, int h, size_t stride, int cn) {
    if (w > 65535 || h > 32767) return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: image too large");
    const size_t mb = BitFrame::words_for(w, h) * 8;
    if (a->mask_w != w || a->mask_h != h) {
        if (a->d_mask) (void)hipFree(a->d_mask);
        if (a->h_mask) (void)hipHostFree(a->h_mask);
        if (a->d_tbits) (void)hipFree(a->d_tbits);
        a->d_mask = a->h_mask = nullptr; a->d_tbits = nullptr; a->mask_w = a->mask_h = 0;
        VS_OBJ_HIP(a, hipMalloc((void**)&a->d_mask, mb));
        VS_OBJ_HIP(a, hipMalloc((void**)&a->d_tbits, (size_t)((w + 63) / 64) * h * 8));
        VS_OBJ_HIP(a, hipHostMalloc((void**)&a->h_mask, mb, hipHostMallocDefault));
        VS_OBJ_HIP(a, hipMemsetAsync(a->d_mask, 0, mb, a->st));          // the frame; the kernel rewrites the inside
        a->mask_w = w; a->mask_h = h;
    }
    BitFrame bf;
    bf.w = w; bf.h = h; bf.pitch = BitFrame::pitch_for(w); bf.F = (const uint64_t*)a->h_mask;
    MaskSources m;
    m.cn = cn;
    VS_OBJ_TRY(a, launch_content_bits((const uint8_t*)d_data, stride, w, h, a->d_tbits, (u64*)a->d_mask, bf.pitch, 1, a->st, m));   // :111-139
    VS_OBJ_HIP(a, hipMemcpyAsync(a->h_mask, a->d_mask, mb, hipMemcpyDeviceToHost, a->st));                 // :142-143
    VS_OBJ_HIP(a, hipStreamSynchronize(a->st));
    crop_from_mask(bf, a->scratch, a->info, nullptr);                                                 // :146-228
    return VS_OK;
}

// Crop + scale (:246-270) or the unchanged frame (:149-152, :238-249), left in flight on a->st.
static int azc_emit(vs_azc* a, const void* d_data, int w, int h, size_t stride, int cn, void* d_out, size_t out_stride) {
    if (!a->info[7]) {
        if (out_stride < (size_t)w * cn) return VS_ERR_INVALID_ARG;
        VS_OBJ_HIP(a, hipMemcpy2DAsync(d_out, out_stride, d_data, stride, (size_t)w * cn, h, hipMemcpyDeviceToDevice, a->st));
        return VS_OK;
    }
    const int ow = a->ow ? a->ow : w, oh = a->oh ? a->oh : h;
    if (out_stride < (size_t)ow * cn) return VS_ERR_INVALID_ARG;
    const int cx = a->info[2], cy = a->info[3], cw = a->info[4], ch = a->info[5];
    // M = [sx 0 0; 0 sy 0] held as CV_32F (:261-262); cv::warpAffine inverts it in double
    const float Mf[6] = {(float)((double)ow / cw), 0.f, 0.f, 0.f, (float)((double)oh / ch), 0.f};
    double Mi[6];
    warp_invert(Mf, Mi);
    const uint8_t* roi = (const uint8_t*)d_data + (size_t)cy * stride + (size_t)cx * cn;
    uint8_t* out = (uint8_t*)d_out;
    VS_OBJ_TRY(a, launch_warp_plane(&roi, &out, 1, stride, cw, ch, out_stride, ow, oh, cn, WarpMaps{Mi, 6, true}, VS_BORDER_BLACK, WarpTabs{}, a->st));
    return VS_OK;
}

// Frame in HBM -> the crop at the output size (ow x oh: 640 x 360, or what vs_azc_set_output_size said) in HBM (or an unchanged copy on
// the fallback paths).  out_stride must fit either outcome (>= max(w, ow) * cn).  The result is left in flight on the object's stream (vs_azc_sync).
int vs_azc_apply_dev(vs_azc* a, const void* d_data, int w, int h, size_t stride, int cn, void* d_out, size_t out_stride,
                     int* out_w, int* out_h) {
    if (!a || !d_data || !d_out || !out_w || !out_h || w <= 0 || h <= 0 || (cn != 1 && cn != 3) || stride < (size_t)w * cn ||
        out_stride < (size_t)std::max(w, a->ow) * cn)
        return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(a, hipSetDevice(a->device));
    int rc = azc_plan(a, d_data, w, h, stride, cn);
    if (rc != VS_OK) return rc;
    rc = azc_emit(a, d_data, w, h, stride, cn, d_out, out_stride);
    if (rc != VS_OK) return rc;
    *out_w = a->info[7] && a->ow ? a->ow : w;
    *out_h = a->info[7] && a->oh ? a->oh : h;
    return VS_OK;
}

// cv::Mat autoZoomCrop(const cv::Mat&, double) on host buffers.  `out` must hold max(w*h, ow*oh)*cn bytes and
// receives packed rows of *out_w * cn bytes.
int vs_azc_apply(vs_azc* a, const uint8_t* data, int w, int h, size_t stride, int cn, uint8_t* out, int* out_w, int* out_h) {
    if (!a || !data || !out || !out_w || !out_h || w <= 0 || h <= 0 || (cn != 1 && cn != 3) || stride < (size_t)w * cn)
        return VS_ERR_INVALID_ARG;
    VS_OBJ_HIP(a, hipSetDevice(a->device));
    const size_t row = (size_t)w * cn, bytes = std::max(row * h, (size_t)(a->ow ? a->ow : w) * (a->oh ? a->oh : h) * cn);
    if (a->io_bytes < bytes) {
        if (a->d_in) (void)hipFree(a->d_in);
        if (a->d_out) (void)hipFree(a->d_out);
        a->d_in = a->d_out = nullptr; a->io_bytes = 0;
        VS_OBJ_HIP(a, hipMalloc((void**)&a->d_in, bytes));
        VS_OBJ_HIP(a, hipMalloc((void**)&a->d_out, bytes));
        a->io_bytes = bytes;
    }
    VS_OBJ_HIP(a, hipMemcpy2DAsync(a->d_in, row, data, stride, row, h, hipMemcpyHostToDevice, a->st));
    int rc = azc_plan(a, a->d_in, w, h, row, cn);
    if (rc != VS_OK) return rc;
    const int ow = a->info[7] && a->ow ? a->ow : w, oh = a->info[7] && a->oh ? a->oh : h;
    rc = azc_emit(a, a->d_in, w, h, row, cn, a->d_out, (size_t)ow * cn);
    if (rc != VS_OK) return rc;
    VS_OBJ_HIP(a, hipMemcpyAsync(out, a->d_out, (size_t)ow * cn * oh, hipMemcpyDeviceToHost, a->st));
    VS_OBJ_HIP(a, hipStreamSynchronize(a->st));
    *out_w = ow; *out_h = oh;
    return VS_OK;
}

// ---- NV12, asynchronous ----------------------------------------------------------------------------------------------------
// (a->mu held) A frame's outcome, the one place a worker publishes it: its result and, for a frame that failed (its masks did not
// arrive, its copy or its batch's crop launch could not be queued), the object's first failure.
static void azc_publish(vs_azc* a, const vs_azc::Result& res) {
    a->results[res.ticket % vs_azc::NRES] = res;
    a->failure.note(res.rc, "auto zoom/crop: a worker's launch failed");
}

// One frame's host part, on a worker thread: the contour logic on the frame's mask once its batch's masks have arrived, then its
// crop-and-scale jobs (or, at once, the copy of the fall-back paths) for every plane on st_out; the worker that finishes a batch's
// last frame queues the batch's jobs as one launch.  The content mask is taken from the luma plane (gray > 1, :121-127 on a picture
// that is gray already); the crop rectangle applies to the luma plane as it is and, shifted, to a subsampled chroma plane;
// each plane is scaled to its share of the frame's output size by the reference's scale matrix (:261-270, ow x oh for 640 x 360).
// An interleaved colour frame is one plane of cn channels: the mask from B, G, R where the format has them (:121-127), one job
// with the rectangle as it is, every channel - the fourth too - scaled as a channel of its own.
static void azc_worker(vs_azc* a) {
    (void)hipSetDevice(a->device);
    CropScratch scratch;
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point p, clk::time_point q) { return std::chrono::duration<double>(q - p).count(); };
    for (;;) {
        std::pair<int, int> job;
        const clk::time_point t_idle = clk::now();
        clk::time_point t_job = t_idle;
        {
            // A frame becomes a job when its batch's masks have arrived.  The batches on their way are waited for in order by ONE
            // worker at a time - whichever has nothing else to do (a blocking wait: no core spent on it) - so that the others
            // stay free for the frames of the batches that are there.  (With a wait per frame the workers stood in front of the
            // copy engine 250 - 330 us per frame; that time is idle time now - beside a stabilizer the stage is bound by the latency
            // of its device part, scratch/README.md.)
            std::unique_lock<std::mutex> lk(a->mu);
            for (;;) {
                if (!a->jobs.empty()) break;
                if (!a->on_the_way.empty() && !a->waiting) {
                    const int slot = a->on_the_way.front();
                    a->on_the_way.pop_front();
                    a->waiting = true;
                    lk.unlock();
                    const clk::time_point t0 = clk::now();
                    const hipError_t e = hipEventSynchronize(a->bslot[slot].ev);
                    const clk::time_point t1 = clk::now();
                    lk.lock();
                    a->waiting = false;
                    a->wt[2] += secs(t0, t1);
                    t_job = t_job + (t1 - t0);                      // (not idle time)
                    a->bslot[slot].arrived = e == hipSuccess ? 2 : 3;
                    a->bslot[slot].t_arrive = t1;
                    for (int i = 0; i < a->bslot[slot].n; i++) a->jobs.emplace_back(slot, i);
                    a->cv_job.notify_all();
                    continue;
                }
                if (a->quit) return;
                a->cv_job.wait(lk);
            }
            job = a->jobs.front();
            a->jobs.pop_front();
        }
        vs_azc::BatchSlot& b = a->bslot[job.first];
        const vs_azc::Frame q = b.fr[job.second];
        vs_azc::Result res;
        res.ticket = q.ticket;
        int rc = b.arrived == 3 ? VS_ERR_HIP : VS_OK;
        WarpJob wj[3];
        int nscaled = 0;                 // crop-and-scale jobs of this frame: one per plane, 0 on the fall-back paths
        const clk::time_point t_masks = clk::now();
        clk::time_point t_contour = t_masks;
        t_job = t_job > t_masks ? t_masks : t_job;
        if (rc == VS_OK) {
            BitFrame bf;
            bf.w = q.w; bf.h = q.h; bf.pitch = BitFrame::pitch_for(q.w);
            bf.F = (const uint64_t*)(b.h_masks + (size_t)job.second * BitFrame::words_for(q.w, q.h) * 8);
            crop_from_mask(bf, scratch, res.info, nullptr);                                                // :146-228
            t_contour = clk::now();
            if (!res.info[7]) {                                                                            // :149-152, :238-249
                res.out_w = q.w; res.out_h = q.h;
                if (copy_planes(q.dst, q.D, q.src, q.S, hipMemcpyDeviceToDevice, a->st_out) != hipSuccess) rc = VS_ERR_HIP;     // the unchanged surface, every plane
            } else {
                res.out_w = q.ow; res.out_h = q.oh;
                // plane by plane: the rectangle as the plane sees it (luma and a colour frame: as it is), scaled to the plane's share of the
                // output size with M = [sx 0 0; 0 sy 0] held as CV_32F (:261-262); every channel a channel of its own
                for (int k = 0; k < q.S.n; k++) {
                    const PlaneRect c = plane_crop(q.S[k], res.info[2], res.info[3], res.info[4], res.info[5]), o = plane_result(q.S[k], q.ow, q.oh);
                    const float M[6] = {(float)((double)o.w / c.w), 0.f, 0.f, 0.f, (float)((double)o.h / c.h), 0.f};
                    warp_invert(M, wj[k].m);
                    wj[k].src = q.src + plane_crop_offset(q.S, k, c); wj[k].dst = q.dst + q.D[k].off;
                    wj[k].sstride = (uint32_t)q.S[k].pitch; wj[k].dstride = (uint32_t)q.D[k].pitch;
                    wj[k].sw = c.w; wj[k].sh = c.h; wj[k].dw = o.w; wj[k].dh = o.h; wj[k].cn = q.S[k].cn;
                    wj[k].border = VS_BORDER_BLACK; wj[k].sb = q.S.sample_bytes;
                }
                nscaled = q.S.n;
            }
        }
        res.rc = rc;
        // The crop-and-scale of the batch's frames is ONE launch when its jobs are of one class, two when some can be staged and some
        // cannot (launch_scale_jobs), queued by the worker that finishes the batch's last contour; a frame counts as complete (vs_azc_sync) when that launch has been queued.
        bool last;
        int njobs = 0;
        WarpJob all[3 * vs_azc::ZB];
        {
            std::lock_guard<std::mutex> g(a->mu);
            azc_publish(a, res);
            for (int k = 0; k < nscaled; k++) b.wj[b.nwj++] = wj[k];
            last = --b.todo == 0;
            if (last) { njobs = b.nwj; memcpy(all, b.wj, sizeof(WarpJob) * njobs); }
        }
        a->cv_done.notify_all();          // (vs_azc_result waits for the host part only)
        // (a batch holds one kind of frame: colour jobs go to the colour instances of the two kernels)
        int lrc = !(last && njobs) ? VS_OK : q.pf->kind == PIX_INTERLEAVED ? launch_scale_jobs_rgb(all, njobs, 0, a->st_out) : launch_scale_jobs(all, njobs, 0, a->st_out);
        {
            std::lock_guard<std::mutex> g(a->mu);
            const clk::time_point t_end = clk::now();
            a->wt[0] += 1; a->wt[1] += secs(t_idle, t_masks) - secs(t_idle, t_job); a->wt[3] += secs(t_masks, t_contour);
            a->wt[4] += secs(t_contour, t_end);
            if (!last) continue;
            if (lrc != VS_OK) {
                for (int i = 0; i < b.n; i++) {
                    vs_azc::Result r = a->results[b.fr[i].ticket % vs_azc::NRES];
                    r.rc = lrc;
                    azc_publish(a, r);
                }
            }
            a->completed += b.n;
            b.left = 0;
            a->bt[0] += 1; a->bt[1] += secs(b.t_issue, b.t_arrive); a->bt[2] += secs(b.t_arrive, t_end);
        }
        a->cv_done.notify_all();
    }
}

// (a->mu held through lk) what has been handed over becomes a batch: mask kernels, one copy, a job per frame
static int azc_issue_batch(vs_azc* a, std::unique_lock<std::mutex>& lk) {
    vs_azc::BatchSlot& b = a->bslot[a->nbatches % vs_azc::NBS];
    {
        const auto t0 = std::chrono::steady_clock::now();
        a->cv_done.wait(lk, [&] { return b.left == 0; });
        a->bt[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    const int n = (int)a->pending.size();
    const int w = a->pending[0].w, h = a->pending[0].h;
    const size_t mb = BitFrame::words_for(w, h) * 8, tw = (size_t)((w + 63) / 64) * h;
    if (!b.ev) {
        VS_OBJ_HIP(a, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming | hipEventBlockingSync));
        VS_OBJ_HIP(a, hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
    }
    if (b.mw != w || b.mh != h) {
        if (b.d_masks) (void)hipFree(b.d_masks);
        if (b.h_masks) (void)hipHostFree(b.h_masks);
        if (b.d_tbits) (void)hipFree(b.d_tbits);
        b.d_masks = b.h_masks = nullptr; b.d_tbits = nullptr; b.mw = b.mh = 0;
        VS_OBJ_HIP(a, hipMalloc((void**)&b.d_masks, mb * vs_azc::ZB));
        VS_OBJ_HIP(a, hipMalloc((void**)&b.d_tbits, tw * 8 * vs_azc::ZB));
        VS_OBJ_HIP(a, hipHostMalloc((void**)&b.h_masks, mb * vs_azc::ZB, hipHostMallocDefault));
        VS_OBJ_HIP(a, hipMemsetAsync(b.d_masks, 0, mb * vs_azc::ZB, b.st));          // the frames of the BitFrames; the kernel rewrites the insides
        b.mw = w; b.mh = h;
    }
    int aligned = 1;
    const uint8_t* srcs[vs_azc::ZB];
    for (int i = 0; i < n; i++) {
        b.fr[i] = a->pending[i];
        srcs[i] = a->pending[i].src;
        if ((uintptr_t)a->pending[i].src & 3) aligned = 0;
    }
    MaskSources m = mask_sources(*a->pending[0].pf);
    m.srcs = srcs; m.frames = n; m.aligned = aligned; m.tfb = tw; m.ofb = mb / 8;
    VS_OBJ_TRY(a, launch_content_bits(nullptr, a->pending[0].S[0].pitch, w, h, b.d_tbits, (u64*)b.d_masks, BitFrame::pitch_for(w), 1, b.st, m));   // :111-139 on the luma planes / the colour frames
    VS_OBJ_HIP(a, hipMemcpyAsync(b.h_masks, b.d_masks, mb * n, hipMemcpyDeviceToHost, b.st));                                          // :142-143
    VS_OBJ_HIP(a, hipEventRecord(b.ev, b.st));
    b.t_issue = std::chrono::steady_clock::now();
    b.n = n; b.left = n; b.todo = n; b.nwj = 0; b.arrived = 0;
    a->on_the_way.push_back((int)(a->nbatches % vs_azc::NBS));
    a->nbatches++;
    a->pending.clear();
    a->cv_job.notify_all();
    return VS_OK;
}

// (a->mu held through lk) azc_issue_batch for the frames handed over.  When it fails, their tickets are out already: they complete
// with the error (the calling API call reports it), and no later call issues them again.
static int azc_flush_pending(vs_azc* a, std::unique_lock<std::mutex>& lk) {
    if (a->pending.empty()) return VS_OK;
    const int rc = azc_issue_batch(a, lk);
    if (rc != VS_OK) {
        for (const vs_azc::Frame& f : a->pending) {
            vs_azc::Result& r = a->results[f.ticket % vs_azc::NRES];
            r = vs_azc::Result{};
            r.ticket = f.ticket;
            r.rc = rc;
        }
        a->completed += (long)a->pending.size();
        a->pending.clear();
        a->cv_done.notify_all();
    }
    return rc;
}

// autoZoomCrop for an NV12 surface in HBM, ASYNCHRONOUS.  d_out receives the result - ow x oh, the object's output size: 640 x 360
// unless vs_azc_set_output_size said otherwise (luma rows of out_pitch bytes, the ow / 2 x oh / 2 interleaved chroma plane
// out_uv_offset bytes behind) - or, on the reference's fall-back paths, the unchanged
// w x h surface - so out_pitch >= max(w, ow) and out_uv_offset >= max(h, oh) * out_pitch.  The call returns at once with a
// ticket; eight consecutive frames of one geometry form a batch (vs_azc_sync and vs_azc_result close an incomplete one).
// vs_azc_result(ticket) tells what came out (it waits for that frame's host part), the pixels are complete after vs_azc_sync.
// Surface and result buffer must stay untouched until then; results of the last 1024 tickets are kept.
// (fr: checked by its entry point, ow / oh still to be set)
static int azc_hand_over(vs_azc* a, vs_azc::Frame fr, int64_t* ticket) {
    if (fr.w > 65535 || fr.h > 32767) return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: image too large");
    fr.ow = a->ow ? a->ow : fr.w; fr.oh = a->oh ? a->oh : fr.h;
    VS_OBJ_HIP(a, hipSetDevice(a->device));
    if (a->workers.empty()) {
        VS_OBJ_HIP(a, hipStreamCreateWithFlags(&a->st_out, hipStreamNonBlocking));
        try {
            if (const char* e = std::getenv("VS_AZC_WORKERS")) a->nw = std::max(1, std::min(std::atoi(e), 16));
            for (int i = 0; i < a->nw; i++) a->workers.emplace_back(azc_worker, a);
        } catch (...) {
            return vs_obj_fail(a, VS_ERR_HIP, "auto zoom/crop: cannot start worker threads");
        }
    }
    std::unique_lock<std::mutex> lk(a->mu);
    // (a change of format, of geometry or of either layout closes the pending batch: a batch's launches take one of each; a change of
    // the output size has closed it already, vs_azc_set_output_size)
    if (!a->pending.empty()) {
        const vs_azc::Frame& p0 = a->pending[0];
        if (p0.pf != fr.pf || p0.w != fr.w || p0.h != fr.h || !same_layout(p0.S, fr.S) || !same_layout(p0.D, fr.D)) {
            const int rc = azc_flush_pending(a, lk);
            if (rc != VS_OK) return rc;
        }
    }
    fr.ticket = a->issued;
    a->pending.push_back(fr);
    if (ticket) *ticket = a->issued;
    a->issued++;
    if ((int)a->pending.size() >= vs_azc::ZB) return azc_flush_pending(a, lk);
    return VS_OK;
}

// The frame record of an entry point: the result's planes are laid out for the larger of the frame and the output size
static vs_azc::Frame azc_frame(const PixFmt& f, int w, int h, const void* d_src, void* d_dst, const Planes& S, const Planes& D) {
    return vs_azc::Frame{StageFrame{&f, w, h, (const uint8_t*)d_src, (uint8_t*)d_dst, S, D}, 0, 0, 0};
}
static int azc_max_w(const vs_azc* a, int w) { return std::max(w, a->ow); }       // (an output size of 0: the frame's own)
static int azc_max_h(const vs_azc* a, int h) { return std::max(h, a->oh); }

// NV12 and P010: luma and the interleaved chroma plane; uv_offset 0 = behind the h luma rows, out_uv_offset has no default
static int azc_luma_uv(vs_azc* a, int fmt, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset, void* d_out, size_t out_pitch,
                       size_t out_uv_offset, int64_t* ticket) {
    const PixFmt& f = *pixfmt(fmt);
    const size_t sb = (size_t)f.sample_bytes;
    if (!a || !d_surface || !d_out) return VS_ERR_INVALID_ARG;
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || pitch < (size_t)w * sb) return VS_ERR_INVALID_ARG;
    const int mw = azc_max_w(a, w), mh = azc_max_h(a, h);
    if (out_pitch < (size_t)mw * sb || out_uv_offset < (size_t)mh * out_pitch) return VS_ERR_INVALID_ARG;
    if (sb == 2 && (((uintptr_t)d_surface | (uintptr_t)d_out | pitch | uv_offset | out_pitch | out_uv_offset) & 1))
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: P010 pointers, pitches and plane offsets must be even");
    return azc_hand_over(a, azc_frame(f, w, h, d_surface, d_out, planes(f, w, h, pitch, ChromaLayout{uv_offset}),
                                      planes(f, mw, mh, out_pitch, ChromaLayout{out_uv_offset})), ticket);
}

int vs_azc_apply_nv12_dev(vs_azc* a, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset, void* d_out, size_t out_pitch,
                          size_t out_uv_offset, int64_t* ticket) {
    return azc_luma_uv(a, VS_FMT_NV12, d_surface, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset, ticket);
}

// n surfaces of one layout in call order; tickets (optional) receives n tickets
int vs_azc_apply_nv12_dev_n(vs_azc* a, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h, size_t pitch, size_t uv_offset,
                            size_t out_pitch, size_t out_uv_offset, int64_t* tickets) {
    if (!a || !d_surfaces || !d_outs || n < 0) return VS_ERR_INVALID_ARG;
    return each_surface(n, [&](int i) {
        return vs_azc_apply_nv12_dev(a, d_surfaces[i], w, h, pitch, uv_offset, d_outs[i], out_pitch, out_uv_offset, tickets ? tickets + i : nullptr);
    });
}

// The same for a P010 surface (vs_pixfmt16; pitches and offsets in bytes, everything even: out_pitch >= 2 * max(w, ow)).  The content
// mask is that of the 8-bit plane of the luma samples' high bytes, (sample >> 8) > 1 - mask, contours, info8 and the crop rectangle are
// those of the NV12 call on that plane -; crop-and-scale on the 16-bit planes with P010's blend (S rounded once, half to even),
// BORDER_CONSTANT 0; on the fall-back paths the surface comes back unchanged, all 16 bits.  NV12 and P010 surfaces may alternate on one
// object: a change of sample size closes the pending batch as a change of geometry does.
int vs_azc_apply_p010_dev(vs_azc* a, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset, void* d_out, size_t out_pitch,
                          size_t out_uv_offset, int64_t* ticket) {
    return azc_luma_uv(a, VS_FMT_P010, d_surface, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset, ticket);
}

int vs_azc_apply_p010_dev_n(vs_azc* a, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h, size_t pitch, size_t uv_offset,
                            size_t out_pitch, size_t out_uv_offset, int64_t* tickets) {
    if (!a || !d_surfaces || !d_outs || n < 0) return VS_ERR_INVALID_ARG;
    return each_surface(n, [&](int i) {
        return vs_azc_apply_p010_dev(a, d_surfaces[i], w, h, pitch, uv_offset, d_outs[i], out_pitch, out_uv_offset, tickets ? tickets + i : nullptr);
    });
}

// The same for a three-plane surface: fmt VS_FMT_I420 (YV12: the two chroma offsets swapped), VS_FMT_I010, VS_FMT_I012, or a 4:2:2 / 4:4:4
// format (VS_FMT_I422, I444, I210, I212, I410, I412; (sx, sy): the format's chroma shifts, w and h even for every format); in / out: where
// the three planes lie (vs_i420_layout: bytes, 0 = the packed default for the chroma pitch - pitch >> sx - and the offsets).  The content
// mask comes from the 8-bit analysis plane of Y - Y itself, or min(sample >> (bits - 8), 255) -; the rectangle (x, y, cw, ch) applies to Y as
// it is and as (x >> sx, y >> sy, max(1, cw >> sx), max(1, ch >> sy)) to U and to V, each scaled to (ow >> sx) x (oh >> sy) as a one-channel
// plane (4:2:0: halved, ow / 2 x oh / 2): the three planes of a batch's surfaces are one launch (two when only some of
// its jobs can be staged).  The result's planes lie where `out` puts them whichever size comes out, so `out` must hold max(w, ow) x
// max(h, oh) - 640 x 360 unless vs_azc_set_output_size said otherwise -: its defaults are those of a surface of that size.  An I420 result is the de-interleaved result of vs_azc_apply_nv12_dev on the same samples.
int vs_azc_apply_i420_dev(vs_azc* a, int fmt, const void* d_surface, int w, int h, const vs_i420_layout* in, void* d_out, const vs_i420_layout* out,
                          int64_t* ticket) {
    if (!a || !d_surface || !d_out) return VS_ERR_INVALID_ARG;
    const PixFmt* f = pixfmt(fmt);
    if (!f || !f->three_planes())
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: the planar entry point takes a three-plane format (VS_FMT_I420, I010, I012, I422, I444, I210, I212, I410, I412)");
    I420Layout sl, dl;
    std::string msg;
    const int ow = a->ow ? a->ow : w, oh = a->oh ? a->oh : h, mw = azc_max_w(a, w), mh = azc_max_h(a, h);
    const std::string what = "auto zoom/crop (result: max(w, " + std::to_string(ow) + ") x max(h, " + std::to_string(oh) + "))";
    if (planar_layout_check(fmt, d_surface, w, h, in, w, h, "auto zoom/crop", &sl, &msg) != VS_OK ||
        planar_layout_check(fmt, d_out, w, h, out, mw, mh, what.c_str(), &dl, &msg) != VS_OK)
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, msg.c_str());
    return azc_hand_over(a, azc_frame(*f, w, h, d_surface, d_out, planes(*f, w, h, sl), planes(*f, mw, mh, dl)), ticket);
}

int vs_azc_apply_i420_dev_n(vs_azc* a, int fmt, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h, const vs_i420_layout* in,
                            const vs_i420_layout* out, int64_t* tickets) {
    if (!a || !d_surfaces || !d_outs || n < 0) return VS_ERR_INVALID_ARG;
    return each_surface(n, [&](int i) { return vs_azc_apply_i420_dev(a, fmt, d_surfaces[i], w, h, in, d_outs[i], out, tickets ? tickets + i : nullptr); });
}

// The same for an interleaved colour frame in HBM: fmt VS_FMT_BGR8, VS_FMT_RGB8, VS_FMT_BGRA8 or VS_FMT_RGBA8, one plane of w x h pixels
// (any w, h >= 1: there is no chroma plane), rows of `stride` bytes.  The content mask is that of BGR2GRAY on B, G, R where the format has
// them - the fourth channel never enters -, so info8 and the rectangle are those of the frame's BGR permutation; the crop is scaled with
// every channel, the fourth included, as a channel of its own (BORDER_CONSTANT 0 on the crop, also for the fourth); on the fall-back
// paths the frame comes back unchanged, all channels.  out_stride >= max(w, ow) * cn, and d_out holds max(h, oh) rows.  A BGR8 result is
// that of vs_azc_apply_dev on the same frame.  Colour frames, NV12, P010 and planar surfaces may alternate on one object.
// Refused before any device call, with a text in vs_azc_last_error that names the call and the formats: another fmt, stride < w * cn,
// out_stride too small, null pointers, w or h < 1, n < 1.
static int azc_rgb_hand_over(vs_azc* a, const char* call, int fmt, const void* d_frame, int w, int h, size_t stride, void* d_out, size_t out_stride,
                             int64_t* ticket) {
    const PixFmt* f = pixfmt(fmt);
    const std::string head = std::string(call) + " (fmt: one of " + RGB_FORMATS + "): ";
    if (!f || f->kind != PIX_INTERLEAVED || f->cn < 3) return vs_obj_fail(a, VS_ERR_INVALID_ARG, head + "not an interleaved colour format");
    if (!d_frame || !d_out) return vs_obj_fail(a, VS_ERR_INVALID_ARG, head + "null frame or result pointer");
    if (w < 1 || h < 1) return vs_obj_fail(a, VS_ERR_INVALID_ARG, head + "w and h must be at least 1");
    const int ow = a->ow ? a->ow : w;
    if (stride < (size_t)w * f->cn || out_stride < (size_t)std::max(w, ow) * f->cn)
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, head + "stride below w * cn, or out_stride below max(w, " + std::to_string(ow) + ") * cn");
    if (stride > UINT32_MAX || out_stride > UINT32_MAX) return vs_obj_fail(a, VS_ERR_INVALID_ARG, head + "strides must be below 4 GiB");
    return azc_hand_over(a, azc_frame(*f, w, h, d_frame, d_out, planes(*f, w, h, stride), planes(*f, azc_max_w(a, w), azc_max_h(a, h), out_stride)), ticket);
}

int vs_azc_apply_rgb_dev(vs_azc* a, int fmt, const void* d_frame, int w, int h, size_t stride, void* d_out, size_t out_stride, int64_t* ticket) {
    if (!a) return VS_ERR_INVALID_ARG;
    return azc_rgb_hand_over(a, "vs_azc_apply_rgb_dev", fmt, d_frame, w, h, stride, d_out, out_stride, ticket);
}

int vs_azc_apply_rgb_dev_n(vs_azc* a, int fmt, const void* const* d_frames, void* const* d_outs, int n, int w, int h, size_t stride, size_t out_stride,
                           int64_t* tickets) {
    if (!a) return VS_ERR_INVALID_ARG;
    if (!d_frames || !d_outs || n < 1)
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, std::string("vs_azc_apply_rgb_dev_n (fmt: one of ") + RGB_FORMATS + "): null pointer lists, or n < 1");
    return each_surface(n, [&](int i) {
        return azc_rgb_hand_over(a, "vs_azc_apply_rgb_dev_n", fmt, d_frames[i], w, h, stride, d_outs[i], out_stride, tickets ? tickets + i : nullptr);
    });
}

// Diagnostics of the asynchronous path: frames through the workers so far and the seconds the workers spent, summed over the
// threads, without a frame / waiting for the masks on their way / in the contour logic / queueing launches and publishing; then
// batches and, summed over them, the seconds from launches to masks, from masks to the crop launch, and the caller's waits for a slot.
int vs_azc_worker_times(vs_azc* a, double* out5) {      // (nine values: include/vs_stab.h)
    if (!a || !out5) return VS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(a->mu);
    for (int i = 0; i < 5; i++) out5[i] = a->wt[i];
    for (int i = 0; i < 4; i++) out5[5 + i] = a->bt[i];
    return VS_OK;
}

// What ticket's frame became: waits for its host part (not for the pixels: vs_azc_sync).
int vs_azc_result(vs_azc* a, int64_t ticket, int* out_w, int* out_h, int32_t* info8) {
    if (!a || ticket < 0) return VS_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(a->mu);
    if (ticket >= a->issued || ticket + vs_azc::NRES <= a->issued) return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: no such ticket (results of the last 1024 frames are kept)");
    if (!a->pending.empty() && ticket >= a->pending[0].ticket) {       // (still waiting for its batch to fill)
        const int frc = azc_flush_pending(a, lk);
        if (frc != VS_OK) return frc;
    }
    a->cv_done.wait(lk, [&] { return a->results[ticket % vs_azc::NRES].ticket == ticket; });
    const vs_azc::Result& r = a->results[ticket % vs_azc::NRES];
    if (out_w) *out_w = r.out_w;
    if (out_h) *out_h = r.out_h;
    if (info8) memcpy(info8, r.info, sizeof r.info);
    if (r.rc != VS_OK) return vs_obj_fail(a, r.rc, "auto zoom/crop: a worker's launch failed");
    return VS_OK;
}

// The output size of the crop-and-scale (the reference's 640 x 360, :246-261, as a setting of the object): both even and in 2 .. 8192,
// or 0, 0 = the size of the surface handed over.  It applies to what is handed over after the call: like a change of geometry it closes
// the pending batch, and the tickets out already keep the size they were issued under (vs_azc::Frame carries it).
int vs_azc_set_output_size(vs_azc* a, int out_w, int out_h) {
    if (!a) return VS_ERR_INVALID_ARG;
    const bool own = out_w == 0 && out_h == 0;
    if (!own && (out_w < 2 || out_h < 2 || out_w > 8192 || out_h > 8192 || (out_w & 1) || (out_h & 1)))
        return vs_obj_fail(a, VS_ERR_INVALID_ARG, "auto zoom/crop: the output size must be even and in 2 .. 8192 both ways, or 0 x 0 (the surface's own size)");
    std::unique_lock<std::mutex> lk(a->mu);
    int rc = VS_OK;
    if (!a->pending.empty() && (a->ow != out_w || a->oh != out_h)) {
        if (hipSetDevice(a->device) != hipSuccess) return vs_obj_fail(a, VS_ERR_HIP, "auto zoom/crop: cannot select the device");
        rc = azc_flush_pending(a, lk);
    }
    a->ow = out_w; a->oh = out_h;
    return rc;
}

int vs_azc_get_output_size(const vs_azc* a, int* out_w, int* out_h) {
    if (!a || !out_w || !out_h) return VS_ERR_INVALID_ARG;
    *out_w = a->ow; *out_h = a->oh;
    return VS_OK;
}

// The stage's crop-and-scale as an operator: the call the batch's last worker makes (launch_scale_jobs), on the caller's jobs.
// (rgb: the jobs of vs_op_scale_jobs_rgb - cn 3 or 4 where the others take 1 or 2)
static int scale_jobs_convert(const vs_scale_job* jobs, int n, int sample_bytes, WarpJob* out, bool rgb = false) {
    if (!jobs || n < 1 || n > WARP_JOBS_MAX || (sample_bytes != 1 && sample_bytes != 2)) return VS_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        const vs_scale_job& s = jobs[i];
        if (!s.src || !s.dst || s.sw < 1 || s.sh < 1 || s.dw < 1 || s.dh < 1 || s.sw > 32767 || s.sh > 32767 || s.dw > 32767 || s.dh > 32767 ||
            (rgb ? s.cn != 3 && s.cn != 4 : s.cn != 1 && s.cn != 2) || s.reserved != 0 || s.src_stride > UINT32_MAX || s.dst_stride > UINT32_MAX ||
            s.src_stride < (size_t)s.sw * s.cn * sample_bytes || s.dst_stride < (size_t)s.dw * s.cn * sample_bytes ||
            (sample_bytes == 2 && (((uintptr_t)s.src | (uintptr_t)s.dst | s.src_stride | s.dst_stride) & 1)))
            return VS_ERR_INVALID_ARG;
        WarpJob& j = out[i];
        j.src = (const uint8_t*)s.src; j.dst = (uint8_t*)s.dst;
        j.sstride = (uint32_t)s.src_stride; j.dstride = (uint32_t)s.dst_stride;
        j.sw = s.sw; j.sh = s.sh; j.dw = s.dw; j.dh = s.dh; j.cn = s.cn; j.border = VS_BORDER_BLACK; j.sb = sample_bytes;
        const float M[6] = {(float)((double)s.dw / s.sw), 0.f, 0.f, 0.f, (float)((double)s.dh / s.sh), 0.f};      // :261-262
        warp_invert(M, j.m);
    }
    return VS_OK;
}

int vs_op_scale_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int path, void* stream) {
    WarpJob wj[WARP_JOBS_MAX];
    if ((path != 0 && path != 1) || scale_jobs_convert(jobs, n, sample_bytes, wj) != VS_OK) {
        set_last_error("scale_jobs: invalid argument (1 .. 24 jobs of one sample size, 1 or 2 bytes; cn 1 or 2; sizes 1 .. 32767; 16-bit pointers and strides even)");
        return VS_ERR_INVALID_ARG;
    }
    VS_TRY(ensure_device());
    return launch_scale_jobs(wj, n, path, (hipStream_t)stream);
}

int vs_op_scale_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int32_t* staged) {
    WarpJob wj[WARP_JOBS_MAX];
    if (!staged || scale_jobs_convert(jobs, n, sample_bytes, wj) != VS_OK) {
        set_last_error("scale_jobs_plan: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; i++) staged[i] = scale_job_staged(wj[i]) ? 1 : 0;
    return VS_OK;
}

// The same operator for crops of interleaved colour frames: 8-bit samples, cn 3 or 4 (a call may mix them), every channel - a fourth one
// included - a channel of its own.  (vs_op_scale_jobs keeps refusing them: its jobs are planes of YUV surfaces.)
int vs_op_scale_jobs_rgb(const vs_scale_job* jobs, int n, int path, void* stream) {
    WarpJob wj[WARP_JOBS_MAX];
    if ((path != 0 && path != 1) || scale_jobs_convert(jobs, n, 1, wj, true) != VS_OK) {
        set_last_error("scale_jobs_rgb: invalid argument (1 .. 24 jobs of 8-bit samples; cn 3 or 4; sizes 1 .. 32767; strides at least a row)");
        return VS_ERR_INVALID_ARG;
    }
    VS_TRY(ensure_device());
    return launch_scale_jobs_rgb(wj, n, path, (hipStream_t)stream);
}

int vs_op_scale_jobs_rgb_plan(const vs_scale_job* jobs, int n, int32_t* staged) {
    WarpJob wj[WARP_JOBS_MAX];
    if (!staged || scale_jobs_convert(jobs, n, 1, wj, true) != VS_OK) {
        set_last_error("scale_jobs_rgb_plan: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; i++) staged[i] = scale_job_staged_rgb(wj[i]) ? 1 : 0;
    return VS_OK;
}

}  // extern "C"
