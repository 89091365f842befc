// What the batched plane-job operators on YUV surfaces share: k_cropzoom.hip (vs_op_resize_jobs), k_yuvpad.hip (vs_op_pad_jobs) and
// k_yuvfade.hip (vs_op_fade_blend_jobs, vs_op_fade_update_jobs); k_resize.hip (vs_op_resample_jobs) uses the sequence, the bisection,
// the split and pj_launch, once per path class, with a lane shape of its own like the zoom.
//
// The scheme.  One launch takes up to a limit of jobs (one plane each) of one sample size, cn 1 and 2 mixed.  It is a flat sequence of
// (job, tile row, tile column) tiles in the XCD-aware order of the warp kernels: workgroup `lin` takes tile xcd_seq(lin, tiles)
// (vs_common.h), XCD c = lin mod 8 the c-th contiguous eighth of the sequence, so that tiles that share lines meet in one L2.  The jobs travel as
// kernel arguments, each with its first tile in the sequence; a workgroup finds its job by bisection over them (scalar loads,
// pj_find) and its tile column and row from the job's row bytes (pj_split).  The job records, their size and their 24-bit tile
// budget are each file's own.
//
// The pad and the fade give a lane PJ_LB = 16 bytes at one place of R rows, a wave being cl lanes side by side times 64 / cl rows
// (PjLane; pj_tb / pj_tr: the tile): 16-byte loads and stores where a lane's bytes are inside the row and aligned - or, for a
// load, at any address (pj_q1) - else sample by sample (pj_gather / pj_scatter).  The zoom has another lane shape and shares only
// the sequence, the bisection, the split and the host side.
//
// The host side: every operator checks the launch and then every job before any device call (pj_launch; the sentences of the
// refusals that more than one operator gives), and counts a job's tiles with pj_tiles.
#ifndef VS_PLANE_JOBS_H
#define VS_PLANE_JOBS_H

#include <initializer_list>
#include <type_traits>

#include "launchers.h"
#include "vs_common.h"

namespace vsd {

constexpr int PJ_LB = 16;                                                         // bytes per lane and row
constexpr int pj_tb(int cl) { return cl * PJ_LB; }                                // tile: bytes ...
constexpr int pj_tr(int waves, int r, int cl) { return waves * r * (64 / cl); }   // ... and rows

// The job of tile seq: the last of a.j[0 .. a.n - 1] whose first tile is not behind it
template <class Args, class First>
__device__ __forceinline__ uint32_t pj_find(const Args& a, uint32_t seq, First first_tile) {
    uint32_t jl = 0, jh = a.n - 1;
    while (jl < jh) {
        const uint32_t mid = (jl + jh + 1) >> 1;
        if (first_tile(a.j[mid]) <= seq) jl = mid;
        else jh = mid - 1;
    }
    return jl;
}

// Tile t of a job whose rows have row_bytes bytes, in tiles tb bytes wide
struct PjTile { int tx, ty; };
__device__ __forceinline__ PjTile pj_split(uint32_t t, uint32_t row_bytes, int tb) {
    const uint32_t gx = (row_bytes + tb - 1) / tb;
    const int ty = (int)(t / gx);
    return {(int)(t - (uint32_t)ty * gx), ty};
}

template <int SB>
__device__ __forceinline__ uint32_t pj_ld(const uint8_t* p) {
    if constexpr (SB == 1) return *p;
    else return *reinterpret_cast<const uint16_t*>(p);
}

typedef uint32_t pj_u4 __attribute__((ext_vector_type(4)));                    // 16 aligned bytes
struct __attribute__((packed, aligned(1))) pj_q1 { uint32_t x, y, z, w; };    // 16 bytes at any address: ONE global_load_dwordx4 (gfx9 global loads take unaligned addresses)

template <class Q>
__device__ __forceinline__ void pj_load16(const uint8_t* p, uint32_t (&o)[4]) {
    const Q q = *reinterpret_cast<const Q*>(p);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
}
__device__ __forceinline__ pj_u4 pj_pack16(const uint32_t (&o)[4]) {
    pj_u4 q;
    q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
    return q;
}

// the first nvb bytes at p, sample by sample (the rest 0)
template <int SB>
__device__ __forceinline__ void pj_gather(const uint8_t* p, int nvb, uint32_t (&o)[4]) {
    constexpr int NEL = PJ_LB / SB, SPD = 4 / SB;
    o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
    for (int i = 0; i < NEL; i++)
        if (i * SB < nvb) o[i / SPD] |= pj_ld<SB>(p + i * SB) << (8 * SB * (i % SPD));
}

template <int SB>
__device__ __forceinline__ void pj_scatter(uint8_t* p, int nvb, const uint32_t (&o)[4]) {
    constexpr int NEL = PJ_LB / SB, SPD = 4 / SB;
#pragma unroll
    for (int i = 0; i < NEL; i++) {
        if (i * SB < nvb) {
            const uint32_t v = o[i / SPD] >> (8 * SB * (i % SPD));
            if constexpr (SB == 1) p[i] = (uint8_t)v;
            else reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)v;
        }
    }
}

// the fill of a lane's 16 bytes, a dword of it (packed: fills[0] | fills[1] << 16, as the job records hold it)
template <int SB, int CN>
__device__ __forceinline__ uint32_t pj_fill_dword(const uint32_t (&fills)[2], uint32_t packed) {
    if constexpr (SB == 1 && CN == 1) return fills[0] * 0x01010101u;
    else if constexpr (SB == 1) return (fills[0] | fills[1] << 8) * 0x00010001u;
    else if constexpr (CN == 1) return fills[0] * 0x00010001u;
    else return packed;
}

// A lane's 16 bytes in a row of w pixels of PB bytes, CL lanes side by side.  (e0 stands in front of the row's bytes, and px0 and
// full() are evaluated where they are used, because the order decides what the compiler hoists out of the cn 1 / cn 2 branches.)
struct PjLane {
    int e0;                                   // its first byte in the row
    int nvb;                                  // its bytes inside the row (a multiple of a pixel's; <= 0: the lane has nothing to do)
    __device__ __forceinline__ int px0(int pb) const { return e0 / pb; }       // its first pixel, pixels of pb bytes
    __device__ __forceinline__ bool full() const { return nvb == PJ_LB; }
};
template <int CL, int PB>
__device__ __forceinline__ PjLane pj_lane(int tx, int lane, int w) {
    const int e0 = (tx * CL + lane) * PJ_LB;
    return {e0, min(PJ_LB, w * PB - e0)};
}

// ---- host ----------------------------------------------------------------------------------------------------------------
inline uint64_t pj_tiles(size_t row_bytes, int rows, int tb, int tr) { return (uint64_t)((row_bytes + tb - 1) / tb) * (uint64_t)((rows + tr - 1) / tr); }
inline uintptr_t pj_end(const void* p, size_t stride, int rows, size_t row) { return (uintptr_t)p + (size_t)(rows - 1) * stride + row; }
inline bool pj_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// The sentences of the refusals; nullptr = nothing to refuse.
inline const char* pj_bad_sizes(std::initializer_list<int> sizes) {
    for (int v : sizes)
        if (v < 1 || v > 32767) return "sizes must be 1 .. 32767";
    return nullptr;
}
inline const char* pj_bad_padded_sizes(int sw, int sh, int bx, int by) {
    if (sw < 1 || sh < 1 || bx < 0 || by < 0 || bx > 32767 || by > 32767 || (int64_t)sw + 2 * (int64_t)bx > 32767 || (int64_t)sh + 2 * (int64_t)by > 32767)
        return "sizes must be at least 1, borders at least 0 and padded sizes at most 32767";
    return nullptr;
}
inline const char* pj_bad_cn(int cn, int64_t reserved) { return (cn != 1 && cn != 2) || reserved != 0 ? "cn must be 1 or 2 and reserved 0" : nullptr; }
inline const char* pj_bad_fill(const uint16_t (&fill)[2], int sample_bytes) {
    return sample_bytes == 1 && (fill[0] > 255 || fill[1] > 255) ? "a fill sample above 255 for 8-bit samples" : nullptr;
}
struct PjPitch { size_t stride, row; };
inline const char* pj_bad_strides(std::initializer_list<PjPitch> planes) {
    for (const PjPitch& p : planes)
        if (p.stride > UINT32_MAX || p.stride < p.row) return "a stride does not hold a row (or exceeds 32 bits)";
    return nullptr;
}
// bits: the pointers and strides of a job, ORed
inline const char* pj_bad_parity(int sample_bytes, uintptr_t bits) { return sample_bytes == 2 && (bits & 1) ? "16-bit pointers and strides must be even" : nullptr; }

// What every launcher refuses about the launch itself
inline bool pj_launch_ok(const void* jobs, int n, int limit, int sample_bytes) { return jobs && n >= 1 && n <= limit && (sample_bytes == 1 || sample_bytes == 2); }

// The launcher of operator `name`.  refuse(job, sample_bytes, &rc) -> the refusal's text or nullptr (rc: VS_ERR_INVALID_ARG unless
// it sets another); pack(job, record, first tile) fills the kernel's record of the job and returns the job's tiles;
// launch(integral_constant<int, sample_bytes>, args, tiles) launches.  Every job is checked before any device call.
template <class Args, class Job, class Refuse, class Pack, class Launch>
int pj_launch(const char* name, const Job* jobs, int n, int limit, int sample_bytes, Args& a, Refuse refuse, Pack pack, Launch launch) {
    if (!pj_launch_ok(jobs, n, limit, sample_bytes)) {
        set_last_error(std::string(name) + ": invalid argument (1 .. " + std::to_string(limit) + " jobs of one sample size, 1 or 2 bytes)");
        return VS_ERR_INVALID_ARG;
    }
    uint64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        int rc = VS_ERR_INVALID_ARG;
        if (const char* why = refuse(jobs[i], sample_bytes, &rc)) {
            set_last_error(std::string(name) + ": job " + std::to_string(i) + ": " + why);
            return rc;
        }
        tiles += pack(jobs[i], a.j[i], (uint32_t)tiles);
    }
    a.n = (uint32_t)n; a.tiles = (uint32_t)tiles;
    VS_TRY(ensure_device());
    if (sample_bytes == 1) launch(std::integral_constant<int, 1>(), a, (unsigned)tiles);
    else launch(std::integral_constant<int, 2>(), a, (unsigned)tiles);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

}  // namespace vsd
#endif
