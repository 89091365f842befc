// Pyramidal Lucas-Kanade tracker for gfx950: device counterpart of
//   cv::calcOpticalFlowPyrLK(prevGray, currGray, prevPts, nextPts, status, err,
//                            Size(win,win), maxLevel, TermCriteria(COUNT+EPS, iters, eps))
// as called at /root/reference/src/Stabilizer.cpp:611-619 (15x15, maxLevel 2,
// 20 iterations, eps 0.03; Stabilizer_legacy.cpp:218-224 uses 21x21).
//
// One wavefront (64 lanes) owns one feature point for ALL pyramid levels
// (coarse to fine), so the whole tracker is a single launch: points are
// independent, levels of one point are sequential.  The win*win window is
// spread over the lanes (ceil(win^2/64) pixels per lane, kept in registers as
// int16 I / dIx / dIy; every sample of the iteration comes from a search region staged in LDS, which
// is staged again around the point if it walks out of it); the 2x2 normal-equation sums (A11,A12,A22 and per
// iteration b1,b2) are exact integer wave reductions, so the float solve that
// follows is bit-identical to the oracle's.  Bound by instruction issue
// (SURVEY.md 8a L1): images are <= 0.5 MB and stay in L2.
//
// Staging: a template patch (PP bytes a row, PP a multiple of 4) and a search region (RW bytes a row) that lie inside the
// level image are loaded as unaligned dwords - PP / 4 and RD = ceil(RW / 4) a row, lane-strided, all in flight before the
// first LDS store - and stored at byte 4 i of their array (the region's LDS row pitch is 4 RD).  Whatever touches a border,
// and a region whose last dword column would leave its row, is staged byte by byte with REFLECT_101.
// Wave sums: the first butterfly steps in 32 bits (bound at wave_sum), then exact on 64-bit pairs.
#include "vs_common.h"

namespace vsd {
namespace {

constexpr int MAX_LEVELS = 8;

struct LKArgs {
    LKLevel levels[MAX_LEVELS];
    int max_level;
    const float* prev_pts;
    float* next_pts;
    uint8_t* status;
    float* err;
    int n;
    const int32_t* d_n;
    int win;
    int max_count;
    double eps2;
};

// ---- exact wave-wide integer sums without LDS traffic -----------------------
// Butterfly inside each 16-lane row with DPP (xor 1, xor 2, half-mirror, mirror),
// then the group totals are read with v_readlane and added on the scalar unit.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
// 64-bit step: the partner's (lo,hi) pair is fetched with two DPP moves and added
// with a normal 64-bit add.  Per-lane partial sums fit int32; the wave total may not.
template <int CTRL>
__device__ __forceinline__ long long dpp_mov64(long long v) {
    const int lo = dpp_mov<CTRL>((int)(unsigned)(unsigned long long)v);
    const int hi = dpp_mov<CTRL>((int)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// The first S butterfly steps run in 32 bits (one v_add_u32 with a DPP operand each).  Bound: a staged intensity is a byte,
// so |diff| <= 8160 (Iw and the sample are descale(.., 9) of weights that sum to 2^14) and |Ix|, |Iy| <= 4081 (descale(.., 14)
// of Scharr taps within +-4080); a lane's partial over NPX pixels is at most NPX * 8160 * 4081 in magnitude, and the total of
// 2^S lanes stays below 2^31 - 1 for S = 4 (NPX = 4), 3 (NPX = 7) and 2 (NPX = 16).  The sum is widened once after that and
// finished exactly: the remaining row steps run on 64-bit pairs as before, then the four row totals are read with v_readlane
// and added on the scalar unit.  (Reading the 64 >> S group totals right after the 32-bit steps and adding them sign-extended
// on the scalar unit has fewer vector but more instructions in all, and measured 3 us slower for 21 x 21: DESIGN 8, round 19.)
constexpr long long LK_LANE_TERM_MAX = 8160ll * 4081ll;
template <int NPX> struct WaveSumSteps {
    static constexpr int S = NPX <= 4 ? 4 : (NPX <= 7 ? 3 : 2);
    static_assert(NPX <= 16 && (long long)NPX * LK_LANE_TERM_MAX * (1 << S) <= 2147483647ll, "the 32-bit butterfly steps must not overflow");
};
template <int S>
__device__ __forceinline__ long long wave_sum(int p) {
    static_assert(S >= 2 && S <= 4, "");
    unsigned u = (unsigned)p;
    u += (unsigned)dpp_mov<0xB1>((int)u);                  // quad_perm [1,0,3,2]
    u += (unsigned)dpp_mov<0x4E>((int)u);                  // quad_perm [2,3,0,1]
    if (S >= 3) u += (unsigned)dpp_mov<0x141>((int)u);     // row_half_mirror
    if (S >= 4) u += (unsigned)dpp_mov<0x140>((int)u);     // row_mirror
    if (S >= 4) {                                          // the row totals are 32-bit: sign-extended on the scalar unit
        long long t = 0;
#pragma unroll
        for (int r = 0; r < 64; r += 16) t += (long long)__builtin_amdgcn_readlane((int)u, r);
        return t;
    }
    long long v = (int)u;
    if (S < 3) v += dpp_mov64<0x141>(v);
    v += dpp_mov64<0x140>(v);
    const int lo = (int)(unsigned)(unsigned long long)v, hi = (int)((unsigned long long)v >> 32);
    long long t = 0;
#pragma unroll
    for (int r = 0; r < 64; r += 16) {
        const unsigned l = (unsigned)__builtin_amdgcn_readlane(lo, r);
        const unsigned h = (unsigned)__builtin_amdgcn_readlane(hi, r);
        t += (long long)(((unsigned long long)h << 32) | l);
    }
    return t;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

struct Weights { int w00, w01, w10, w11; };

__device__ __forceinline__ Weights make_weights(float a, float b) {
    Weights w;
    w.w00 = f_round((1.f - a) * (1.f - b) * 16384.f);
    w.w01 = f_round(a * (1.f - b) * 16384.f);
    w.w10 = f_round((1.f - a) * b * 16384.f);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// A pointer every lane of the wave holds the same value of, as a global-memory pointer in scalar registers.
typedef const __attribute__((address_space(1))) uint8_t* gmem_u8;
__device__ __forceinline__ gmem_u8 uniform_global(const uint8_t* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (gmem_u8)(((unsigned long long)hi << 32) | lo);
}

// A dword at any byte address of global memory (gfx950 code objects assume unaligned access: one global_load_dword).
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
typedef const __attribute__((address_space(1))) u32_unaligned* gmem_u32u;

constexpr int LK_MARGIN = 6;                       // search region = window + 1 + 2*margin
constexpr int LK_WIN_MAX = 31;



// i / d and i % d for 0 <= i < 4096, 1 <= d <= 64 (exact: the float product is
// off by < 1e-3 from the true quotient and we add 0.5/d of slack)
__device__ __forceinline__ void divmod_small(int i, int d, float inv_d, int& q, int& r) {
    q = (int)(((float)i + 0.5f) * inv_d);
    r = i - q * d;
}

template <int NPX>
__device__ __forceinline__ void lk_track(const LKArgs& a, const int pt) {
    // Per level everything the wave will touch is staged into LDS with ONE round of global loads: the template patch of
    // the previous image with a one-pixel rim, and the search region of the next image (pyramid padding already applied).
    // The patch's Scharr derivatives are then computed in LDS from the staged bytes (the pyramid writes no derivative
    // images: at 960 x 540 they were 2.7 MB per frame of HBM writes, read back here at 4 bytes per patch pixel).
    // sized by the window class of the instantiation (NPX pixels per lane: windows up to 16 / 21 / 31): with the
    // arrays of the largest class a 21x21 tracker held 7 KB, 22 waves fitted a CU and the 6400 points of a
    // 32-frame batch took two rounds on 5632 slots; 3.6 KB leaves the wave limit (32 per CU) as the only one
    constexpr int WM = NPX <= 4 ? 16 : (NPX <= 7 ? 21 : LK_WIN_MAX);
    constexpr int PWM = WM + 1, RWM = WM + 1 + 2 * LK_MARGIN;
    // The staged patch holds rows and columns -1 .. PW of the template patch at a row pitch PP = PW + 2 rounded up to whole
    // dwords (the derivative pass reads it as dwords).  The derivatives are stored at the same index as the pixel they belong
    // to, so that one offset per window pixel serves both arrays.  A lane of the derivative pass takes DR rows x 4 columns,
    // sized so that one round of the wave covers the patch.
    constexpr int DR = NPX <= 7 ? 3 : 5;
    constexpr int PPM = (PWM + 2 + 3) & ~3;
    constexpr int SRM = (PWM + 1 + 3) / 4, NGM = (PWM + DR - 1) / DR;       // column strips, row groups
    static_assert(SRM * NGM <= 64, "one derivative round per level");
    // elements per lane of the lane-strided staging walks; the arrays are padded to whole rounds of 64 so that the stores of a
    // round need no bounds check (the padding is never read).  The patch array also holds what the derivative pass reads
    // beside the staged bytes (results that are not stored or never read): the dword in front of row 0, the rows past the
    // last staged one up to the end of the last row group, and the dword past that.
    // The interior walks move dwords: PPM / 4 per patch row, RDM = ceil(RWM / 4) per region row; the region's row pitch in
    // LDS is 4 * RD bytes, so that in both arrays element i of a walk lands at byte 4 * i.
    constexpr int RDM = (RWM + 3) / 4;
    constexpr int PN = ((PPM / 4) * (PWM + 2) + 63) / 64, RN = (RDM * RWM + 63) / 64;
    constexpr int PBYTES = (PN * 256 > PPM * (NGM * DR + 2) + 4 ? PN * 256 : PPM * (NGM * DR + 2) + 4);
    static_assert((WM - 1) * 4 * RDM + (WM - 1) < 65536 && (WM + 1) * PPM < 65536, "packed window offsets are 16 bits each");
    constexpr int WS = WaveSumSteps<NPX>::S;
    __shared__ __attribute__((aligned(16))) uint8_t pI_[4 + PBYTES];
    uint8_t* const pI = pI_ + 4;
    __shared__ __attribute__((aligned(16))) short2 pD[(PWM + 1) * PPM];
    __shared__ __attribute__((aligned(16))) uint8_t region[RN * 256];
    const int lane = threadIdx.x;
    int n = a.n;
    if (a.d_n) { int dn = *a.d_n; n = dn < n ? dn : n; }
    if (pt >= n) return;
    const int win = a.win, area = win * win;
    const int PW = win + 1, PP = (PW + 2 + 3) & ~3;
    const int RW = win + 1 + 2 * LK_MARGIN;
    const int PD = PP >> 2, RD = (RW + 3) >> 2, RP = 4 * RD;    // dwords per staged row; the region's row pitch
    const float inv_pp = 1.0f / (float)PP, inv_rw = 1.0f / (float)RW, inv_win = 1.0f / (float)win;
    // per window pixel of this lane: offsets into the staged patch and its derivatives (low half) and the search region
    // (high half); kept packed, and the (x, y) of a pixel is recomputed where the rare
    // out-of-region path needs it: the register budget decides how many points a SIMD tracks at once
    uint32_t off[NPX];
#pragma unroll
    for (int k = 0; k < NPX; k++) {
        const int p = lane + 64 * k;
        int yy = 0, xx = 0;
        if (p < area) divmod_small(p, win, inv_win, yy, xx);
        off[k] = (uint32_t)((yy + 1) * PP + xx + 1) | ((uint32_t)(yy * RP + xx) << 16);
    }
#define LK_VALID(k) (lane + 64 * (k) < area)
#define LK_POFF(k) ((int)(off[k] & 0xFFFFu))
#define LK_ROFF(k) ((int)(off[k] >> 16))
    // lane-strided dword walks over the PD x (PW + 2) patch and the RD x RW region: start and step
    int p_y0, p_x0, p_sy, p_sx, r_y0, r_x0, r_sy, r_sx;
    divmod_small(lane, PD, 1.0f / (float)PD, p_y0, p_x0);
    divmod_small(64, PD, 1.0f / (float)PD, p_sy, p_sx);
    divmod_small(lane, RD, 1.0f / (float)RD, r_y0, r_x0);
    divmod_small(64, RD, 1.0f / (float)RD, r_sy, r_sx);
    const float halfWin = (win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    const float px0 = a.prev_pts[2 * pt], py0 = a.prev_pts[2 * pt + 1];
    float outx = 0.f, outy = 0.f;  // nextPts[pt]
    int status = 1;
    float err = 0.f;

    for (int level = a.max_level; level >= 0; level--) {
        const LKLevel L = a.levels[level];
        const float scale = (float)(1. / (double)(1 << level));
        float prevx = px0 * scale, prevy = py0 * scale;
        if (level == a.max_level) { outx = prevx; outy = prevy; }
        else { outx = outx * 2.f; outy = outy * 2.f; }
        prevx -= halfWin; prevy -= halfWin;
        const int ipx = f_floor(prevx), ipy = f_floor(prevy);
        if (ipx < -win || ipx >= L.w || ipy < -win || ipy >= L.h) {
            if (level == 0) { status = 0; err = 0.f; }
            continue;
        }
        float cx = outx - halfWin, cy = outy - halfWin;
        int rx0 = f_floor(cx) - LK_MARGIN, ry0 = f_floor(cy) - LK_MARGIN;
        // ---- stage (all loads of the level are in flight together).  Lane-strided element
        // walk with incremental (row, col); patches that lie inside the image (the common
        // case) skip the border arithmetic.
        __syncthreads();
        // Patches and regions that lie inside the image (the common case) are staged by straight-line code: every load of the
        // level goes out before the first LDS store waits for one (elements past the end of a walk repeat element 0 and land in
        // the arrays' padding).  Written as loops over a run-time count the compiler had turned each walk into load - wait -
        // store per element: 26 dependent round trips per level and point, two thirds of the tracker's time
        // (SQ_WAIT_ANY 68 % of its wave cycles, profiles/r03_c_configs1_pmc.txt).
        // (Batches of at most ten loads: the values and offsets of a batch are all that is live, 128 registers - four waves per
        // SIMD - hold without spills; three to four round trips per level instead of 26.)
        // No load may touch a byte outside [0, w) of a row < h.  Patch: the condition below puts rows ipy - 1 .. ipy + PW and
        // bytes ipx - 1 .. ipx - 2 + PP of each inside the image, and the PD dwords of a row are exactly those PP bytes.
        // Region: rows ry0 .. ry0 + RW - 1 and bytes rx0 .. rx0 + 4 RD - 1, which the dword test of stage_region() demands.
        const int pcount = PP * (PW + 2);
        if (ipx >= 1 && ipy >= 1 && ipx - 1 + PP <= L.w && ipy + PW + 1 <= L.h) {
            // (the wave tracks ONE point: base in scalar registers, global - not flat - loads with a 32-bit lane offset)
            const gmem_u8 pbase = uniform_global(L.prev + ((size_t)(ipy - 1) * L.stride + (ipx - 1)));
            uint32_t vI[PN];
            int y = p_y0, x = p_x0;
#pragma unroll
            for (int k = 0; k < PN; k++) {
                const bool ok = lane + 64 * k < (pcount >> 2);
                vI[k] = *(gmem_u32u)(pbase + (ok ? (uint32_t)(y * (int)L.stride + 4 * x) : 0u));
                x += p_sx; y += p_sy;
                if (x >= PD) { x -= PD; y++; }
            }
#pragma unroll
            for (int k = 0; k < PN; k++) reinterpret_cast<uint32_t*>(pI)[lane + 64 * k] = vI[k];
            __builtin_amdgcn_sched_barrier(0);
        } else {                               // REFLECT_101 intensities; the derivative pass masks what lies outside
            for (int i = lane; i < pcount; i += 64) {
                int y, x;
                divmod_small(i, PP, inv_pp, y, x);
                const int X = ipx - 1 + x, Y = ipy - 1 + y;
                pI[i] = L.prev[(size_t)reflect101(Y, L.h) * L.stride + reflect101(X, L.w)];
            }
        }
        // the search region of the next image around (rx0, ry0); staged again, re-centred, if the point walks out
        // of it (more than LK_MARGIN pixels at one level), so every sample of the iteration comes from LDS
        auto stage_region = [&]() {
            // (a region whose last one to three dword columns would leave the row takes the byte walk below)
            const bool inside = rx0 >= 0 && ry0 >= 0 && rx0 + RP <= L.w && ry0 + RW <= L.h;
            int y = r_y0, x = r_x0;
            asm volatile("" : "+v"(x), "+v"(y));       // (the offsets of the walk are recomputed at every call: hoisted out of the iteration loop they cost 40 registers)
            if (inside) {
                const gmem_u8 rbase = uniform_global(L.next + ((size_t)ry0 * L.stride + rx0));
                uint32_t vR[RN];
#pragma unroll
                for (int k = 0; k < RN; k++) {
                    const bool ok = lane + 64 * k < RD * RW;
                    vR[k] = *(gmem_u32u)(rbase + (ok ? (uint32_t)(y * (int)L.stride + 4 * x) : 0u));
                    x += r_sx; y += r_sy;
                    if (x >= RD) { x -= RD; y++; }
                }
#pragma unroll
                for (int k = 0; k < RN; k++) reinterpret_cast<uint32_t*>(region)[lane + 64 * k] = vR[k];
                __builtin_amdgcn_sched_barrier(0);
            } else {                           // a region that leaves the image: element by element, reflected
                for (int i = lane; i < RW * RW; i += 64) {
                    divmod_small(i, RW, inv_rw, y, x);
                    const int X = rx0 + x, Y = ry0 + y;
                    region[y * RP + x] = L.next[(size_t)reflect101(Y, L.h) * L.stride + reflect101(X, L.w)];
                }
            }
        };
        stage_region();
        __syncthreads();
        // ---- Scharr derivatives of the patch (scharr_kernel's stencil and border rule: the staged rim is the REFLECT_101 of
        // the image), 0 at positions outside the level image (cv::calcOpticalFlowPyrLK pads the derivative image with
        // BORDER_CONSTANT).  Staged columns 4 c .. 4 c + 3 of rows y .. y + DR - 1 per lane: three dwords per staged row (the
        // byte left of the group, the group, the byte right of it), a rolling window of three rows (one output row at a time
        // keeps the pass inside the tracker's register budget), one 16-byte store per output row.
        {
            const int sr = (PW + 1 + 3) >> 2;
            int g, c;
            divmod_small(lane, sr, 1.0f / (float)sr, g, c);
            const int y = 1 + g * DR, x = 4 * c;
            if (y <= PW) {
                // staged pixels (x .. x + 3, y + r) are inside the level image: all of them when the patch is
                const bool masked = !(ipx >= 0 && ipy >= 0 && ipx + PW <= L.w && ipy + PW <= L.h);
                int t[3][6];                                            // staged columns x - 1 .. x + 4
                auto load_row = [&](int j, int* tj) {
                    const uint32_t* q = reinterpret_cast<const uint32_t*>(pI + j * PP) + c;
                    const uint32_t lo = q[-1], mid = q[0], hi = q[1];
                    tj[0] = lo >> 24;
                    tj[1] = mid & 255u; tj[2] = (mid >> 8) & 255u; tj[3] = (mid >> 16) & 255u; tj[4] = mid >> 24;
                    tj[5] = hi & 255u;
                };
                load_row(y - 1, t[0]);
                load_row(y, t[1]);
#pragma unroll
                for (int r = 0; r < DR; r++) {
                    const int* t0 = t[r % 3];
                    const int* t1 = t[(r + 1) % 3];
                    int* t2 = t[(r + 2) % 3];
                    load_row(y + r + 1, t2);
                    int av[6], bv[6];                                   // vertical smoothing / difference per column
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        av[k] = (t0[k] + t2[k]) * 3 + t1[k] * 10;
                        bv[k] = t2[k] - t0[k];
                    }
                    uint32_t o[4];                                      // (dx, dy) as two 16-bit halves
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int dx = av[k + 2] - av[k], dy = (bv[k + 2] + bv[k]) * 3 + bv[k + 1] * 10;
                        o[k] = ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16);
                        if (masked && ((unsigned)(ipx - 1 + x + k) >= (unsigned)L.w || (unsigned)(ipy - 1 + y + r) >= (unsigned)L.h)) o[k] = 0u;
                    }
                    if (y + r <= PW) *reinterpret_cast<uint4*>(&pD[(y + r) * PP + x]) = make_uint4(o[0], o[1], o[2], o[3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();
        // ---- template window, its gradients and the 2x2 matrix
        // (the LDS addresses of the window pixels are derived here at every level: hoisted out of the level loop they cost 20 registers)
#pragma unroll
        for (int k = 0; k < NPX; k++) asm volatile("" : "+v"(off[k]));
        Weights wt = make_weights(prevx - ipx, prevy - ipy);
        short Iw[NPX], Ix[NPX], Iy[NPX];
        int pA11 = 0, pA12 = 0, pA22 = 0;
#pragma unroll
        for (int k = 0; k < NPX; k++) {
            // invalid slots read offset 0 and are zeroed afterwards
            const int o = LK_POFF(k);
            int ival = descale(__mul24((int)pI[o], wt.w00) + __mul24((int)pI[o + 1], wt.w01) +
                               __mul24((int)pI[o + PP], wt.w10) + __mul24((int)pI[o + PP + 1], wt.w11), 9);
            const short2 d00 = pD[o], d01 = pD[o + 1], d10 = pD[o + PP], d11 = pD[o + PP + 1];
            int ixval = descale(__mul24((int)d00.x, wt.w00) + __mul24((int)d01.x, wt.w01) +
                                __mul24((int)d10.x, wt.w10) + __mul24((int)d11.x, wt.w11), 14);
            int iyval = descale(__mul24((int)d00.y, wt.w00) + __mul24((int)d01.y, wt.w01) +
                                __mul24((int)d10.y, wt.w10) + __mul24((int)d11.y, wt.w11), 14);
            if (!LK_VALID(k)) { ival = 0; ixval = 0; iyval = 0; }
            Iw[k] = (short)ival; Ix[k] = (short)ixval; Iy[k] = (short)iyval;
            pA11 += __mul24(ixval, ixval);
            pA12 += __mul24(ixval, iyval);
            pA22 += __mul24(iyval, iyval);
        }
        const long long sA11 = wave_sum<WS>(pA11), sA12 = wave_sum<WS>(pA12), sA22 = wave_sum<WS>(pA22);
        const float A11 = (float)sA11 * FLT_SCALE, A12 = (float)sA12 * FLT_SCALE, A22 = (float)sA22 * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                             (float)(2 * win * win);
        if (minEig < 1e-4f || D < FLT_EPSILON) {
            if (level == 0) status = 0;
            continue;
        }
        D = 1.f / D;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_count; j++) {
            const int inx = f_floor(cx), iny = f_floor(cy);
            if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
                if (level == 0) status = 0;
                break;
            }
            wt = make_weights(cx - inx, cy - iny);
            int lx = inx - rx0, ly = iny - ry0;
            if (!(lx >= 0 && ly >= 0 && lx + win + 1 <= RW && ly + win + 1 <= RW)) {    // wave-uniform
                __syncthreads();
                rx0 = inx - LK_MARGIN; ry0 = iny - LK_MARGIN;
                stage_region();
                __syncthreads();
                lx = LK_MARGIN; ly = LK_MARGIN;
            }
            int pb1 = 0, pb2 = 0;
            {
                // every slot is computed unconditionally (invalid slots carry Ix = Iy = 0 and a
                // safe offset), so the LDS reads of all pixels are in flight together
                const int rbase = ly * RP + lx;
#pragma unroll
                for (int k = 0; k < NPX; k++) {
                    const uint8_t* r0 = &region[rbase + LK_ROFF(k)];
                    // signed 24-bit multiplies: w11 = 2^14 - w00 - w01 - w10 can be -1
                    const int v = descale(__mul24((int)r0[0], wt.w00) + __mul24((int)r0[1], wt.w01) +
                                          __mul24((int)r0[RP], wt.w10) + __mul24((int)r0[RP + 1], wt.w11), 9);
                    const int diff = v - Iw[k];
                    pb1 += __mul24(diff, (int)Ix[k]);
                    pb2 += __mul24(diff, (int)Iy[k]);
                }
            }
            const long long sb1 = wave_sum<WS>(pb1), sb2 = wave_sum<WS>(pb2);
            const float b1 = (float)sb1 * FLT_SCALE, b2 = (float)sb2 * FLT_SCALE;
            const float dx = (A12 * b2 - A22 * b1) * D;
            const float dy = (A12 * b1 - A11 * b2) * D;
            cx += dx; cy += dy;
            outx = cx + halfWin; outy = cy + halfWin;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= a.eps2) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (status && level == 0) {
            const float npx = outx - halfWin, npy = outy - halfWin;
            const int inx = f_floor(npx), iny = f_floor(npy);
            if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
                status = 0;
            } else {
                wt = make_weights(npx - inx, npy - iny);
                int lx = inx - rx0, ly = iny - ry0;
                if (!(lx >= 0 && ly >= 0 && lx + win + 1 <= RW && ly + win + 1 <= RW)) {
                    __syncthreads();
                    rx0 = inx - LK_MARGIN; ry0 = iny - LK_MARGIN;
                    stage_region();
                    __syncthreads();
                    lx = LK_MARGIN; ly = LK_MARGIN;
                }
                int es = 0;
                {
                    const int rbase = ly * RP + lx;
#pragma unroll
                    for (int k = 0; k < NPX; k++) {
                        const uint8_t* r0 = &region[rbase + LK_ROFF(k)];
                        const int v = descale(__mul24((int)r0[0], wt.w00) + __mul24((int)r0[1], wt.w01) +
                                              __mul24((int)r0[RP], wt.w10) + __mul24((int)r0[RP + 1], wt.w11), 9);
                        const int diff = v - Iw[k];
                        es += LK_VALID(k) ? (diff < 0 ? -diff : diff) : 0;
                    }
                }
                const long long est = wave_sum<WS>(es);
                err = (float)est * 1.f / (float)(32 * win * win);
            }
        }
    }
#undef LK_VALID
#undef LK_POFF
#undef LK_ROFF
    if (lane == 0) {
        a.next_pts[2 * pt] = outx;
        a.next_pts[2 * pt + 1] = outy;
        a.status[pt] = (uint8_t)status;
        a.err[pt] = err;
    }
}

template <int NPX>
__global__ __launch_bounds__(64) void lk_kernel(LKArgs a) { lk_track<NPX>(a, blockIdx.x); }

// Several frames per launch: blockIdx.y selects the frame's argument block in a device table.
template <int NPX>
__global__ __launch_bounds__(64) void lk_batch_kernel(const LKArgs* __restrict__ table) {
    lk_track<NPX>(table[blockIdx.y], blockIdx.x);
}

int fill_lk_args(LKArgs& a, const LKLevel* levels, int max_level, const float* d_prev_pts, int n, const int32_t* d_n,
                 float* d_next_pts, uint8_t* d_status, float* d_err, int win, int max_iters, double eps) {
    if (!levels || max_level < 0 || max_level >= MAX_LEVELS || n < 0 || win < 3 || win > 31 ||
        !d_prev_pts || !d_next_pts || !d_status || !d_err) {
        set_last_error("pyr_lk: invalid argument (3 <= win <= 31, max_level < 8)");
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i <= max_level; i++) a.levels[i] = levels[i];
    for (int i = max_level + 1; i < MAX_LEVELS; i++) a.levels[i] = levels[max_level];
    a.max_level = max_level;
    a.prev_pts = d_prev_pts; a.next_pts = d_next_pts; a.status = d_status; a.err = d_err;
    a.n = n; a.d_n = d_n; a.win = win;
    // SparsePyrLKOpticalFlowImpl::calc: clamp criteria, epsilon is squared
    a.max_count = max_iters < 0 ? 0 : (max_iters > 100 ? 100 : max_iters);
    double e = eps < 0 ? 0. : (eps > 10. ? 10. : eps);
    a.eps2 = e * e;
    return VS_OK;
}

}  // namespace

// ---- batched form: one argument block per frame in a device table (see stabilizer.cpp) ----
size_t lk_item_bytes() { return sizeof(LKArgs); }

int lk_fill_item(void* host_item, const LKLevel* levels, int max_level, const float* d_prev_pts, int n,
                 const int32_t* d_n, float* d_next_pts, uint8_t* d_status, float* d_err, int win, int max_iters,
                 double eps) {
    return fill_lk_args(*static_cast<LKArgs*>(host_item), levels, max_level, d_prev_pts, n, d_n, d_next_pts, d_status,
                        d_err, win, max_iters, eps);
}

// items frames, at most n_max points each, all with the same window
int launch_pyr_lk_batch(const void* d_table, int items, int n_max, int win, hipStream_t st) {
    if (!d_table || items < 1 || items > 65535 || n_max < 0 || win < 3 || win > 31) {
        set_last_error("pyr_lk_batch: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    if (n_max == 0) return VS_OK;
    const LKArgs* t = static_cast<const LKArgs*>(d_table);
    const int npx = (win * win + 63) / 64;
    dim3 grid(n_max, items), block(64);
    if (npx <= 4) hipLaunchKernelGGL(lk_batch_kernel<4>, grid, block, 0, st, t);
    else if (npx <= 7) hipLaunchKernelGGL(lk_batch_kernel<7>, grid, block, 0, st, t);
    else hipLaunchKernelGGL(lk_batch_kernel<16>, grid, block, 0, st, t);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

int launch_pyr_lk(const LKLevel* levels, int max_level, const float* d_prev_pts, int n,
                  const int32_t* d_n, float* d_next_pts, uint8_t* d_status, float* d_err, int win,
                  int max_iters, double eps, hipStream_t st) {
    LKArgs a;
    VS_TRY(fill_lk_args(a, levels, max_level, d_prev_pts, n, d_n, d_next_pts, d_status, d_err, win, max_iters, eps));
    if (n == 0) return VS_OK;
    const int npx = (win * win + 63) / 64;
    dim3 grid(n), block(64);
    if (npx <= 4) hipLaunchKernelGGL(lk_kernel<4>, grid, block, 0, st, a);
    else if (npx <= 7) hipLaunchKernelGGL(lk_kernel<7>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(lk_kernel<16>, grid, block, 0, st, a);
    VS_HIP_TRY(hipGetLastError());
    return VS_OK;
}

// vs_op_pyr_lk: builds both pyramids, then tracks.
int run_pyr_lk_op(const uint8_t* d_prev, const uint8_t* d_next, size_t stride, int w, int h,
                  const float* d_prev_pts, int n, float* d_next_pts, uint8_t* d_status,
                  float* d_err, int win, int max_level, int max_iters, double eps, hipStream_t st) {
    if (!d_prev || !d_next || w <= 0 || h <= 0 || max_level < 0 || max_level >= MAX_LEVELS) {
        set_last_error("pyr_lk: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    // buildOpticalFlowPyramid: stop when the next level would not exceed the window
    int lw[MAX_LEVELS], lh[MAX_LEVELS];
    int levels = 0;
    {
        int sw = w, sh = h;
        for (int level = 0; level <= max_level; level++) {
            lw[level] = sw; lh[level] = sh;
            levels = level;
            sw = (sw + 1) / 2; sh = (sh + 1) / 2;
            if (sw <= win || sh <= win) break;
        }
    }
    size_t img_bytes = 0;
    for (int i = 1; i <= levels; i++) img_bytes += (size_t)lw[i] * lh[i];
    uint8_t* scratch = nullptr;
    VS_HIP_TRY(hipMalloc((void**)&scratch, 2 * img_bytes + 64));
    LKLevel L[MAX_LEVELS];
    uint8_t* pp = scratch;
    uint8_t* pn = scratch + img_bytes;
    int rc = VS_OK;
    for (int i = 0; i <= levels && rc == VS_OK; i++) {
        L[i].w = lw[i]; L[i].h = lh[i];
        if (i == 0) { L[i].prev = d_prev; L[i].next = d_next; L[i].stride = stride; }
        else {
            rc = launch_pyr_down(L[i - 1].prev, L[i - 1].stride, lw[i - 1], lh[i - 1], pp, lw[i], st);
            if (rc == VS_OK) rc = launch_pyr_down(L[i - 1].next, L[i - 1].stride, lw[i - 1], lh[i - 1], pn, lw[i], st);
            L[i].prev = pp; L[i].next = pn; L[i].stride = lw[i];
            pp += (size_t)lw[i] * lh[i]; pn += (size_t)lw[i] * lh[i];
        }
    }
    if (rc == VS_OK) rc = launch_pyr_lk(L, levels, d_prev_pts, n, nullptr, d_next_pts, d_status, d_err, win, max_iters, eps, st);
    hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (rc == VS_OK && e != hipSuccess) { set_last_error(hipGetErrorString(e)); rc = VS_ERR_HIP; }
    return rc;
}

}  // namespace vsd
