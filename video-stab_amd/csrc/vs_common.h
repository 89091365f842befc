// Internal header of libvideo-stab (gfx950).  Not part of the C ABI.
#ifndef VS_COMMON_H
#define VS_COMMON_H

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>
#include <cfloat>
#include <cmath>
#include <string>
#include <utility>

#include "../../include/vs_stab.h"

namespace vsd {

// ---- error plumbing ---------------------------------------------------------
// One policy for the whole library.  A failed call returns a status; its message goes to the calling thread's last error
// (vs_last_error), for a failed HIP call as "<expr>: <hipGetErrorString>".  Ops use VS_HIP_TRY / VS_TRY.  A call on an object
// (vs_stab, vs_batch, vs_roll, vs_azc, vs_enh) uses VS_OBJ_HIP / VS_OBJ_TRY / vs_obj_fail, which also copy the message into
// the object's `err` (vs_<obj>_last_error).
// Thread rule: an object's `err` is written only inside that object's API calls, on the caller's thread.  Worker threads use
// the op-level macros only and hand their first failure over in a FirstFailure under the object's mutex; the API call that
// reports it (vs_roll_sync, vs_azc_sync) copies it into `err`.
void set_last_error(const std::string& msg);
const char* get_last_error();

// Sets the last error for the failed HIP call `expr` and returns its status.
inline int hip_fail(hipError_t e, const char* expr) {
    set_last_error(std::string(expr) + ": " + hipGetErrorString(e));
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver || e == hipErrorNoBinaryForGpu)
               ? VS_ERR_NO_DEVICE
               : VS_ERR_HIP;
}

template <typename Obj>
int vs_obj_fail(Obj* o, int code, const std::string& msg) {
    o->err = msg;
    set_last_error(msg);
    return code;
}

#define VS_HIP_TRY(expr)                                     \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return vsd::hip_fail(_e, #expr); \
    } while (0)

#define VS_TRY(expr)                      \
    do {                                  \
        int _s = (expr);                  \
        if (_s != VS_OK) return _s;       \
    } while (0)

#define VS_OBJ_HIP(o, expr)                                                            \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            const int _s = vsd::hip_fail(_e, #expr);                                   \
            (o)->err = vsd::get_last_error();                                          \
            return _s;                                                                 \
        }                                                                              \
    } while (0)

#define VS_OBJ_TRY(o, expr)                                                            \
    do {                                                                               \
        int _s = (expr);                                                               \
        if (_s != VS_OK) { (o)->err = vsd::get_last_error(); return _s; }             \
    } while (0)

// The first failure of an object's worker threads; noted and taken under the object's mutex.
struct FirstFailure {
    int rc = VS_OK;
    std::string msg;
    void note(int code, const std::string& m) {
        if (rc == VS_OK && code != VS_OK) { rc = code; msg = m; }
    }
    FirstFailure take() {   // the record for the reporting call; this one starts again
        FirstFailure f;
        std::swap(f, *this);
        return f;
    }
};

int ensure_device();  // VS_OK when a gfx950-class device is usable

// ---- device helpers: same integer semantics as OpenCV's cvRound/cvFloor -------
#ifdef __HIPCC__
__device__ __forceinline__ int d_round(double v) { return __double2int_rn(v); }
__device__ __forceinline__ int f_round(float v) { return __float2int_rn(v); }
__device__ __forceinline__ int f_floor(float v) { return __float2int_rd(v); }
__device__ __forceinline__ int sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ int reflect101(int p, int len) {
    // cv::borderInterpolate(BORDER_REFLECT_101)
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}
// XCD-aware tile order.  The hardware hands consecutive workgroups to the 8 XCDs in turn (linear id mod 8), and every XCD has an L2
// of its own.  Workgroup `lin` of n takes tile xcd_seq(lin, n) of the launch's tile sequence: XCD c = lin mod 8 takes the c-th
// contiguous eighth of it, so that tiles that share source lines meet in one L2 (k_warp.hip at tile_id has the traffic figures).
__device__ __forceinline__ uint32_t xcd_seq(uint32_t lin, uint32_t n) {
    const uint32_t c = lin & 7u, k = lin >> 3, q = n >> 3, r = n & 7u;
    return c * q + (c < r ? c : r) + k;
}
#endif

// cv::warpAffine's inversion of the forward 2x3 matrix, in double (imgwarp.cpp).  The same
// IEEE operation sequence on host and device (no FMA contraction in either build).
// The library has one configuration: kernel and schedule variants measured in earlier rounds live in scratch/ as patches, not
// behind switches.  What remains behind VS_LAB=1 are two test hooks (VS_STAB_DEBUG_DELAY_US: a spin kernel that widens a window
// an ordering test looks into; VS_STAB_HOST_HELPER=0: the pipelined host call without its helper thread).  (The documented
// runtime settings - VS_STAB_DEVICE, VS_STAB_HOST_PIPELINE, VS_STAB_HELPER_SPIN_US - are ordinary environment variables.)
inline const char* lab_env(const char* name) {
    const char* e = std::getenv("VS_LAB");
    return (e && e[0] == '1') ? std::getenv(name) : nullptr;
}

// T = float (CV_32F matrices) or double.
template <typename T>
#ifdef __HIPCC__
__host__ __device__
#endif
inline void warp_invert(const T* Mf, double* inv) {
    double M[6];
    for (int i = 0; i < 6; i++) M[i] = (double)Mf[i];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    double b1 = -M[0] * M[2] - M[1] * M[5];
    double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; i++) inv[i] = M[i];
}

// ---- stage launchers (device pointers, asynchronous on `st`) -----------------
// Warps (k_warp.hip).  Frames are given one by one; all frames of a call share one geometry.  A call warps its frames in launches
// of WARP_BATCH_MAX; a launch of WARP_TAB_MIN frames or more builds coordinate tables (warp_tab.h) when it is given a place for
// them: the coordinate terms are then built once per frame by a small launch in front of the warp instead of once per tile.
constexpr int WARP_BATCH_MAX = 32;
constexpr int WARP_TAB_MIN = 4;
// Edge fill on YUV surfaces (vs_stab_set_yuv_edge_fill, vs_op_warp_affine_yuv_fill): BORDER_CONSTANT with a colour - a tap outside a
// plane reads the plane's fill sample.  An internal border code of the YUV launchers (launch_warp_nv12, launch_warp_i420) behind the six
// values of the public border_type enum, which it is not part of; it fits the three border bits of the kernels' flags.
constexpr int VS_BORDER_FILL = 6;
static_assert(VS_BORDER_FILL > VS_BORDER_FADE && VS_BORDER_FILL < 8, "an internal code behind the public border types, in three bits");
// The fill of such a launch, samples as they lie in memory (8-bit formats: at most 255).  (0, 0, 0) gives VS_BORDER_BLACK's bytes.
struct WarpFill { uint32_t y = 0, u = 0, v = 0; };
// Ints of table workspace a launch over `frames` frames of dw x dh needs (packed tables).
size_t warp_tabs_ints(int dw, int dh, int frames);
// The INVERSE maps (warp_invert of the forward matrices), 6 doubles per frame and `stride` doubles from frame to frame: on the
// device, or on the host (they then travel as kernel arguments).  NV12: the chroma plane's map follows the luma map (m + 6).
struct WarpMaps {
    const double* m;
    int stride;
    bool host;
};
// what: the whole launch, or its two halves apart (tables of the frames now, the warp later from the same tables).
enum { VS_WARP_ALL = 0, VS_WARP_TABLES_ONLY = 1, VS_WARP_ONLY = 2 };
// Where a call's coordinate tables go: nowhere; the caller's buffer (`stride` ints from frame to frame, 0 = packed; NV12 calls
// take blocks of nv12_tab_ints); or a grow-only scratch block per stream (the standalone operators).
struct WarpTabs {
    enum Kind { NONE, CALLER, SCRATCH };
    Kind kind = NONE;
    int32_t* tabs = nullptr;
    int stride = 0;
    int what = VS_WARP_ALL;
};
// One plane of cn channels per frame (1 .. 3), border VS_BORDER_BLACK or VS_BORDER_REPLICATE.
// sample_bytes = 2: planes of 16-bit samples (cn 1 or 2, strides in bytes, pointers and strides even, no tables): P010's blend.
int launch_warp_plane(const uint8_t* const* srcs, uint8_t* const* dsts, int n, size_t sstride, int sw, int sh, size_t dstride, int dw,
                      int dh, int cn, WarpMaps maps, int border, WarpTabs tabs, hipStream_t st, int sample_bytes = 1);
// NV12 surfaces of w x h (even) luma pixels: luma planes ys -> yd, interleaved chroma planes us -> ud (half size, two channels).
// Launches with tables warp both planes of their surfaces in ONE grid when the chroma planes lie one offset behind the luma
// planes; other launches go plane by plane.
// sample_bytes = 2: P010 surfaces - planes of 16-bit samples, pitches and pointers in bytes and even; a call with the scratch tables
// builds them for any number of surfaces.
// border VS_BORDER_FILL: taps outside a plane read `fill` (Y; the (U, V) pair); with the scratch tables every launch builds them.
int launch_warp_nv12(const uint8_t* const* ys, uint8_t* const* yd, const uint8_t* const* us, uint8_t* const* ud, int n, size_t sstride,
                     size_t dstride, int w, int h, WarpMaps maps, int border, WarpTabs tabs, hipStream_t st, int sample_bytes = 1,
                     WarpFill fill = WarpFill());
// One warp of a multi-job launch (launch_warp_jobs, k_warp.hip): any geometry, inverse map in double on the host.
struct WarpJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sstride, dstride;
    int32_t sw, sh, dw, dh, cn, border;
    double m[6];
    int32_t sb = 1;              // bytes of a sample: 1, or 2 (planes of 16-bit samples, cn 1 or 2, P010's blend); one value per launch
};
// (24: the three planes of eight planar 4:2:0 surfaces - the table travels as a kernel argument, 24 x 104 = 2496 of the 4096 bytes
// a launch may carry)
constexpr int WARP_JOBS_MAX = 24;
int launch_warp_jobs(const WarpJob* jobs, int n, hipStream_t st);
// Crop-and-scale jobs (diagonal maps, as AutoZoomCrop builds them): those whose tiles' source boxes fit the staging area go to the
// staged kernel as one launch, the others to launch_warp_jobs as one launch.  path 0: as scale_job_staged says per job; 1: all
// through launch_warp_jobs.  scale_job_staged is host arithmetic on the job's inverse map alone.
bool scale_job_staged(const WarpJob& j);
int launch_scale_jobs(const WarpJob* jobs, int n, int path, hipStream_t st);
// The same for jobs on interleaved colour frames: 8-bit samples, cn 3 or 4 (mixed freely), every channel a channel of its own - the
// colour instances of the two kernels; one staging bound for all pixel sizes (a staged pixel is a dword).
bool scale_job_staged_rgb(const WarpJob& j);
int launch_scale_jobs_rgb(const WarpJob* jobs, int n, int path, hipStream_t st);
int launch_resize_gray(const uint8_t* d_src, size_t sstride, int sw, int sh, int fmt,
                       uint8_t* d_dst, size_t dstride, int dw, int dh, hipStream_t st);
// Batched forms (batch mode): the images of `items` frames in one launch; d_pairs = device table of
// (source, destination) pointers, all of one geometry.
struct ImgPair { const void* src; void* dst; };
int launch_resize_gray_batch(const ImgPair* d_pairs, int items, size_t sstride, int sw, int sh, int fmt, size_t dstride,
                             int dw, int dh, int aligned, hipStream_t st);
// One pyramid level of `items` images: Scharr derivatives (d_scharr_pairs: image -> derivative image) and/or the pyrDown
// (d_pyr_pairs: image -> next level); when both tables are given, their sources are the same images.
int launch_pyr_level_batch(const ImgPair* d_scharr_pairs, const ImgPair* d_pyr_pairs, int items, size_t sstride, int w, int h,
                           size_t dstride, hipStream_t st);
int launch_pyr_down(const uint8_t* d_src, size_t sstride, int sw, int sh, uint8_t* d_dst,
                    size_t dstride, hipStream_t st);
int launch_scharr(const uint8_t* d_src, size_t sstride, int w, int h, int16_t* d_dst,
                  hipStream_t st);

struct LKLevel {
    const uint8_t* prev;
    const uint8_t* next;
    int w, h;
    size_t stride;
};
// Tracks n points over levels[max_level..0]; n may be a device count (d_n) or host n.
int launch_pyr_lk(const LKLevel* levels, int max_level, const float* d_prev_pts, int n,
                  const int32_t* d_n, float* d_next_pts, uint8_t* d_status, float* d_err, int win,
                  int max_iters, double eps, hipStream_t st);

struct GfttWork {            // device scratch owned by the caller
    float* eig;              // w*h
    uint64_t* cand;          // cap candidates (key = value bits << 32 | index)
    int32_t* counters;       // [0]=ncand [1]=maxbits [2]=overflow [3]=n_out  (+ spare)
    int cap;
};
// Candidates a w x h image can have: the interior.  A candidate is an interior pixel that EQUALS its 3x3 maximum, so on a plateau
// (a picture of period blockSize has a constant map) every interior pixel is one; only strict maxima exclude their neighbours.
// The list is never truncated with this cap; a buffer sized for a larger image holds the list of every smaller one.
inline int gftt_cand_cap(int w, int h) { return w > 2 && h > 2 ? (w - 2) * (h - 2) : 1; }
size_t gftt_work_bytes(int w, int h, int cap);
void gftt_work_carve(void* base, int w, int h, int cap, GfttWork* out);
int launch_gftt(const uint8_t* d_gray, size_t stride, int w, int h, int max_corners,
                double quality, double min_distance, int block_size, const GfttWork& wk,
                float* d_pts, int32_t* d_count, hipStream_t st);

}  // namespace vsd
#endif
