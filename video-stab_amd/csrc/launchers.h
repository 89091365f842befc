// Stage launchers of the stabilizer pipeline that vs_common.h does not declare: the per-frame RANSAC / trajectory / border
// kernels and the batched forms, whose argument blocks are opaque to the host (sized and filled through *_bytes / *_fill_*).
// Host-only: included by stabilizer.cpp, batch_schedule.cpp and vs_api.cpp, defined in the k_*.hip file named with each group.
#ifndef VS_LAUNCHERS_H
#define VS_LAUNCHERS_H

#include <algorithm>
#include <string>

#include "pixfmt.h"
#include "planar_layout.h"
#include "traj_state.h"
#include "vs_common.h"
#include "warp_tab.h"

namespace vsd {

// ---- k_ransac.hip: estimateAffinePartial2D + trajectory append of one frame, and the batched scoring / ordered tail
struct RansacTables;
int get_ransac_tables(int max_m, int iters, const RansacTables** out);
int launch_ransac(const float* d_from, const float* d_to, const uint8_t* d_status, int n, const int32_t* d_n, float* d_vp, float* d_vc, int32_t* d_m,
                  int min_points, double thr, int iters, const RansacTables* tab, int32_t* d_counts, double* d_model, uint8_t* d_inliers,
                  int32_t* d_info, TrajState* traj, const TrajParams* tp, vs_debug_frame* dbg, int have_prev_gray, hipStream_t st);
size_t ransac_item_bytes();
int ransac_fill_item(void* host_item, const float* d_from, const float* d_to, const uint8_t* d_status, int n, const int32_t* d_n, float* d_vp,
                     float* d_vc, int32_t* d_m, int min_points, double thr, int iters, const RansacTables* tab, int32_t* d_counts, double* d_model,
                     uint8_t* d_inliers, int32_t* d_info, TrajState* traj, const TrajParams* tp, vs_debug_frame* dbg, int have_prev_gray);
void ransac_item_set_tail_in(void* host_item, void* d_tail_in);
void ransac_item_set_last(void* host_item, int last);      // the last frame of its stream in the step
int launch_ransac_score_batch(const void* d_table, int items, int iters, int n_max, hipStream_t st);
size_t tail_item_bytes();
void tail_fill_item(void* host_item, int out_due, int out_idx, double* d_Minv_out, const WarpTabJob* tabs);   // tabs: two jobs
void tail_item_set_seg(void* host_item, int seg);
size_t tail_in_bytes();
void tail_in_fill(void* host_tail_in, const double* model, int ok, int nprev, int have_prev_gray);              // vs_op_trajectory
void ransac_fill_item_traj(void* host_item, TrajState* traj, const TrajParams* tp, vs_debug_frame* dbg);         // vs_op_trajectory
size_t tail_seg_bytes();        // a segment = the frames of one stream in the step
void tail_fill_seg(void* host_seg, int first, int n, float* d_M_out, TrajState* traj, vs_debug_frame* dbg, int smoothing_method);
int launch_ransac_tail_group(const void* d_table, const void* d_tail, const void* d_segs, const void* d_tail_in, int nsegs, int max_n, int items,
                             int any_apart, hipStream_t st);

// ---- k_lk.hip, k_gftt.hip: batched tracker and detector (what: 1 reset, 4 min-eigen, 5 NMS, 3 selection)
size_t lk_item_bytes();
int lk_fill_item(void* host_item, const LKLevel* levels, int max_level, const float* d_prev_pts, int n, const int32_t* d_n, float* d_next_pts,
                 uint8_t* d_status, float* d_err, int win, int max_iters, double eps);
int launch_pyr_lk_batch(const void* d_table, int items, int n_max, int win, hipStream_t st);
size_t gftt_item_bytes();
int gftt_fill_item(void* host_item, const uint8_t* d_gray, size_t stride, int w, int h, int max_corners, double quality, double min_distance,
                   int block_size, const GfttWork& wk, float* d_pts, int32_t* d_count);
int launch_gftt_batch(const void* d_table, int items, int w, int h, int block_size, hipStream_t st, int what);

// ---- k_warp.hip: planar surfaces (I420 / YV12, I010 / I012; 4:2:2 and 4:4:4: I422, I444, I210, I212, I410, I412) of w x h luma pixels
// (I420Layout, i420_layout: planar_layout.h)
// Launches with tables warp the three planes of their surfaces in ONE grid (warp_i420_kernel); the tables are an NV12 surface's
// (planar_tab_ints per frame: luma table, then one chroma table whose pointer records name the U planes), the maps as for NV12
// (m: luma, m + 6: chroma).  A call with the scratch tables builds them for any number of surfaces.
// sample_bytes = 2: I010 / I012 surfaces - the same planes with 16-bit samples; layouts in bytes, pointers, pitches and offsets even.
// sx, sy: the chroma shifts (4:2:0 needs even w and h, 4:2:2 an even w, 4:4:4 takes any size).
// Host maps, 4:2:2 and VS_BORDER_REPLICATE (the roll stage, vs_op_warp_affine_planar): a launch in which some surface's chroma tiles may
// outgrow the staged box and can fit the taller one goes to the instances with THP + 17 staged rows (k_warp.hip, warp_i422_tall_kernel).
// border VS_BORDER_FILL (vs_common.h): taps outside a plane read that plane's sample of `fill`.
int launch_warp_i420(const uint8_t* const* ys, uint8_t* const* yd, int n, I420Layout src, I420Layout dst, int w, int h, WarpMaps maps, int border,
                     WarpTabs tabs, hipStream_t st, int sample_bytes = 1, int sx = 1, int sy = 1, WarpFill fill = WarpFill());

// ---- the plane list (planar_layout.h) on the device: what the stream, the batch schedule and the roll / zoom stages share
// The warp of n <= WARP_BATCH_MAX surfaces (planes S, at the size of S's luma) into surfaces with planes D, one launch: the one
// plane of an interleaved format; luma and the interleaved chroma plane - half size, two channels, the map with the halved
// translation (m + 6) -; or Y, U and V, whose one chroma table serves both U and V.
inline int warp_planes(const uint8_t* const* srcs, uint8_t* const* dsts, int n, const Planes& S, const Planes& D, WarpMaps maps, int border, WarpFill fill,
                       WarpTabs tabs, hipStream_t st) {
    if (S.n == 1) return launch_warp_plane(srcs, dsts, n, S[0].pitch, S[0].w, S[0].h, D[0].pitch, S[0].w, S[0].h, S[0].cn, maps, border, tabs, st, S.sample_bytes);
    if (S.n == 3)
        return launch_warp_i420(srcs, dsts, n, S.i420(), D.i420(), S[0].w, S[0].h, maps, border, tabs, st, S.sample_bytes, S[1].sx, S[1].sy, fill);
    const uint8_t* us[WARP_BATCH_MAX];
    uint8_t* ud[WARP_BATCH_MAX];
    for (int i = 0; i < n; i++) { us[i] = srcs[i] + S[1].off; ud[i] = dsts[i] + D[1].off; }
    return launch_warp_nv12(srcs, dsts, us, ud, n, S[0].pitch, D[0].pitch, S[0].w, S[0].h, maps, border, tabs, st, S.sample_bytes, fill);
}
// A surface from one layout to another, one copy per plane (S and D: the planes of one format; S says how much of each)
inline hipError_t copy_planes(uint8_t* dst, const Planes& D, const uint8_t* src, const Planes& S, hipMemcpyKind kind, hipStream_t st) {
    for (int k = 0; k < S.n; k++) {
        const hipError_t e = hipMemcpy2DAsync(dst + D[k].off, D[k].pitch, src + S[k].off, S[k].pitch, S.row_bytes(k), S[k].h, kind, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- k_roll.hip, k_azc.hip: the geometry and layout rules of their three-plane surfaces are planar_layout_check, a frame of
// theirs is a StageFrame (planar_layout.h)
constexpr char RGB_FORMATS[] = "VS_FMT_BGR8, VS_FMT_RGB8, VS_FMT_BGRA8, VS_FMT_RGBA8";
// The *_dev_n forms: n surfaces in call order (what n calls of the per-surface entry point do, without n trips through a binding);
// one(i) hands surface i over, the first refusal ends the call
template <class One>
int each_surface(int n, One one) {
    for (int i = 0; i < n; i++) {
        const int rc = one(i);
        if (rc != VS_OK) return rc;
    }
    return VS_OK;
}

// ---- k_cvt.hip: YUV surfaces <-> interleaved 8-bit RGB (vs_op_cvt_yuv_to_rgb, vs_op_cvt_rgb_to_yuv, vs_enh_apply_yuv_dev)
constexpr int CVT_MAX_SURFACES = 32;        // of one launch: their pointers are kernel arguments
// What the conversions refuse about the YUV side - format family, geometry, pitches, 16-bit alignment, the planes of the layout -
// decided on the host before any device call (comp_op.cpp).  n surface pointers (checked: non-null, even for 16-bit samples).
// Fills *l with the defaults resolved (NV12 / P010: u = the interleaved plane, cpitch = pitch), or *msg with a text that names the
// call and the format.
int cvt_check_yuv(const char* call, int yuv_fmt, const void* const* surfaces, int n, const vs_i420_layout* lay, int w, int h, I420Layout* l,
                  std::string* msg);
// The integers of a colour space as the kernels take them (cvt_px.h).  cvt_resolve: what the conversions refuse about a descriptor
// (a field outside its enum, reserved != 0; *msg names the call and the field), else its integers; cs == nullptr: the default.
struct CvtCoef;
int cvt_resolve(const char* call, const vs_cvt_colorimetry* cs, CvtCoef* k, std::string* msg);
// n <= CVT_MAX_SURFACES surfaces of one geometry and layout in one launch (grid z = surface); rf: BGR8, RGB8, BGRA8 or RGBA8
int launch_cvt_yuv_to_rgb(const PixFmt& yf, const void* const* surfaces, const I420Layout& l, const PixFmt& rf, void* const* rgb, size_t rgb_stride,
                          int n, int w, int h, const CvtCoef& k, hipStream_t st);
int launch_cvt_rgb_to_yuv(const PixFmt& rf, const void* const* rgb, size_t rgb_stride, const PixFmt& yf, void* const* surfaces, const I420Layout& l,
                          int n, int w, int h, const CvtCoef& k, hipStream_t st);

// ---- k_yuvcvt.hip: YUV surfaces of one format -> YUV surfaces of another (vs_op_cvt_yuv_to_yuv)
// The depth step of a conversion as the kernel takes it: out = min(((min(sample, in_max) + add) >> down) << up, out_max).
// yuv_depth: the values for a pair of formats (a format's b bits: 8; 10 / 12 in the low bits; P010: the whole word, 16) and a
// vs_yuv_depth_down rule; equal depths copy the word (no clamp).
struct YuvDepth { uint32_t in_max, add, down, up, out_max; };
inline int yuv_value_bits(const PixFmt& f) { return f.luma_uv() && f.sample_bytes == 2 ? 16 : f.bits; }
inline bool yuv_low_bit(const PixFmt& f) { return f.three_planes() && f.sample_bytes == 2; }
// ... for a source of bi bits (low_in: a low-bit format) and a destination of bo bits
inline YuvDepth yuv_depth_bits(int bi, bool low_in, int bo, bool round) {
    const int d = bi - bo;
    YuvDepth k = {0xffffu, 0u, 0u, 0u, 0xffffu};
    if (d == 0) return k;
    if (low_in) k.in_max = (1u << bi) - 1u;      // a low-bit source: bits above its range clamp
    if (d < 0) k.up = (uint32_t)-d;
    else {
        k.down = (uint32_t)d;
        k.add = round ? 1u << (d - 1) : 0u;
        k.out_max = (1u << bo) - 1u;
    }
    return k;
}
inline YuvDepth yuv_depth(const PixFmt& sf, const PixFmt& df, bool round) {
    return yuv_depth_bits(yuv_value_bits(sf), yuv_low_bit(sf), yuv_value_bits(df), round);
}
// n <= CVT_MAX_SURFACES surfaces of one geometry in one launch (grid z = surface); the layouts as cvt_check_yuv resolved them
int launch_cvt_yuv_to_yuv(const PixFmt& sf, const void* const* src, const I420Layout& in, const PixFmt& df, void* const* dst, const I420Layout& out,
                          int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st);

// ---- k_yuvpacked.hip: packed 4:2:2 capture formats <-> YUV surfaces (vs_op_cvt_packed_to_yuv, vs_op_cvt_yuv_to_packed)
// What the kernels know of a vs_packed_fmt: its kind, and for the 8-bit orders the v_perm_b32 selector that makes a macropixel
// Y0 U Y1 V (each order is its own inverse, so the selector also packs).  The rest of a format - name, depth, row bytes, pitch and
// alignment rules - is host business (comp_op.cpp).
enum PackedKind { PACKED_8 = 0, PACKED_16 = 1, PACKED_V210 = 2 };
// n <= CVT_MAX_SURFACES surfaces of one geometry in one launch (grid z = surface); the surface side as cvt_check_yuv resolved it,
// the packed pitch resolved; depth: yuv_depth_bits with the packed side's bits (a v210 destination of a 10-bit source: in_max 1023)
int launch_cvt_packed_to_yuv(int kind, uint32_t sel, const void* const* src, size_t src_pitch, const PixFmt& df, void* const* dst, const I420Layout& out,
                             int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st);
int launch_cvt_yuv_to_packed(const PixFmt& sf, const void* const* src, const I420Layout& in, int kind, uint32_t sel, void* const* dst, size_t dst_pitch,
                             int n, int w, int h, const YuvDepth& depth, bool mean, hipStream_t st);

// ---- the plane-job operators on YUV surfaces (k_cropzoom.hip, k_yuvpad.hip, k_yuvfade.hip): what their kernels and launchers share -
// tile sequence, job search, launch check, the sentences of the refusals - is in plane_jobs.h.
// ---- k_cropzoom.hip: the zoom of crop-and-zoom on YUV surfaces (vs_op_resize_jobs; a stream with vs_stab_set_yuv_crop_zoom)
// n <= CZ_MAX_JOBS crops (src = the crop's first sample, sw x sh) resized to their planes (dw x dh, dw >= sw, dh >= sh) in ONE launch:
// 32 surfaces of up to three planes; cn 1 and 2 may be mixed, the sample size is the launch's.  Checks every job on the host first
// (a text in vs_last_error that names the job).
constexpr int CZ_MAX_JOBS = 96;
int launch_cropzoom(const vs_scale_job* jobs, int n, int sample_bytes, hipStream_t st);

// ---- k_resize.hip: the resize to an output size (vs_op_resample_jobs, vs_op_resize_yuv, vs_op_resize_rgb)
// n <= RS_MAX_JOBS planes (sw x sh samples of cn channels: 1 .. 4 with 8-bit samples, 1 or 2 with 16-bit samples) resized to dw x dh
// in any ratio, interp a vs_interp, results clamped to 0 .. max_value (0: the sample type's maximum); one launch per path class.
// Checks the launch and every job on the host first (a text in vs_last_error that names `name` and the job).  A call that meets
// an axis (src, dst, interp) for the first time on its device builds and uploads that axis' table and may block meanwhile.
constexpr int RS_MAX_JOBS = 96;
int launch_resample(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int interp, int max_value, int path, hipStream_t st);
int resample_plan(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int interp, int32_t* staged);     // host only
// ... and the area-averaging downscale (vs_op_area_jobs, vs_op_area_yuv, vs_op_area_rgb): the same jobs with dw <= sw and dh <= sh
// (an upscale: VS_ERR_UNSUPPORTED), cv::resize(INTER_AREA) arithmetic, ONE launch whatever the jobs' classes; cls[i]: 2 = the
// 2 x 2 mean, 1 = integer box, 0 = general (tables in the same arena, under a key of their own)
int launch_area(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int max_value, hipStream_t st);
int area_plan(const char* name, const vs_scale_job* jobs, int n, int sample_bytes, int32_t* cls);                         // host only

// ---- k_deint.hip: interlaced sources (vs_op_deint_jobs, vs_op_deint_yuv, vs_op_interlace_yuv)
// n <= DI_MAX_JOBS planes (w x h pixels of cn channels: 1 .. 4 with 8-bit samples, 1 or 2 with 16-bit samples) deinterlaced in ONE
// launch, mode a vs_deint_mode, or 2: the weave (cur = the first frame in time, next = the second; rows of parity keep from cur).
// Checks the launch and every job on the host first (a text in vs_last_error that names `name` and the job).
constexpr int DI_MAX_JOBS = 96;
int launch_deint(const char* name, const vs_deint_job* jobs, int n, int sample_bytes, int mode, hipStream_t st);

// ---- k_yuvpad.hip: the pad of border pad on YUV surfaces (vs_op_pad_jobs; a stream with vs_stab_set_yuv_border_pad)
// n <= YP_MAX_JOBS planes (sw x sh samples) padded by bx columns and by rows on every side in ONE launch: 32 surfaces of up to three
// planes; cn 1 and 2 may be mixed, the sample size is the launch's.  Checks every job on the host first (a text in vs_last_error
// that names the job).
constexpr int YP_MAX_JOBS = 96;
int launch_yuvpad(const vs_pad_job* jobs, int n, int sample_bytes, hipStream_t st);

// ---- k_yuvfade.hip: the fade border on YUV surfaces (vs_op_fade_blend_jobs, vs_op_fade_update_jobs; a stream with vs_stab_set_yuv_fade)
// blend: n <= YF_MAX_JOBS planes padded with their fill and blended with their history in ONE launch (dst = addWeighted(hist,
// alpha, padded src, beta)); update: hist = (T)((1 - 0.1f) * hist + 0.1f * res) over n planes in ONE launch.  cn 1 and 2 may be
// mixed, the sample size is the launch's.  Both check every job on the host first (a text in vs_last_error that names the job).
constexpr int YF_MAX_JOBS = 32;
int launch_yuvfade_blend(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, hipStream_t st);
int launch_yuvfade_update(const vs_fade_update_job* jobs, int n, int sample_bytes, hipStream_t st);

// ---- k_traj.hip: the map of output `idx` (t_out: its correction, for the virtual canvas), the fade border, a test delay
int launch_traj_emit(TrajState* s, const TrajParams& p, int idx, float* M_out, double* Minv_out, vs_debug_frame* dbg, hipStream_t st,
                     float* t_out = nullptr);
int launch_traj_append(TrajState* s, const TrajParams& p, const double* d_model, int ok, int nprev, int have_prev_gray, vs_debug_frame* dbg,
                       hipStream_t st);     // vs_op_trajectory
int launch_traj_reset(TrajState* s, int smoothing_radius, hipStream_t st);
int launch_spin(int microseconds, hipStream_t st);
int launch_fade_blend(const uint8_t* d_hist, uint8_t* d_frame, size_t bytes, float alpha, float beta, hipStream_t st);
int launch_fade_update(uint8_t* d_hist, const uint8_t* d_stab, size_t sstride, int row_bytes, int rows, hipStream_t st);
int launch_make_border(const uint8_t* src, size_t sstride, int w, int h, int cn, uint8_t* dst, size_t dstride, int b, int border, hipStream_t st);
// ---- k_gray.hip
int launch_resize_linear(const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, uint8_t* d_dst, size_t dstride, int dw, int dh, hipStream_t st);

}  // namespace vsd
#endif
