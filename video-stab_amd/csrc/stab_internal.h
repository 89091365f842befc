// What stabilizer.cpp (the stream object and its per-frame pipeline) and batch_schedule.cpp (the batch schedule that steps
// the frames such streams have queued) share: the stream object itself, the schedule's interface towards a stream, and the
// few helpers both sides use.  Host-only; everything else stays private to its file.
#ifndef VS_STAB_INTERNAL_H
#define VS_STAB_INTERNAL_H

#include <algorithm>
#include <deque>
#include <initializer_list>
#include <memory>
#include <vector>

#include "canvas.h"
#include "host_helper.h"
#include "launchers.h"
#include "pixfmt.h"

namespace vsd {

constexpr int BATCH_MAX = 64;        // frames analysed per launch in batch mode (vs_stab_set_batch)
// Batch mode: the warps of a step's due frames are issued WARP_LAG steps after the step that analysed them (batch_schedule.cpp;
// 1: with the next step, in front of its tracker; 2: one step later still, so that a step's tail runs beside the warps of the
// step before it).  Everything that must outlive a step because of it is sized from this one constant: the Ready records and
// the warps_due() test of vs_batch, the pyramid ring (batch_pyr_slots) and the frame queue ring (batch_ring_frames).
constexpr int WARP_LAG = 2;
constexpr int FRAME_RING = 128;     // <= 35 queued frames (clamp(smoothingRadius,5,35)) + slack so that a
                                    // slot is reused several frames after the warp that released it
constexpr int RING_SLACK = 29;
// Batch mode (copy-in): a frame's slot is released behind its warp.  Held at worst: 35 queued frames + the batch being
// collected + WARP_LAG steps whose warps are still to come, + the same slack.  Steps of up to 32 frames and of up to 64 (s->ring_frames).
constexpr int batch_ring_frames(int B) { return 35 + (1 + WARP_LAG) * (B > 32 ? BATCH_MAX : 32) + RING_SLACK; }
constexpr int FRAME_RING_MAX = batch_ring_frames(BATCH_MAX);
// Pyramid ring of a batch stream: the slots step k writes were last read by the analysis of step k - (WARP_LAG + 1), whose tail
// `pre` has waited for in front of the warps it issued in step k - 1 (step_issue_pre); + 2: the previous frame of a step's first.
constexpr int PYR_STEPS = WARP_LAG + 1;
constexpr int batch_pyr_slots(int B) { return PYR_STEPS * B + 2; }
constexpr int MAX_PYR = 8;
constexpr int NPYR = 3;             // pyramid buffers: frame k writes k%3 while LK(k-1) still reads (k-1)%3,(k-2)%3
constexpr int EVR = 4;              // per-frame event ring

struct Pyramid {
    uint8_t* img[MAX_PYR] = {};
};

}  // namespace vsd

// ---- the batch schedule as a stream sees it (batch_schedule.cpp)
struct vs_batch;
int group_run(vs_batch* g);                                     // one step over everything the members have queued
int group_drain(vs_batch* g);                                   // ... and the warps of that step issued as well
bool group_holds_warps(const vs_batch* g);
const vsd::FirstFailure& group_failure(const vs_batch* g);      // rc VS_OK: the group has not failed
vs_batch* group_new_own(vs_stab* s);                            // the private group of one of a standalone instance
void group_delete(vs_batch* g);

struct vs_stab {
    vs_params_c p;
    int device = 0;
    // batch mode: the schedule that runs this stream's batches (one launch per stage over the frames of all its streams) - the
    // vs_batch the stream was created in, or the private group of one a standalone instance owns (`own`, made by allocate())
    vs_batch* group = nullptr;
    vs_batch* own = nullptr;
    bool member = false;            // stream of a vs_batch_create group: driven through vs_batch_* only
    bool group_call = false;        // ... which set this around the vs_stab_* calls they make on a member
    hipStream_t st = nullptr;       // main
    hipStream_t st_pre = nullptr;
    hipStream_t st_det = nullptr;
    hipStream_t st_warp = nullptr;  // deferred (batched) warps, high priority
    bool shared_streams = false;    // the four streams belong to the per-device pool
    std::string err;
    // geometry, fixed by the first frame
    bool allocated = false;
    int w = 0, h = 0, fmt = VS_FMT_BGR8, cn = 3;
    const vsd::PixFmt* pf = vsd::pixfmt(VS_FMT_BGR8);     // the table row of fmt (pixfmt.h), set with it in allocate_buffers
    size_t row_bytes = 0, frame_bytes = 0;
    size_t src_pitch = 0;               // row pitch of the frames the pipeline reads: row_bytes (queue ring) or the caller's (zero-copy)
    // surfaces of the device entry points: where the chroma of the frames pushed (`in`) and of the surfaces filled (`out`) lies
    vsd::ChromaLayout in, out;
    int rows_total = 0;
    int aw = 960, ah = 540;
    int levels = 0;                 // max pyramid level actually used
    int lw[vsd::MAX_PYR], lh[vsd::MAX_PYR];
    // frame queue (Stabilizer.h:311-312)
    uint8_t* d_ring = nullptr;
    std::deque<int> q_slot, q_idx;      // ring slot (-1: the caller's own buffer, zero-copy mode) and frame index
    std::deque<const uint8_t*> q_ptr;   // where the queued frame lives
    bool zero_copy = false;             // vs_stab_set_zero_copy
    std::deque<int> free_slots;     // FIFO: the slot released longest ago is reused first
    bool first = true;
    int next_index = 0;             // index of the frame being pushed (nextFrameIndex_)
    int detect_counter = 0;
    int n_transforms = 0;           // transforms_.size(), mirrored on the host
    int last_out_w = 0, last_out_h = 0;
    int orig_w = 0, orig_h = 0;
    int host_radius = 30;
    int dbg_delay_us = 0;           // VS_STAB_DEBUG_DELAY_US: a spin kernel between tracking and RANSAC (ordering tests)
    // analysis images
    uint8_t* d_first_gray = nullptr;     // 480x270 (Stabilizer.cpp:277)
    std::vector<vsd::Pyramid> pyr;      // ring: NPYR buffers, batch_pyr_slots(batch) in batch mode
    int npyr = vsd::NPYR;
    bool prev_small = false;
    bool have_prev_gray = false;
    // keypoints (ping-pong: LK reads pts[pp], a re-detection writes pts[pp^1])
    int ncap = 0;
    // keypoint buffers: [0],[1] ping-pong per frame; batch mode cycles through all of them
    std::vector<float*> d_pts;
    std::vector<int32_t*> d_npts;
    std::vector<int> pts_cap;
    int pp = 0;
    int last_lk_pp = 0;
    float *d_next = nullptr, *d_err = nullptr, *d_vp = nullptr, *d_vc = nullptr;
    uint8_t *d_status = nullptr, *d_inliers = nullptr;
    int32_t *d_m = nullptr, *d_info = nullptr, *d_counts = nullptr;
    double* d_model = nullptr;
    void* d_gftt_scratch = nullptr;
    vsd::GfttWork gw;
    const vsd::RansacTables* tab = nullptr;
    vsd::TrajState* d_traj = nullptr;
    vsd::TrajParams tp;
    float* d_M = nullptr;               // [0..5] frame matrix, [6..11] chroma matrix
    double* d_Minv = nullptr;           // their inverse maps (what the warp kernels consume)
    vs_debug_frame* d_dbg = nullptr;
    int last_detect_pp = -1;            // buffer that holds the points detected on the last push
    bool last_detected = false;
    int last_gray_buf = 0;
    // scratch for border / host I/O
    uint8_t* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    uint8_t* d_fade = nullptr;          // borderType "fade": borderHistory_ (padded frame, packed rows)
    bool fade_valid = false;
    vsd::Canvas* canvas = nullptr;      // enableVirtualCanvas: temporal buffer and canvas geometry (outlive clean(), like the fade history)
    float* d_ct = nullptr;              // the correction (dx, dy, da) of the output being produced, for the canvas
    int fade_count = 0, fade_w = 0, fade_h = 0;     // fadeFrameCount_; geometry of the history
    uint8_t* d_padB = nullptr;          // batch mode with a border: one padded (or to-be-cropped) frame per frame of a batch
    size_t pad_frame_bytes = 0;
    // A YUV stream with crop-and-zoom, border pad or the fade border (at most one of them acts) has scratch surfaces in d_padB: the
    // format's packed default layout of border_plan's size at scratch_pitch, one per frame of a batch and one more (scratch_own)
    // for the per-frame path (scratch_planes, scratch_allocate).
    size_t scratch_pitch = 0;
    int scratch_own = 0;
    // crop-and-zoom (vs_stab_set_yuv_crop_zoom): the warps go into the scratch surfaces and one k_cropzoom launch resizes their
    // crops into the results
    bool yuv_cz = false;
    // border pad (vs_stab_set_yuv_border_pad): one k_yuvpad launch pads the planes of the frames into the scratch surfaces, which
    // the warps read under BORDER_REPLICATE
    bool yuv_pad = false, pad_fill_given = false;
    vs_yuv_fill pad_fill = {0, 0, 0, 0};        // the caller's; not given: the format's video black
    // edge fill (vs_stab_set_yuv_edge_fill): the warps of UNPADDED surfaces - the plain stream's, and the one into the scratch surface of
    // crop-and-zoom - read this colour outside the picture (VS_BORDER_FILL) where they otherwise read 0, which in YUV is green.
    // No buffer, no launch more: the mode picks other instances of the same warp kernels.
    bool yuv_efill = false, efill_given = false;
    vs_yuv_fill efill = {0, 0, 0, 0};           // the caller's; not given: the format's video black
    // the fade border (vs_stab_set_yuv_fade): one k_yuvfade launch pads the planes of a frame and blends them with the history
    // into the scratch surface, the warp reads that under BORDER_REPLICATE, and a second launch folds the result into the
    // history.  The history has the scratch surface's layout; like d_fade it outlives vs_stab_clean, so it remembers the geometry
    // it was made for.
    bool yuv_fade = false, yfade_fill_given = false, yfade_valid = false;
    vs_yuv_fill yfade_fill = {0, 0, 0, 0};
    uint8_t* d_yfade = nullptr;
    int yfade_count = 0, yfade_w = 0, yfade_h = 0, yfade_b = 0, yfade_fmt = -1;
    uint8_t* d_out = nullptr;
    size_t out_bytes = 0;
    // host pipeline (vs_stab_set_host_pipeline): the result of a call stays in d_hold[] and travels to the host during the
    // NEXT call, next to that call's upload and ahead of its analysis
    bool host_pipe = false, hold_valid = false;
    uint8_t* d_hold[2] = {nullptr, nullptr};
    int hold_cur = 0, hold_w = 0, hold_h = 0;
    hipEvent_t ev_hold = nullptr;
    std::unique_ptr<vsd::HostHelper> helper;     // issues the download when the caller's output buffer is pageable (push_host_pipelined)
    uint8_t* d_all = nullptr;           // one allocation for the small buffers
    vs_counters counters;
    // cross-stream dependencies
    hipEvent_t ev_gray[vsd::NPYR] = {}, ev_pre[vsd::NPYR] = {};
    hipEvent_t ev_lk[vsd::EVR] = {}, ev_det[vsd::EVR] = {};
    bool det_valid[vsd::EVR] = {false, false, false, false};
    hipEvent_t ev_first = nullptr;
    hipEvent_t ev_slot[vsd::FRAME_RING_MAX] = {};
    bool slot_valid[vsd::FRAME_RING_MAX] = {};
    int ring_frames = vsd::FRAME_RING;
    hipEvent_t pts_event[2] = {nullptr, nullptr};   // recorded by the detection that filled pts[i]
    bool pts_pending[2] = {false, false};
    // deferred output (vs_stab_set_warp_batch): warps of consecutive outputs wait for each other and
    // go out as ONE launch over up to WARP_BATCH_MAX frames, each into its caller's buffer
    int warp_batch = 1;
    struct PendWarp { const uint8_t* src; uint8_t* dst; int slot; };
    std::vector<PendWarp> pend;
    size_t pend_stride = 0;
    double* d_MinvB[2] = {nullptr, nullptr};   // inverse maps of the pending frames, 12 doubles each; two sets
    int32_t* d_tabs_def = nullptr;              // coordinate tables of a deferred warp launch
    int pend_set = 0;
    hipEvent_t ev_emit = nullptr, ev_warp[2] = {nullptr, nullptr};
    bool warp_valid[2] = {false, false};
    // batch mode (vs_stab_set_batch): a push only queues its frame (bq, batch_enqueue); the analysis, the ordered tail and the
    // warps of `batch` consecutive frames are issued together by the stream's schedule (`group`, batch_schedule.cpp), which
    // keeps the maps, tables and events of those warps - the deferred list above belongs to the per-frame pipeline.
    int batch = 1;
    bool batch_active = false;
    struct BFrame {
        int f, c, pv;
        const uint8_t* frame; bool prev_small;
        bool detect; int det_buf;
        int lk_buf, lk_cap;
        bool out_due; int out_slot, out_idx; const uint8_t* out_frame; uint8_t* d_out; size_t out_stride;
        int have_prev_gray;
    };
    std::vector<BFrame> bq;
    int kp_cur = 0, kp_next = 1;
    std::vector<vsd::GfttWork> gws;                  // one GFTT scratch per detection of a batch
    struct ItemBufs { float *next, *err, *vp, *vc; uint8_t *status, *inliers; int32_t *m, *info, *counts; double* model; };
    std::vector<ItemBufs> items;
    // what the debug getters read (last analysed frame)
    const float* dbg_prev_pts = nullptr; const float* dbg_next = nullptr;
    const uint8_t *dbg_status = nullptr, *dbg_inliers = nullptr;
    const float* dbg_det_pts = nullptr; const int32_t* dbg_det_n = nullptr;
    const int32_t* dbg_gftt_counters = nullptr;
    // stage profiling (HIP events on the stream the stage runs on)
    int prof_mode = 0;
    struct Pending { hipEvent_t a, b; int stage; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
};

namespace vsd {

// Stabilizer.cpp:383-389: a push lets the oldest queued frame go once the queue holds clamp(smoothingRadius, 5, 35) frames
// (the per-frame path, the batch schedule and the trajectory operator all ask here)
inline int effective_radius(int r) { return std::max(5, std::min(r, 35)); }
inline bool release_due(size_t queued, int host_radius) { return (int)queued >= effective_radius(host_radius); }
void fill_traj_params(const vs_params_c& p, TrajParams& t);


// Records an event pair around one stage when profiling is on.
struct StageScope {
    vs_stab* s;
    int stage;
    hipStream_t st;
    bool on = false;
    hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t get(vs_stab* s) {
        if (!s->ev_pool.empty()) { hipEvent_t e = s->ev_pool.back(); s->ev_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    StageScope(vs_stab* s_, int stage_, hipStream_t st_) : s(s_), stage(stage_), st(st_) {
        if (s->prof_mode == 2 || (s->prof_mode == 1 && stage == VS_STAGE_WARP) ||
            (s->prof_mode == 3 && (stage == VS_STAGE_WARP || stage == VS_STAGE_WARP_TABLES))) {
            a = get(s); b = get(s);
            if (a && b && hipEventRecord(a, st) == hipSuccess) on = true;
        }
    }
    ~StageScope() {
        if (on && hipEventRecord(b, st) == hipSuccess) s->pending.push_back({a, b, stage});
    }
};

// enableVirtualCanvas acts where the reference reaches it: not behind the crop-and-zoom returns (Stabilizer.cpp:1108-1127)
inline bool canvas_on(const vs_stab* s) { return s->p.enable_virtual_canvas && !s->p.crop_n_zoom; }

inline void out_size(const vs_stab* s, int w, int h, int* ow, int* oh) {
    const int b = s->p.border_size;
    if (canvas_on(s)) { *ow = w; *oh = h; return; }     // the canvas window has the size of the unpadded frame (:2121-2126)
    if (b > 0 && !s->p.crop_n_zoom) { *ow = w + 2 * b; *oh = h + 2 * b; return; }
    *ow = w; *oh = h;   // crop+zoom resizes back to origSize_ == frame size
}

// What border_size asks of a stream's warps.  pad (Stabilizer.cpp:981-990): the frame gets a border of b pixels and the padded
// frame (pw x ph, rows of prow bytes) is warped into a result of that size.  crop (:1108-1124, crop-and-zoom): the frame is
// warped at its own size into a scratch frame whose inner part, b pixels in, is resized to the result.  Neither: pw x ph = w x h.
struct BorderPlan {
    bool pad, crop;
    int b, pw, ph;
    size_t prow;
};
inline BorderPlan border_plan(const vs_stab* s) {
    BorderPlan bp;
    bp.b = s->p.border_size;
    bp.pad = bp.b > 0 && !s->p.crop_n_zoom;
    bp.crop = bp.b > 0 && s->p.crop_n_zoom && s->w - 2 * bp.b > 0 && s->h - 2 * bp.b > 0;
    bp.pw = bp.pad ? s->w + 2 * bp.b : s->w;
    bp.ph = bp.pad ? s->h + 2 * bp.b : s->h;
    bp.prow = (size_t)bp.pw * s->cn;
    return bp;
}

// Crop-and-zoom on a YUV stream: the mode is on, the parameters ask for it and the crop is not empty (an empty crop: the frame is
// only warped, as for BGR8).  Off, a YUV stream with a border never gets as far as its first allocation (pixfmt.h, check_input).
inline bool yuv_cz_on(const vs_stab* s) { return s->yuv_cz && s->pf->kind != PIX_INTERLEAVED && border_plan(s).crop; }

// Border pad on a YUV stream: the mode is on and the parameters ask for a pad of cv::copyMakeBorder's (not the fade).  Off, a YUV
// stream with a border never gets as far as its first allocation (pixfmt.h, check_input).
inline bool yuv_pad_wanted(const vs_stab* s) { return s->yuv_pad && !s->p.crop_n_zoom && s->p.border_size > 0 && s->p.border_type <= VS_BORDER_WRAP; }
inline bool yuv_pad_on(const vs_stab* s) { return yuv_pad_wanted(s) && s->pf->kind != PIX_INTERLEAVED; }
// The fade border on a YUV stream: the mode is on and the parameters ask for the fade.  (With the virtual canvas on as well the
// stream is refused at its first allocation: check_canvas.)
inline bool yuv_fade_wanted(const vs_stab* s) { return s->yuv_fade && !s->p.crop_n_zoom && s->p.border_size > 0 && s->p.border_type == VS_BORDER_FADE; }
inline bool yuv_fade_on(const vs_stab* s) { return yuv_fade_wanted(s) && s->pf->kind != PIX_INTERLEAVED; }
// Either of the two: the stream's warp reads a padded scratch surface and its result is padded
inline bool yuv_padded(const vs_stab* s) { return yuv_pad_on(s) || yuv_fade_on(s); }
inline vs_yuv_fill yuv_pad_fill(const vs_stab* s) { return s->pad_fill_given ? s->pad_fill : yuv_video_black(*s->pf); }
inline vs_yuv_fill yuv_fade_fill(const vs_stab* s) { return s->yfade_fill_given ? s->yfade_fill : yuv_video_black(*s->pf); }
// Edge fill on a YUV stream: the mode is on and the stream's warp reads an unpadded surface (border pad and fade keep their
// replicate-warp of the padded one: the mode does nothing there).
inline bool yuv_edge_fill_on(const vs_stab* s) { return s->yuv_efill && s->pf->kind != PIX_INTERLEAVED && !yuv_padded(s); }
inline vs_yuv_fill yuv_edge_fill(const vs_stab* s) { return s->efill_given ? s->efill : yuv_video_black(*s->pf); }

inline int build_pyramid(vs_stab* s, int k, hipStream_t st) {
    Pyramid& P = s->pyr[k];
    for (int l = 1; l <= s->levels; l++)
        VS_OBJ_TRY(s, launch_pyr_down(P.img[l - 1], s->lw[l - 1], s->lw[l - 1], s->lh[l - 1], P.img[l], s->lw[l], st));
    return VS_OK;
}

// The tracker's level table of a frame pair: pyramid ring slots pv (previous frame) and c (this frame)
inline void fill_lk_levels(const vs_stab* s, int pv, int c, LKLevel* L) {
    for (int l = 0; l <= s->levels; l++) {
        L[l].prev = s->pyr[pv].img[l]; L[l].next = s->pyr[c].img[l];
        L[l].w = s->lw[l]; L[l].h = s->lh[l]; L[l].stride = s->lw[l];
    }
}

// ---- the surfaces of a YUV stream as plane lists (planar_layout.h): the ONE place that says where their planes lie
// A queued frame.  The queue ring holds the packed default layout; the caller's layout (vs_stab_set_nv12_layout,
// vs_stab_set_i420_layout) applies to zero-copy input.
inline Planes queued_planes(const vs_stab* s) { return planes(*s->pf, s->w, s->h, s->src_pitch, s->zero_copy ? s->in : ChromaLayout()); }
// A scratch surface (crop-and-zoom: the frame's size; border pad and fade: the padded size), and surface `idx`
inline Planes scratch_planes(const vs_stab* s) { const BorderPlan bp = border_plan(s); return planes(*s->pf, bp.pw, bp.ph, s->scratch_pitch); }
inline uint8_t* scratch(const vs_stab* s, int idx) { return s->d_padB + (size_t)idx * s->pad_frame_bytes; }
// A result: a device surface in the caller's output layout, or the staging of the host entry points (s->d_out), which holds the
// packed default layout.  The padded size, and offsets counted from it, where the result is padded.
inline Planes result_planes(const vs_stab* s, const uint8_t* d_out, size_t out_stride) {
    const bool pad = yuv_padded(s);
    return planes(*s->pf, pad ? border_plan(s).pw : s->w, pad ? border_plan(s).ph : s->h, out_stride, d_out != s->d_out ? s->out : ChromaLayout());
}
// What the warp of a YUV stream reads (the padded scratch surface, or the queued frame) and fills (the scratch surface whose crop
// is zoomed into the result, or the result)
inline Planes warp_src_planes(const vs_stab* s) { return yuv_padded(s) ? scratch_planes(s) : queued_planes(s); }
inline Planes warp_dst_planes(const vs_stab* s, const uint8_t* d_out, size_t out_stride) {
    return yuv_cz_on(s) ? scratch_planes(s) : result_planes(s, d_out, out_stride);
}

// The border of a YUV stream's warp, for the per-frame path and the batch schedule alike - the ONE place that chooses it: the edge
// of a padded scratch surface is its border (border pad, fade); an unpadded surface has zeros around it, or with edge fill the
// stream's fill colour.
// (The batch schedule issues a step's warps WARP_LAG steps after it queued their frames and asks here when it issues them.  The
// answer is still the one the frames were queued under: the setters of these modes take effect only while the frame queue is
// empty, and a queue only empties through a flush or a clean, which issue every pending warp first.)
struct YuvBorder { int border; WarpFill fill; };
inline YuvBorder yuv_warp_border(const vs_stab* s) {
    if (yuv_padded(s)) return {VS_BORDER_REPLICATE, WarpFill()};
    if (!yuv_edge_fill_on(s)) return {VS_BORDER_BLACK, WarpFill()};
    const vs_yuv_fill c = yuv_edge_fill(s);
    WarpFill f;
    f.y = c.y; f.u = c.u; f.v = c.v;
    return {VS_BORDER_FILL, f};
}

// (the warp itself: warp_planes, launchers.h)

// The zoom of n warped scratch surfaces into their results (device surfaces in the caller's output layout, or the staging of the
// host entry points): ONE k_cropzoom launch over all their planes (stabilizer.cpp)
int cz_launch(const vs_stab* s, const uint8_t* const* scratch, uint8_t* const* outs, int n, size_t out_stride, hipStream_t st);
// The pad of n frames (in the stream's input layout) into their scratch surfaces: ONE k_yuvpad launch over all their planes (stabilizer.cpp)
int pad_launch(const vs_stab* s, const uint8_t* const* frames, uint8_t* const* scratch, int n, hipStream_t st);
// ... the same with the border mode and the fill given (the first history of the fade border: VS_BORDER_BLACK with the fade's fill)
int pad_planes(const vs_stab* s, const uint8_t* const* frames, uint8_t* const* scratch, int n, int border, const vs_yuv_fill& c, hipStream_t st);

// A ring slot goes back to the free list behind the work on `st` that reads it.  A slot whose event cannot be recorded stays out
// of the ring: its next writer would have nothing to wait for.
inline int release_slot(vs_stab* s, int slot, hipStream_t st) {
    if (slot < 0) return VS_OK;          // zero-copy: the frame is the caller's
    VS_HIP_TRY(hipEventRecord(s->ev_slot[slot], st));
    s->slot_valid[slot] = true;
    s->free_slots.push_back(slot);
    return VS_OK;
}

// Waits for the streams of an object, in the order given (streams it does not have yet are skipped).  Every stream is waited
// for, whatever the ones before it answered; the first error is returned for the caller to report or to ignore.
inline hipError_t sync_streams(std::initializer_list<hipStream_t> streams) {
    hipError_t first = hipSuccess;
    for (hipStream_t st : streams) {
        const hipError_t e = st ? hipStreamSynchronize(st) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

}  // namespace vsd
#endif
