// vs_stab_*: one video stream = the device-resident mirror of vs::Stabilizer
// (/root/reference/include/video/Stabilizer.h:70-198, src/Stabilizer.cpp:50-1172).
//
// The host side only keeps what is decidable without looking at pixels: the
// frame queue bookkeeping (which ring slot holds which frame index, when the
// warm-up ends, on which frames features are re-detected).  Everything that
// depends on image content stays on the GPU between kernels: keypoints and
// their count, LK status, the RANSAC model, the trajectory history and the
// warp matrix.  A steady-state stabilize() is a fixed set of asynchronous
// launches with no host synchronisation, spread over three HIP streams so that
// independent work of consecutive frames overlaps:
//
//   pre   : copy-in -> resize+gray -> pyramid + Scharr      (frame k+1 ...)
//   det   : goodFeaturesToTrack on the new gray image        (frame k, every 2nd)
//   main  : LK -> RANSAC+append -> trajectory emit -> warp   (... while frame k tracks)
//
// Cross-stream order is expressed with events only where data demands it
// (pyramid ready, keypoints ready, buffer no longer read).  Pyramids are
// triple-buffered and the frame ring has spare slots so that `pre` of the next
// frame never waits for `main` of the current one.
//
// Batch mode (vs_stab_set_batch, device entry points): the same decisions are taken per
// push, but the device work of `batch` consecutive frames is issued together - one
// launch per stage over all frames (argument tables in device memory), one ordered
// tail kernel (selection + trajectory append + smoothing, state in LDS), one warp
// launch for the frames of a batch.  This file only queues the frames (batch_enqueue); there is ONE
// batch schedule, group_run() in batch_schedule.cpp: a vs_batch group runs it over the frames of all
// its streams, and a standalone instance in batch mode owns a private group of one.  The stream
// object itself is in stab_internal.h; DESIGN.md section 5 has the schedule.
#include <array>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <new>

#include "stab_internal.h"

using namespace vsd;

namespace {

// A refusal of the rules (pixfmt.h) becomes the stream's error.
#define VS_REFUSE(s, expr) do { const Refusal r_ = (expr); if (r_.rc != VS_OK) return vs_obj_fail((s), r_.rc, r_.text); } while (0)

// A stream of a vs_batch is driven by its group (which sets group_call around the vs_stab_* calls it makes on a member).
#define VS_CALLER_DRIVES(s) do { if ((s)->member && !(s)->group_call) return vs_obj_fail((s), VS_ERR_INVALID_ARG, \
    "this stream belongs to a vs_batch: drive it through vs_batch_* (its getters remain available)"); } while (0)

int flush_warps(vs_stab* s);

// Batch mode: everything queued so far is analysed and its warps are issued (nothing stays deferred).
int drain_batch(vs_stab* s) {
    if (!s->group) return VS_OK;
    const int rc = group_drain(s->group);
    if (rc != VS_OK) s->err = get_last_error();
    return rc;
}

int sync_all(vs_stab* s) {
    VS_OBJ_HIP(s, hipSetDevice(s->device));
    VS_OBJ_TRY(s, drain_batch(s));
    VS_OBJ_TRY(s, flush_warps(s));
    VS_OBJ_HIP(s, sync_streams({s->st_warp, s->st_pre, s->st_det, s->st}));
    return VS_OK;
}

// Whatever the streams hold, failed or not, has run (before buffers go).
void wait_streams(vs_stab* s) {
    (void)hipSetDevice(s->device);
    (void)sync_streams({s->st_pre, s->st_det, s->st, s->st_warp});
}

void free_all(vs_stab* s) {
    if (s->d_ring) (void)hipFree(s->d_ring);
    if (s->d_all) (void)hipFree(s->d_all);
    if (s->d_gftt_scratch) (void)hipFree(s->d_gftt_scratch);
    if (s->d_tmp) (void)hipFree(s->d_tmp);
    if (s->d_padB) (void)hipFree(s->d_padB);
    s->d_padB = nullptr;
    s->scratch_pitch = 0;
    if (s->own) {                       // the private schedule goes with the buffers it was sized for
        group_delete(s->own);
        s->own = nullptr; s->group = nullptr;
    }
    // (d_fade, the fade history, outlives vs_stab_clean like borderHistory_ outlives Stabilizer::clean())
    if (s->d_out) (void)hipFree(s->d_out);
    for (auto& h : s->d_hold) { if (h) (void)hipFree(h); h = nullptr; }
    s->hold_valid = false;
    s->d_ring = s->d_all = s->d_tmp = s->d_out = nullptr;
    s->d_gftt_scratch = nullptr;
    s->allocated = false;
}

void analysis_size(const vs_stab* s, int w, int h, int* aw, int* ah) {
    *aw = 960; *ah = 540;                                  // Stabilizer.cpp:410
    if (s->p.drone_high_freq_mode) {                       // :2447-2466
        int maxWidth = std::min(s->p.hf_analysis_max_width, w);
        float aspect = (float)h / (float)w;
        int height = (int)(maxWidth * aspect);
        *aw = (maxWidth / 2) * 2;
        *ah = (height / 2) * 2;
    }
}

int allocate_buffers(vs_stab* s, int w, int h, int fmt);

// The scratch surfaces of a YUV stream (only with crop-and-zoom, border pad or the fade border on): the packed default layout of
// border_plan's size - the frame's for crop-and-zoom, the PADDED one otherwise - at a pitch of whole 256-byte lines (aligned stores
// and loads for the warps, 16-byte stores for the pad, whatever w is); one per frame of a batch, and one for the per-frame path
// (the frames a flush hands out while the last step's warps may still run).
int scratch_allocate(vs_stab* s) {
    const BorderPlan bp = border_plan(s);
    s->scratch_pitch = (bp.prow + 255) & ~(size_t)255;
    s->pad_frame_bytes = s->scratch_pitch * (size_t)s->pf->rows(bp.ph);
    s->scratch_own = s->batch_active ? s->batch : 0;
    VS_OBJ_HIP(s, hipMalloc((void**)&s->d_padB, s->pad_frame_bytes * (size_t)(s->scratch_own + 1)));
    return VS_OK;
}

// A failure half way leaves nothing behind: the next push starts from scratch instead of overwriting live pointers.
int allocate(vs_stab* s, int w, int h, int fmt) {
    const int rc = allocate_buffers(s, w, h, fmt);
    if (rc != VS_OK) {
        if (s->st) (void)hipStreamSynchronize(s->st);
        free_all(s);
    }
    return rc;
}

int allocate_buffers(vs_stab* s, int w, int h, int fmt) {
    const PixFmt& f = *pixfmt(fmt);      // (prepare() has refused anything else)
    s->w = w; s->h = h; s->fmt = fmt; s->pf = &f;
    s->cn = f.cn;
    s->rows_total = f.rows(h);
    s->row_bytes = (size_t)w * s->cn;
    s->frame_bytes = s->row_bytes * s->rows_total;
    s->src_pitch = s->row_bytes;
    // the chroma matrix that goes with the frame matrix (traj_matrix_lane): by the subsampling of the stream's chroma planes
    s->tp.chroma = !f.three_planes() || f.sy ? TRAJ_CHROMA_420 : f.sx ? TRAJ_CHROMA_422 : TRAJ_CHROMA_444;
    analysis_size(s, w, h, &s->aw, &s->ah);
    if (s->aw < 3 || s->ah < 3) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "analysis size too small");
    VS_REFUSE(s, check_canvas(f, canvas_on(s)));
    // buildOpticalFlowPyramid: levels that fit the window
    {
        int sw = s->aw, sh = s->ah;
        for (int level = 0; level <= s->p.lk_max_level; level++) {
            s->lw[level] = sw; s->lh[level] = sh;
            s->levels = level;
            sw = (sw + 1) / 2; sh = (sh + 1) / 2;
            if (sw <= s->p.lk_win_size || sh <= s->p.lk_win_size) break;
        }
    }
    // (adaptive smoothing stays with the per-frame pipeline: whether a push produces a frame then depends on the data - the
    // radius moves the warm-up threshold, Stabilizer.cpp:383,1482-1486 - and a push answers that at once)
    // (so does borderType "fade": each output is blended with a history the output before it has just updated)
    const bool fade = s->p.border_type == VS_BORDER_FADE && s->p.border_size > 0 && !s->p.crop_n_zoom;
    // (and the virtual canvas: the window offset and the temporal fill are host decisions on each output's correction)
    s->batch_active = s->batch > 1 && !s->p.adaptive_smoothing && !fade && !canvas_on(s);
    const int B = s->batch_active ? s->batch : 1;
    s->npyr = s->batch_active ? batch_pyr_slots(B) : NPYR;
    // keypoint buffers: one per detection, recycled after two batches' worth of detections
    const int nkp = s->batch_active ? B + 4 : 2, ngw = s->batch_active ? B / 2 + 1 : 1;
    s->pyr.assign(s->npyr, Pyramid());
    s->d_pts.assign(nkp, nullptr); s->d_npts.assign(nkp, nullptr); s->pts_cap.assign(nkp, 0);
    s->items.assign(B, vs_stab::ItemBufs());
    s->bq.clear(); s->kp_cur = 0; s->kp_next = 1;
    if (s->batch_active && !s->group) {            // a standalone instance: a group of one runs its batches
        s->own = group_new_own(s);
        if (!s->own) return vs_obj_fail(s, VS_ERR_HIP, get_last_error());
        s->group = s->own;
    }
    // (the frame queue ring - 128 frames and more, 3.2 GB at 4K BGR8 - is allocated by the first push that copies a frame in: a
    // stream that only ever hands over device frames in zero-copy mode never needs it)
    s->free_slots.clear();
    s->ring_frames = s->batch_active ? batch_ring_frames(B) : FRAME_RING;      // (batch mode: WARP_LAG more steps of frames wait for their warps)
    for (int i = 0; i < s->ring_frames; i++) { s->free_slots.push_back(i); s->slot_valid[i] = false; }
    s->ncap = std::max(s->p.max_corners, 1);
    const int ncap = s->ncap;
    // carve the small buffers out of one allocation (256-byte aligned pieces)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    size_t o_first = take((size_t)480 * 270);
    std::vector<std::array<size_t, MAX_PYR>> o_img(s->npyr);
    for (int k = 0; k < s->npyr; k++)
        for (int l = 0; l <= s->levels; l++) o_img[k][l] = take((size_t)s->lw[l] * s->lh[l]);
    std::vector<size_t> o_pts(nkp), o_npts(nkp);
    for (int k = 0; k < nkp; k++) { o_pts[k] = take((size_t)ncap * 8); o_npts[k] = take(16); }
    struct ItemOff { size_t next, err, vp, vc, status, inl, m, info, counts, model; };
    std::vector<ItemOff> o_it(B);
    for (int k = 0; k < B; k++) {
        o_it[k].next = take((size_t)ncap * 8); o_it[k].err = take((size_t)ncap * 4);
        o_it[k].vp = take((size_t)ncap * 8); o_it[k].vc = take((size_t)ncap * 8);
        o_it[k].status = take(ncap); o_it[k].inl = take(ncap);
        o_it[k].m = take(16); o_it[k].info = take(16); o_it[k].counts = take((size_t)s->p.ransac_max_iters * 4);
        o_it[k].model = take(48);
    }
    size_t o_traj = take(sizeof(TrajState)), o_M = take(96), o_Minv = take(96), o_dbg = take(sizeof(vs_debug_frame));
    size_t o_MinvB[2] = {take((size_t)BATCH_MAX * 96), take((size_t)BATCH_MAX * 96)};
    int tow, toh;
    out_size(s, w, h, &tow, &toh);
    const size_t o_tabs = take(warp_tabs_ints(std::max(w, tow), std::max(h, toh), WARP_BATCH_MAX) * sizeof(int32_t));
    VS_OBJ_HIP(s, hipMalloc((void**)&s->d_all, off));
    VS_OBJ_HIP(s, hipMemsetAsync(s->d_all, 0, off, s->st));
    uint8_t* b = s->d_all;
    s->d_first_gray = b + o_first;
    for (int k = 0; k < s->npyr; k++)
        for (int l = 0; l <= s->levels; l++) s->pyr[k].img[l] = b + o_img[k][l];
    for (int k = 0; k < nkp; k++) { s->d_pts[k] = (float*)(b + o_pts[k]); s->d_npts[k] = (int32_t*)(b + o_npts[k]); }
    for (int k = 0; k < B; k++) {
        vs_stab::ItemBufs& it = s->items[k];
        it.next = (float*)(b + o_it[k].next); it.err = (float*)(b + o_it[k].err);
        it.vp = (float*)(b + o_it[k].vp); it.vc = (float*)(b + o_it[k].vc);
        it.status = b + o_it[k].status; it.inliers = b + o_it[k].inl;
        it.m = (int32_t*)(b + o_it[k].m); it.info = (int32_t*)(b + o_it[k].info); it.counts = (int32_t*)(b + o_it[k].counts);
        it.model = (double*)(b + o_it[k].model);
    }
    // the per-frame path works on item 0
    s->d_next = s->items[0].next; s->d_err = s->items[0].err; s->d_vp = s->items[0].vp; s->d_vc = s->items[0].vc;
    s->d_status = s->items[0].status; s->d_inliers = s->items[0].inliers;
    s->d_m = s->items[0].m; s->d_info = s->items[0].info; s->d_counts = s->items[0].counts; s->d_model = s->items[0].model;
    s->d_traj = (TrajState*)(b + o_traj);
    s->d_M = (float*)(b + o_M); s->d_Minv = (double*)(b + o_Minv); s->d_dbg = (vs_debug_frame*)(b + o_dbg);
    s->d_MinvB[0] = (double*)(b + o_MinvB[0]); s->d_MinvB[1] = (double*)(b + o_MinvB[1]);
    s->d_tabs_def = (int32_t*)(b + o_tabs);
    s->pend.clear(); s->pend_set = 0; s->warp_valid[0] = s->warp_valid[1] = false;
    // GFTT scratch sized for the larger of the two detection images
    const int gmaxw = std::max(s->aw, 480), gmaxh = std::max(s->ah, 270);
    const int cap = gftt_cand_cap(gmaxw, gmaxh);
    const size_t gwb = (gftt_work_bytes(gmaxw, gmaxh, cap) + 255) & ~(size_t)255;
    VS_OBJ_HIP(s, hipMalloc(&s->d_gftt_scratch, gwb * ngw));
    s->gws.assign(ngw, GfttWork());
    for (int k = 0; k < ngw; k++) gftt_work_carve((uint8_t*)s->d_gftt_scratch + gwb * k, gmaxw, gmaxh, cap, &s->gws[k]);
    s->gw = s->gws[0];
    s->dbg_gftt_counters = s->gw.counters;
    VS_OBJ_TRY(s, get_ransac_tables(ncap, s->p.ransac_max_iters, &s->tab));
    int ow, oh;
    out_size(s, w, h, &ow, &oh);
    s->out_bytes = (size_t)ow * s->cn * f.rows(oh);
    VS_OBJ_HIP(s, hipMalloc((void**)&s->d_out, s->out_bytes));
    s->tmp_bytes = std::max(s->out_bytes, s->frame_bytes);
    VS_OBJ_HIP(s, hipMalloc((void**)&s->d_tmp, s->tmp_bytes + 16));
    if (yuv_cz_on(s) || yuv_padded(s)) {
        VS_OBJ_TRY(s, scratch_allocate(s));
    } else if (s->batch_active && s->p.border_size > 0) {
        s->pad_frame_bytes = (s->tmp_bytes + 255) & ~(size_t)255;
        VS_OBJ_HIP(s, hipMalloc((void**)&s->d_padB, s->pad_frame_bytes * B));
    }
    VS_OBJ_TRY(s, launch_traj_reset(s->d_traj, s->p.smoothing_radius, s->st));
    // the zero-fill and the reset ran on `main`; nothing may touch the buffers before that
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st));
    for (int i = 0; i < EVR; i++) s->det_valid[i] = false;
    s->pts_pending[0] = s->pts_pending[1] = false;
    s->allocated = true;
    return VS_OK;
}


// The result of a host call from its staging buffer (rows of `orow` bytes, `orows` of them; three planes: the packed layout at that
// pitch) into the caller's frame.  rw x rh: the size of the frame delivered (vs_stab_last_out_dims), which a YUV stream goes by: a
// padded result, or the unpadded last frame of a flush with the default offsets of ITS size.
int download_result(vs_stab* s, uint8_t* out, size_t out_stride, const uint8_t* d_src, size_t orow, int orows, hipStream_t st, int rw, int rh) {
    const bool pad = yuv_padded(s);     // (luma and UV plane lie behind each other: one copy)
    if (s->pf->three_planes()) VS_OBJ_HIP(s, copy_planes(out, planes(*s->pf, rw, rh, out_stride), d_src, planes(*s->pf, rw, rh, orow), hipMemcpyDeviceToHost, st));
    else VS_OBJ_HIP(s, hipMemcpy2DAsync(out, out_stride, d_src, orow, pad ? (size_t)rw * s->cn : orow, pad ? s->pf->rows(rh) : orows, hipMemcpyDeviceToHost, st));
    return VS_OK;
}

// `pre` stream, part 1: the frame enters the queue ring (waits until the slot's last reader is done)
int enqueue_copy_in(vs_stab* s, int slot, const void* src, size_t stride, hipMemcpyKind kind) {
    if (s->slot_valid[slot]) VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_pre, s->ev_slot[slot], 0));
    StageScope t(s, VS_STAGE_COPY_IN, s->st_pre);
    uint8_t* dst = s->d_ring + (size_t)slot * s->frame_bytes;
    // plane by plane into the slot's packed layout: three planes, from the caller's layout (device surfaces) or the packed default
    // at the caller's pitch (host frames), and a decoder's NV12 / P010 surface whose planes lie apart; anything else is ONE copy
    const ChromaLayout in = kind == hipMemcpyDeviceToDevice ? s->in : ChromaLayout();
    if (s->pf->three_planes() || (s->pf->luma_uv() && in.uv_off))
        VS_OBJ_HIP(s, copy_planes(dst, planes(*s->pf, s->w, s->h, s->row_bytes), (const uint8_t*)src, planes(*s->pf, s->w, s->h, stride, in), kind, s->st_pre));
    else VS_OBJ_HIP(s, hipMemcpy2DAsync(dst, s->row_bytes, src, stride, s->row_bytes, s->rows_total, kind, s->st_pre));
    return VS_OK;
}

// generateTransform (Stabilizer.cpp:402-761) for frame index f >= 1 held in `d_frame`
int generate_transform(vs_stab* s, const uint8_t* d_frame, int f) {
    const vs_params_c& p = s->p;
    const int c = f % NPYR, pv = (f - 1) % NPYR;
    // ---- pre: gray + pyramid into buffer c.  Its previous readers were LK(f-2) (as "prev")
    // and, if frame f-3 re-detected, the detector.
    if (f - 2 >= 1) VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_pre, s->ev_lk[(f - 2) % EVR], 0));
    if (f - 3 >= 1 && s->det_valid[(f - 3) % EVR]) VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_pre, s->ev_det[(f - 3) % EVR], 0));
    {
        StageScope t(s, VS_STAGE_GRAY, s->st_pre);
        VS_OBJ_TRY(s, launch_resize_gray(d_frame, s->src_pitch, s->w, s->h, s->pf->gray_source, s->pyr[c].img[0], s->aw, s->aw, s->ah, s->st_pre));  // :448-450
    }
    VS_OBJ_HIP(s, hipEventRecord(s->ev_gray[c], s->st_pre));
    {
        StageScope t(s, VS_STAGE_PYRAMID, s->st_pre);
        VS_OBJ_TRY(s, build_pyramid(s, c, s->st_pre));
        if (s->prev_small) {   // :598-603 (once: 480x270 -> analysis size)
            VS_OBJ_TRY(s, launch_resize_gray(s->d_first_gray, 480, 480, 270, VS_FMT_GRAY8, s->pyr[pv].img[0], s->aw, s->aw, s->ah, s->st_pre));
            VS_OBJ_TRY(s, build_pyramid(s, pv, s->st_pre));
            s->prev_small = false;
        }
    }
    VS_OBJ_HIP(s, hipEventRecord(s->ev_pre[c], s->st_pre));

    // ---- det: every second call re-detects on the new gray image (:696-746).  Needs only
    // img[0]; its output buffer pts[pp^1] was last read by LK(f-2), which `pre` waited for.
    const int pp = s->pp;
    s->last_detected = false;
    s->det_valid[f % EVR] = false;
    int next_pp = pp;
    if ((++s->detect_counter % 2) == 0) {
        const int q = pp ^ 1;
        const int mc = std::min(p.max_corners, 200);
        VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_det, s->ev_gray[c], 0));
        {
            StageScope t(s, VS_STAGE_GFTT, s->st_det);
            VS_OBJ_TRY(s, launch_gftt(s->pyr[c].img[0], s->aw, s->aw, s->ah, mc, 0.02, 15.0, 3, s->gw, s->d_pts[q],
                                 s->d_npts[q], s->st_det));
        }
        VS_OBJ_HIP(s, hipEventRecord(s->ev_det[f % EVR], s->st_det));
        s->det_valid[f % EVR] = true;
        s->pts_event[q] = s->ev_det[f % EVR];
        s->pts_pending[q] = true;
        s->pts_cap[q] = mc;
        next_pp = q;
        s->last_detected = true;
        s->last_detect_pp = q;
        s->dbg_det_pts = s->d_pts[q]; s->dbg_det_n = s->d_npts[q];
        s->counters.detections++;
    }

    // ---- main: LK needs this frame's pyramid and the keypoints of the last detection
    VS_OBJ_HIP(s, hipStreamWaitEvent(s->st, s->ev_pre[c], 0));
    if (s->pts_pending[pp]) {
        VS_OBJ_HIP(s, hipStreamWaitEvent(s->st, s->pts_event[pp], 0));
        s->pts_pending[pp] = false;
    }
    LKLevel L[MAX_PYR];
    fill_lk_levels(s, pv, c, L);
    const int cap = s->pts_cap[pp];
    {
        StageScope t(s, VS_STAGE_LK, s->st);
        VS_OBJ_TRY(s, launch_pyr_lk(L, s->levels, s->d_pts[pp], cap, s->d_npts[pp], s->d_next, s->d_status, s->d_err,
                               p.lk_win_size, p.lk_max_iters, p.lk_epsilon, s->st));   // :611-619
    }
    s->last_lk_pp = pp;
    if (s->dbg_delay_us > 0) VS_OBJ_TRY(s, launch_spin(s->dbg_delay_us, s->st));        // test hook: widen the window between LK and RANSAC
    {
        // status compaction (:629-641) + estimateAffinePartial2D (:644-659) + transform append (:660-693)
        StageScope t(s, VS_STAGE_RANSAC, s->st);
        VS_OBJ_TRY(s, launch_ransac(s->d_pts[pp], s->d_next, s->d_status, std::max(cap, 0), s->d_npts[pp], s->d_vp, s->d_vc,
                               s->d_m, 4, p.ransac_threshold, p.ransac_max_iters, s->tab, s->d_counts, s->d_model,
                               s->d_inliers, s->d_info, s->d_traj, &s->tp, s->d_dbg, s->have_prev_gray ? 1 : 0, s->st));
    }
    // `pre` (pyramid buffers) and `det` (keypoint buffer pts[pp^1] two frames on) wait for this event: the tracker AND the
    // scoring / selection kernels have read pts[pp] and its count by then (recorded right behind the tracker, a re-detection
    // two frames later could overwrite the buffer under the RANSAC kernels)
    VS_OBJ_HIP(s, hipEventRecord(s->ev_lk[f % EVR], s->st));
    s->dbg_prev_pts = s->d_pts[pp]; s->dbg_next = s->d_next; s->dbg_status = s->d_status; s->dbg_inliers = s->d_inliers;
    s->n_transforms++;
    s->pp = next_pp;
    s->last_gray_buf = c;
    s->have_prev_gray = true;                                                         // :757-759
    return VS_OK;
}

// One launch for all pending warps of the per-frame pipeline; releases their ring slots.  On the high-priority warp
// stream, so that the analysis of the next frames is not held up.
int flush_warps(vs_stab* s) {
    if (s->pend.empty()) return VS_OK;
    hipStream_t ws = s->st_warp;
    const int n = (int)s->pend.size(), set = s->pend_set;
    const uint8_t* srcs[WARP_BATCH_MAX];
    uint8_t* dsts[WARP_BATCH_MAX];
    for (int i = 0; i < n; i++) { srcs[i] = s->pend[i].src; dsts[i] = s->pend[i].dst; }
    VS_OBJ_HIP(s, hipEventRecord(s->ev_emit, s->st));             // the maps of this batch are written on `main`
    VS_OBJ_HIP(s, hipStreamWaitEvent(ws, s->ev_emit, 0));
    int rc;
    {
        StageScope t(s, VS_STAGE_WARP, ws);
        rc = launch_warp_plane(srcs, dsts, n, s->src_pitch, s->w, s->h, s->pend_stride, s->w, s->h, s->cn, WarpMaps{s->d_MinvB[set], 12, false},
                               VS_BORDER_BLACK, WarpTabs{WarpTabs::CALLER, s->d_tabs_def}, ws);
    }
    const hipError_t ew = hipEventRecord(s->ev_warp[set], ws);
    if (ew == hipSuccess) s->warp_valid[set] = true;
    else if (rc == VS_OK) rc = hip_fail(ew, "hipEventRecord(s->ev_warp[set], ws)");
    for (int i = 0; i < n; i++) {
        const int rrc = release_slot(s, s->pend[i].slot, ws);
        if (rc == VS_OK) rc = rrc;
    }
    s->pend.clear();
    s->pend_set = set ^ 1;
    if (rc != VS_OK) { s->err = get_last_error(); return rc; }
    return VS_OK;
}

// Deferred output: only the map of output `idx` is computed now (on `main`, in trajectory order); its warp
// joins the next batched launch.
int defer_output(vs_stab* s, int idx, const uint8_t* frame, uint8_t* d_out, size_t out_stride, int slot) {
    hipStream_t st = s->st;
    if (!s->pend.empty() && s->pend_stride != out_stride) VS_OBJ_TRY(s, flush_warps(s));
    const int set = s->pend_set, j = (int)s->pend.size();
    if (j == 0 && s->warp_valid[set]) {      // the previous user of this set of maps must have read them
        VS_OBJ_HIP(s, hipStreamWaitEvent(st, s->ev_warp[set], 0));
        s->warp_valid[set] = false;
    }
    {
        StageScope t(s, VS_STAGE_TRAJ, st);
        VS_OBJ_TRY(s, launch_traj_emit(s->d_traj, s->tp, idx, s->d_M, s->d_MinvB[set] + 12 * j, s->d_dbg, st));
    }
    s->pend.push_back({frame, d_out, slot});
    s->pend_stride = out_stride;
    if ((int)s->pend.size() >= s->warp_batch) VS_OBJ_TRY(s, flush_warps(s));
    return VS_OK;
}

// One frame of the stream's channels by its current map (d_Minv), w x h in and out
int warp_frame(const vs_stab* s, const uint8_t* src, size_t sstride, int w, int h, uint8_t* dst, size_t dstride, hipStream_t st) {
    return launch_warp_plane(&src, &dst, 1, sstride, w, h, dstride, w, h, s->cn, WarpMaps{s->d_Minv, 6, false}, VS_BORDER_BLACK, WarpTabs{}, st);
}

// The fade border on a YUV stream, in front of the warp (Stabilizer.cpp:914-978 per plane): the first padded frame is the history
// (:917-926; also after a change of geometry or format, and after vs_stab_set_yuv_fade), alpha ramps with the count (:953-961), and
// ONE k_yuvfade launch pads the planes of `frame` and blends them with the history into the scratch surface `psrc`.
int yuv_fade_blend(vs_stab* s, const uint8_t* frame, uint8_t* psrc, hipStream_t st) {
    const vs_params_c& p = s->p;
    const int b = p.border_size, w = s->w, h = s->h;
    if (!s->d_yfade || s->yfade_w != w || s->yfade_h != h || s->yfade_b != b || s->yfade_fmt != s->fmt) {
        if (s->d_yfade) { (void)hipStreamSynchronize(st); (void)hipFree(s->d_yfade); s->d_yfade = nullptr; }
        VS_OBJ_HIP(s, hipMalloc((void**)&s->d_yfade, s->pad_frame_bytes));
        s->yfade_w = w; s->yfade_h = h; s->yfade_b = b; s->yfade_fmt = s->fmt; s->yfade_valid = false;
    }
    const vs_yuv_fill c = yuv_fade_fill(s);
    if (!s->yfade_valid) {
        VS_OBJ_TRY(s, pad_planes(s, &frame, &s->d_yfade, 1, VS_BORDER_BLACK, c, st));
        s->yfade_valid = true; s->yfade_count = 0;
    }
    float alpha = p.fade_alpha;
    if (s->yfade_count < p.fade_duration) {
        alpha = alpha * (static_cast<float>(s->yfade_count) / p.fade_duration);
        s->yfade_count++;
    }
    const Planes S = queued_planes(s), D = scratch_planes(s);       // (the history has the scratch surface's planes)
    vs_fade_job jobs[3];
    for (int k = 0; k < S.n; k++)
        jobs[k] = vs_fade_job{frame + S[k].off, S[k].pitch, S[k].w, S[k].h, s->d_yfade + D[k].off, D[k].pitch, psrc + D[k].off, D[k].pitch,
                              b >> S[k].sx, b >> S[k].sy, {plane_fill(c, S, k, 0), plane_fill(c, S, k, 1)}, S[k].cn, 0};
    VS_OBJ_TRY(s, launch_yuvfade_blend(jobs, S.n, S.sample_bytes, alpha, 1.0f - alpha, st));
    return VS_OK;
}

// ... and behind it (:1086-1100 per plane): ONE launch folds the planes of the result, read through the output layout, into the history
int yuv_fade_update(vs_stab* s, const uint8_t* d_out, size_t out_stride, hipStream_t st) {
    const Planes H = scratch_planes(s), D = result_planes(s, d_out, out_stride);
    vs_fade_update_job jobs[3];
    for (int k = 0; k < H.n; k++)
        jobs[k] = vs_fade_update_job{s->d_yfade + H[k].off, H[k].pitch, d_out + D[k].off, D[k].pitch, H[k].w, H[k].h, H[k].cn, 0};
    VS_OBJ_TRY(s, launch_yuvfade_update(jobs, H.n, H.sample_bytes, st));
    return VS_OK;
}

// applyNextSmoothTransform (Stabilizer.cpp:763-1137) into d_out (device), on `main`
int apply_next(vs_stab* s, uint8_t* d_out, size_t out_stride, bool may_defer) {
    const vs_params_c& p = s->p;
    const int slot = s->q_slot.front(), idx = s->q_idx.front();
    const uint8_t* frame = s->q_ptr.front();
    s->q_slot.pop_front(); s->q_idx.pop_front(); s->q_ptr.pop_front();
    hipStream_t st = s->st;
    int ow, oh;
    out_size(s, s->w, s->h, &ow, &oh);
    s->last_out_w = ow; s->last_out_h = oh;
    const bool plain = idx < s->n_transforms && s->pf->kind == PIX_INTERLEAVED && p.border_size <= 0 && !canvas_on(s);
    const BorderPlan bp = border_plan(s);
    if (may_defer && plain && s->warp_batch > 1) {
        VS_OBJ_TRY(s, defer_output(s, idx, frame, d_out, out_stride, slot));
        s->counters.frames_out++;
        return VS_OK;
    }
    {
        StageScope t(s, VS_STAGE_TRAJ, st);
        if (canvas_on(s) && !s->d_ct) VS_OBJ_HIP(s, hipMalloc((void**)&s->d_ct, 4 * sizeof(float)));
        VS_OBJ_TRY(s, launch_traj_emit(s->d_traj, s->tp, idx, s->d_M, s->d_Minv, s->d_dbg, st, canvas_on(s) ? s->d_ct : nullptr));
    }
    int rc = VS_OK;
    if (idx >= s->n_transforms) {
        // Stabilizer.cpp:774-780: no transform exists for this frame (last frame of a
        // flush): the queued frame is returned as is, at its own size (no border pad).
        // (border pad on a YUV stream: the frame alone is written, with the default offsets of its own size)
        const bool ypad = yuv_padded(s);
        if (!ypad && (ow != s->w || oh != s->h))
            VS_OBJ_HIP(s, hipMemset2DAsync(d_out, out_stride, 0, (size_t)ow * s->cn, oh, st));
        VS_OBJ_HIP(s, copy_planes(d_out, ypad ? planes(*s->pf, s->w, s->h, out_stride) : result_planes(s, d_out, out_stride), frame, queued_planes(s),
                                  hipMemcpyDeviceToDevice, st));
        s->last_out_w = s->w; s->last_out_h = s->h;
    } else if (canvas_on(s)) {                                                        // :1130-1134
        // the canvas replaces the warped frame, so the warp (and a fade history behind it) cannot be observed and is not run
        if (!s->canvas && !(s->canvas = canvas_new())) return vs_obj_fail(s, VS_ERR_HIP, "out of host memory");
        StageScope t(s, VS_STAGE_WARP, st);
        rc = canvas_apply(s->canvas, p, frame, s->src_pitch, s->w, s->h, s->d_ct, s->d_traj, d_out, out_stride, st);
    } else if (s->pf->kind != PIX_INTERLEAVED) {
        StageScope t(s, VS_STAGE_WARP, st);
        // crop-and-zoom: the warp goes into the stream's scratch surface, whose crops one launch resizes into d_out
        // border pad: one launch pads the planes into the stream's scratch surface, which is warped at the padded size, taps
        // outside it taking its edge (the border)
        // fade: one launch pads the planes and blends them with the history into that surface; one more, behind the warp, folds
        // the result into the history
        const bool cz = yuv_cz_on(s), fade = yuv_fade_on(s), pad = yuv_padded(s);
        uint8_t* scr = cz || pad ? scratch(s, s->scratch_own) : nullptr;
        if (fade) rc = yuv_fade_blend(s, frame, scr, st);
        else if (pad) rc = pad_launch(s, &frame, &scr, 1, st);
        const uint8_t* wsrc = pad ? scr : frame;
        uint8_t* wdst = cz ? scr : d_out;
        // (P010 and the three-plane formats go through the one-launch kernel even for one surface: its tables are built in the
        // stream's scratch; so does NV12 under edge fill, whose instances of the general kernels read every tap from memory)
        const YuvBorder wb = yuv_warp_border(s);
        if (rc == VS_OK)
            rc = warp_planes(&wsrc, &wdst, 1, warp_src_planes(s), warp_dst_planes(s, d_out, out_stride), WarpMaps{s->d_Minv, 12, false}, wb.border, wb.fill,
                             s->fmt == VS_FMT_NV12 && wb.border != VS_BORDER_FILL ? WarpTabs{} : WarpTabs{WarpTabs::SCRATCH}, st);
        if (cz && rc == VS_OK) rc = cz_launch(s, &wdst, &d_out, 1, out_stride, st);
        if (fade && rc == VS_OK) rc = yuv_fade_update(s, d_out, out_stride, st);
    } else if (bp.pad && p.border_type == VS_BORDER_FADE) {                               // :914-978, :1069-1106
        const int bw = bp.pw, bh = bp.ph;
        const size_t prow = bp.prow, nb = prow * bh;
        rc = launch_make_border(frame, s->src_pitch, s->w, s->h, s->cn, s->d_tmp, prow, bp.b, VS_BORDER_BLACK, st);
        if (rc == VS_OK && (!s->d_fade || s->fade_w != bw || s->fade_h != bh)) {     // :917-926 the first padded frame is the history
            if (s->d_fade) { (void)hipStreamSynchronize(st); (void)hipFree(s->d_fade); s->d_fade = nullptr; }
            VS_OBJ_HIP(s, hipMalloc((void**)&s->d_fade, (nb + 3) & ~(size_t)3));
            s->fade_w = bw; s->fade_h = bh; s->fade_valid = false;
        }
        if (rc == VS_OK && !s->fade_valid) {
            VS_OBJ_HIP(s, hipMemcpyAsync(s->d_fade, s->d_tmp, nb, hipMemcpyDeviceToDevice, st));
            s->fade_valid = true; s->fade_count = 0;
        }
        float alpha = p.fade_alpha;                                                       // :953-961
        if (s->fade_count < p.fade_duration) {
            alpha = alpha * (static_cast<float>(s->fade_count) / p.fade_duration);
            s->fade_count++;
        }
        if (rc == VS_OK) rc = launch_fade_blend(s->d_fade, s->d_tmp, (nb + 3) & ~(size_t)3, alpha, 1.0f - alpha, st);
        {
            StageScope t(s, VS_STAGE_WARP, st);
            if (rc == VS_OK) rc = warp_frame(s, s->d_tmp, prow, bw, bh, d_out, out_stride, st);
        }
        if (rc == VS_OK) rc = launch_fade_update(s->d_fade, d_out, out_stride, (int)prow, bh, st);
    } else if (bp.pad) {                                                              // :981-990
        rc = launch_make_border(frame, s->src_pitch, s->w, s->h, s->cn, s->d_tmp, bp.prow, bp.b, p.border_type, st);
        StageScope t(s, VS_STAGE_WARP, st);
        if (rc == VS_OK) rc = warp_frame(s, s->d_tmp, bp.prow, bp.pw, bp.ph, d_out, out_stride, st);
    } else if (bp.crop) {                                                             // :1108-1124
        StageScope t(s, VS_STAGE_WARP, st);
        rc = warp_frame(s, frame, s->src_pitch, s->w, s->h, s->d_tmp, bp.prow, st);
        if (rc == VS_OK)
            rc = launch_resize_linear(s->d_tmp + ((size_t)bp.b * s->w + bp.b) * s->cn, bp.prow, s->w - 2 * bp.b, s->h - 2 * bp.b,
                                      s->cn, d_out, out_stride, s->orig_w, s->orig_h, st);
    } else {                                                                          // :1056-1060
        StageScope t(s, VS_STAGE_WARP, st);
        rc = warp_frame(s, frame, s->src_pitch, s->w, s->h, d_out, out_stride, st);
    }
    // the slot may be overwritten once this warp has read it
    const int rrc = release_slot(s, slot, st);
    if (rc == VS_OK) rc = rrc;
    if (rc != VS_OK) { s->err = get_last_error(); return rc; }
    s->counters.frames_out++;
    return VS_OK;
}

// ---- batch mode --------------------------------------------------------------------------------------
// Frame f (>= 1) enters: its gray image and pyramid are built at once on `pre` (ring slot f % npyr); the
// analysis is postponed until `batch` frames wait.  All host-side decisions of generateTransform that do not
// depend on data (detection cadence :696, keypoint buffer hand-over, warm-up :383-387) are taken here, in
// push order, so the device work is the same as in the per-frame path.
int batch_enqueue(vs_stab* s, const uint8_t* frame, int slot, int f, uint8_t* d_out, size_t out_stride, int* produced) {
    const vs_params_c& p = s->p;
    const int N = s->npyr, c = f % N, pv = (f - 1) % N;
    const FirstFailure& gf = group_failure(s->group);
    if (gf.rc != VS_OK) return vs_obj_fail(s, gf.rc, gf.msg);
    // one output pitch per batched warp launch: a change of pitch closes the batch that is being collected
    for (const vs_stab::BFrame& q : s->bq)
        if (q.out_due && q.out_stride != out_stride) { VS_OBJ_TRY(s, drain_batch(s)); break; }
    vs_stab::BFrame b;
    memset(&b, 0, sizeof b);
    b.f = f; b.c = c; b.pv = pv;
    b.frame = frame; b.prev_small = s->prev_small;
    s->prev_small = false;
    b.lk_buf = s->kp_cur; b.lk_cap = s->pts_cap[s->kp_cur];
    b.have_prev_gray = s->have_prev_gray ? 1 : 0;
    b.detect = (++s->detect_counter % 2) == 0;
    if (b.detect) {
        const int q = s->kp_next;
        s->kp_next = (s->kp_next + 1) % (int)s->d_pts.size();
        b.det_buf = q;
        s->pts_cap[q] = std::min(p.max_corners, 200);
        s->kp_cur = q;
        s->counters.detections++;
    }
    s->n_transforms++;
    s->have_prev_gray = true;
    s->last_gray_buf = c;
    s->q_slot.push_back(slot); s->q_idx.push_back(f); s->q_ptr.push_back(frame);     // :376-377
    if (release_due(s->q_idx.size(), s->host_radius)) {                              // :383-389
        b.out_due = true;
        b.out_slot = s->q_slot.front(); b.out_idx = s->q_idx.front(); b.out_frame = s->q_ptr.front();
        s->q_slot.pop_front(); s->q_idx.pop_front(); s->q_ptr.pop_front();
        b.d_out = d_out; b.out_stride = out_stride;
        out_size(s, s->w, s->h, &s->last_out_w, &s->last_out_h);
        s->counters.frames_out++;
        *produced = 1;
    }
    s->bq.push_back(b);
    // a full batch runs (a vs_batch runs the batches of its streams together: vs_batch_push_dev decides)
    if (s->group == s->own && (int)s->bq.size() >= s->batch) {
        VS_OBJ_TRY(s, group_run(s->group));
    }
    return VS_OK;
}

int check_params(const vs_params_c* p, std::string* why) {
    if (!p || p->struct_size != (int32_t)sizeof(vs_params_c)) { *why = "params: struct_size mismatch"; return VS_ERR_INVALID_ARG; }
    if (p->enable_virtual_canvas && !p->crop_n_zoom) {
        // temporalBufferSize < 0 never trims in the reference (size_t compare, Stabilizer.cpp:2159); a blend weight outside
        // [0, 1] leaves the range of the uchar cast of :2392-2396
        if (p->temporal_buffer_size < 0 || p->temporal_buffer_size > 256) { *why = "temporalBufferSize must be in [0,256]"; return VS_ERR_INVALID_ARG; }
        if (!(p->canvas_blend_weight >= 0.0f && p->canvas_blend_weight <= 1.0f)) { *why = "canvasBlendWeight must be in [0,1]"; return VS_ERR_UNSUPPORTED; }
        if (!(p->canvas_scale_factor > 0.0f && p->canvas_scale_factor <= 16.0f) || !(p->min_canvas_scale > 0.0f) || !(p->max_canvas_scale <= 16.0f)) {
            *why = "canvas scale factors must be in (0,16]"; return VS_ERR_INVALID_ARG;
        }
    }
    if (p->max_corners < 1 || p->max_corners > 4096) { *why = "maxCorners must be in [1,4096]"; return VS_ERR_INVALID_ARG; }
    if (p->block_size < 1 || p->block_size > 7) { *why = "blockSize must be in [1,7]"; return VS_ERR_INVALID_ARG; }
    if (p->lk_win_size < 3 || p->lk_win_size > 31 || p->lk_max_level < 0 || p->lk_max_level > 7) { *why = "LK window/levels out of range"; return VS_ERR_INVALID_ARG; }
    if (p->ransac_max_iters < 1 || p->ransac_max_iters > 4096) { *why = "ransac_max_iters out of range"; return VS_ERR_INVALID_ARG; }
    if (p->border_size < 0 || p->border_type < 0 || p->border_type > VS_BORDER_FADE) { *why = "border parameters out of range"; return VS_ERR_INVALID_ARG; }
    if (p->smoothing_method < 0 || p->smoothing_method > VS_SMOOTH_KALMAN) { *why = "smoothing_method out of range"; return VS_ERR_INVALID_ARG; }
    if (p->smoothing_method == VS_SMOOTH_GAUSSIAN) {
        // gaussianFilterConvolve's kernel has max(3, ceil(6 sigma)) taps (Stabilizer.cpp:1368-1370); the device evaluates one
        // tap per lane of a wave, at most GAUSS_MAX: a wider kernel would be cut short without a word
        const float sigma = (float)p->gaussian_sigma;
        if (!(sigma > 0.0f)) { *why = "gaussianSigma must be positive"; return VS_ERR_INVALID_ARG; }
        int ks = std::max(3, (int)std::ceil(6 * sigma));
        if (ks % 2 == 0) ks++;
        if (!(sigma <= 1e6f) || ks > GAUSS_MAX) { *why = "gaussianSigma above 10.5 (a smoothing kernel of more than 63 taps) is outside the accelerated path"; return VS_ERR_UNSUPPORTED; }
    }
    return VS_OK;
}

// Shared body of stabilize(): the frame is already on its way into ring slot `slot` (on `pre`).
int push_common(vs_stab* s, int slot, const uint8_t* zc_frame, uint8_t* d_out, size_t out_stride, int* produced, bool may_defer) {
    const vs_params_c& p = s->p;
    const uint8_t* frame = slot >= 0 ? s->d_ring + (size_t)slot * s->frame_bytes : zc_frame;
    *produced = 0;
    s->counters.frames_in++;
    if (p.crop_n_zoom && s->orig_w == 0) { s->orig_w = s->w; s->orig_h = s->h; }   // :267-269
    if (s->first) {                                                                  // :271-368
        VS_OBJ_TRY(s, launch_resize_gray(frame, s->src_pitch, s->w, s->h, s->pf->gray_source, s->d_first_gray, 480, 480, 270, s->st_pre));  // :304-305
        VS_OBJ_HIP(s, hipEventRecord(s->ev_first, s->st_pre));
        VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_det, s->ev_first, 0));
        VS_OBJ_TRY(s, launch_gftt(s->d_first_gray, 480, 480, 270, p.max_corners, p.quality_level, p.min_distance,
                             p.block_size, s->gw, s->d_pts[0], s->d_npts[0], s->st_det));   // :354-358
        VS_OBJ_HIP(s, hipEventRecord(s->ev_det[0], s->st_det));
        s->pts_event[0] = s->ev_det[0];
        s->pts_pending[0] = true;
        s->pp = 0; s->pts_cap[0] = p.max_corners;
        s->last_detected = true; s->last_detect_pp = 0;
        s->dbg_det_pts = s->d_pts[0]; s->dbg_det_n = s->d_npts[0];
        s->counters.detections++;
        s->prev_small = true; s->have_prev_gray = true;
        s->q_slot.push_back(slot); s->q_idx.push_back(0); s->q_ptr.push_back(frame);
        s->first = false; s->next_index = 1;
        return VS_OK;
    }
    if (s->batch_active) {
        VS_OBJ_TRY(s, batch_enqueue(s, frame, slot, s->next_index, d_out, out_stride, produced));
        s->next_index++;
        if (!may_defer) { VS_OBJ_TRY(s, drain_batch(s)); VS_OBJ_TRY(s, flush_warps(s)); }
        return VS_OK;
    }
    s->q_slot.push_back(slot); s->q_idx.push_back(s->next_index); s->q_ptr.push_back(frame);   // :376-377
    VS_OBJ_TRY(s, generate_transform(s, frame, s->next_index));                          // :380
    if (p.adaptive_smoothing) {
        // params_.smoothingRadius is data dependent in this mode (:1482-1486) and
        // moves the warm-up threshold (:383): read it back (synchronises).
        int r = 0;
        VS_OBJ_HIP(s, hipMemcpyAsync(&r, &s->d_traj->smoothing_radius, sizeof r, hipMemcpyDeviceToHost, s->st));
        VS_OBJ_HIP(s, hipStreamSynchronize(s->st));
        s->host_radius = r;
    }
    if (!release_due(s->q_idx.size(), s->host_radius)) { s->next_index++; return VS_OK; }   // :383-387
    VS_OBJ_TRY(s, apply_next(s, d_out, out_stride, may_defer));                          // :389
    s->next_index++;
    *produced = 1;
    return VS_OK;
}

int take_slot(vs_stab* s, int* slot) {
    if (!s->d_ring) VS_OBJ_HIP(s, hipMalloc((void**)&s->d_ring, s->frame_bytes * s->ring_frames));
    if (s->free_slots.empty()) return vs_obj_fail(s, VS_ERR_CAPACITY, "frame ring exhausted");
    *slot = s->free_slots.front();
    s->free_slots.pop_front();
    return VS_OK;
}

// What every push asks first: the rules of the input side (pixfmt.h), then the stream allocates for its first frame.
int prepare(vs_stab* s, int w, int h, int fmt, size_t stride) {
    VS_REFUSE(s, check_input(pixfmt(fmt), w, h, stride, s->in, s->out, s->p.border_size, s->yuv_cz && s->p.crop_n_zoom, yuv_pad_wanted(s), yuv_fade_wanted(s)));
    if (yuv_fade_wanted(s) && s->yfade_fill_given && pixfmt(fmt)->kind != PIX_INTERLEAVED)
        VS_REFUSE(s, check_yuv_fill(*pixfmt(fmt), s->yfade_fill, "vs_stab_set_yuv_fade"));
    if (yuv_pad_wanted(s) && s->pad_fill_given && pixfmt(fmt)->kind != PIX_INTERLEAVED) VS_REFUSE(s, check_yuv_fill(*pixfmt(fmt), s->pad_fill));
    if (s->yuv_efill && s->efill_given && pixfmt(fmt)->kind != PIX_INTERLEAVED) VS_REFUSE(s, check_yuv_fill(*pixfmt(fmt), s->efill, "vs_stab_set_yuv_edge_fill"));
    VS_OBJ_HIP(s, hipSetDevice(s->device));
    if (!s->allocated) return allocate(s, w, h, fmt);
    if (w != s->w || h != s->h || fmt != s->fmt) return vs_obj_fail(s, VS_ERR_SIZE_CHANGED, "frame geometry changed; call vs_stab_clean()");
    return VS_OK;
}

// Border pad or fade on a YUV stream: the pitch of a device surface that receives a result holds a padded row
Refusal check_padded_out(const vs_stab* s, const char* call, size_t out_stride) {
    if (!yuv_padded(s) || out_stride >= border_plan(s).prow) return Refusal();
    return refuse(VS_ERR_INVALID_ARG, std::string(call) + (yuv_fade_on(s) ? ": fade on " : ": border pad on ") + s->pf->name + ": out_stride must hold a padded row (" +
                                          std::to_string(border_plan(s).prow) + " bytes)");
}

void destroy_events(vs_stab* s) {
    auto kill = [](hipEvent_t& e) { if (e) { (void)hipEventDestroy(e); e = nullptr; } };
    for (auto& e : s->ev_gray) kill(e);
    for (auto& e : s->ev_pre) kill(e);
    for (auto& e : s->ev_lk) kill(e);
    for (auto& e : s->ev_det) kill(e);
    for (auto& e : s->ev_slot) kill(e);
    kill(s->ev_first); kill(s->ev_hold);
    kill(s->ev_emit); kill(s->ev_warp[0]); kill(s->ev_warp[1]);
}

int create_events(vs_stab* s) {
    auto mk = [&](hipEvent_t& e) { return hipEventCreateWithFlags(&e, hipEventDisableTiming); };
    for (auto& e : s->ev_gray) VS_OBJ_HIP(s, mk(e));
    for (auto& e : s->ev_pre) VS_OBJ_HIP(s, mk(e));
    for (auto& e : s->ev_lk) VS_OBJ_HIP(s, mk(e));
    for (auto& e : s->ev_det) VS_OBJ_HIP(s, mk(e));
    for (auto& e : s->ev_slot) VS_OBJ_HIP(s, mk(e));
    VS_OBJ_HIP(s, mk(s->ev_first)); VS_OBJ_HIP(s, mk(s->ev_hold));
    VS_OBJ_HIP(s, mk(s->ev_emit)); VS_OBJ_HIP(s, mk(s->ev_warp[0])); VS_OBJ_HIP(s, mk(s->ev_warp[1]));
    return VS_OK;
}

}  // namespace

int vsd::pad_launch(const vs_stab* s, const uint8_t* const* frames, uint8_t* const* scratch, int n, hipStream_t st) {
    return pad_planes(s, frames, scratch, n, s->p.border_type, yuv_pad_fill(s), st);
}

int vsd::pad_planes(const vs_stab* s, const uint8_t* const* frames, uint8_t* const* scratch, int n, int border, const vs_yuv_fill& c, hipStream_t st) {
    const Planes S = queued_planes(s), D = scratch_planes(s);
    const int b = s->p.border_size;
    vs_pad_job jobs[YP_MAX_JOBS];
    int nj = 0;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < S.n; k++)
            jobs[nj++] = vs_pad_job{frames[i] + S[k].off, S[k].pitch, S[k].w, S[k].h, scratch[i] + D[k].off, D[k].pitch, b >> S[k].sx, b >> S[k].sy,
                                    S[k].cn, border, {plane_fill(c, S, k, 0), plane_fill(c, S, k, 1)}, 0};
    return launch_yuvpad(jobs, nj, S.sample_bytes, st);
}

int vsd::cz_launch(const vs_stab* s, const uint8_t* const* scratch, uint8_t* const* outs, int n, size_t out_stride, hipStream_t st) {
    const Planes S = scratch_planes(s);
    const int b = s->p.border_size;
    vs_scale_job jobs[CZ_MAX_JOBS];
    int nj = 0;
    for (int i = 0; i < n; i++) {
        const Planes D = result_planes(s, outs[i], out_stride);
        // one plane: its crop - the luma crop (b, b, w - 2b, h - 2b) shifted by (sx, sy) - in the scratch surface -> the plane of the result
        for (int k = 0; k < S.n; k++) {
            const Plane& p = S[k];
            const size_t crop = (size_t)(b >> p.sy) * p.pitch + (size_t)(b >> p.sx) * p.cn * S.sample_bytes;
            jobs[nj++] = vs_scale_job{scratch[i] + p.off + crop, p.pitch, (s->w - 2 * b) >> p.sx, (s->h - 2 * b) >> p.sy, outs[i] + D[k].off, D[k].pitch,
                                      D[k].w, D[k].h, p.cn, 0};
        }
    }
    return launch_cropzoom(jobs, nj, S.sample_bytes, st);
}

void vsd::fill_traj_params(const vs_params_c& p, TrajParams& t) {
    memset(&t, 0, sizeof t);
    t.method = p.smoothing_method;
    t.horizon_lock = p.horizon_lock;
    t.drone = p.drone_high_freq_mode;
    t.adaptive = p.adaptive_smoothing;
    t.min_radius = p.min_smoothing_radius;
    t.max_radius = p.max_smoothing_radius;
    t.hf_shake_px = p.hf_shake_px;
    t.hf_rot_lp_alpha = p.hf_rot_lp_alpha;
    t.hf_dead_zone = p.hf_dead_zone_threshold;
    t.hf_decay = p.hf_motion_accumulator_decay;
    t.hf_freeze_duration = p.hf_freeze_duration;
    // gaussianFilterConvolve kernel (Stabilizer.cpp:1368-1386), built with the host libm
    float sigma = (float)p.gaussian_sigma;
    int ks = std::max(3, (int)std::ceil(6 * sigma));
    if (ks % 2 == 0) ks++;
    if (ks > GAUSS_MAX) ks = GAUSS_MAX;
    t.gauss_ksize = ks;
    float sum = 0.0f;
    int center = ks / 2;
    for (int i = 0; i < ks; i++) {
        float x = (float)(i - center);
        t.gauss_kernel[i] = std::exp(-(x * x) / (2 * sigma * sigma));
        sum += t.gauss_kernel[i];
    }
    for (int i = 0; i < ks; i++) t.gauss_kernel[i] /= sum;
}

// All instances of a process on one device share ONE set of four HIP streams.  Every instance's launches are already wide in batch mode, and the runtime maps HIP streams onto a
// handful of hardware queues: with four private streams per instance, 2 instances ran at 0.9x and 8 instances
// at 0.15x of ONE instance's total throughput; on shared streams the instances simply take turns.
namespace {
struct StreamPool {
    hipStream_t st = nullptr, pre = nullptr, det = nullptr, warp = nullptr;
    // (the batched warps of every schedule on the device run on `pre`, in the order they were issued: instances sharing the pool are
    //  driven from ONE host thread - INTEGRATION.md)
    int refs = 0;
};
std::mutex g_pool_mutex;
std::map<int, StreamPool> g_pools;

hipError_t make_streams(hipStream_t* st, hipStream_t* pre, hipStream_t* det, hipStream_t* warp) {
    hipError_t e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(pre, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(det, hipStreamNonBlocking);
    if (e == hipSuccess) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        e = hipStreamCreateWithPriority(warp, hipStreamNonBlocking, greatest);
    }
    return e;
}

hipError_t acquire_streams(vs_stab* s) {
    std::lock_guard<std::mutex> g(g_pool_mutex);
    StreamPool& p = g_pools[s->device];
    if (p.refs == 0) {
        hipError_t e = make_streams(&p.st, &p.pre, &p.det, &p.warp);
        if (e != hipSuccess) return e;
    }
    p.refs++;
    s->st = p.st; s->st_pre = p.pre; s->st_det = p.det; s->st_warp = p.warp;
    s->shared_streams = true;
    return hipSuccess;
}

void release_streams(vs_stab* s) {
    if (!s->shared_streams) return;
    std::lock_guard<std::mutex> g(g_pool_mutex);
    StreamPool& p = g_pools[s->device];
    if (--p.refs == 0) {
        (void)hipStreamDestroy(p.st); (void)hipStreamDestroy(p.pre); (void)hipStreamDestroy(p.det); (void)hipStreamDestroy(p.warp);
        p.st = p.pre = p.det = p.warp = nullptr; p.refs = 0;
    }
}
}  // namespace

extern "C" {

int vs_stab_create(const vs_params_c* params, int device, vs_stab** out) {
    if (!out) return VS_ERR_INVALID_ARG;
    *out = nullptr;
    std::string why;
    int rc = check_params(params, &why);
    if (rc != VS_OK) { set_last_error(why); return rc; }
    VS_TRY(ensure_device());
    int ndev = 0;
    VS_HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_last_error("vs_stab_create: bad device index"); return VS_ERR_INVALID_ARG; }
    VS_HIP_TRY(hipSetDevice(device));
    vs_stab* s = new (std::nothrow) vs_stab();
    if (!s) return VS_ERR_HIP;
    s->p = *params;
    s->device = device;
    s->host_radius = params->smoothing_radius;
    if (const char* e = lab_env("VS_STAB_DEBUG_DELAY_US")) s->dbg_delay_us = std::max(0, std::min(std::atoi(e), 20000));
    memset(&s->counters, 0, sizeof s->counters);
    fill_traj_params(s->p, s->tp);
    hipError_t e = acquire_streams(s);
    if (e != hipSuccess || create_events(s) != VS_OK) {
        set_last_error(e != hipSuccess ? hipGetErrorString(e) : s->err);
        vs_stab_destroy(s);
        return VS_ERR_HIP;
    }
    *out = s;
    return VS_OK;
}

void vs_stab_destroy(vs_stab* s) {
    if (!s || s->member) return;        // (a stream of a vs_batch goes with its group: vs_batch_destroy)
    // the destructor may race in-flight work (vsg.cpp:1374): drain the streams first
    wait_streams(s);
    free_all(s);
    if (s->d_fade) (void)hipFree(s->d_fade);
    if (s->d_yfade) (void)hipFree(s->d_yfade);
    if (s->d_ct) (void)hipFree(s->d_ct);
    canvas_delete(s->canvas);
    for (auto& pe : s->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : s->ev_pool) (void)hipEventDestroy(e);
    destroy_events(s);
    if (s->st) release_streams(s);
    delete s;
}

int vs_stab_clean(vs_stab* s) {   // Stabilizer.cpp:221-256
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (s->own && group_failure(s->own).rc != VS_OK) wait_streams(s);     // (a failed private group is not drained: it goes)
    else VS_OBJ_TRY(s, sync_all(s));
    free_all(s);
    s->q_slot.clear(); s->q_idx.clear(); s->q_ptr.clear();
    s->hold_valid = false; s->hold_cur = 0;
    s->first = true; s->next_index = 0; s->w = s->h = 0; s->orig_w = s->orig_h = 0; s->n_transforms = 0;
    s->have_prev_gray = false; s->prev_small = false; s->pp = 0;
    s->host_radius = s->p.smoothing_radius;
    return VS_OK;
}

int vs_stab_out_size(const vs_stab* s, int w, int h, int* out_w, int* out_h) {
    if (!s || !out_w || !out_h) return VS_ERR_INVALID_ARG;
    out_size(s, w, h, out_w, out_h);
    return VS_OK;
}

int vs_stab_push_dev(vs_stab* s, const void* d_data, int w, int h, size_t stride, int fmt, void* d_out,
                     size_t out_stride, int* produced) {
    if (!s || !produced) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    *produced = 0;
    if (!d_data) return VS_OK;   // empty frame -> empty result (Stabilizer.cpp:263-265)
    int rc = prepare(s, w, h, fmt, stride);
    if (rc != VS_OK) return rc;
    VS_REFUSE(s, check_surface(*s->pf, true, (uintptr_t)d_data | (uintptr_t)d_out, out_stride, s->out.c_pitch));
    VS_REFUSE(s, check_padded_out(s, "push", out_stride));
    if (s->zero_copy) {
        // the frame is read where it is: it must stay valid and unchanged until its own result has been produced
        // one pitch for all frames in flight (the batched launches take it once): it may change when nothing is queued
        if (stride != s->src_pitch) {
            if (!s->q_slot.empty() || !s->bq.empty() || !s->pend.empty() || group_holds_warps(s->group))
                return vs_obj_fail(s, VS_ERR_INVALID_ARG, "zero-copy mode: the row pitch may only change while no frame is queued");
            s->src_pitch = stride;
        }
        return push_common(s, -1, (const uint8_t*)d_data, (uint8_t*)d_out, out_stride, produced, true);
    }
    int slot;
    VS_OBJ_TRY(s, take_slot(s, &slot));
    VS_OBJ_TRY(s, enqueue_copy_in(s, slot, d_data, stride, hipMemcpyDeviceToDevice));
    return push_common(s, slot, nullptr, (uint8_t*)d_out, out_stride, produced, true);
}

// n consecutive pushes of one geometry: result j of them (in the order they become due) goes to d_outs[j]; *produced = how many
// became due.  What n calls of vs_stab_push_dev do, without n trips through a binding.
int vs_stab_push_dev_n(vs_stab* s, const void* const* d_frames, int n, int w, int h, size_t stride, int fmt, void* const* d_outs, size_t out_stride,
                       int* produced) {
    if (!s || !d_frames || !d_outs || !produced || n < 0) return VS_ERR_INVALID_ARG;
    int k = 0;
    for (int i = 0; i < n; i++) {
        int now = 0;
        const int rc = vs_stab_push_dev(s, d_frames[i], w, h, stride, fmt, d_outs[k], out_stride, &now);
        if (rc != VS_OK) { *produced = k; return rc; }
        k += now;
    }
    *produced = k;
    return VS_OK;
}

static int flush_dev_impl(vs_stab* s, void* d_out, size_t out_stride, int* produced, bool may_defer_flush) {
    if (!s || !produced) return VS_ERR_INVALID_ARG;
    *produced = 0;
    if (!s->allocated || s->q_slot.empty()) return VS_OK;
    VS_REFUSE(s, check_surface(*s->pf, true, (uintptr_t)d_out, out_stride, d_out != s->d_out ? s->out.c_pitch : 0));   // (s->d_out: the staging of vs_stab_flush)
    VS_REFUSE(s, check_padded_out(s, "flush", out_stride));
    VS_OBJ_HIP(s, hipSetDevice(s->device));
    VS_OBJ_TRY(s, drain_batch(s));
    VS_OBJ_TRY(s, apply_next(s, (uint8_t*)d_out, out_stride, may_defer_flush));
    *produced = 1;
    return VS_OK;
}

int vs_stab_flush_dev(vs_stab* s, void* d_out, size_t out_stride, int* produced) {   // Stabilizer.cpp:394-400
    if (!s || !produced) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    return flush_dev_impl(s, d_out, out_stride, produced, true);
}

// Host pipeline: a call returns the frame that the call before it computed.  Its download runs on the copy stream while
// this call's frame is uploaded (PCIe is full duplex) and the call returns as soon as both transfers are done: the
// analysis and the warp of this call's frame go on behind the caller's back and are picked up by the next call.
static int push_host_pipelined(vs_stab* s, const uint8_t* data, int w, int h, size_t stride, int fmt, uint8_t* out,
                               size_t out_stride, int* produced) {
    int ow, oh;
    out_size(s, w, h, &ow, &oh);
    const size_t orow = (size_t)ow * s->cn;
    const int orows = s->pf->rows(oh);
    const bool have_prev = s->hold_valid;
    // (as in the synchronous call: the buffer is only looked at when a frame will be delivered into it; a held frame is
    // always a full-size one - pass-through frames only come out of vs_stab_flush's synchronous part)
    if (have_prev) VS_REFUSE(s, check_host_out("push", out != nullptr, out_stride, orow));
    VS_REFUSE(s, check_surface(*s->pf, false, 0, out_stride, 0));
    for (auto& hld : s->d_hold)
        if (!hld) VS_OBJ_HIP(s, hipMalloc((void**)&hld, s->out_bytes));
    // A copy to or from PAGEABLE memory (the frames of a cv::Mat) keeps its caller inside hipMemcpy for the whole transfer -
    // about 0.2 ms per direction at 1080p, through the runtime's bounce buffers -, so download and upload issued from this
    // thread run one after the other: 2 520 frames/s against 4 730 with page-locked frames.  With a pageable output buffer the
    // download is therefore issued by the instance's helper thread, beside this thread's upload (VS_STAB_HOST_HELPER=0: from
    // this thread, as before).  (Staging both directions through page-locked buffers of our own with a pool of copy threads
    // was measured first and lost to the runtime's path: scratch/README.md.)
    static const bool use_helper = [] { const char* e = lab_env("VS_STAB_HOST_HELPER"); return !(e && e[0] == '0'); }();
    struct Join {           // the helper's job refers to the caller's buffer: no way out of this call without waiting for it
        HostHelper* h = nullptr;
        ~Join() { if (h) (void)h->wait(); }
        int wait() { HostHelper* t = h; h = nullptr; return t ? t->wait() : 0; }
    } join;
    const int held_w = s->hold_w, held_h = s->hold_h;
    if (have_prev) {       // the held result: on its way while this call's frame comes in
        VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_warp, s->ev_hold, 0));
        const uint8_t* d_src = s->d_hold[s->hold_cur ^ 1];

        bool helped = false;
        if (use_helper && !s->pf->three_planes() && !host_ptr_page_locked(out)) {
            try {           // (no exception leaves the C ABI: without a helper thread the download goes out from this one)
                if (!s->helper) s->helper.reset(new HostHelper);
                const int dev = s->device;
                hipStream_t stw = s->st_warp;
                s->helper->start([=]() -> int {
                    hipError_t e = hipSetDevice(dev);
                    if (e == hipSuccess) e = hipMemcpy2DAsync(out, out_stride, d_src, orow, orow, orows, hipMemcpyDeviceToHost, stw);
                    if (e == hipSuccess) e = hipStreamSynchronize(stw);
                    return (int)e;
                });
                join.h = s->helper.get();
                helped = true;
            } catch (...) {
                s->helper.reset();
            }
        }
        if (!helped) {
            VS_OBJ_TRY(s, download_result(s, out, out_stride, d_src, orow, orows, s->st_warp, held_w, held_h));
        }
    }
    int slot;
    VS_OBJ_TRY(s, take_slot(s, &slot));
    VS_OBJ_TRY(s, enqueue_copy_in(s, slot, data, stride, hipMemcpyHostToDevice));
    int now = 0;
    int rc = push_common(s, slot, nullptr, s->d_hold[s->hold_cur], orow, &now, false);
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st_pre));        // the caller's frame has been consumed
    if (join.h) VS_OBJ_HIP(s, (hipError_t)join.wait());
    else if (have_prev) VS_OBJ_HIP(s, hipStreamSynchronize(s->st_warp));
    if (rc != VS_OK) return rc;
    s->hold_valid = now != 0;
    if (now) {
        VS_OBJ_HIP(s, hipEventRecord(s->ev_hold, s->st));
        s->hold_cur ^= 1;
        s->hold_w = s->last_out_w; s->hold_h = s->last_out_h;
    }
    *produced = have_prev ? 1 : 0;
    if (have_prev) { s->last_out_w = held_w; s->last_out_h = held_h; }     // vs_stab_last_out_dims: the frame that was handed out
    return VS_OK;
}

int vs_stab_push(vs_stab* s, const uint8_t* data, int w, int h, size_t stride, int fmt, uint8_t* out,
                 size_t out_stride, int* produced) {
    if (!s || !produced) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    *produced = 0;
    if (!data) return VS_OK;
    int rc = prepare(s, w, h, fmt, stride);
    if (rc != VS_OK) return rc;
    if (s->zero_copy && (s->src_pitch != s->row_bytes || (s->pf->luma_uv() && s->in.uv_off) || (s->pf->three_planes() && s->in.planar_bits())))
        return vs_obj_fail(s, VS_ERR_INVALID_ARG, "push: host frames cannot join a queue of pitched zero-copy surfaces");
    // (host frames hold the packed default layout at their pitch: the frame pushed, and the buffer of the result if there is one)
    VS_REFUSE(s, check_surface(*s->pf, false, 0, stride, 0));
    VS_REFUSE(s, check_surface(*s->pf, false, 0, out ? out_stride : 0, 0));
    if (s->host_pipe && !s->batch_active) return push_host_pipelined(s, data, w, h, stride, fmt, out, out_stride, produced);
    int ow, oh;
    out_size(s, w, h, &ow, &oh);
    const size_t orow = (size_t)ow * s->cn;
    // (the output buffer is checked before the frame is consumed: a bad call loses nothing)
    const int R = effective_radius(s->host_radius);
    if (!s->first && (int)s->q_idx.size() + 1 >= R) VS_REFUSE(s, check_host_out("push", out != nullptr, out_stride, orow));
    int slot;
    VS_OBJ_TRY(s, take_slot(s, &slot));
    rc = enqueue_copy_in(s, slot, data, stride, hipMemcpyHostToDevice);
    if (rc == VS_OK) rc = drain_batch(s);
    if (rc == VS_OK) rc = flush_warps(s);
    if (rc == VS_OK) rc = push_common(s, slot, nullptr, s->d_out, orow, produced, false);
    if (rc != VS_OK) {
        (void)hipStreamSynchronize(s->st_pre);       // the upload from the caller's buffer may still be in flight
        return rc;
    }
    if (*produced) {
        const Refusal small = check_host_out("push", out != nullptr, out_stride, orow);
        if (small.rc != VS_OK) {
            (void)hipStreamSynchronize(s->st_pre);
            return vs_obj_fail(s, small.rc, small.text);
        }
        const int orows = s->pf->rows(oh);
        VS_OBJ_HIP(s, hipStreamSynchronize(s->st_warp));   // (per-frame pipeline: the warp ran on the warp stream)
        if (s->batch_active) VS_OBJ_HIP(s, hipStreamSynchronize(s->st_pre));     // batch mode: the warps run on `pre` (group_launch_ready)
        VS_OBJ_TRY(s, download_result(s, out, out_stride, s->d_out, orow, orows, s->st, s->last_out_w, s->last_out_h));
    }
    // the caller's frame must be consumed and its result delivered before returning
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st_pre));
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st));
    return VS_OK;
}

int vs_stab_flush(vs_stab* s, uint8_t* out, size_t out_stride, int* produced) {
    if (!s || !produced) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    *produced = 0;
    if (!s->allocated) return VS_OK;
    if (s->hold_valid) {      // host pipeline: the frame the last push computed
        const size_t orow = (size_t)s->hold_w * s->cn;
        VS_REFUSE(s, check_host_out("flush", out != nullptr, out_stride, orow));
        const int orows = s->pf->rows(s->hold_h);
        VS_OBJ_HIP(s, hipStreamWaitEvent(s->st_warp, s->ev_hold, 0));
        VS_REFUSE(s, check_surface(*s->pf, false, 0, out_stride, 0));
        VS_OBJ_TRY(s, download_result(s, out, out_stride, s->d_hold[s->hold_cur ^ 1], orow, orows, s->st_warp, s->hold_w, s->hold_h));
        VS_OBJ_HIP(s, hipStreamSynchronize(s->st_warp));
        s->hold_valid = false;
        s->last_out_w = s->hold_w; s->last_out_h = s->hold_h;
        *produced = 1;
        return VS_OK;
    }
    if (s->q_slot.empty()) return VS_OK;
    int ow, oh;
    out_size(s, s->w, s->h, &ow, &oh);
    const size_t orow = (size_t)ow * s->cn;
    VS_REFUSE(s, check_host_out("flush", out != nullptr, out_stride, orow));
    VS_REFUSE(s, check_surface(*s->pf, false, 0, out_stride, 0));
    VS_OBJ_TRY(s, drain_batch(s));
    VS_OBJ_TRY(s, flush_warps(s));
    int rc = flush_dev_impl(s, s->d_out, orow, produced, false);
    if (rc != VS_OK) return rc;
    const int orows = s->pf->rows(oh);
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st_warp));
    if (s->batch_active) VS_OBJ_HIP(s, hipStreamSynchronize(s->st_pre));         // batch mode: the warps run on `pre`
    VS_OBJ_TRY(s, download_result(s, out, out_stride, s->d_out, orow, orows, s->st, s->last_out_w, s->last_out_h));
    VS_OBJ_HIP(s, hipStreamSynchronize(s->st));
    return VS_OK;
}

// Host pipeline for vs_stab_push / vs_stab_flush (see push_host_pipelined): one more call of latency, the transfers of
// consecutive calls overlap each other and the device work.  To be chosen while no frame is queued.
int vs_stab_set_host_pipeline(vs_stab* s, int enable) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty() || s->hold_valid) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_host_pipeline: the frame queue must be empty");
    s->host_pipe = enable != 0;
    return VS_OK;
}

// Deferred output for the device entry points: up to `frames` consecutive results are warped by one
// launch.  A result is complete after vs_stab_sync(); every push must then be given its own d_out.
int vs_stab_set_warp_batch(vs_stab* s, int frames) {
    if (!s || frames < 1 || frames > WARP_BATCH_MAX) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (s->allocated) { VS_OBJ_HIP(s, hipSetDevice(s->device)); VS_OBJ_TRY(s, flush_warps(s)); }
    s->warp_batch = frames;
    return VS_OK;
}

// Batch mode for the device entry points: the analysis of `frames` consecutive pushes (feature detection,
// tracking, hypothesis scoring) runs as one launch per stage, and their warps as one launch (implies
// vs_stab_set_warp_batch(frames)).  To be chosen before the first frame (or after vs_stab_clean).
int vs_stab_set_batch(vs_stab* s, int frames) {
    if (!s || frames < 1 || frames > BATCH_MAX) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (s->allocated) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_batch: call before the first frame or after vs_stab_clean");
    s->batch = frames;
    if (frames > 1) s->warp_batch = std::min(frames, WARP_BATCH_MAX);
    return VS_OK;
}

// Zero-copy input for vs_stab_push_dev: the frame is not copied into the instance's queue but read where the
// caller put it (a decoder surface pool, a resident clip).  It must stay valid and unchanged until the result
// of the SAME push count has been produced, i.e. for clamp(smoothingRadius,5,35) further pushes plus 1 + WARP_LAG
// times the batch depth and a vs_stab_sync, or until vs_stab_flush_dev has drained the queue.  Tightly packed frames.
int vs_stab_set_zero_copy(vs_stab* s, int enable) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_zero_copy: the frame queue must be empty");
    s->zero_copy = enable != 0;
    s->src_pitch = s->row_bytes;
    return VS_OK;
}

// NV12 surfaces of the device entry points as hardware decoders export them (rocDecode, VA-API): Y and interleaved
// UV plane with a common pitch, the UV plane `uv_offset` bytes behind the Y pointer.  0 = contiguous (h * pitch).
int vs_stab_set_nv12_layout(vs_stab* s, size_t in_uv_offset, size_t out_uv_offset) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_nv12_layout: the frame queue must be empty");
    if (s->allocated) VS_REFUSE(s, check_set_nv12_layout(*s->pf, in_uv_offset, out_uv_offset));
    s->in.uv_off = in_uv_offset;
    s->out.uv_off = out_uv_offset;
    return VS_OK;
}

// I420 / YV12 (and I010 / I012) surfaces of the device entry points: where the U and V planes start behind the Y pointer and the pitch of their rows,
// for the frames pushed (`in`: zero-copy and copy-in alike) and for the surfaces filled (`out`).  0 = the packed default per field.
int vs_stab_set_i420_layout(vs_stab* s, size_t in_u_off, size_t in_v_off, size_t in_c_pitch, size_t out_u_off, size_t out_v_off, size_t out_c_pitch) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_i420_layout: the frame queue must be empty");
    ChromaLayout in = s->in, out = s->out;       // (the NV12 offsets are the other setter's)
    in.u_off = in_u_off; in.v_off = in_v_off; in.c_pitch = in_c_pitch;
    out.u_off = out_u_off; out.v_off = out_v_off; out.c_pitch = out_c_pitch;
    if (s->allocated) VS_REFUSE(s, check_set_i420_layout(*s->pf, s->w, in, out));
    s->in = in; s->out = out;
    return VS_OK;
}

// Crop-and-zoom on YUV surfaces (NV12, P010 and the three-plane formats), off by default: with it a stream whose parameters say
// crop_n_zoom with a border_size warps into scratch surfaces and resizes their crops back to the frame's size (k_cropzoom.hip);
// without it such a stream is refused as ever.
int vs_stab_set_yuv_crop_zoom(vs_stab* s, int enable) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_crop_zoom: the frame queue must be empty");
    s->yuv_cz = enable != 0;
    return VS_OK;
}

// Border pad on YUV surfaces (NV12, P010 and the three-plane formats), off by default: with it a stream whose parameters say
// border_size without crop_n_zoom and a border type of cv::copyMakeBorder pads the planes of a frame into a scratch surface
// (k_yuvpad.hip) and warps that at the padded size under BORDER_REPLICATE; without it such a stream is refused as ever.
// fill: the colour VS_BORDER_BLACK writes; NULL: the format's video black.
int vs_stab_set_yuv_border_pad(vs_stab* s, int enable, const vs_yuv_fill* fill) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_border_pad: the frame queue must be empty");
    if (fill && fill->reserved != 0) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_border_pad: fill->reserved must be 0");
    if (enable && fill && s->allocated && s->pf->kind != PIX_INTERLEAVED) VS_REFUSE(s, check_yuv_fill(*s->pf, *fill));
    // (a stream whose parameters ask for a pad was allocated with the mode on - off, its first push was refused - so the scratch
    // surfaces are there whenever the mode is on)
    s->yuv_pad = enable != 0;
    s->pad_fill_given = enable && fill;
    if (s->pad_fill_given) s->pad_fill = *fill;
    return VS_OK;
}

// The fade border on YUV surfaces, off by default: with it a stream whose parameters say border_size without crop_n_zoom and
// borderType "fade" pads and blends the planes of a frame with a history (k_yuvfade.hip), warps the padded surface under
// BORDER_REPLICATE and folds the result into the history; without it such a stream is refused as ever.  Every accepted call drops
// the history: the next padded frame is the history, count 0.
int vs_stab_set_yuv_fade(vs_stab* s, int enable, const vs_yuv_fill* fill) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_fade: the frame queue must be empty");
    if (fill && fill->reserved != 0) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_fade: fill->reserved must be 0");
    if (enable && fill && s->allocated && s->pf->kind != PIX_INTERLEAVED) VS_REFUSE(s, check_yuv_fill(*s->pf, *fill, "vs_stab_set_yuv_fade"));
    // (a stream whose parameters ask for the fade was allocated with the mode on - off, its first push was refused - so the scratch
    // surface is there whenever the mode is on)
    s->yuv_fade = enable != 0;
    s->yfade_fill_given = enable && fill;
    if (s->yfade_fill_given) s->yfade_fill = *fill;
    s->yfade_valid = false; s->yfade_count = 0;
    return VS_OK;
}

// Edge fill on YUV surfaces (NV12, P010 and the three-plane formats), off by default: with it the warps of a stream's unpadded
// surfaces - the plain stream's, and the one into the scratch surface of crop-and-zoom - are cv::warpAffine(..., BORDER_CONSTANT,
// fill) per plane instead of BORDER_CONSTANT 0 (green): the VS_BORDER_FILL instances of the warp kernels (k_warp.hip).  Nothing is
// allocated and no launch is added; border pad and fade, which warp a padded surface under BORDER_REPLICATE, are not touched.
// fill: the colour outside the picture; NULL: the format's video black.
// (The queue rule is also what makes the lagged warps of batch mode use the fill their frames were queued under: yuv_warp_border.)
int vs_stab_set_yuv_edge_fill(vs_stab* s, int enable, const vs_yuv_fill* fill) {
    if (!s) return VS_ERR_INVALID_ARG;
    VS_CALLER_DRIVES(s);
    if (!s->q_slot.empty()) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_edge_fill: the frame queue must be empty");
    if (fill && fill->reserved != 0) return vs_obj_fail(s, VS_ERR_INVALID_ARG, "vs_stab_set_yuv_edge_fill: fill->reserved must be 0");
    if (enable && fill && s->allocated && s->pf->kind != PIX_INTERLEAVED) VS_REFUSE(s, check_yuv_fill(*s->pf, *fill, "vs_stab_set_yuv_edge_fill"));
    s->yuv_efill = enable != 0;
    s->efill_given = enable && fill;
    if (s->efill_given) s->efill = *fill;
    return VS_OK;
}

int vs_yuv_video_black(int fmt, vs_yuv_fill* out) {
    const PixFmt* f = pixfmt(fmt);
    if (!out || !f || f->kind == PIX_INTERLEAVED) { set_last_error("vs_yuv_video_black: fmt must be a YUV surface format (NV12, P010, I420 ... I412)"); return VS_ERR_INVALID_ARG; }
    *out = yuv_video_black(*f);
    return VS_OK;
}

int vs_stab_sync(vs_stab* s) {
    if (!s) return VS_ERR_INVALID_ARG;
    return sync_all(s);
}

int vs_stab_get_counters(vs_stab* s, vs_counters* out) {
    if (!s || !out) return VS_ERR_INVALID_ARG;
    *out = s->counters;
    if (s->allocated) {
        VS_OBJ_TRY(s, sync_all(s));
        vs_debug_frame d;
        int32_t c[4] = {0, 0, 0, 0};
        VS_OBJ_HIP(s, hipMemcpy(&d, s->d_dbg, sizeof d, hipMemcpyDeviceToHost));
        VS_OBJ_HIP(s, hipMemcpy(c, s->dbg_gftt_counters, sizeof c, hipMemcpyDeviceToHost));
        out->last_features = d.n_prev;
        out->last_tracked = d.n_valid;
        out->last_inliers = d.n_inliers;
        out->last_candidates = c[0];
        out->gftt_overflow = c[2];
    }
    return VS_OK;
}

int vs_stab_canvas_info(const vs_stab* s, int32_t info[8]) {
    if (!s || !info) return VS_ERR_INVALID_ARG;
    canvas_info(s->canvas, info);
    return VS_OK;
}

int vs_stab_get_debug(vs_stab* s, vs_debug_frame* out) {
    if (!s || !out) return VS_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->out_index = -1;
    if (!s->allocated) return VS_OK;
    VS_OBJ_TRY(s, sync_all(s));
    VS_OBJ_HIP(s, hipMemcpy(out, s->d_dbg, sizeof *out, hipMemcpyDeviceToHost));
    out->detected = s->last_detected ? 1 : 0;
    out->n_detected = 0;
    if (s->last_detected) {
        int32_t n = 0;
        VS_OBJ_HIP(s, hipMemcpy(&n, s->dbg_det_n, sizeof n, hipMemcpyDeviceToHost));
        out->n_detected = n;
    }
    if (s->counters.frames_in <= 1) { out->n_prev = 0; out->n_valid = 0; out->out_index = -1; }
    return VS_OK;
}

int vs_stab_get_debug_arrays(vs_stab* s, float* prev_pts, float* curr_pts, uint8_t* status, uint8_t* inliers,
                             float* detected_pts, uint8_t* gray, int* aw, int* ah) {
    if (!s) return VS_ERR_INVALID_ARG;
    vs_debug_frame d;
    int rc = vs_stab_get_debug(s, &d);
    if (rc != VS_OK) return rc;
    if (!s->allocated) return VS_OK;
    const bool first_only = s->counters.frames_in <= 1;
    if (d.n_prev > 0 && !first_only) {
        if (prev_pts) VS_OBJ_HIP(s, hipMemcpy(prev_pts, s->dbg_prev_pts, (size_t)d.n_prev * 8, hipMemcpyDeviceToHost));
        if (curr_pts) VS_OBJ_HIP(s, hipMemcpy(curr_pts, s->dbg_next, (size_t)d.n_prev * 8, hipMemcpyDeviceToHost));
        if (status) VS_OBJ_HIP(s, hipMemcpy(status, s->dbg_status, (size_t)d.n_prev, hipMemcpyDeviceToHost));
    }
    if (d.n_valid > 0 && inliers && !first_only) VS_OBJ_HIP(s, hipMemcpy(inliers, s->dbg_inliers, (size_t)d.n_valid, hipMemcpyDeviceToHost));
    if (d.n_detected > 0 && detected_pts)
        VS_OBJ_HIP(s, hipMemcpy(detected_pts, s->dbg_det_pts, (size_t)d.n_detected * 8, hipMemcpyDeviceToHost));
    if (first_only) {
        if (gray) VS_OBJ_HIP(s, hipMemcpy(gray, s->d_first_gray, (size_t)480 * 270, hipMemcpyDeviceToHost));
        if (aw) *aw = 480;
        if (ah) *ah = 270;
    } else {
        if (gray) VS_OBJ_HIP(s, hipMemcpy(gray, s->pyr[s->last_gray_buf].img[0], (size_t)s->aw * s->ah, hipMemcpyDeviceToHost));
        if (aw) *aw = s->aw;
        if (ah) *ah = s->ah;
    }
    return VS_OK;
}

int vs_stab_last_out_dims(const vs_stab* s, int* w, int* h) {
    if (!s || !w || !h) return VS_ERR_INVALID_ARG;
    *w = s->last_out_w; *h = s->last_out_h;
    return VS_OK;
}

const char* vs_stab_last_error(const vs_stab* s) { return s ? s->err.c_str() : ""; }
void* vs_stab_stream(vs_stab* s) { return s ? (void*)s->st : nullptr; }

int vs_stab_set_profiling(vs_stab* s, int mode) {
    if (!s || mode < 0 || mode > 3) return VS_ERR_INVALID_ARG;
    s->prof_mode = mode;
    return VS_OK;
}

int vs_stab_get_stage_times(vs_stab* s, double* total_ms, int64_t* launches) {
    if (!s || !total_ms || !launches) return VS_ERR_INVALID_ARG;
    for (int i = 0; i < VS_STAGE_COUNT; i++) { total_ms[i] = 0; launches[i] = 0; }
    if (!s->st) return VS_OK;
    VS_OBJ_TRY(s, sync_all(s));
    for (auto& pe : s->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess && pe.stage >= 0 && pe.stage < VS_STAGE_COUNT) {
            total_ms[pe.stage] += ms;
            launches[pe.stage]++;
        }
        s->ev_pool.push_back(pe.a);
        s->ev_pool.push_back(pe.b);
    }
    s->pending.clear();
    return VS_OK;
}

}  // extern "C"
