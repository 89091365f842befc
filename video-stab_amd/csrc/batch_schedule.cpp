// The batch schedule: vs_batch, group_* and the vs_batch_* entry points.
// ONE schedule runs every batch: a vs_batch steps the frames that all its streams have queued (BASELINE configs[4]: 64 streams =
// 8 per GPU), and a standalone instance in batch mode owns a private group of one (vs_stab::own).  N instances that each ran
// their own batches took turns on the device's streams: every stage launched once per instance, the chains of one queued behind
// the waits of another (8 instances: 101.7 k frames/s in total against 109.1 k for one, round 2).  A group goes through ONE
// step for its members: the frames that all of them have queued since the last step go into one argument table per stage - the
// tables hold one block per frame anyway, and a block names its frame's buffers, so a launch does not care whose frame it is -,
// the ordered tails run as one launch with a workgroup per stream, and all due warps leave in launches of 32 frames.  The members
// stay ordinary vs_stab instances (queues, pyramid rings, keypoint buffers, trajectory state, counters and debug records of
// their own); host and device tables, the events of the schedule, the inverse maps and coordinate tables of the pending warps
// belong to the group.
//
// One step (group_step: its phases in the order they are issued), three streams and the upload stream:
//   up  :  the step's tables, ONE copy                                            (a step or two ahead of the GPU)
//   pre :  gray(n, two parts: re-detecting frames first) -> pyramid level(n) x levels -> [warps of step k - WARP_LAG]
//   det :  zero -> min_eigen -> nms -> select                 (starts behind the first gray part)
//   main:  LK(n x 200 waves) -> RANSAC score -> select(n waves) -> ordered tail (1 WG per stream)
//          -> releases (1 WG per push) -> coordinate tables of this step's warps
// `main` waits for `pre` - through the event behind the warps that `pre` issues in this step once the wide launches of `det` of
// this step are through - and for `det`: at that point the rest of pre/det of this step is done (it overlapped the tracking and
// tail of the step before) and its tracking has not started, and `pre` of the next step lies behind these warps - the HBM-bound
// warp has the GPU to itself (on a stream of its own it overlapped the tracker, which holds ~90 KB of LDS per CU: 3 warp
// workgroups per CU instead of 8).  The warps in that window are those of step k - WARP_LAG (stab_internal.h), not of the step
// before: with a lag of 1 they waited for the whole chain tracker -> scoring -> selection -> tail -> releases of step k - 1, launches
// that keep few compute units busy, and that chain plus the hand-over back to `pre` closed the period.  With a lag of 2 their
// maps and tables are a period old, and the tail chain of step k runs on `main` beside the warps that `pre` issues in step k + 1.
// DESIGN.md section 5 lists every buffer two streams touch with the event that orders them.
#include <cstring>
#include <new>

#include "stab_internal.h"

using namespace vsd;

struct vs_batch {
    int device = 0, S = 0, B = 0, cap = 0;
    bool own = false;                       // the private schedule of one standalone instance
    std::vector<vs_stab*> m;
    // The member whose geometry shapes the group's launches and tables, and on which its stage times are booked: the
    // lowest-numbered member with frames in the step that allocated the group (member 0 unless it had none yet).  Members
    // cannot change their geometry (vs_stab_clean is refused on them): it stays the reference until the group is freed.
    vs_stab* ref = nullptr;
    std::string err;
    // A step that failed after it was numbered leaves its tables and events half done: the group stays failed, and every later
    // step, drain or push of its members returns this first error.  (A standalone instance starts again with vs_stab_clean, which
    // deletes its private group; vs_batch_destroy and vs_stab_destroy work on a failed group.)
    FirstFailure failure;
    hipStream_t st = nullptr, st_pre = nullptr, st_det = nullptr, st_up = nullptr;      // st_up: the table uploads (the pool's warp stream: idle in batch mode)
    bool allocated = false;
    // Host images of the argument tables of a step, in page-locked memory so that their uploads are asynchronous (from pageable
    // memory hipMemcpyAsync holds the host until the stream gets to the copy, and the host then no longer runs ahead of the
    // GPU): host_set().  On the device the tracker / scoring / tail tables exist twice (dev_set()): step k+1's are uploaded
    // while step k's are still read on `main`.
    uint8_t* h_tables = nullptr;
    size_t h_set_bytes = 0, ho_pairs = 0, ho_lk = 0, ho_rs = 0, ho_tail = 0, ho_gf = 0, ho_seg = 0;
    uint8_t* d_all = nullptr;
    uint8_t *d_lk[2] = {nullptr, nullptr}, *d_rs[2] = {nullptr, nullptr}, *d_tail[2] = {nullptr, nullptr}, *d_seg[2] = {nullptr, nullptr}, *d_gf = nullptr;
    uint8_t* d_tin[2] = {nullptr, nullptr};         // per frame of a step: what the selection leaves for the tail
    ImgPair* d_pairs[2] = {nullptr, nullptr};     // (per table set: a step's pair table goes up with its other tables, one copy)
    size_t up_bytes = 0;                 // bytes of a table set that go to the device: pairs, tracker, scoring, tail, segments
    int pre_rel_step = -1;               // the latest step whose tail `pre` has waited for (through the event of its warps' maps)
    double* d_MinvB[2] = {nullptr, nullptr};        // inverse maps of the due frames of a step, 12 doubles each; two sets
    int32_t* d_tabs[2] = {nullptr, nullptr};        // coordinate tables of those frames (warp_tab.h), tab_ints per frame; two sets
    int tab_ints = 0;                               // one plane's table, or an NV12 / I420 surface's block of two
    hipEvent_t ev_bpre = nullptr, ev_bgray = nullptr, ev_bnms = nullptr, ev_bdet[4] = {}, ev_blk[4] = {}, ev_warp[2] = {}, ev_rel[2] = {}, ev_up[2] = {}, ev_go = nullptr;
    bool bdet_valid[4] = {false, false, false, false}, warp_valid[2] = {false, false}, rel_valid[2] = {false, false};
    int last_det_batch = -1, last_warp_set = -1, batch_id = 0, pend_set = 0;
    struct Ready {
        bool valid = false, tabs_built = false;
        int n = 0, set = 0, step = -1;         // step: the group_run that analysed these frames
        size_t stride = 0;
        std::vector<const uint8_t*> srcs;
        std::vector<uint8_t*> dsts;
        std::vector<int> slots, pad_idx;       // pad_idx: which of its owner's scratch frames (border pad / crop-and-zoom)
        std::vector<vs_stab*> owner;
    };
    // The steps whose tails are queued and whose warps are still to come, oldest first (at most WARP_LAG between two steps), and
    // behind them the record of the step being built: pending(i), building().
    static constexpr int NRQ = WARP_LAG + 1;
    Ready rq[NRQ];
    int rq_head = 0, rq_n = 0;
    Ready& pending(int i) { return rq[(rq_head + i) % NRQ]; }
    Ready& building() { return rq[(rq_head + rq_n) % NRQ]; }
    void pop_pending() { rq_head = (rq_head + 1) % NRQ; rq_n--; }

    // ---- which set or event step k uses, and when it comes free: the only places that turn a step number into an index
    // Host images: four sets.  Step k fills its set once blk_event(k - 4), the same event as its own, has passed: the tail of
    // step k-4 is the last reader of anything uploaded from the set.
    struct HostSet { uint8_t* base; ImgPair* pairs; uint8_t *lk, *rs, *tail, *seg, *gf; };
    HostSet host_set(int k) const {
        uint8_t* b = h_tables + (size_t)(k % 4) * h_set_bytes;
        return {b, reinterpret_cast<ImgPair*>(b + ho_pairs), b + ho_lk, b + ho_rs, b + ho_tail, b + ho_seg, b + ho_gf};
    }
    // Device tables, d_tin, ev_up: two sets.  Step k's upload overwrites what step k-2 read: it waits for blk_event(k - 2).
    int dev_set(int k) const { return k & 1; }
    // Recorded on `main` behind the tail of step k: the tables, pyramid slots and keypoint buffers the step read may be reused.
    hipEvent_t blk_event(int k) const { return ev_blk[k % 4]; }
    // Recorded on `det` behind the corner selection of step k, if it detected (det_valid).
    hipEvent_t det_event(int k) const { return ev_bdet[k % 4]; }
    bool& det_valid(int k) { return bdet_valid[k % 4]; }
    // d_MinvB, d_tabs, ev_warp, ev_rel: two sets, taken in turn by the steps that have outputs (pend_set: the next such step's).
    // A set comes free when the warps that read it have run: ev_warp[set], waited for on `main` in front of the tail.  Two are
    // enough for a lag of 1 or 2: the step that takes a set again is the second step with outputs after the one that filled it, so
    // at least two steps later, and the warps of step j are issued in step j + WARP_LAG at the latest, in front of that step's
    // phase on `main` (DESIGN.md section 5 has the argument in full).
    static_assert(WARP_LAG >= 1 && WARP_LAG <= 2, "d_MinvB / d_tabs / ev_warp / ev_rel: two sets cover a lag of at most two steps");
    void flip_pend_set() { pend_set ^= 1; }
    // (WARP_LAG itself stands in stab_internal.h, because the stream sizes its pyramid and frame rings from it.)
    // The warps of a pending step go out in step k once it lies WARP_LAG steps back (every step is numbered, with or without
    // outputs: a step without due frames does not hold up an older one's warps).
    bool warps_due(int k) { return rq_n > 0 && pending(0).step <= k - WARP_LAG; }

    template <typename F>
    void each_event(F f) {          // creation and destruction visit the same events
        for (hipEvent_t* e : {&ev_bpre, &ev_bgray, &ev_bnms, &ev_warp[0], &ev_warp[1], &ev_rel[0], &ev_rel[1], &ev_up[0], &ev_up[1], &ev_go}) f(*e);
        for (auto& e : ev_bdet) f(e);
        for (auto& e : ev_blk) f(e);
    }
};

namespace {

void group_free(vs_batch* g) {
    if (g->h_tables) (void)hipHostFree(g->h_tables);
    if (g->d_all) (void)hipFree(g->d_all);
    g->h_tables = nullptr; g->d_all = nullptr;
    g->allocated = false;
    g->ref = nullptr;
}

bool group_make_events(vs_batch* g) {
    bool ok = true;
    g->each_event([&](hipEvent_t& e) { ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; });
    return ok;
}

// What the members must agree on: everything that shapes a launch (frame and analysis geometry, pitch, input mode, pyramid
// depth, tracking window, hypothesis count, border mode).  Smoothing radius and method, horizon lock, the drone filters'
// settings, corner count and thresholds are per stream: they live in each frame's argument block or in the stream's state.
// (border pad on YUV surfaces: whether it acts - a switch that cannot act, with border_size 0 or behind crop_n_zoom, shapes no
// launch - and the colour its launches fill with: ONE pad launch serves the frames of all members, pad_launch)
static bool same_yuv_pad(const vs_stab* a, const vs_stab* b) {
    const bool on = yuv_pad_on(a);
    if (on != yuv_pad_on(b)) return false;
    if (!on) return true;
    const vs_yuv_fill x = yuv_pad_fill(a), y = yuv_pad_fill(b);
    return x.y == y.y && x.u == y.u && x.v == y.v;
}
// (edge fill on YUV surfaces: whether it acts, and the resolved colour: ONE warp launch serves the frames of all members)
static bool same_yuv_edge_fill(const vs_stab* a, const vs_stab* b) {
    const bool on = yuv_edge_fill_on(a);
    if (on != yuv_edge_fill_on(b)) return false;
    if (!on) return true;
    const vs_yuv_fill x = yuv_edge_fill(a), y = yuv_edge_fill(b);
    return x.y == y.y && x.u == y.u && x.v == y.v;
}
bool same_launch_shape(const vs_stab* a, const vs_stab* b) {
    const vs_params_c &p = a->p, &q = b->p;
    return a->w == b->w && a->h == b->h && a->fmt == b->fmt && a->src_pitch == b->src_pitch && a->zero_copy == b->zero_copy &&
           a->in == b->in && a->out == b->out && a->yuv_cz == b->yuv_cz && same_yuv_pad(a, b) && same_yuv_edge_fill(a, b) &&
           a->aw == b->aw && a->ah == b->ah && a->levels == b->levels &&
           p.lk_win_size == q.lk_win_size && p.ransac_max_iters == q.ransac_max_iters && p.border_size == q.border_size &&
           p.crop_n_zoom == q.crop_n_zoom && (p.border_size <= 0 || p.border_type == q.border_type);
}

// Tables and workspaces for cap = S * B frames per step, once the members know their geometry (g->ref's).
int group_allocate(vs_batch* g) {
    const vs_stab* s0 = g->ref;
    const int cap = g->cap, ngf = g->S * (g->B / 2 + 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_gf = take(gftt_item_bytes() * ngf);
    // a table set on the device = its image on the host (pairs, tracker items, scoring items, tail items, segments: ONE upload per step)
    size_t ho = 0;
    auto htake = [&](size_t bytes) { size_t o = ho; ho += (bytes + 255) & ~(size_t)255; return o; };
    g->ho_pairs = htake(sizeof(ImgPair) * cap * MAX_PYR);
    g->ho_lk = htake(lk_item_bytes() * cap); g->ho_rs = htake(ransac_item_bytes() * cap);
    g->ho_tail = htake(tail_item_bytes() * cap); g->ho_seg = htake(tail_seg_bytes() * g->S);
    g->up_bytes = ho;
    g->ho_gf = htake(gftt_item_bytes() * ngf);
    g->h_set_bytes = ho;
    const size_t o_set[2] = {take(g->up_bytes), take(g->up_bytes)};
    const size_t o_ti[2] = {take(tail_in_bytes() * cap), take(tail_in_bytes() * cap)};
    const size_t o_minv[2] = {take((size_t)cap * 96), take((size_t)cap * 96)};
    int tow, toh;
    out_size(s0, s0->w, s0->h, &tow, &toh);
    // (a YUV stream: tow x toh is the frame's size, or with border pad the padded one, which its warps run at)
    g->tab_ints = s0->pf->three_planes() ? planar_tab_ints(tow, toh, s0->pf->sx, s0->pf->sy) : s0->pf->luma_uv() ? nv12_tab_ints(tow, toh) : (int)warp_tabs_ints(std::max(s0->w, tow), std::max(s0->h, toh), 1);
    size_t o_tabs[2];
    for (auto& o : o_tabs) o = take((size_t)g->tab_ints * cap * sizeof(int32_t));
    VS_OBJ_HIP(g, hipMalloc((void**)&g->d_all, off));
    VS_OBJ_HIP(g, hipMemsetAsync(g->d_all, 0, off, g->st));
    uint8_t* b = g->d_all;
    g->d_gf = b + o_gf;
    for (int i = 0; i < 2; i++) {
        uint8_t* ds = b + o_set[i];
        g->d_pairs[i] = (ImgPair*)(ds + g->ho_pairs);
        g->d_lk[i] = ds + g->ho_lk; g->d_rs[i] = ds + g->ho_rs; g->d_tail[i] = ds + g->ho_tail; g->d_seg[i] = ds + g->ho_seg; g->d_tin[i] = b + o_ti[i];
        g->d_MinvB[i] = (double*)(b + o_minv[i]);
    }
    for (int i = 0; i < 2; i++) g->d_tabs[i] = (int32_t*)(b + o_tabs[i]);
    VS_OBJ_HIP(g, hipHostMalloc((void**)&g->h_tables, 4 * ho));
    memset(g->h_tables, 0, 4 * ho);
    VS_OBJ_HIP(g, hipStreamSynchronize(g->st));
    for (vs_batch::Ready& r : g->rq) {
        r.srcs.assign(cap, nullptr); r.dsts.assign(cap, nullptr); r.slots.assign(cap, -1); r.pad_idx.assign(cap, 0); r.owner.assign(cap, nullptr);
    }
    g->allocated = true;
    return VS_OK;
}

// Where the frames of a step's warps come from and go to (border pad: the padded scratch frame is the source; crop-and-zoom: the
// scratch frame is the destination, resized into the result afterwards).
struct WarpEnds { const uint8_t* src; uint8_t* dst; };
WarpEnds warp_ends(const vs_stab* o, const uint8_t* frame, uint8_t* d_out, int pad_idx, const BorderPlan& bp) {
    if (!bp.pad && !bp.crop) return {frame, d_out};
    return bp.pad ? WarpEnds{scratch(o, pad_idx), d_out} : WarpEnds{frame, scratch(o, pad_idx)};
}

// The warps of one pending step, 32 frames per launch (`what` = VS_WARP_ONLY / VS_WARP_ALL), or only their
// coordinate tables (VS_WARP_TABLES_ONLY: steps whose release workgroups have not built them - a Kalman stream's releases stay
// inside its tail workgroup).  The frames' tables lie tab_ints apart in d_tabs[set].
int group_ready_launches(vs_batch* g, vs_batch::Ready& R, int what, hipStream_t st) {
    const vs_stab* s0 = g->ref;
    const BorderPlan bp = border_plan(s0);
    const bool cz = yuv_cz_on(s0);      // a YUV stream with crop-and-zoom: bp.crop, the scratch surfaces in their own layout
    const bool yp = yuv_pad_on(s0);     // a YUV stream with border pad: bp.pad, the padded scratch surfaces in their own layout
    // (the border of a YUV stream's warps - the edge of a padded plane is its border; edge fill - is chosen where the per-frame path
    // chooses it.  These warps were queued WARP_LAG steps ago: the fill is still theirs, see yuv_warp_border.)
    const YuvBorder wb = s0->pf->kind != PIX_INTERLEAVED ? yuv_warp_border(s0) : YuvBorder{VS_BORDER_BLACK, WarpFill()};
    int rc = VS_OK;
    // (launch by launch: the pads of a launch's frames are queued right in front of it, their crops right behind it)
    for (int i0 = 0; i0 < R.n && rc == VS_OK; i0 += WARP_BATCH_MAX) {
        const int m = std::min(WARP_BATCH_MAX, R.n - i0);
        const uint8_t* srcs[WARP_BATCH_MAX];
        uint8_t* dsts[WARP_BATCH_MAX];
        for (int i = 0; i < m; i++) {
            const WarpEnds e = warp_ends(R.owner[i0 + i], R.srcs[i0 + i], R.dsts[i0 + i], R.pad_idx[i0 + i], bp);
            srcs[i] = e.src; dsts[i] = e.dst;
            // pad: the frames get their border first and the padded frames are warped into the (larger) results
            if (bp.pad && !yp && what != VS_WARP_TABLES_ONLY && rc == VS_OK)
                rc = launch_make_border(R.srcs[i0 + i], s0->src_pitch, s0->w, s0->h, s0->cn, const_cast<uint8_t*>(e.src), bp.prow, bp.b, s0->p.border_type, st);
        }
        // border pad on YUV surfaces: ONE launch in front of the warps pads all the planes of their frames
        if (yp && what != VS_WARP_TABLES_ONLY && rc == VS_OK) rc = pad_launch(s0, &R.srcs[i0], const_cast<uint8_t* const*>(srcs), m, st);
        if (rc != VS_OK) break;
        const WarpMaps maps{g->d_MinvB[R.set] + 12 * i0, 12, false};
        const WarpTabs tabs{WarpTabs::CALLER, g->d_tabs[R.set] + (size_t)i0 * g->tab_ints, g->tab_ints, what};
        if (s0->pf->kind != PIX_INTERLEAVED) {
            // (one output layout per launch: the due frames of a step are all the caller's surfaces or all the host staging)
            rc = warp_planes(srcs, dsts, m, warp_src_planes(s0), warp_dst_planes(s0, dsts[0], R.stride), maps, wb.border, wb.fill, tabs, st);
            // crop-and-zoom on YUV surfaces: ONE launch behind the warps resizes the crops of all their planes into the results
            if (cz && what != VS_WARP_TABLES_ONLY && rc == VS_OK) rc = cz_launch(s0, dsts, &R.dsts[i0], m, R.stride, st);
            continue;
        }
        rc = launch_warp_plane(srcs, dsts, m, bp.pad ? bp.prow : s0->src_pitch, bp.pw, bp.ph, bp.crop ? bp.prow : R.stride, bp.pw, bp.ph, s0->cn, maps,
                               VS_BORDER_BLACK, tabs, st);
        // crop-and-zoom: the inner part of the warped scratch frames is resized to the results
        for (int i = 0; bp.crop && what != VS_WARP_TABLES_ONLY && i < m && rc == VS_OK; i++)
            rc = launch_resize_linear(dsts[i] + ((size_t)bp.b * s0->w + bp.b) * s0->cn, bp.prow, s0->w - 2 * bp.b, s0->h - 2 * bp.b, s0->cn,
                                      R.dsts[i0 + i], R.stride, R.owner[i0 + i]->orig_w, R.owner[i0 + i]->orig_h, st);
    }
    if (rc != VS_OK) g->err = get_last_error();
    return rc;
}

// The warps of the oldest pending step.  They run on `pre`, behind the gray / pyramid work of the step that issues them and in front of
// the next step's: the cycle warps -> gray -> pyramid -> warps that sets the step time is then the order of ONE stream (as launches
// on `main` with events in both directions - the pyramid's to `main`, the warps' back to `pre` - every period paid two event hand-overs,
// 2 x 25 us of 545).  Their maps and tables come from the tail on `main`: ev_rel.
int group_launch_ready(vs_batch* g, hipEvent_t det_done = nullptr) {
    if (g->rq_n == 0) return VS_OK;
    vs_batch::Ready& R = g->pending(0);
    hipStream_t st = g->st_pre;
    int rc;
    // what the warps wait for: the step's maps and tables (ev_rel) and the wide launches of the detector (det_done).  With a lag of
    // 2 ev_rel is a period old and det_done is the one live event: `pre` waits for both itself, det_done last - one hand-over, det ->
    // pre, on the loop that closes the period (gathered into ev_go as below: 0.464 ms a step instead of 0.454, DESIGN.md section 8
    // round 28).  With a lag of 1 both are live, and they are gathered on the upload stream into ONE event: one packet in front of
    // the warps on `pre` instead of two.
    if (g->rel_valid[R.set] || det_done) {
        hipError_t e = hipSuccess;
        if (WARP_LAG >= 2) {
            if (g->rel_valid[R.set]) e = hipStreamWaitEvent(st, g->ev_rel[R.set], 0);
            if (e == hipSuccess && det_done) e = hipStreamWaitEvent(st, det_done, 0);
        } else {
            if (det_done) e = hipStreamWaitEvent(g->st_up, det_done, 0);
            if (e == hipSuccess && g->rel_valid[R.set]) e = hipStreamWaitEvent(g->st_up, g->ev_rel[R.set], 0);
            if (e == hipSuccess) e = hipEventRecord(g->ev_go, g->st_up);
            if (e == hipSuccess) e = hipStreamWaitEvent(st, g->ev_go, 0);
        }
        if (e != hipSuccess) return vs_obj_fail(g, VS_ERR_HIP, "hipStreamWaitEvent failed");
        if (g->rel_valid[R.set]) g->pre_rel_step = std::max(g->pre_rel_step, R.step);
        g->rel_valid[R.set] = false;
    }
    {
        StageScope t(g->ref, VS_STAGE_WARP, st);   // (stage times of a group are booked on its reference member)
        rc = group_ready_launches(g, R, R.tabs_built ? VS_WARP_ONLY : VS_WARP_ALL, st);
    }
    const hipError_t ew = hipEventRecord(g->ev_warp[R.set], st);
    if (ew == hipSuccess) { g->warp_valid[R.set] = true; g->last_warp_set = R.set; }
    else if (rc == VS_OK) rc = hip_fail(ew, "hipEventRecord(g->ev_warp[R.set], st)");
    for (int i = 0; i < R.n; i++) {
        if (!R.owner[i]) continue;
        const int rrc = release_slot(R.owner[i], R.slots[i], st);
        if (rc == VS_OK) rc = rrc;
    }
    R.valid = false;
    g->pop_pending();
    if (rc != VS_OK) g->err = get_last_error();
    return rc;
}

// ---- one step, phase by phase (group_step has the order) -------------------------------------------------------------------

// What the host decides about a step while it fills the tables, for the phases that issue it.
struct StepPlan {
    int k = 0;                          // the step's number
    int n = 0, max_n = 0;               // its frames: in all, the most of one stream
    int n_max = 0;                      // the most keypoints one of them tracks
    int ndet = 0;                       // frames that re-detect
    int npend = 0, nseg = 0;            // outputs that become due; streams (= tail segments)
    int aligned = 1;                    // every frame starts on an 8-byte boundary (what the gray kernels' wide loads need)
    int any_apart = 0, all_apart = 1;   // streams whose releases run apart from their tail workgroup (all but Kalman ones)
    size_t pend_stride = 0;             // output pitch of the due frames
};

// Tracker, scoring and tail items of one stream's frames (table rows first .. first + ns - 1), the stream's tail segment, and its
// part of the step's Ready record: which outputs become due and where their maps go is known on the host.
int fill_stream_items(vs_batch* g, vs_stab* s, const vs_batch::HostSet& H, const BorderPlan& bp, int ndue, int first, StepPlan& P) {
    const vs_params_c& p = s->p;
    const int ns = (int)s->bq.size(), dset = g->dev_set(P.k), set = g->pend_set;
    vs_batch::Ready& R = g->building();     // (the pending records still hold the warps of the steps before)
    int npad = 0;
    for (int i = 0; i < ns; i++) {
        const int idx = first + i;
        const vs_stab::BFrame& b = s->bq[i];
        const vs_stab::ItemBufs& it = s->items[i];
        LKLevel L[MAX_PYR];
        fill_lk_levels(s, b.pv, b.c, L);
        const int cap = std::max(b.lk_cap, 0);
        P.n_max = std::max(P.n_max, cap);
        uint8_t *rs = H.rs + ransac_item_bytes() * idx, *tail = H.tail + tail_item_bytes() * idx;
        VS_OBJ_TRY(g, lk_fill_item(H.lk + lk_item_bytes() * idx, L, s->levels, s->d_pts[b.lk_buf], cap, s->d_npts[b.lk_buf], it.next, it.status, it.err,
                              p.lk_win_size, p.lk_max_iters, p.lk_epsilon));                                    // :611-619
        VS_OBJ_TRY(g, ransac_fill_item(rs, s->d_pts[b.lk_buf], it.next, it.status, cap, s->d_npts[b.lk_buf], it.vp, it.vc, it.m, 4, p.ransac_threshold,
                                  p.ransac_max_iters, s->tab, it.counts, it.model, it.inliers, it.info, s->d_traj, &s->tp, s->d_dbg, b.have_prev_gray));
        ransac_item_set_last(rs, i == ns - 1 ? 1 : 0);
        ransac_item_set_tail_in(rs, g->d_tin[dset] + tail_in_bytes() * idx);
        double* minv = nullptr;
        WarpTabJob jobs[2] = {{nullptr, nullptr, nullptr, 0, 0}, {nullptr, nullptr, nullptr, 0, 0}};
        if (b.out_due) {
            const int j = P.npend++;
            minv = g->d_MinvB[set] + 12 * j;
            R.srcs[j] = b.out_frame; R.dsts[j] = b.d_out; R.slots[j] = b.out_slot; R.owner[j] = s; R.pad_idx[j] = npad;
            // the coordinate tables of a due frame's warp are built by the workgroup that releases the frame (every stream but a
            // Kalman one: those maps come out of the tail workgroup, and the step's tables are a launch of their own behind it)
            // (launches of fewer than four frames - the rest of a step's due frames beyond a multiple of 32 - run without tables)
            if (P.all_apart && std::min(WARP_BATCH_MAX, ndue - j / WARP_BATCH_MAX * WARP_BATCH_MAX) >= WARP_TAB_MIN) {
                const WarpEnds e = warp_ends(s, b.out_frame, b.d_out, npad, bp);
                int32_t* T = g->d_tabs[set] + (size_t)j * g->tab_ints;
                jobs[0] = WarpTabJob{T, e.src, e.dst, bp.pw, bp.ph};
                // the chroma table, in pixels of plane 1 of what the warp reads and fills (a scratch surface with border pad or
                // crop-and-zoom): the UV plane, or the U plane - ONE table, a V tile adds the launch's V - U
                if (s->pf->kind != PIX_INTERLEAVED) {
                    const Planes S = warp_src_planes(s), D = warp_dst_planes(s, e.dst, b.out_stride);
                    jobs[1] = WarpTabJob{T + tab_layout(bp.pw, bp.ph).stride, e.src + S[1].off, e.dst + D[1].off, S[1].w, S[1].h};
                }
            }
            npad++;
            P.pend_stride = b.out_stride;
        }
        tail_fill_item(tail, b.out_due ? 1 : 0, b.out_idx, minv, jobs);
        tail_item_set_seg(tail, P.nseg);
    }
    tail_fill_seg(H.seg + tail_seg_bytes() * P.nseg, first, ns, s->d_M, s->d_traj, s->d_dbg, p.smoothing_method);
    P.any_apart |= p.smoothing_method != VS_SMOOTH_KALMAN;
    P.nseg++;
    return VS_OK;
}

// Pair tables of the gray / pyramid launches: [0] frame -> img[0]; [1..levels] img[l-1] -> img[l].  Level-0 pairs: the frames
// that re-detect first, so that the detector can start after a first, smaller launch.
void fill_pair_tables(const vs_batch* g, const std::vector<vs_stab*>& act, ImgPair* h_pairs, StepPlan& P) {
    const int L = g->ref->levels;
    int n_first = 0, n_rest = 0, i = 0;
    for (vs_stab* s : act)
        for (const vs_stab::BFrame& b : s->bq) {
            const Pyramid& py = s->pyr[b.c];
            const int slot = b.detect ? n_first++ : P.ndet + n_rest++;
            h_pairs[slot] = ImgPair{b.frame, py.img[0]};
            if ((uintptr_t)b.frame % 8) P.aligned = 0;
            for (int l = 1; l <= L; l++) h_pairs[(size_t)l * P.n + i] = ImgPair{py.img[l - 1], py.img[l]};
            i++;
        }
}

// Detector items: every frame of the step that re-detects (and what the members' debug getters will read)
int fill_detector_items(vs_batch* g, const std::vector<vs_stab*>& act, uint8_t* h_gf) {
    int ndet = 0;
    for (vs_stab* s : act) {
        int local = 0;
        for (const vs_stab::BFrame& b : s->bq) {
            if (!b.detect) continue;
            VS_OBJ_TRY(g, gftt_fill_item(h_gf + gftt_item_bytes() * ndet, s->pyr[b.c].img[0], s->aw, s->aw, s->ah, s->pts_cap[b.det_buf], 0.02, 15.0, 3,
                                    s->gws[local], s->d_pts[b.det_buf], s->d_npts[b.det_buf]));                      // :740-744
            s->dbg_det_pts = s->d_pts[b.det_buf]; s->dbg_det_n = s->d_npts[b.det_buf];
            s->dbg_gftt_counters = s->gws[local].counters;
            local++; ndet++;
        }
        s->last_detected = s->bq.back().detect;
    }
    return VS_OK;
}

// Phase 1, host only: the host images of the step's tables (they do not depend on this step's images) and the plan.  The caller
// has made sure that the host set is free.
int step_fill_tables(vs_batch* g, const std::vector<vs_stab*>& act, StepPlan& P) {
    const vs_batch::HostSet H = g->host_set(P.k);
    int ndue = 0;
    for (vs_stab* s : act) {
        for (const vs_stab::BFrame& b : s->bq) { ndue += b.out_due ? 1 : 0; P.ndet += b.detect ? 1 : 0; }
        if (s->p.smoothing_method == VS_SMOOTH_KALMAN) P.all_apart = 0;
    }
    const BorderPlan bp = border_plan(g->ref);
    int first = 0;
    for (vs_stab* s : act) {
        VS_OBJ_TRY(g, fill_stream_items(g, s, H, bp, ndue, first, P));
        first += (int)s->bq.size();
    }
    fill_pair_tables(g, act, H.pairs, P);
    return fill_detector_items(g, act, H.gf);
}

// Phase 2, `up` and `pre`: the table upload, then gray images and pyramids of all frames of the step, one launch per stage and level.
int step_issue_pre(vs_batch* g, const std::vector<vs_stab*>& act, const StepPlan& P, bool warps_go) {
    const vs_stab* s0 = g->ref;
    const int k = P.k, n = P.n, dset = g->dev_set(k);
    hipStream_t pre = g->st_pre;
    if (k >= PYR_STEPS && g->pre_rel_step < k - PYR_STEPS) {
        // ring reuse: these pyramid slots were read by the analysis PYR_STEPS = WARP_LAG + 1 steps ago (batch_pyr_slots).  (When that
        // step had outputs this stream has waited for its tail already, in front of its warps, which it issued in the step before
        // this one: nothing to wait for.  The ring holds one step more than the analysis needs so that this stays true with the
        // warps a step later: a wait for the tail of step k - 2 would be one more packet in front of the gray kernels every step.)
        VS_OBJ_HIP(g, hipStreamWaitEvent(pre, g->blk_event(k - PYR_STEPS), 0));
        if (g->det_valid(k - PYR_STEPS)) VS_OBJ_HIP(g, hipStreamWaitEvent(pre, g->det_event(k - PYR_STEPS), 0));
    }
    // (The HBM-bound warps stay alone on the GPU although the host runs steps ahead: they are launches on this stream, behind the
    // pyramid of the step that issues them and in front of the next step's gray kernels - group_launch_ready.  Round 3 had them on
    // `main` and an event from there that this stream waited for; without that guard 99.0 - 102.4 k frames/s against 112.4 - 114.2 k,
    // warps 182 us instead of 86.)
    for (vs_stab* s : act)
        if (s->bq[0].prev_small) {   // Stabilizer.cpp:598-603 (once per stream: 480x270 -> analysis size)
            StageScope t(g->ref, VS_STAGE_PYRAMID, pre);
            VS_OBJ_TRY(g, launch_resize_gray(s->d_first_gray, 480, 480, 270, VS_FMT_GRAY8, s->pyr[s->bq[0].pv].img[0], s->aw, s->aw, s->ah, pre));
            VS_OBJ_TRY(g, build_pyramid(s, s->bq[0].pv, pre));
        }
    // ONE upload per step: the pair tables of the gray / pyramid launches and, behind them in the set, the tables of the tracker,
    // the scoring and the tail.  (As five copies - the four small ones in the middle of `pre`, which had slack
    // while the warps ran on `main` - they stood 46 us on what is the step's longest chain since the warps run on this stream.)
    // The copy runs on a stream of its own: the host is a step or two ahead of the GPU, so the tables are there long before `pre`
    // gets to this step (as a copy on `pre` it stood between the warps and the gray kernels: 26 us of hand-over to the copy engine
    // and back on the step's longest chain).  The set was last used by step k - 2: its tail must have run.
    ImgPair* const d_pairs = g->d_pairs[dset];
    if (k >= 2) VS_OBJ_HIP(g, hipStreamWaitEvent(g->st_up, g->blk_event(k - 2), 0));
    VS_OBJ_HIP(g, hipMemcpyAsync(d_pairs, g->host_set(k).base, g->up_bytes, hipMemcpyHostToDevice, g->st_up));
    VS_OBJ_HIP(g, hipEventRecord(g->ev_up[dset], g->st_up));
    VS_OBJ_HIP(g, hipStreamWaitEvent(pre, g->ev_up[dset], 0));
    {
        StageScope t(g->ref, VS_STAGE_GRAY, pre);
        // NV12, I420: the Y plane is the gray image (no reference path; same policy as the per-frame pipeline); P010: the high bytes
        // of the Y plane's samples are, I010 / I012: their values shifted down to 8 bits (the resize kernels read them in place)
        const int gfmt = s0->pf->gray_source;
        const int n_a = (P.ndet > 0 && P.ndet < n) ? P.ndet : n;
        VS_OBJ_TRY(g, launch_resize_gray_batch(d_pairs, n_a, s0->src_pitch, s0->w, s0->h, gfmt, s0->aw, s0->aw, s0->ah, P.aligned, pre));  // :448-450
        VS_OBJ_HIP(g, hipEventRecord(g->ev_bgray, pre));      // the detector needs the analysis images of its frames only
        if (n_a < n)
            VS_OBJ_TRY(g, launch_resize_gray_batch(d_pairs + n_a, n - n_a, s0->src_pitch, s0->w, s0->h, gfmt, s0->aw, s0->aw, s0->ah, P.aligned, pre));
    }
    {
        StageScope t(g->ref, VS_STAGE_PYRAMID, pre);
        // One pyrDown launch per level (pyr_level_kernel): the tracker computes the derivatives it needs from the images.
        for (int l = 0; l < s0->levels; l++)
            VS_OBJ_TRY(g, launch_pyr_level_batch(nullptr, d_pairs + (size_t)(l + 1) * n, n, s0->lw[l], s0->lw[l], s0->lh[l], s0->lw[l + 1], pre));
    }
    // (`main` waits for the event behind this step's warps when there are any: it covers the pyramid, which lies in front of them)
    if (!warps_go) VS_OBJ_HIP(g, hipEventRecord(g->ev_bpre, pre));
    return VS_OK;
}

// Phase 3, `det`: every frame of the step that re-detects, one launch per GFTT stage.
int step_issue_det(vs_batch* g, const StepPlan& P) {
    const vs_stab* s0 = g->ref;
    const int k = P.k, ndet = P.ndet;
    hipStream_t sd = g->st_det;
    g->det_valid(k) = ndet > 0;
    if (ndet == 0) return VS_OK;
    // starts as soon as the analysis images of its frames exist, next to the pyramid levels of this step and the tracking of
    // the previous one (the table and the reset of the counters first: they are through by the time the images are)
    VS_OBJ_HIP(g, hipMemcpyAsync(g->d_gf, g->host_set(k).gf, gftt_item_bytes() * ndet, hipMemcpyHostToDevice, sd));
    // keypoint buffers are recycled after B + 4 detections (two steps): the tracking of the step before the previous one
    // must have read them (the GFTT scratch is only touched on this stream)
    if (k >= 2) VS_OBJ_HIP(g, hipStreamWaitEvent(sd, g->blk_event(k - 2), 0));
    VS_OBJ_TRY(g, launch_gftt_batch(g->d_gf, ndet, s0->aw, s0->ah, 3, sd, 1));
    VS_OBJ_HIP(g, hipStreamWaitEvent(sd, g->ev_bgray, 0));
    {
        StageScope t(g->ref, VS_STAGE_GFTT, sd);
        VS_OBJ_TRY(g, launch_gftt_batch(g->d_gf, ndet, s0->aw, s0->ah, 3, sd, 4));
        VS_OBJ_TRY(g, launch_gftt_batch(g->d_gf, ndet, s0->aw, s0->ah, 3, sd, 5));
        // the wide launches of the detection are through: the warps of the step before may go; the selection -
        // one workgroup per image - runs beside them
        VS_OBJ_HIP(g, hipEventRecord(g->ev_bnms, sd));
        VS_OBJ_TRY(g, launch_gftt_batch(g->d_gf, ndet, s0->aw, s0->ah, 3, sd, 3));
    }
    VS_OBJ_HIP(g, hipEventRecord(g->det_event(k), sd));
    g->last_det_batch = k;
    return VS_OK;
}

// Phase 5, `main`: tracking and hypothesis scoring of all frames, one launch each, and the ordered tails.  warps_go: warps of
// an earlier step were issued in front of this phase; kd: the step whose detection selected the corners the tracker reads (-1: none
// that `main` has not waited for).
int step_issue_main(vs_batch* g, const std::vector<vs_stab*>& act, const StepPlan& P, bool warps_go, int kd) {
    const vs_stab* s0 = g->ref;
    const int dset = g->dev_set(P.k), set = g->pend_set;
    hipStream_t st = g->st;
    // waits for this step's gray / pyramid work, its corners and - the tracker takes every vector register of every SIMD,
    // beside it the warps would crawl - the warps just issued
    if (warps_go && g->last_warp_set >= 0) VS_OBJ_HIP(g, hipStreamWaitEvent(st, g->ev_warp[g->last_warp_set], 0));
    else VS_OBJ_HIP(g, hipStreamWaitEvent(st, g->ev_bpre, 0));
    for (vs_stab* s : act)
        if (s->pts_pending[0]) { VS_OBJ_HIP(g, hipStreamWaitEvent(st, s->pts_event[0], 0)); s->pts_pending[0] = false; }
    if (kd >= 0) VS_OBJ_HIP(g, hipStreamWaitEvent(st, g->det_event(kd), 0));       // the tracker needs the selected corners
    {
        StageScope t(g->ref, VS_STAGE_LK, st);
        VS_OBJ_TRY(g, launch_pyr_lk_batch(g->d_lk[dset], P.n, P.n_max, s0->p.lk_win_size, st));
    }
    {
        StageScope t(g->ref, VS_STAGE_RANSAC, st);
        VS_OBJ_TRY(g, launch_ransac_score_batch(g->d_rs[dset], P.n, s0->p.ransac_max_iters, P.n_max, st));
    }
    for (vs_stab* s : act)
        if (s->dbg_delay_us > 0) { VS_OBJ_TRY(g, launch_spin(s->dbg_delay_us, st)); break; }
    // ---- ordered tails, ONE launch (a workgroup per stream): per frame in push order the trajectory append (:644-693), then
    // the map of the output that has become due (applyNextSmoothTransform sees exactly the transforms appended so far)
    if (P.npend > 0 && g->warp_valid[set]) {         // the previous user of this set of maps must have read them
        VS_OBJ_HIP(g, hipStreamWaitEvent(st, g->ev_warp[set], 0));
        g->warp_valid[set] = false;
    }
    {
        StageScope t(g->ref, VS_STAGE_TRAJ, st);
        VS_OBJ_TRY(g, launch_ransac_tail_group(g->d_rs[dset], g->d_tail[dset], g->d_seg[dset], g->d_tin[dset], P.nseg, P.max_n, P.n, P.any_apart, st));
    }
    // the keypoint and pyramid buffers of this step may be recycled (two steps on) once the tail, which still reads the points
    // and their counts, has run
    VS_OBJ_HIP(g, hipEventRecord(g->blk_event(P.k), st));
    return VS_OK;
}

// Phase 6: the step's due frames become the newest pending record.  Their warps wait for step k + WARP_LAG (or a drain); their
// maps exist once the tail has run, and the coordinate tables are built right behind it.
int step_publish(vs_batch* g, const std::vector<vs_stab*>& act, const StepPlan& P) {
    const int set = g->pend_set;
    vs_batch::Ready& R = g->building();
    R.n = P.npend; R.set = set; R.stride = P.pend_stride; R.valid = P.npend > 0; R.tabs_built = P.all_apart != 0; R.step = P.k;
    if (R.valid) {
        g->rq_n++;                           // (at most WARP_LAG pending now: this step has issued what lay that far back)
        g->flip_pend_set();
        if (!R.tabs_built) {                 // (a Kalman stream in the step: the tables as a launch behind the tail)
            StageScope t(g->ref, VS_STAGE_WARP_TABLES, g->st);
            VS_OBJ_TRY(g, group_ready_launches(g, R, VS_WARP_TABLES_ONLY, g->st));
            R.tabs_built = true;
        }
        VS_OBJ_HIP(g, hipEventRecord(g->ev_rel[set], g->st));          // maps and tables of this step's warps exist
        g->rel_valid[set] = true;
    }
    for (vs_stab* s : act) {
        const vs_stab::BFrame& lb = s->bq.back();
        const int nl = (int)s->bq.size();
        s->dbg_prev_pts = s->d_pts[lb.lk_buf]; s->dbg_next = s->items[nl - 1].next;
        s->dbg_status = s->items[nl - 1].status; s->dbg_inliers = s->items[nl - 1].inliers;
        s->bq.clear();
    }
    return VS_OK;
}

// The step numbered k over the frames of `act` (n in all, at most max_n per stream), once group_run has accepted them.
int group_step(vs_batch* g, const std::vector<vs_stab*>& act, int n, int max_n, int k) {
    StepPlan P;
    P.k = k; P.n = n; P.max_n = max_n;
    // the host set of step k-4: its tail has run by now unless the host is four steps ahead of the GPU - then it waits here
    if (k >= 4) VS_OBJ_HIP(g, hipEventSynchronize(g->blk_event(k - 4)));
    VS_OBJ_TRY(g, step_fill_tables(g, act, P));
    const bool warps_go = g->warps_due(k);
    VS_OBJ_TRY(g, step_issue_pre(g, act, P, warps_go));
    VS_OBJ_TRY(g, step_issue_det(g, P));
    // The warps of step k - WARP_LAG go out here, on `pre` behind this step's pyramid, once the wide launches of this step's
    // detection are through: nothing but the corner selection (a workgroup per image) and, with a lag of 2, the tail chain of
    // the step before runs beside them.  (A step without a detection: once the selection of the step before, whose corners the
    // tracker still needs, is through.)  Their maps and tables (ev_rel) are WARP_LAG - 1 periods old.
    const int kd = (g->last_det_batch >= 0 && g->last_det_batch >= k - 1) ? g->last_det_batch : -1;
    const hipEvent_t det_done = kd == k ? g->ev_bnms : (kd >= 0 ? g->det_event(kd) : (hipEvent_t) nullptr);
    while (g->warps_due(k)) VS_OBJ_TRY(g, group_launch_ready(g, det_done));      // (one record per step: one turn, oldest first)
    VS_OBJ_TRY(g, step_issue_main(g, act, P, warps_go, kd));
    return step_publish(g, act, P);
}

}  // namespace

bool group_holds_warps(const vs_batch* g) { return g && g->rq_n > 0; }

const FirstFailure& group_failure(const vs_batch* g) { return g->failure; }

// One step: everything the members have queued.  What refuses a step is decided before it is numbered; a failure after that
// leaves the group failed (group_failure).
int group_run(vs_batch* g) {
    if (g->failure.rc != VS_OK) return vs_obj_fail(g, g->failure.rc, g->failure.msg);
    std::vector<vs_stab*> act;
    int n = 0, max_n = 0;
    for (vs_stab* s : g->m)
        if (!s->bq.empty()) { act.push_back(s); n += (int)s->bq.size(); max_n = std::max(max_n, (int)s->bq.size()); }
    if (n == 0) return VS_OK;
    VS_OBJ_HIP(g, hipSetDevice(g->device));
    // every member with frames in this step has the reference's launch shape; the group's first step makes its first active
    // member the reference (a member that has had no frame yet - a camera that connects late - has no geometry to compare)
    const vs_stab* s0 = g->ref ? g->ref : act[0];
    size_t out_stride = 0;
    int ndue = 0;
    for (vs_stab* s : act) {
        if (!s->allocated || !s->batch_active || !same_launch_shape(s, s0))
            return vs_obj_fail(g, VS_ERR_INVALID_ARG, "vs_batch: the streams of a group share one frame geometry, pitch, input mode and launch shape "
                                                "(analysis size, pyramid depth, tracking window, hypothesis count, border mode)");
        for (const vs_stab::BFrame& b : s->bq) {
            if (!b.out_due) continue;
            if (ndue++ > 0 && out_stride != b.out_stride) return vs_obj_fail(g, VS_ERR_INVALID_ARG, "batch mode: one output pitch per step");
            out_stride = b.out_stride;
        }
    }
    if (n > g->cap || max_n > BATCH_MAX) return vs_obj_fail(g, VS_ERR_CAPACITY, "vs_batch: more frames queued than a step holds");
    if (!g->allocated) {
        g->ref = act[0];
        const int rc = group_allocate(g);
        if (rc != VS_OK) { group_free(g); return rc; }
    }
    const int rc = group_step(g, act, n, max_n, g->batch_id++);
    g->failure.note(rc, g->err);
    return rc;
}

// Everything the members have queued is analysed and its warps are issued.  (The warps of a step normally go out WARP_LAG steps
// later, between that step's detection and its tracking; group_run issues the ones that are due on its way, and whatever is
// still pending then - up to WARP_LAG steps - goes out here, oldest first, each step's warps with their own stage scope and ev_warp.)
int group_drain(vs_batch* g) {
    VS_OBJ_HIP(g, hipSetDevice(g->device));
    VS_OBJ_TRY(g, group_run(g));                 // (nothing queued: nothing done)
    int rc = VS_OK;
    while (g->rq_n > 0 && rc == VS_OK) rc = group_launch_ready(g);
    g->failure.note(rc, g->err);
    return rc;
}

void group_delete(vs_batch* g) {
    if (!g) return;
    group_free(g);
    g->each_event([](hipEvent_t& e) { if (e) { (void)hipEventDestroy(e); e = nullptr; } });
    delete g;
}

// The private schedule of a standalone instance in batch mode: a group of one, steps of `batch` frames.
vs_batch* group_new_own(vs_stab* s) {
    vs_batch* g = new (std::nothrow) vs_batch();
    if (!g) { set_last_error("out of host memory"); return nullptr; }
    g->device = s->device; g->S = 1; g->B = s->batch; g->cap = s->batch; g->own = true;
    g->m.push_back(s);
    g->st = s->st; g->st_pre = s->st_pre; g->st_det = s->st_det; g->st_up = s->st_warp;
    if (!group_make_events(g)) { set_last_error("hipEventCreate failed"); group_delete(g); return nullptr; }
    return g;
}

namespace {
// vs_stab_* calls that vs_batch_* makes on a member
struct MemberCall {
    vs_stab* s;
    explicit MemberCall(vs_stab* s_) : s(s_) { s->group_call = true; }
    ~MemberCall() { s->group_call = false; }
};
}  // namespace

extern "C" {

// params: ONE block for all streams (per_stream = 0) or n_streams blocks.  Per-stream blocks may differ in everything that does
// not shape a launch (same_launch_shape): smoothing radius and method, horizon lock, the drone filters' settings, corner count.
static int batch_create(int device, int n_streams, const vs_params_c* params, int per_stream, int frames_per_step, vs_batch** out) {
    if (!out) return VS_ERR_INVALID_ARG;
    *out = nullptr;
    if (!params || n_streams < 1 || n_streams > 256 || frames_per_step < 1 || frames_per_step > BATCH_MAX) {
        set_last_error("vs_batch_create: 1..256 streams, 1..64 frames per stream and step");
        return VS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < (per_stream ? n_streams : 1); i++) {
        const vs_params_c& p = params[i];
        if (p.struct_size != (int32_t)sizeof(vs_params_c)) { set_last_error("params: struct_size mismatch"); return VS_ERR_INVALID_ARG; }
        // modes whose outputs depend on each other or on a host decision per output run in the per-frame pipeline only
        if (p.adaptive_smoothing || (p.border_size > 0 && !p.crop_n_zoom && p.border_type == VS_BORDER_FADE) || (p.enable_virtual_canvas && !p.crop_n_zoom)) {
            set_last_error("vs_batch_create: adaptive smoothing, the fade border and the virtual canvas are per-stream modes (use vs_stab_*)");
            return VS_ERR_UNSUPPORTED;
        }
    }
    vs_batch* g = new (std::nothrow) vs_batch();
    if (!g) return VS_ERR_HIP;
    g->device = device; g->S = n_streams; g->B = frames_per_step; g->cap = n_streams * frames_per_step;
    for (int i = 0; i < n_streams; i++) {
        vs_stab* s = nullptr;
        int rc = vs_stab_create(&params[per_stream ? i : 0], device, &s);
        if (rc == VS_OK) rc = vs_stab_set_batch(s, frames_per_step);
        if (rc != VS_OK) { if (s) vs_stab_destroy(s); vs_batch_destroy(g); return rc; }
        s->group = g; s->member = true;
        g->m.push_back(s);
    }
    g->st = g->m[0]->st; g->st_pre = g->m[0]->st_pre; g->st_det = g->m[0]->st_det; g->st_up = g->m[0]->st_warp;
    if (!group_make_events(g)) { set_last_error("vs_batch_create: hipEventCreate failed"); vs_batch_destroy(g); return VS_ERR_HIP; }
    *out = g;
    return VS_OK;
}

int vs_batch_create(int device, int n_streams, const vs_params_c* params, int frames_per_step, vs_batch** out) {
    return batch_create(device, n_streams, params, 0, frames_per_step, out);
}

int vs_batch_create_params(int device, int n_streams, const vs_params_c* params_per_stream, int frames_per_step, vs_batch** out) {
    return batch_create(device, n_streams, params_per_stream, 1, frames_per_step, out);
}

void vs_batch_destroy(vs_batch* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)sync_streams({g->st_pre, g->st_det, g->st});
    for (vs_stab* s : g->m) { s->group = nullptr; s->member = false; s->bq.clear(); vs_stab_destroy(s); }
    group_delete(g);
}

int vs_batch_streams(const vs_batch* g) { return g ? g->S : 0; }
vs_stab* vs_batch_stream(vs_batch* g, int i) { return (g && i >= 0 && i < g->S) ? g->m[(size_t)i] : nullptr; }
const char* vs_batch_last_error(const vs_batch* g) { return g ? g->err.c_str() : ""; }

int vs_batch_set_zero_copy(vs_batch* g, int enable) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) { MemberCall mc(s); const int rc = vs_stab_set_zero_copy(s, enable); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

int vs_batch_set_nv12_layout(vs_batch* g, size_t in_uv_offset, size_t out_uv_offset) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) { MemberCall mc(s); const int rc = vs_stab_set_nv12_layout(s, in_uv_offset, out_uv_offset); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

int vs_batch_set_i420_layout(vs_batch* g, size_t in_u_off, size_t in_v_off, size_t in_c_pitch, size_t out_u_off, size_t out_v_off, size_t out_c_pitch) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) {
        MemberCall mc(s);
        const int rc = vs_stab_set_i420_layout(s, in_u_off, in_v_off, in_c_pitch, out_u_off, out_v_off, out_c_pitch);
        if (rc != VS_OK) { g->err = s->err; return rc; }
    }
    return VS_OK;
}

int vs_batch_set_yuv_crop_zoom(vs_batch* g, int enable) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) { MemberCall mc(s); const int rc = vs_stab_set_yuv_crop_zoom(s, enable); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

int vs_batch_set_yuv_border_pad(vs_batch* g, int enable, const vs_yuv_fill* fill) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) { MemberCall mc(s); const int rc = vs_stab_set_yuv_border_pad(s, enable, fill); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

int vs_batch_set_yuv_edge_fill(vs_batch* g, int enable, const vs_yuv_fill* fill) {
    if (!g) return VS_ERR_INVALID_ARG;
    for (vs_stab* s : g->m) { MemberCall mc(s); const int rc = vs_stab_set_yuv_edge_fill(s, enable, fill); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

int vs_batch_push_dev(vs_batch* g, const void* const* d_frames, int w, int h, size_t stride, int fmt, void* const* d_outs, size_t out_stride,
                      int* produced) {
    if (!g || !d_frames || !d_outs || !produced) return VS_ERR_INVALID_ARG;
    for (int i = 0; i < g->S; i++) produced[i] = 0;
    if (g->failure.rc != VS_OK) return vs_obj_fail(g, g->failure.rc, g->failure.msg);
    bool full = false;
    for (int i = 0; i < g->S; i++) {
        if (!d_frames[i]) continue;                       // no frame for this stream in this call
        vs_stab* s = g->m[(size_t)i];
        MemberCall mc(s);
        const int rc = vs_stab_push_dev(s, d_frames[i], w, h, stride, fmt, d_outs[i], out_stride, &produced[i]);
        if (rc != VS_OK) { g->err = s->err; return rc; }
        full |= (int)s->bq.size() >= g->B;
    }
    if (full) return group_run(g);
    return VS_OK;
}

int vs_batch_flush_dev(vs_batch* g, void* const* d_outs, size_t out_stride, int* produced) {
    if (!g || !d_outs || !produced) return VS_ERR_INVALID_ARG;
    int rc = group_drain(g);
    if (rc != VS_OK) return rc;
    for (int i = 0; i < g->S; i++) {
        produced[i] = 0;
        MemberCall mc(g->m[(size_t)i]);
        rc = vs_stab_flush_dev(g->m[(size_t)i], d_outs[i], out_stride, &produced[i]);
        if (rc != VS_OK) { g->err = g->m[(size_t)i]->err; return rc; }
    }
    return VS_OK;
}

int vs_batch_sync(vs_batch* g) {
    if (!g) return VS_ERR_INVALID_ARG;
    int rc = group_drain(g);
    if (rc != VS_OK) return rc;
    for (vs_stab* s : g->m) { rc = vs_stab_sync(s); if (rc != VS_OK) { g->err = s->err; return rc; } }
    return VS_OK;
}

}  // extern "C"
