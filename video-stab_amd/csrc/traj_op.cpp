// vs_op_trajectory (include/vs_stab.h): the trajectory kernels of the pipeline driven with given models.  Nothing is computed
// here: the append is traj_append_device (through a one-lane kernel), the per-frame release launch_traj_emit, the batch form
// launch_ransac_tail_group with tables filled as batch_schedule.cpp fills them, and the queue rule is release_due().
#include <cmath>
#include <cstring>
#include <deque>
#include <vector>

#include "stab_internal.h"

using namespace vsd;

namespace {

struct DevMem {                       // device allocations of one call, freed on every way out
    std::vector<void*> p;
    hipStream_t st = nullptr;
    ~DevMem() {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T> int get(T** out, size_t bytes) {
        void* q = nullptr;
        VS_HIP_TRY(hipMalloc(&q, bytes ? bytes : 16));
        p.push_back(q);
        *out = static_cast<T*>(q);
        return VS_OK;
    }
};

struct Stream {
    TrajState* traj = nullptr; float* M = nullptr; double* Minv = nullptr; vs_debug_frame* dbg = nullptr; double* models = nullptr;
    std::deque<int> queue;            // frames waiting for their release (Stabilizer.cpp:376-377)
    int host_radius = 0, next = 0, n_dbg = 0, n_rel = 0;
};

int fetch_dbg(Stream& s, vs_debug_frame* out, hipStream_t st) {
    VS_HIP_TRY(hipMemcpyAsync(&out[s.n_dbg], s.dbg, sizeof(vs_debug_frame), hipMemcpyDeviceToHost, st));
    VS_HIP_TRY(hipStreamSynchronize(st));
    s.n_dbg++;
    return VS_OK;
}

// one release through the per-frame emit kernel (apply_next / flush_dev_impl of stabilizer.cpp)
int emit_one(Stream& s, const TrajParams& tp, int push, int n_seen, vs_traj_release* rel, hipStream_t st) {
    const int idx = s.queue.front();
    s.queue.pop_front();
    VS_TRY(launch_traj_emit(s.traj, tp, idx, s.M, s.Minv, s.dbg, st));
    vs_traj_release& r = rel[s.n_rel++];
    r.push = push; r.idx = idx; r.n_seen = n_seen; r.has_M = 1;
    VS_HIP_TRY(hipMemcpyAsync(r.M, s.M, sizeof r.M, hipMemcpyDeviceToHost, st));
    VS_HIP_TRY(hipMemcpyAsync(r.Minv, s.Minv, sizeof r.Minv, hipMemcpyDeviceToHost, st));
    VS_HIP_TRY(hipStreamSynchronize(st));
    return VS_OK;
}

}  // namespace

extern "C" int vs_op_trajectory(const vs_params_c* params, int n_streams, const double* const* models, const int32_t* const* kinds,
                                const int32_t* n_push, int form, const int32_t* steps, int n_steps, vs_debug_frame* const* dbg_out,
                                int32_t* n_dbg, vs_traj_release* const* rel_out, int32_t* n_rel) {
    if (!params || params->struct_size != (int32_t)sizeof(vs_params_c) || n_streams < 1 || n_streams > 64 || !models || !kinds || !n_push ||
        (form != 0 && form != 1) || !dbg_out || !n_dbg || !rel_out || !n_rel || (form == 0 && n_streams != 1) ||
        (form == 1 && (!steps || n_steps < 1))) {
        set_last_error("vs_op_trajectory: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    for (int k = 0; form == 1 && k < n_steps; k++)
        if (steps[k] < 1 || steps[k] > 64) { set_last_error("vs_op_trajectory: a step holds 1 to 64 pushes"); return VS_ERR_INVALID_ARG; }
    for (int s = 0; s < n_streams; s++)
        if (n_push[s] < 0 || !models[s] || !kinds[s] || !dbg_out[s] || !rel_out[s]) { set_last_error("vs_op_trajectory: invalid stream"); return VS_ERR_INVALID_ARG; }
    const vs_params_c& p = *params;
    if (p.smoothing_method < 0 || p.smoothing_method > VS_SMOOTH_KALMAN) { set_last_error("smoothing_method out of range"); return VS_ERR_INVALID_ARG; }
    if (p.smoothing_method == VS_SMOOTH_GAUSSIAN) {
        const float sigma = (float)p.gaussian_sigma;
        int ks = sigma > 0.0f ? std::max(3, (int)std::ceil(6 * sigma)) : GAUSS_MAX + 1;
        if (ks % 2 == 0) ks++;
        if (ks > GAUSS_MAX) { set_last_error("gaussianSigma outside the accelerated path"); return VS_ERR_UNSUPPORTED; }
    }
    if (form == 1 && p.adaptive_smoothing) { set_last_error("adaptive smoothing is a per-frame mode"); return VS_ERR_UNSUPPORTED; }
    VS_TRY(ensure_device());
    TrajParams tp;
    fill_traj_params(p, tp);
    DevMem mem;
    VS_HIP_TRY(hipStreamCreateWithFlags(&mem.st, hipStreamNonBlocking));
    hipStream_t st = mem.st;
    std::vector<Stream> S((size_t)n_streams);
    for (int s = 0; s < n_streams; s++) {
        Stream& x = S[(size_t)s];
        VS_TRY(mem.get(&x.traj, sizeof(TrajState)));
        VS_TRY(mem.get(&x.M, 12 * sizeof(float)));
        VS_TRY(mem.get(&x.Minv, 12 * sizeof(double)));
        VS_TRY(mem.get(&x.dbg, sizeof(vs_debug_frame)));
        VS_TRY(mem.get(&x.models, (size_t)n_push[s] * 6 * sizeof(double)));
        VS_HIP_TRY(hipMemsetAsync(x.traj, 0, sizeof(TrajState), st));
        VS_HIP_TRY(hipMemsetAsync(x.M, 0, 12 * sizeof(float), st));
        VS_HIP_TRY(hipMemsetAsync(x.dbg, 0, sizeof(vs_debug_frame), st));
        if (n_push[s] > 0) VS_HIP_TRY(hipMemcpyAsync(x.models, models[s], (size_t)n_push[s] * 6 * sizeof(double), hipMemcpyHostToDevice, st));
        VS_TRY(launch_traj_reset(x.traj, p.smoothing_radius, st));
        x.host_radius = p.smoothing_radius;
        x.queue.push_back(0);             // the first frame only enters the queue (push_common)
    }
    VS_HIP_TRY(hipStreamSynchronize(st));

    if (form == 0) {
        Stream& x = S[0];
        for (int i = 0; i < n_push[0]; i++) {
            const int kind = kinds[0][i];
            x.queue.push_back(i + 1);
            VS_TRY(launch_traj_append(x.traj, tp, x.models + 6 * (size_t)i, kind > 0 ? 1 : 0, kind < 0 ? 0 : 1, 1, x.dbg, st));
            if (p.adaptive_smoothing) {       // the radius is data dependent in this mode and moves the queue's threshold (push_common)
                VS_HIP_TRY(hipMemcpyAsync(&x.host_radius, &x.traj->smoothing_radius, sizeof(int), hipMemcpyDeviceToHost, st));
                VS_HIP_TRY(hipStreamSynchronize(st));
            }
            if (release_due(x.queue.size(), x.host_radius)) VS_TRY(emit_one(x, tp, i, i + 1, rel_out[0], st));
            VS_TRY(fetch_dbg(x, dbg_out[0], st));
        }
    } else {
        const size_t rb = ransac_item_bytes(), tb = tail_item_bytes(), sb = tail_seg_bytes(), ib = tail_in_bytes();
        const size_t cap = (size_t)n_streams * 64;
        std::vector<uint8_t> h_rs(rb * cap), h_tail(tb * cap), h_seg(sb * (size_t)n_streams), h_tin(ib * cap);
        uint8_t *d_rs, *d_tail, *d_seg, *d_tin;
        double* d_minv;
        VS_TRY(mem.get(&d_rs, h_rs.size())); VS_TRY(mem.get(&d_tail, h_tail.size())); VS_TRY(mem.get(&d_seg, h_seg.size()));
        VS_TRY(mem.get(&d_tin, h_tin.size())); VS_TRY(mem.get(&d_minv, cap * 12 * sizeof(double)));
        std::vector<double> h_minv(cap * 12);
        struct Due { int stream, push, idx, n_seen, last; };
        for (int k = 0;; k++) {
            const int step = steps[k % n_steps];
            int items = 0, nseg = 0, max_n = 0, any_apart = 0;
            std::vector<Due> due;
            std::vector<int> act;
            for (int s = 0; s < n_streams; s++) {
                Stream& x = S[(size_t)s];
                const int ns = std::min(step, n_push[s] - x.next);
                if (ns <= 0) continue;
                const int first = items;
                int last_due = -1;
                for (int j = 0; j < ns; j++, items++) {
                    const int i = x.next + j, kind = kinds[s][i];
                    ransac_fill_item_traj(h_rs.data() + rb * (size_t)items, x.traj, &tp, x.dbg);
                    ransac_item_set_last(h_rs.data() + rb * (size_t)items, j == ns - 1 ? 1 : 0);
                    tail_in_fill(h_tin.data() + ib * (size_t)items, models[s] + 6 * (size_t)i, kind > 0 ? 1 : 0, kind < 0 ? 0 : 1, 1);
                    x.queue.push_back(i + 1);                                       // batch_enqueue
                    int out_due = 0, out_idx = 0;
                    double* minv = nullptr;
                    if (release_due(x.queue.size(), x.host_radius)) {
                        out_due = 1; out_idx = x.queue.front();
                        x.queue.pop_front();
                        minv = d_minv + 12 * due.size();
                        last_due = (int)due.size();
                        due.push_back(Due{s, i, out_idx, i + 1, 0});
                    }
                    tail_fill_item(h_tail.data() + tb * (size_t)items, out_due, out_idx, minv, nullptr);
                    tail_item_set_seg(h_tail.data() + tb * (size_t)items, nseg);
                }
                if (last_due >= 0) due[(size_t)last_due].last = 1;
                tail_fill_seg(h_seg.data() + sb * (size_t)nseg, first, ns, x.M, x.traj, x.dbg, p.smoothing_method);
                any_apart |= p.smoothing_method != VS_SMOOTH_KALMAN;              // fill_stream_items
                max_n = std::max(max_n, ns);
                x.next += ns;
                act.push_back(s);
                nseg++;
            }
            if (items == 0) break;
            VS_HIP_TRY(hipMemcpyAsync(d_rs, h_rs.data(), rb * (size_t)items, hipMemcpyHostToDevice, st));
            VS_HIP_TRY(hipMemcpyAsync(d_tail, h_tail.data(), tb * (size_t)items, hipMemcpyHostToDevice, st));
            VS_HIP_TRY(hipMemcpyAsync(d_seg, h_seg.data(), sb * (size_t)nseg, hipMemcpyHostToDevice, st));
            VS_HIP_TRY(hipMemcpyAsync(d_tin, h_tin.data(), ib * (size_t)items, hipMemcpyHostToDevice, st));
            VS_TRY(launch_ransac_tail_group(d_rs, d_tail, d_seg, d_tin, nseg, max_n, items, any_apart, st));
            if (!due.empty()) VS_HIP_TRY(hipMemcpyAsync(h_minv.data(), d_minv, due.size() * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
            VS_HIP_TRY(hipStreamSynchronize(st));
            for (size_t j = 0; j < due.size(); j++) {
                Stream& x = S[(size_t)due[j].stream];
                vs_traj_release& r = rel_out[due[j].stream][x.n_rel++];
                memset(&r, 0, sizeof r);
                r.push = due[j].push; r.idx = due[j].idx; r.n_seen = due[j].n_seen; r.has_M = due[j].last;
                memcpy(r.Minv, h_minv.data() + 12 * j, sizeof r.Minv);
                if (due[j].last) VS_HIP_TRY(hipMemcpy(r.M, x.M, sizeof r.M, hipMemcpyDeviceToHost));
            }
            for (int s : act) VS_TRY(fetch_dbg(S[(size_t)s], dbg_out[s], st));
        }
    }
    // vs_stab_flush_dev: the frames still queued leave one by one through the per-frame kernel
    for (int s = 0; s < n_streams; s++) {
        Stream& x = S[(size_t)s];
        while (!x.queue.empty()) {
            VS_TRY(emit_one(x, tp, -1, n_push[s], rel_out[s], st));
            VS_TRY(fetch_dbg(x, dbg_out[s], st));
        }
        n_dbg[s] = x.n_dbg; n_rel[s] = x.n_rel;
    }
    return VS_OK;
}
