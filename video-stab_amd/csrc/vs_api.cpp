// C ABI of libvideo-stab (include/vs_stab.h): library-level entry points,
// device memory helpers and the stage operators.  The per-stream pipeline
// (vs_stab_*) lives in stabilizer.cpp, the batch schedule (vs_batch_*) in batch_schedule.cpp.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "launchers.h"
#include "vs_common.h"

namespace vsd {

static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
const char* get_last_error() { return g_last_error.c_str(); }

int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_last_error(std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0") +
                       " (libvideo-stab has no CPU fallback)");
        return VS_ERR_NO_DEVICE;
    }
    return VS_OK;
}

int run_copy_rate(size_t bytes, int iters, double* gbps);
int run_libm_checksum(int fn, uint64_t start, uint64_t count, uint64_t* result);
int run_estimate_affine_partial2d(const float* d_from, const float* d_to, int n, double thr,
                                  int max_iters, double* d_model, uint8_t* d_inliers,
                                  int32_t* d_info, hipStream_t st);
int run_pyr_lk_op(const uint8_t* d_prev, const uint8_t* d_next, size_t stride, int w, int h,
                  const float* d_prev_pts, int n, float* d_next_pts, uint8_t* d_status,
                  float* d_err, int win, int max_level, int max_iters, double eps, hipStream_t st);
int run_gftt_op(const uint8_t* d_gray, size_t stride, int w, int h, int max_corners, double quality,
                double min_distance, int block_size, float* d_pts, int32_t* d_count, float* d_eig,
                hipStream_t st);

// The frames base + k * frame_bytes + off, k < n, as the pointer list of the warp launchers.
template <typename P>
std::vector<P> frame_list(P base, size_t frame_bytes, int n, size_t off = 0) {
    std::vector<P> v((size_t)n);
    for (int k = 0; k < n; k++) v[k] = base + (size_t)k * frame_bytes + off;
    return v;
}

}  // namespace vsd

using namespace vsd;

extern "C" {

int vs_abi_version(void) { return VS_STAB_ABI_VERSION; }
#ifndef VS_BUILD_TAG
#define VS_BUILD_TAG "untagged"
#endif
const char* vs_build_tag(void) { return VS_BUILD_TAG; }

int vs_host_alloc(void** p, size_t bytes) {
    if (!p) return VS_ERR_INVALID_ARG;
    *p = nullptr;
    VS_TRY(vsd::ensure_device());
    VS_HIP_TRY(hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault));
    return VS_OK;
}
int vs_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return VS_ERR_INVALID_ARG;
    VS_TRY(ensure_device());
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); set_last_error(std::string("vs_host_register: ") + hipGetErrorString(e)); return VS_ERR_HIP; }
    return VS_OK;
}
int vs_host_unregister(void* p) {
    if (!p) return VS_OK;
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); set_last_error(std::string("vs_host_unregister: ") + hipGetErrorString(e)); return VS_ERR_HIP; }
    return VS_OK;
}
void vs_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

const char* vs_build_info(void) {
    return "libvideo-stab gfx950 (CDNA4, wave64) hipcc -ffp-contract=off; warp=classic-fixed-point";
}

int vs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Defaults of vs::Stabilizer::Parameters (Stabilizer.h:76-175) and of the
// constants hard-coded at Stabilizer.cpp:611-619, :647-649.
void vs_params_default(vs_params_c* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (int32_t)sizeof *p;
    p->smoothing_radius = 30;
    p->max_corners = 200;
    p->quality_level = 0.01;
    p->min_distance = 30.0;
    p->block_size = 3;
    p->border_type = VS_BORDER_BLACK;
    p->smoothing_method = VS_SMOOTH_BOX;
    p->gaussian_sigma = 2.0;
    p->min_smoothing_radius = 5;
    p->max_smoothing_radius = 50;
    p->fade_alpha = 0.1f;
    p->fade_duration = 30;
    p->canvas_scale_factor = 1.5f;
    p->temporal_buffer_size = 30;
    p->canvas_blend_weight = 0.7f;
    p->adaptive_canvas_size = 1;
    p->max_canvas_scale = 2.0f;
    p->min_canvas_scale = 1.2f;
    p->edge_blend_radius = 20;
    p->hf_shake_px = 1.5f;
    p->hf_analysis_max_width = 960;
    p->hf_rot_lp_alpha = 0.2f;
    p->enable_conditional_clahe = 1;
    p->hf_dead_zone_threshold = 2.0f;
    p->hf_freeze_duration = 10;
    p->hf_motion_accumulator_decay = 0.9f;
    p->lk_win_size = 15;
    p->lk_max_level = 2;
    p->lk_max_iters = 20;
    p->lk_epsilon = 0.03;
    p->ransac_max_iters = 500;
    p->ransac_threshold = 5.0;
}

const char* vs_status_string(int status) {
    switch (status) {
        case VS_OK: return "ok";
        case VS_ERR_INVALID_ARG: return "invalid argument";
        case VS_ERR_NO_DEVICE: return "no usable HIP device";
        case VS_ERR_HIP: return "HIP runtime error";
        case VS_ERR_UNSUPPORTED: return "unsupported parameter combination";
        case VS_ERR_SIZE_CHANGED: return "frame size changed";
        case VS_ERR_CAPACITY: return "device capacity exceeded";
        default: return "unknown status";
    }
}

const char* vs_last_error(void) { return get_last_error(); }

// ---- device memory helpers ---------------------------------------------------
int vs_dev_set_device(int device) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipSetDevice(device));
    return VS_OK;
}
int vs_dev_malloc(void** d_ptr, size_t bytes) {
    if (!d_ptr) return VS_ERR_INVALID_ARG;
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipMalloc(d_ptr, bytes));
    return VS_OK;
}
int vs_dev_free(void* d_ptr) {
    if (!d_ptr) return VS_OK;
    VS_HIP_TRY(hipFree(d_ptr));
    return VS_OK;
}
int vs_dev_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return VS_OK;
}
int vs_dev_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return VS_OK;
}
int vs_dev_memset(void* d_dst, int value, size_t bytes) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipMemset(d_dst, value, bytes));
    return VS_OK;
}
int vs_dev_sync(void) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipDeviceSynchronize());
    return VS_OK;
}
int vs_dev_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes) {
    VS_TRY(ensure_device());
    VS_HIP_TRY(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
    return VS_OK;
}
int vs_op_libm_checksum(int fn, uint64_t start, uint64_t count, uint64_t* result) {
    if (fn < 0 || fn > 3 || !result || count == 0) return VS_ERR_INVALID_ARG;
    VS_TRY(ensure_device());
    return vsd::run_libm_checksum(fn, start, count, result);
}
int vs_dev_copy_rate(size_t bytes, int iters, double* gbytes_per_s) {
    if (!gbytes_per_s || bytes < 4096 || iters < 1 || iters > 1000) return VS_ERR_INVALID_ARG;
    VS_TRY(ensure_device());
    return vsd::run_copy_rate(bytes, iters, gbytes_per_s);
}

// ---- stage operators -----------------------------------------------------------
int vs_op_warp_affine(const void* d_src, size_t src_stride, size_t src_frame_bytes, void* d_dst,
                      size_t dst_stride, size_t dst_frame_bytes, int w, int h, int cn,
                      const float* M, int batch, void* stream) {
    VS_TRY(ensure_device());
    if (!d_src || !d_dst || !M || batch <= 0) { set_last_error("warp_affine: invalid argument"); return VS_ERR_INVALID_ARG; }
    std::vector<double> Minv(6 * (size_t)batch);
    for (int b = 0; b < batch; b++) warp_invert(M + 6 * (size_t)b, &Minv[6 * (size_t)b]);   // cv::warpAffine inverts on the host too
    const auto srcs = frame_list((const uint8_t*)d_src, src_frame_bytes, batch);
    const auto dsts = frame_list((uint8_t*)d_dst, dst_frame_bytes, batch);
    return launch_warp_plane(srcs.data(), dsts.data(), batch, src_stride, w, h, dst_stride, w, h, cn, WarpMaps{Minv.data(), 6, true},
                             VS_BORDER_BLACK, WarpTabs{WarpTabs::SCRATCH}, (hipStream_t)stream);
}

// NV12 (sample_bytes 1) and P010 (2) surfaces: one body, strides and frame distances in bytes
// src_uv / dst_uv: bytes from a surface's luma pointer to its UV plane (0: behind the h luma rows); border VS_BORDER_FILL with `fill`:
// vs_op_warp_affine_yuv_fill
static int warp_affine_two_planes(const void* d_src, size_t src_stride, void* d_dst, size_t dst_stride, int w, int h, const float* M, int batch,
                                  size_t src_frame_bytes, size_t dst_frame_bytes, void* stream, int sample_bytes, size_t src_uv = 0, size_t dst_uv = 0,
                                  int border = VS_BORDER_BLACK, WarpFill fill = WarpFill()) {
    VS_TRY(ensure_device());
    if (!d_src || !d_dst || !M || batch <= 0) {
        set_last_error(sample_bytes == 2 ? "warp_affine_p010: invalid argument" : "warp_affine_nv12: invalid argument");
        return VS_ERR_INVALID_ARG;
    }
    if (sample_bytes == 2 && ((src_frame_bytes | dst_frame_bytes) & 1)) {
        set_last_error("warp_affine_p010: frame distances must be even (16-bit samples)");
        return VS_ERR_INVALID_ARG;
    }
    // luma: the full matrix; chroma: the half-size two-channel plane, same rotation, translation halved
    std::vector<double> Minv(12 * (size_t)batch);
    for (int b = 0; b < batch; b++) {
        const float* m = M + 6 * (size_t)b;
        const float c[6] = {m[0], m[1], m[2] * 0.5f, m[3], m[4], m[5] * 0.5f};
        warp_invert(m, &Minv[12 * (size_t)b]);
        warp_invert(c, &Minv[12 * (size_t)b + 6]);
    }
    const size_t suv = src_uv ? src_uv : (size_t)h * src_stride, duv = dst_uv ? dst_uv : (size_t)h * dst_stride;
    const auto ys = frame_list((const uint8_t*)d_src, src_frame_bytes, batch), us = frame_list((const uint8_t*)d_src, src_frame_bytes, batch, suv);
    const auto yd = frame_list((uint8_t*)d_dst, dst_frame_bytes, batch), ud = frame_list((uint8_t*)d_dst, dst_frame_bytes, batch, duv);
    return launch_warp_nv12(ys.data(), yd.data(), us.data(), ud.data(), batch, src_stride, dst_stride, w, h, WarpMaps{Minv.data(), 12, true},
                            border, WarpTabs{WarpTabs::SCRATCH}, (hipStream_t)stream, sample_bytes, fill);
}

int vs_op_warp_affine_nv12(const void* d_src, size_t src_stride, void* d_dst, size_t dst_stride,
                           int w, int h, const float* M, int batch, size_t src_frame_bytes,
                           size_t dst_frame_bytes, void* stream) {
    return warp_affine_two_planes(d_src, src_stride, d_dst, dst_stride, w, h, M, batch, src_frame_bytes, dst_frame_bytes, stream, 1);
}

int vs_op_warp_affine_p010(const void* d_src, size_t src_stride, void* d_dst, size_t dst_stride,
                           int w, int h, const float* M, int batch, size_t src_frame_bytes,
                           size_t dst_frame_bytes, void* stream) {
    return warp_affine_two_planes(d_src, src_stride, d_dst, dst_stride, w, h, M, batch, src_frame_bytes, dst_frame_bytes, stream, 2);
}

// I420 / YV12 (sample_bytes 1) and I010 / I012 (2): luma under the full matrix; U and V - one-channel planes of half the size -
// under the matrix with the halved translation.  0 = the packed default of a layout field; everything in bytes.
// sx, sy: the chroma shifts of planar 4:2:2 (1, 0) and 4:4:4 (0, 0) surfaces - chroma planes of (w >> sx) x (h >> sy) samples under
// Mc = S^-1 M S, S = diag(2^sx, 2^sy): every product exact in float, then inverted in double like any matrix.
static int warp_affine_three_planes(const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch, void* d_dst,
                                    size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch, int w, int h, const float* M, int batch,
                                    size_t src_frame_bytes, size_t dst_frame_bytes, int border, void* stream, int sample_bytes, int sx = 1, int sy = 1,
                                    WarpFill fill = WarpFill()) {
    VS_TRY(ensure_device());
    // (the default chroma pitch is the stride >> sx, and holds whole samples)
    const size_t half = sx ? 2 * (size_t)sample_bytes - 1 : 0;
    if (!d_src || !d_dst || !M || batch <= 0 || w < 1 || h < 1 || (w >> sx) < 1 || (h >> sy) < 1 || (w & ((1 << sx) - 1)) || (h & ((1 << sy) - 1)) ||
        (!src_c_pitch && (src_stride & half)) || (!dst_c_pitch && (dst_stride & half))) {
        if (sy == 0) set_last_error(sx ? "warp_affine_planar: 4:2:2: invalid argument (w must be even and, for the default chroma pitch, the strides hold two chroma rows)"
                                       : "warp_affine_planar: 4:4:4: invalid argument");
        else set_last_error(sample_bytes == 2 ? "warp_affine_i010: invalid argument (w and h must be even and, for the default chroma pitch, the strides multiples of 4)"
                                              : "warp_affine_i420: invalid argument (w, h and, for the default chroma pitch, the strides must be even)");
        return VS_ERR_INVALID_ARG;
    }
    if (sample_bytes == 2 && ((src_frame_bytes | dst_frame_bytes) & 1)) {
        set_last_error(sy == 0 ? "warp_affine_planar: frame distances must be even (16-bit samples)" : "warp_affine_i010: frame distances must be even (16-bit samples)");
        return VS_ERR_INVALID_ARG;
    }
    std::vector<double> Minv(12 * (size_t)batch);
    for (int b = 0; b < batch; b++) {
        const float* m = M + 6 * (size_t)b;
        float c[6] = {m[0], m[1], m[2] * 0.5f, m[3], m[4], m[5] * 0.5f};
        if (sx == 1 && sy == 0) { c[1] = m[1] * 0.5f; c[3] = m[3] * 2.0f; c[5] = m[5]; }
        else if (sx == 0) { c[2] = m[2]; c[5] = m[5]; }
        warp_invert(m, &Minv[12 * (size_t)b]);
        warp_invert(c, &Minv[12 * (size_t)b + 6]);
    }
    const I420Layout sl = i420_layout(src_stride, h, src_u_off, src_v_off, src_c_pitch, sx, sy), dl = i420_layout(dst_stride, h, dst_u_off, dst_v_off, dst_c_pitch, sx, sy);
    const auto ys = frame_list((const uint8_t*)d_src, src_frame_bytes, batch);
    const auto yd = frame_list((uint8_t*)d_dst, dst_frame_bytes, batch);
    return launch_warp_i420(ys.data(), yd.data(), batch, sl, dl, w, h, WarpMaps{Minv.data(), 12, true}, border, WarpTabs{WarpTabs::SCRATCH},
                            (hipStream_t)stream, sample_bytes, sx, sy, fill);
}

int vs_op_warp_affine_i420(const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch, void* d_dst, size_t dst_stride,
                           size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch, int w, int h, const float* M, int batch, size_t src_frame_bytes,
                           size_t dst_frame_bytes, int border, void* stream) {
    return warp_affine_three_planes(d_src, src_stride, src_u_off, src_v_off, src_c_pitch, d_dst, dst_stride, dst_u_off, dst_v_off, dst_c_pitch, w, h, M,
                                    batch, src_frame_bytes, dst_frame_bytes, border, stream, 1);
}

int vs_op_warp_affine_i010(const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch, void* d_dst, size_t dst_stride,
                           size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch, int w, int h, const float* M, int batch, size_t src_frame_bytes,
                           size_t dst_frame_bytes, int border, void* stream) {
    return warp_affine_three_planes(d_src, src_stride, src_u_off, src_v_off, src_c_pitch, d_dst, dst_stride, dst_u_off, dst_v_off, dst_c_pitch, w, h, M,
                                    batch, src_frame_bytes, dst_frame_bytes, border, stream, 2);
}

// Any planar format (VS_FMT_I420 ... VS_FMT_I412): the arguments of vs_op_warp_affine_i010 with the format in front.
int vs_op_warp_affine_planar(int fmt, const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch, void* d_dst,
                             size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch, int w, int h, const float* M, int batch,
                             size_t src_frame_bytes, size_t dst_frame_bytes, int border, void* stream) {
    const PixFmt* pf = pixfmt(fmt);
    if (!pf || !pf->three_planes()) {
        VS_TRY(ensure_device());
        set_last_error("warp_affine_planar: fmt must be a planar format (VS_FMT_I420 ... VS_FMT_I412)");
        return VS_ERR_INVALID_ARG;
    }
    return warp_affine_three_planes(d_src, src_stride, src_u_off, src_v_off, src_c_pitch, d_dst, dst_stride, dst_u_off, dst_v_off, dst_c_pitch, w, h, M,
                                    batch, src_frame_bytes, dst_frame_bytes, border, stream, pf->sample_bytes, pf->sx, pf->sy);
}

// The warp of edge fill on YUV streams as an operator: any YUV surface format, BORDER_CONSTANT with the fill colour.  What concerns
// the format, the fill and null arguments is refused first, without a device; the launchers check the rest before they launch.
int vs_op_warp_affine_yuv_fill(int fmt, const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch, void* d_dst,
                               size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch, int w, int h, const float* M, int batch,
                               size_t src_frame_bytes, size_t dst_frame_bytes, const vs_yuv_fill* fill, void* stream) {
    const PixFmt* pf = pixfmt(fmt);
    if (!pf || pf->kind == PIX_INTERLEAVED) {
        set_last_error("vs_op_warp_affine_yuv_fill: fmt must be a YUV surface format (NV12, P010, I420 ... I412)");
        return VS_ERR_INVALID_ARG;
    }
    if (fill && fill->reserved != 0) { set_last_error("vs_op_warp_affine_yuv_fill: fill->reserved must be 0"); return VS_ERR_INVALID_ARG; }
    const vs_yuv_fill c = fill ? *fill : yuv_video_black(*pf);
    const Refusal r = check_yuv_fill(*pf, c, "vs_op_warp_affine_yuv_fill");
    if (r.rc != VS_OK) { set_last_error(r.text); return r.rc; }
    if (!d_src || !d_dst || !M || batch <= 0 || w < 1 || h < 1) { set_last_error("vs_op_warp_affine_yuv_fill: invalid argument"); return VS_ERR_INVALID_ARG; }
    WarpFill f;
    f.y = c.y; f.u = c.u; f.v = c.v;
    if (pf->luma_uv())
        return warp_affine_two_planes(d_src, src_stride, d_dst, dst_stride, w, h, M, batch, src_frame_bytes, dst_frame_bytes, stream, pf->sample_bytes,
                                      src_u_off, dst_u_off, VS_BORDER_FILL, f);
    return warp_affine_three_planes(d_src, src_stride, src_u_off, src_v_off, src_c_pitch, d_dst, dst_stride, dst_u_off, dst_v_off, dst_c_pitch, w, h, M,
                                    batch, src_frame_bytes, dst_frame_bytes, VS_BORDER_FILL, stream, pf->sample_bytes, pf->sx, pf->sy, f);
}

int vs_op_resize_gray(const void* d_src, size_t src_stride, int sw, int sh, int fmt, void* d_dst,
                      size_t dst_stride, int dw, int dh, void* stream) {
    VS_TRY(ensure_device());
    return launch_resize_gray((const uint8_t*)d_src, src_stride, sw, sh, fmt, (uint8_t*)d_dst,
                              dst_stride, dw, dh, (hipStream_t)stream);
}

int vs_op_pyr_down(const void* d_src, size_t src_stride, int sw, int sh, void* d_dst,
                   size_t dst_stride, void* stream) {
    VS_TRY(ensure_device());
    return launch_pyr_down((const uint8_t*)d_src, src_stride, sw, sh, (uint8_t*)d_dst, dst_stride,
                           (hipStream_t)stream);
}

int vs_op_scharr(const void* d_src, size_t src_stride, int w, int h, void* d_dst, void* stream) {
    VS_TRY(ensure_device());
    return launch_scharr((const uint8_t*)d_src, src_stride, w, h, (int16_t*)d_dst, (hipStream_t)stream);
}

int vs_op_pyr_level(const void* d_src, size_t src_stride, size_t src_frame_bytes, int w, int h, void* d_der, void* d_next,
                    size_t next_stride, size_t next_frame_bytes, int items, void* stream) {
    VS_TRY(ensure_device());
    if (!d_src || !d_der || items < 1 || items > 4096 || w <= 0 || h <= 0) { set_last_error("pyr_level: invalid argument"); return VS_ERR_INVALID_ARG; }
    // the kernel takes device tables of (source, destination) pairs: built here for the call (an operator for tests and probes)
    std::vector<ImgPair> t(2 * (size_t)items);
    for (int i = 0; i < items; i++) {
        const uint8_t* s = (const uint8_t*)d_src + (size_t)i * src_frame_bytes;
        t[i] = ImgPair{s, (uint8_t*)d_der + (size_t)i * w * h * 4};
        t[items + i] = ImgPair{s, d_next ? (uint8_t*)d_next + (size_t)i * next_frame_bytes : nullptr};
    }
    ImgPair* d_t = nullptr;
    VS_HIP_TRY(hipMalloc((void**)&d_t, sizeof(ImgPair) * t.size()));
    hipStream_t st = (hipStream_t)stream;
    int rc = VS_OK;
    if (hipMemcpyAsync(d_t, t.data(), sizeof(ImgPair) * t.size(), hipMemcpyHostToDevice, st) != hipSuccess) rc = VS_ERR_HIP;
    if (rc == VS_OK) rc = launch_pyr_level_batch(d_t, d_next ? d_t + items : nullptr, items, src_stride, w, h, next_stride, st);
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_t);
    return rc;
}

int vs_op_pyr_lk(const void* d_prev, const void* d_next, size_t stride, int w, int h,
                 const float* d_prev_pts, int n, float* d_next_pts, uint8_t* d_status, float* d_err,
                 int win, int max_level, int max_iters, double eps, void* stream) {
    VS_TRY(ensure_device());
    return run_pyr_lk_op((const uint8_t*)d_prev, (const uint8_t*)d_next, stride, w, h, d_prev_pts, n,
                         d_next_pts, d_status, d_err, win, max_level, max_iters, eps,
                         (hipStream_t)stream);
}

int vs_op_gftt(const void* d_gray, size_t stride, int w, int h, int max_corners, double quality,
               double min_distance, int block_size, float* d_pts, int32_t* d_count, float* d_eig,
               void* stream) {
    VS_TRY(ensure_device());
    return run_gftt_op((const uint8_t*)d_gray, stride, w, h, max_corners, quality, min_distance,
                       block_size, d_pts, d_count, d_eig, (hipStream_t)stream);
}

int vs_op_estimate_affine_partial2d(const float* d_from, const float* d_to, int n, double thr,
                                    int max_iters, double* d_model, uint8_t* d_inliers,
                                    int32_t* d_info, void* stream) {
    VS_TRY(ensure_device());
    return run_estimate_affine_partial2d(d_from, d_to, n, thr, max_iters, d_model, d_inliers, d_info,
                                         (hipStream_t)stream);
}

}  // extern "C"
