/*
 * vs_stab.h - C ABI of libvideo-stab (MI355X / gfx950 build).
 *
 * This is the drop-in boundary for the per-frame stabilization hot path of
 * OmerMersin/video-stab: everything `vs::Stabilizer::stabilize(frame)` does
 * (reference: include/video/Stabilizer.h:177-198, src/Stabilizer.cpp:258-1172).
 * The reference has no FFI of its own (it is a C++ class over cv::Mat); the
 * binding a maintainer adds is the thin C++ class in include/video/Stabilizer.h
 * of this repo, which forwards to the entry points below.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch/OpenCV types cross this ABI;
 *  - every function returns a vs_status; nothing throws across the ABI;
 *  - images are 8-bit, row-major, with an explicit row stride in BYTES (the one exception: VS_FMT_P010
 *    surfaces hold 16-bit samples; their strides and plane offsets are in BYTES all the same);
 *  - `*_dev` entry points take DEVICE pointers and are asynchronous on the
 *    instance's HIP stream; the host-pointer forms copy in/out and synchronise;
 *  - there is no CPU fallback: if no gfx950 device is usable every compute
 *    entry point fails with VS_ERR_NO_DEVICE.
 */
#ifndef VS_STAB_H
#define VS_STAB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: VS_STAGE_COUNT grew to 9 (VS_STAGE_WARP_TABLES: the arrays of vs_stab_get_stage_times), vs_stab_enable_graph is gone
 *    (round 2), vs_batch_* and vs_dev_copy_rate / vs_dev_memcpy_d2d added.  (The pipelined host call is chosen with
 *    vs_stab_set_host_pipeline - Parameters::hostPipeline of the C++ class - not through vs_params_c, whose layout is unchanged.)
 *    Added since without a layout change: vs_batch_create_params (round 4); the pixel formats VS_FMT_BGRA8,
 *    VS_FMT_RGBA8 and VS_FMT_RGB8; VS_FMT_P010 (enum vs_pixfmt16) with vs_op_warp_affine_p010; VS_FMT_I420 (enum
 *    vs_pixfmt_planar) with vs_stab_set_i420_layout, vs_batch_set_i420_layout and vs_op_warp_affine_i420; VS_FMT_I010 and
 *    VS_FMT_I012 (enum vs_pixfmt_planar16) with vs_op_warp_affine_i010; roll correction and auto zoom/crop on P010 surfaces:
 *    vs_roll_correct_p010_dev, vs_roll_correct_p010_dev_n, vs_azc_apply_p010_dev, vs_azc_apply_p010_dev_n and
 *    vs_op_warp_affine16_ex; the same two stages on I420 / I010 / I012 surfaces: struct vs_i420_layout with
 *    vs_roll_correct_i420_dev, vs_roll_correct_i420_dev_n, vs_azc_apply_i420_dev and vs_azc_apply_i420_dev_n; planar 4:2:2 and
 *    4:4:4 - VS_FMT_I422, VS_FMT_I444, VS_FMT_I210, VS_FMT_I212, VS_FMT_I410, VS_FMT_I412 (enum vs_pixfmt_planar4xx) - with
 *    vs_op_warp_affine_planar, and as fmt of the four roll / zoom entry points above; the output size of auto zoom/crop: vs_azc_set_output_size, vs_azc_get_output_size, struct
 *    vs_scale_job with vs_op_scale_jobs and vs_op_scale_jobs_plan; roll correction and auto zoom/crop on interleaved colour frames (BGR8, RGB8, BGRA8,
 *    RGBA8), asynchronous: vs_roll_correct_rgb_dev, vs_roll_correct_rgb_dev_n, vs_azc_apply_rgb_dev, vs_azc_apply_rgb_dev_n,
 *    vs_op_scale_jobs_rgb and vs_op_scale_jobs_rgb_plan; the compositing operators vs_op_copy_make_border, vs_op_fade_blend,
 *    vs_op_fade_update and vs_op_canvas_create / apply / info / destroy; colour conversion on the device: vs_op_cvt_yuv_to_rgb,
 *    vs_op_cvt_rgb_to_yuv and vs_enh_apply_yuv_dev; the enhancer on a batch of YUV surfaces in one fused launch:
 *    vs_enh_apply_yuv_batch_dev, vs_enh_last_fused and vs_enh_yuv_plan; the colour space of the conversions: struct
 *    vs_cvt_colorimetry with vs_op_cvt_yuv_to_rgb_cs, vs_op_cvt_rgb_to_yuv_cs, vs_enh_set_yuv_colorimetry, vs_cvt_coefficients and
 *    vs_cvt_colorimetry_guess; conversion between the YUV surface formats: struct vs_yuv_cvt_desc with vs_op_cvt_yuv_to_yuv and
 *    vs_yuv_surface_layout; crop-and-zoom on YUV streams: vs_stab_set_yuv_crop_zoom, vs_batch_set_yuv_crop_zoom and vs_op_resize_jobs;
 *    border pad on YUV streams: struct vs_yuv_fill with vs_stab_set_yuv_border_pad, vs_batch_set_yuv_border_pad and
 *    vs_yuv_video_black, struct vs_pad_job with vs_op_pad_jobs; the fade border on YUV streams: vs_stab_set_yuv_fade, struct
 *    vs_fade_job with vs_op_fade_blend_jobs, struct vs_fade_update_job with vs_op_fade_update_jobs; edge fill on YUV streams:
 *    vs_stab_set_yuv_edge_fill, vs_batch_set_yuv_edge_fill and vs_op_warp_affine_yuv_fill; the packed 4:2:2 capture formats: enum
 *    vs_packed_fmt with vs_op_cvt_packed_to_yuv, vs_op_cvt_yuv_to_packed and vs_packed_layout; the resize to an output size: enum
 *    vs_interp with vs_op_resample_jobs, vs_op_resample_jobs_plan, vs_op_resize_yuv, vs_op_resize_rgb and vs_resize_axis_table; the area-averaging downscale:
 *    vs_op_area_jobs, vs_op_area_jobs_plan, vs_op_area_yuv, vs_op_area_rgb and vs_area_axis_table; interlaced sources: enum
 *    vs_deint_mode and struct vs_deint_job with vs_op_deint_jobs, vs_op_deint_yuv and vs_op_interlace_yuv (the definition of the
 *    deinterlacer stands in front of them)
 *    (new entry points, new values and new structs only: no existing struct or entry point changed, so
 *    the version stays). */
#define VS_STAB_ABI_VERSION 2

typedef enum vs_status {
    VS_OK = 0,
    VS_ERR_INVALID_ARG = 1,
    VS_ERR_NO_DEVICE = 2,     /* no HIP device / kernels cannot run          */
    VS_ERR_HIP = 3,           /* a HIP runtime call failed (see last_error)   */
    VS_ERR_UNSUPPORTED = 4,   /* parameter combination outside the hot path   */
    VS_ERR_SIZE_CHANGED = 5,  /* frame size differs from the instance's       */
    VS_ERR_CAPACITY = 6       /* a device-side capacity was exceeded          */
} vs_status;

typedef enum vs_pixfmt {
    VS_FMT_BGR8 = 0,          /* interleaved B,G,R  (cv::Mat CV_8UC3)         */
    VS_FMT_NV12 = 1,          /* Y plane (h rows) followed by UV plane (h/2)  */
    VS_FMT_GRAY8 = 2,
    VS_FMT_BGRA8 = 3,         /* interleaved B,G,R,A (cv::Mat CV_8UC4; BGRx) */
    VS_FMT_RGBA8 = 4,         /* interleaved R,G,B,A                          */
    VS_FMT_RGB8 = 5           /* interleaved R,G,B                            */
} vs_pixfmt;

/* Formats with 16-bit samples, numbered on from vs_pixfmt in the same `int fmt`.
 * P010 (rocDecode / VA-API output of HEVC Main10, AV1 10-bit, VP9 profile 2): the NV12 layout with one little-endian 16-bit
 * word per sample, the ten significant bits at the top.  A surface of w x h (both even) is a luma plane of h rows of w uint16
 * samples followed by an interleaved chroma plane of h/2 rows of w/2 (U, V) uint16 pairs.  Pitch and plane offset are in
 * BYTES, exactly as for NV12 (`stride`, vs_stab_set_nv12_layout; offset 0 = h * pitch); pointers, pitches and the plane offset
 * must be even (VS_ERR_INVALID_ARG otherwise).  Nothing assumes that the low six bits are zero: P012 / P016 content passes
 * through the same code and the same definitions:
 *  - analysis: the gray image is that of the 8-bit plane made of the luma samples' high bytes (sample >> 8: truncation, what
 *    a decoder's own 8-bit export holds), resized as the luma plane of an NV12 frame is - so keypoints, tracks, model,
 *    trajectory and warp matrix are bit-identical to those of the NV12 (or GRAY8) stream of the high bytes;
 *  - warp: cv::warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) on the CV_16UC1 luma plane and, with the translation halved, on the
 *    CV_16UC2 chroma plane: source coordinates as for 8 bits (AB_BITS = 10, 1/32 px), blend = the exact integer
 *    S = sum v_i n_i over the four taps (n = (32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy fx; sum 1024; taps outside the picture
 *    are 0, each by itself), rounded once, half to even: (S + 511 + ((S >> 10) & 1)) >> 10.  For ten-bit content that is
 *    what OpenCV's float blend gives; for arbitrary 16-bit content it is the definition (docs/opencv_semantics.md);
 *  - everything else follows NV12: the last frame of a flush comes back unwarped; border pad, crop-and-zoom, fade and the
 *    virtual canvas are refused as for NV12 (crop-and-zoom, border pad and fade unless the stream opts in: vs_stab_set_yuv_crop_zoom, vs_stab_set_yuv_border_pad, vs_stab_set_yuv_fade).
 * The two stages around the stabilizer take P010 surfaces too (vs_roll_correct_p010_dev, vs_azc_apply_p010_dev):
 *  - analysis plane: both analyse the 8-bit plane of the luma samples' high bytes (sample >> 8), the plane the stabilizer analyses.
 *    Smoothed and detected angle, line counts, content mask, contours, info8 and the crop rectangle are bit-identical to those of
 *    the NV12 call on the high-byte surface; the mask rule gray > 1 reads (sample >> 8) > 1;
 *  - roll rotation: the matrix the NV12 path builds (centre, angle; the chroma plane with the translation halved), applied to the
 *    CV_16UC1 luma plane and the CV_16UC2 chroma plane: INTER_LINEAR, BORDER_REPLICATE (a tap outside the plane takes the nearest
 *    edge sample, each tap by itself), the coordinate path of 8 bits (AB_BITS = 10, 1/32 px), the blend above: S over the four
 *    taps, rounded once, half to even;
 *  - zoom crop-and-scale: the rectangle as found for luma, halved for the chroma plane (x/2, y/2, max(1, w/2), max(1, h/2)); each
 *    plane scaled to its share of 640 x 360 by the reference's scale matrix; BORDER_CONSTANT 0, the same blend.  On the fall-back
 *    paths the surface comes back unchanged, all 16 bits;
 *  - low bits: nothing here assumes that the low six bits are zero either.
 * Not built: the C++ classes vs::RollCorrection / vs::AutoZoomCrop keep taking 8-bit cv::Mats.  (I420 / I010 / I012 surfaces go
 * through these two stages with entry points of their own: vs_pixfmt_planar, vs_pixfmt_planar16.) */
typedef enum vs_pixfmt16 {
    VS_FMT_P010 = 6           /* Y plane (h rows of w uint16) followed by UV plane (h/2 rows of w/2 uint16 pairs) */
} vs_pixfmt16;

/* Planar 4:2:0 - `yuv420p`, I420, YV12: what software decoders emit (FFmpeg / PyAV, libvpx, dav1d, GStreamer's
 * video/x-raw,format=I420) and software encoders take -, numbered on in the same `int fmt`.  A frame of w x h (both even,
 * VS_ERR_INVALID_ARG otherwise) has three planes: Y, h rows of w bytes at pitch `stride`; U and V, h/2 rows of w/2 bytes each.
 * Packed default layout: chroma pitch = stride / 2 (`stride` and `out_stride` must be even, VS_ERR_INVALID_ARG otherwise), U
 * starts h * stride bytes behind the Y pointer, V (h/2) * (chroma pitch) bytes behind U.  The host entry points take and fill
 * this layout; device surfaces may differ from it: vs_stab_set_i420_layout.
 *  - YV12 is I420 with the two plane offsets swapped (V first): give u_off = h * stride + (h/2) * c_pitch and v_off = h * stride.
 *  - An FFmpeg AVFrame whose linesize[1] is not linesize[0] / 2 is described by c_pitch = linesize[1] (= linesize[2]), the
 *    offsets being data[1] - data[0] and data[2] - data[0] when the three planes come from one allocation.
 * Neither needs a format value of its own.  Definitions - every observable of an I420 stream is that of the NV12 stream that
 * holds the same samples:
 *  - analysis: the gray image is that of the Y plane, through the kernels an NV12 luma plane takes;
 *  - warp: Y as an NV12 luma plane; U and V each as a CV_8UC1 plane of w/2 x h/2 under the matrix with the translation halved
 *    in float (cv::warpAffine treats channels independently: these are the two channels of the NV12 chroma plane's warp),
 *    INTER_LINEAR, BORDER_CONSTANT 0;
 *  - the last frame of a flush comes back unwarped, all three planes; border pad, crop-and-zoom, fade and the virtual canvas
 *    are refused as for NV12 (VS_ERR_UNSUPPORTED; crop-and-zoom, border pad and fade unless the stream opts in: vs_stab_set_yuv_crop_zoom, vs_stab_set_yuv_border_pad, vs_stab_set_yuv_fade); the
 *    enhancer and the C++ classes do not take it.
 * The two stages around the stabilizer take I420 surfaces (vs_roll_correct_i420_dev, vs_azc_apply_i420_dev; layouts as
 * struct vs_i420_layout): every observable is again that of the NV12 call on the same samples, the planes de-interleaved -
 *  - analysis plane: Y itself (line search of the roll stage, content mask of the zoom stage);
 *  - roll rotation: about the picture centre, BORDER_REPLICATE; Y under M, U and V each as a CV_8UC1 plane of w/2 x h/2 under M with
 *    the translation halved (the chroma matrix of the NV12 path), vs_op_warp_affine_ex's arithmetic;
 *  - zoom crop-and-scale: the rectangle as found for Y, halved for U and for V (x/2, y/2, max(1, w/2), max(1, h/2)); Y scaled to
 *    640 x 360, U and V to 320 x 180 each by the reference's scale matrix, BORDER_CONSTANT 0; on the fall-back paths the surface
 *    comes back unchanged, all three planes. */
typedef enum vs_pixfmt_planar {
    VS_FMT_I420 = 7           /* Y plane (h rows of w), U plane, V plane (h/2 rows of w/2 each) */
} vs_pixfmt_planar;

/* Planar 4:2:0 with 16-bit samples - `yuv420p10le` / `yuv420p12le`, GStreamer's I420_10LE / I420_12LE: what software decoders of
 * 10- and 12-bit video emit (dav1d, libde265, FFmpeg's HEVC decoder, libvpx profile 2) -, numbered on in the same `int fmt`.
 * The planes of I420 with the samples of P010: one little-endian 16-bit word per sample, but the value in the LOW bits.
 * `stride`, the chroma pitch and the plane offsets are in BYTES; pointers, pitches and offsets must be even (VS_ERR_INVALID_ARG
 * otherwise).  Packed default layout: chroma pitch = stride / 2 (so `stride` and `out_stride` must be multiples of 4), U starts
 * h * stride bytes behind the Y pointer, V (h/2) * (chroma pitch) bytes behind U; other layouts - a linesize[1] of its own,
 * planes apart, V before U - through vs_stab_set_i420_layout / vs_batch_set_i420_layout.  A chroma pitch below w bytes is
 * VS_ERR_INVALID_ARG.  Definitions:
 *  - analysis: the gray image is that of the 8-bit plane min(sample >> (bits - 8), 255) of the Y plane (shift 2 for I010, 4 for
 *    I012), resized as the luma plane of an NV12 frame is.  The saturation says what out-of-range content does: nothing assumes
 *    that the high bits are zero.  Keypoints, tracks, model, trajectory and warp matrix are bit-identical to those of the NV12 /
 *    GRAY8 stream of those bytes, and for in-range content to those of the P010 stream that holds sample << (16 - bits);
 *  - warp: Y as a CV_16UC1 plane under M; U and V each as a CV_16UC1 plane of w/2 x h/2 under the matrix with the translation
 *    halved in float; INTER_LINEAR, BORDER_CONSTANT 0, the blend of P010 to the letter (S rounded once, half to even).  The warp
 *    does not depend on the bit depth;
 *  - the last frame of a flush comes back unwarped, all three planes; border pad, crop-and-zoom, fade and the virtual canvas
 *    are VS_ERR_UNSUPPORTED (crop-and-zoom, border pad and fade unless the stream opts in: vs_stab_set_yuv_crop_zoom, vs_stab_set_yuv_border_pad, vs_stab_set_yuv_fade); the enhancer and the C++
 *    classes do not take these formats.
 * The two stages around the stabilizer take I010 / I012 surfaces (vs_roll_correct_i420_dev, vs_azc_apply_i420_dev with fmt
 * VS_FMT_I010 / VS_FMT_I012):
 *  - analysis plane: min(sample >> (bits - 8), 255) of Y, exactly the byte the stabilizer's analysis uses.  Smoothed and detected
 *    angle, line counts, content mask (byte > 1), contours, info8 and the crop rectangle are those of the NV12 / GRAY8 call on
 *    that plane;
 *  - roll rotation: BORDER_REPLICATE, Y under M, U and V each as a CV_16UC1 plane of w/2 x h/2 under M with the translation
 *    halved; P010's blend, S rounded once, half to even (vs_op_warp_affine16_ex, cn 1).  The rotation does not depend on the bit
 *    depth, and it is NOT the P010 round trip's picture for out-of-range content (the one rounding does not commute with a shift);
 *  - zoom crop-and-scale: the rectangle for Y, halved for U and V; 640 x 360 / 320 x 180 / 320 x 180, BORDER_CONSTANT 0, the same
 *    blend; on the fall-back paths the surface comes back unchanged, all three planes, all 16 bits. */
typedef enum vs_pixfmt_planar16 {
    VS_FMT_I010 = 8,          /* yuv420p10le: Y (h rows of w uint16), U, V (h/2 rows of w/2 uint16 each); value in bits 0..9  */
    VS_FMT_I012 = 9           /* yuv420p12le: the same planes, value in bits 0..11 */
} vs_pixfmt_planar16;

/* Planar 4:2:2 and 4:4:4, 8-, 10- and 12-bit, numbered on in the same `int fmt`: what software decoders emit for camera and drone
 * masters, ProRes, DNxHR and XAVC (yuv422p10le) and for screen and graphics content (yuv444p).  Three planes, as I420 / I010:
 *      value  name          FFmpeg / GStreamer            planes
 *      10     VS_FMT_I422   yuv422p      / Y42B           Y w x h, U and V (w/2) x h, 8-bit
 *      11     VS_FMT_I444   yuv444p      / Y444           three planes w x h, 8-bit
 *      12     VS_FMT_I210   yuv422p10le  / I422_10LE      as I422, little-endian 16-bit words, value in bits 0..9
 *      13     VS_FMT_I212   yuv422p12le  / I422_12LE      value in bits 0..11
 *      14     VS_FMT_I410   yuv444p10le  / Y444_10LE      as I444, 16-bit words, value in bits 0..9
 *      15     VS_FMT_I412   yuv444p12le  / Y444_12LE      value in bits 0..11
 * With the chroma shifts (sx, sy) = (1, 0) for 4:2:2 and (0, 0) for 4:4:4 (4:2:0 is (1, 1)) a chroma plane has (w >> sx) x (h >> sy)
 * samples.  4:2:2 needs an even w (h may be odd); 4:4:4 takes any w, h.  Pitches and offsets are in BYTES; for the 16-bit formats
 * pointers, pitches and offsets must be even (VS_ERR_INVALID_ARG otherwise).
 * Packed default layout: chroma pitch = stride >> sx (stride / 2 for 4:2:2, stride for 4:4:4), U starts h * stride bytes behind
 * the Y pointer, V h * (chroma pitch) bytes behind U.  Because of the default chroma pitch `stride` and `out_stride` must be even
 * for I422 and multiples of 4 for I210 / I212.  The host entry points take and fill this layout.  Other layouts - an AVFrame's
 * linesize[1], planes apart, V before U (swap the offsets) - go through the unchanged vs_stab_set_i420_layout /
 * vs_batch_set_i420_layout: 0 = the default of that field, for that format.  A chroma pitch below one chroma row's bytes is
 * VS_ERR_INVALID_ARG, with a text that names the format.  Definitions:
 *  - analysis: the gray image is that of the Y plane (8-bit formats), or of the 8-bit plane min(sample >> (bits - 8), 255) of Y
 *    (16-bit formats: shift 2 for I210 / I410, 4 for I212 / I412), through the kernels I420 / I010 take.  Keypoints, tracks, model,
 *    trajectory and warp matrix are bit-identical to those of the NV12 / GRAY8 stream of those bytes;
 *  - warp: Y under M; U and V each as a one-channel plane under the chroma matrix Mc = S^-1 M S, M conjugated by the subsampling
 *    S = diag(2^sx, 2^sy) - the convention that gives 4:2:0 its "translation halved":
 *        4:4:4: Mc = M;      4:2:2: Mc = [[m0, m1 * 0.5f, m2 * 0.5f], [m3 * 2.0f, m4, m5]]    (every product exact in float).
 *    cv::warpAffine then inverts Mc in double like any other matrix; INTER_LINEAR, BORDER_CONSTANT 0.  8-bit planes:
 *    vs_op_warp_affine_ex's arithmetic (CV_8UC1); 16-bit planes: P010's blend to the letter - the exact integer S, rounded once,
 *    half to even (vs_pixfmt16) - which does not depend on the bit depth.  (For 4:2:2, Mc is not a rotation.)
 *  - the last frame of a flush comes back unwarped, all three planes;
 *  - border pad, crop-and-zoom, fade and the virtual canvas are VS_ERR_UNSUPPORTED, with a text that names the format, exactly
 *    where I420 is refused (crop-and-zoom, border pad and fade unless the stream opts in: vs_stab_set_yuv_crop_zoom, vs_stab_set_yuv_border_pad, vs_stab_set_yuv_fade).  The C++ classes do not take these formats.  Semi-planar 4:2:2 / 4:4:4 (NV16, P210, NV24),
 *    yuv4xxp16le and big-endian samples are not built.
 * The two stages around the stabilizer take these formats through the entry points of the 4:2:0 ones (vs_roll_correct_i420_dev,
 * vs_roll_correct_i420_dev_n, vs_azc_apply_i420_dev, vs_azc_apply_i420_dev_n; layouts as struct vs_i420_layout, whose default chroma
 * pitch is pitch >> sx).  In these two stages w and h are even for every format (odd-height 4:2:2 and odd 4:4:4 pictures are a stated
 * limitation).  The definitions are those of vs_pixfmt_planar / vs_pixfmt_planar16 with the shifts made explicit:
 *  - analysis, both stages: the 8-bit plane of Y - Y itself, or min(sample >> (bits - 8), 255).  Angle, line counts, content mask,
 *    contours and info8 are those of the NV12 call on that plane; they do not depend on the chroma subsampling;
 *  - roll rotation: Y under the double matrix M of cv::getRotationMatrix2D((w / 2.0f, h / 2.0f), angle, 1); U and V under
 *    Mc = S^-1 M S in double, S = diag(2^sx, 2^sy):
 *        [[m0, m1 * 2^(sy - sx), m2 / 2^sx], [m3 * 2^(sx - sy), m4, m5 / 2^sy]]      (exact products by powers of two;
 *    (1, 1) is "the translation halved" to the letter).  BORDER_REPLICATE; 8-bit planes vs_op_warp_affine_ex's arithmetic, 16-bit
 *    planes P010's blend (S rounded once, half to even);
 *  - zoom crop-and-scale: the rectangle (x, y, cw, ch) applies to Y as found and as (x >> sx, y >> sy, uw = max(1, cw >> sx),
 *    uh = max(1, ch >> sy)) to U and to V; Y is scaled to ow x oh, U and V each to (ow >> sx) x (oh >> sy) by
 *    [(float)((double)(ow >> sx) / uw), 0, 0; 0, (float)((double)(oh >> sy) / uh), 0]; INTER_LINEAR, BORDER_CONSTANT 0 at the crop's
 *    edge - vs_op_scale_jobs' arithmetic for that sample size.  On the fall-back paths (no contour, empty crop) the three planes
 *    come back unchanged at their own sizes, laid where `out` puts them.  vs_azc_set_output_size applies as to the other formats. */
typedef enum vs_pixfmt_planar4xx {
    VS_FMT_I422 = 10,         /* yuv422p:     Y (h rows of w), U, V (h rows of w/2 each) */
    VS_FMT_I444 = 11,         /* yuv444p:     Y, U, V (h rows of w each) */
    VS_FMT_I210 = 12,         /* yuv422p10le: the planes of I422, uint16, value in bits 0..9 */
    VS_FMT_I212 = 13,         /* yuv422p12le: value in bits 0..11 */
    VS_FMT_I410 = 14,         /* yuv444p10le: the planes of I444, uint16, value in bits 0..9 */
    VS_FMT_I412 = 15          /* yuv444p12le: value in bits 0..11 */
} vs_pixfmt_planar4xx;

/* Stabilizer.cpp:31-38 mapBorderMode() */
typedef enum vs_border {
    VS_BORDER_BLACK = 0,
    VS_BORDER_REFLECT = 1,
    VS_BORDER_REFLECT_101 = 2,
    VS_BORDER_REPLICATE = 3,
    VS_BORDER_WRAP = 4,
    VS_BORDER_FADE = 5
} vs_border;

/* Stabilizer.cpp:797-823 */
typedef enum vs_smoothing {
    VS_SMOOTH_BOX = 0,
    VS_SMOOTH_GAUSSIAN = 1,
    VS_SMOOTH_KALMAN = 2
} vs_smoothing;

/*
 * Flat POD mirror of vs::Stabilizer::Parameters (Stabilizer.h:76-175).
 * Only the fields the live hot path reads are present;
 * strings became enums.  Fill with vs_params_default() first.
 */
typedef struct vs_params_c {
    int32_t struct_size;          /* = sizeof(vs_params_c), ABI check          */
    int32_t logging;              /* Stabilizer.h:79                           */
    int32_t smoothing_radius;     /* :81  default 30                           */
    int32_t max_corners;          /* :82  default 200                          */
    double  quality_level;        /* :83  default 0.01                         */
    double  min_distance;         /* :84  default 30.0                         */
    int32_t block_size;           /* :85  default 3                            */
    int32_t border_type;          /* :87  vs_border, default BLACK             */
    int32_t border_size;          /* :88  default 0                            */
    int32_t crop_n_zoom;          /* :89  default 0                            */
    int32_t smoothing_method;     /* :92  vs_smoothing, default BOX            */
    int32_t horizon_lock;         /* :95  default 0                            */
    double  gaussian_sigma;       /* :93  default 2.0                          */
    int32_t adaptive_smoothing;   /* :114 default 0                            */
    int32_t min_smoothing_radius; /* :115 default 5                            */
    int32_t max_smoothing_radius; /* :116 default 50                           */
    float   fade_alpha;           /* :128 default 0.1                          */
    int32_t fade_duration;        /* :129 default 30                           */
    int32_t enable_virtual_canvas;/* :154 default 0 (BGR8 streams only)        */
    int32_t drone_high_freq_mode; /* :165 default 0                            */
    float   hf_shake_px;          /* :166 default 1.5                          */
    int32_t hf_analysis_max_width;/* :167 default 960                          */
    float   hf_rot_lp_alpha;      /* :168 default 0.2                          */
    int32_t enable_conditional_clahe; /* :169 default 1                        */
    float   hf_dead_zone_threshold;   /* :172 default 2.0                      */
    int32_t hf_freeze_duration;       /* :173 default 10                       */
    float   hf_motion_accumulator_decay; /* :174 default 0.9                   */
    /* --- extensions: constants hard-coded in Stabilizer.cpp:611-619 --------- */
    int32_t lk_win_size;          /* 15  (Stabilizer_legacy.cpp:218 uses 21)   */
    int32_t lk_max_level;         /* 2   (3 pyramid levels)                    */
    int32_t lk_max_iters;         /* 20                                        */
    double  lk_epsilon;           /* 0.03                                      */
    int32_t ransac_max_iters;     /* 500 (Stabilizer.cpp:649)                  */
    double  ransac_threshold;     /* 5.0                                       */
    /* --- virtual canvas (Stabilizer.h:155-162), read when enable_virtual_canvas != 0; carved out of the
     *     reserved tail, so sizeof(vs_params_c) did not change.  preserveEdgeQuality (:161) is never read
     *     by the reference and has no field. ------------------------------------------------------------ */
    float   canvas_scale_factor;  /* :155 default 1.5                          */
    int32_t temporal_buffer_size; /* :156 default 30   (0..256)                */
    float   canvas_blend_weight;  /* :157 default 0.7  (0..1)                  */
    int32_t adaptive_canvas_size; /* :158 default 1                            */
    float   max_canvas_scale;     /* :159 default 2.0                          */
    float   min_canvas_scale;     /* :160 default 1.2                          */
    int32_t edge_blend_radius;    /* :162 default 20                           */
    int32_t reserved[1];
} vs_params_c;

/* Throughput / health counters ("Metrics"). */
typedef struct vs_counters {
    uint64_t frames_in;
    uint64_t frames_out;
    uint64_t detections;          /* goodFeaturesToTrack runs                  */
    int32_t  last_features;       /* points handed to LK on the last frame     */
    int32_t  last_tracked;        /* status != 0                               */
    int32_t  last_inliers;        /* RANSAC inliers of the chosen model        */
    int32_t  last_candidates;     /* GFTT local maxima above the threshold     */
    int32_t  gftt_overflow;       /* !=0: candidate list was truncated         */
    int32_t  reserved[7];
} vs_counters;

/* Per-frame device results, for parity tests and diagnostics. */
typedef struct vs_debug_frame {
    int32_t n_prev;               /* keypoints handed to LK                    */
    int32_t n_valid;              /* pairs after status compaction             */
    int32_t ransac_best_iter;     /* hypothesis index kept (-1: none)          */
    int32_t ransac_iters_run;     /* final niters                              */
    int32_t n_inliers;
    int32_t detected;             /* 1 if GFTT ran on this frame               */
    int32_t n_detected;
    int32_t box_radius;           /* S1 radius actually used (0 if not box)    */
    int32_t intent;               /* MotionIntent chosen for the output frame  */
    int32_t out_index;            /* index of the frame that was warped, or -1 */
    float   transform[3];         /* (dx,dy,da) measured for this frame        */
    float   smoothed[3];          /* smoothed path at out_index                */
    float   warp_matrix[6];       /* T handed to the warp                      */
    double  model[6];             /* refined 2x3 model (double)                */
} vs_debug_frame;

/* Flat mirror of vs::RollCorrection::Parameters (include/video/RollCorrection.h:16-38). */
typedef struct vs_roll_params_c {
    int32_t struct_size;
    int32_t canny_aperture;          /* 3 (only 3 is supported)                */
    double  scale_factor;            /* 0.25                                   */
    double  canny_threshold_low;     /* 50                                     */
    double  canny_threshold_high;    /* 150                                    */
    float   hough_rho;               /* 1                                      */
    float   hough_theta;             /* pi/180                                 */
    int32_t hough_threshold;         /* 100                                    */
    int32_t reserved0;
    double  angle_filter_min;        /* -10 deg                                */
    double  angle_filter_max;        /* +10 deg                                */
    double  angle_smoothing_alpha;   /* 0.1                                    */
    double  angle_decay;             /* 0.995                                  */
    double  max_angle_change_deg;    /* 0.5                                    */
} vs_roll_params_c;

/* Flat mirror of vs::Enhancer::Parameters (include/video/Enhancer.h:12-43). */
typedef struct vs_enh_params_c {
    int32_t struct_size;
    float   brightness;              /* 0   added to every sample (convertTo beta)  */
    float   contrast;                /* 1   multiplies every sample (convertTo alpha) */
    int32_t enable_white_balance;    /* 0                                      */
    float   wb_strength;             /* 1                                      */
    int32_t enable_vibrance;         /* 0                                      */
    float   vibrance_strength;       /* 0.3                                    */
    int32_t enable_unsharp;          /* 0                                      */
    float   sharpness;               /* 0                                      */
    float   blur_sigma;              /* 1   (kernel 2*round(3*sigma)+1 taps, at most 33) */
    int32_t enable_clahe;            /* 0                                      */
    float   clahe_clip_limit;        /* 2                                      */
    int32_t clahe_tile_grid_size;    /* 8   (1..16)                            */
    int32_t enable_denoise;          /* 0   fastNlMeansDenoisingColored(h, h, 7, 21) */
    float   denoise_strength;        /* 10                                     */
    float   gamma;                   /* 1                                      */
    int32_t use_cuda;                /* 0: stage order of the reference's CPU branch, 1: of its CUDA branch */
    int32_t reserved0;
} vs_enh_params_c;

typedef struct vs_stab vs_stab;   /* opaque instance (one video stream)        */
typedef struct vs_roll vs_roll;   /* opaque roll-correction state              */
typedef struct vs_enh vs_enh;     /* opaque enhancer scratch (tables, stream)  */

/* ---- library ------------------------------------------------------------- */
int          vs_abi_version(void);
/* Short tag of the kernel sources this library was built from (hash of the .hip files): measurements that are kept
 * in files (profiles/warp_traffic.json) name the build they belong to. */
const char*  vs_build_tag(void);
const char*  vs_build_info(void);          /* arch, compiler, feature string  */
int          vs_device_count(void);        /* 0 when no usable GPU            */
void         vs_params_default(vs_params_c* p);
const char*  vs_status_string(int status);

/* ---- vs::Stabilizer (Stabilizer.h:177-198) ------------------------------- */
/* Stabilizer(const Parameters&) - Stabilizer.cpp:50-164 */
int vs_stab_create(const vs_params_c* params, int device, vs_stab** out);
/* ~Stabilizer() - Stabilizer.cpp:216-219 */
void vs_stab_destroy(vs_stab* s);
/* clean() - Stabilizer.cpp:221-256 */
int vs_stab_clean(vs_stab* s);
/*
 * stabilize(frame) - Stabilizer.cpp:258-392.  Host frame in, host frame out.
 * *produced = 1 and `out` filled when a stabilized frame is ready, 0 during
 * the warm-up (the reference returns an empty Mat, :263-265,:384-387).
 * `out` must hold out_h rows of out_stride bytes; query with vs_stab_out_size().
 */
int vs_stab_push(vs_stab* s, const uint8_t* data, int w, int h, size_t stride,
                 int fmt, uint8_t* out, size_t out_stride, int* produced);
/* flush() - Stabilizer.cpp:394-400 */
int vs_stab_flush(vs_stab* s, uint8_t* out, size_t out_stride, int* produced);
/* Device-pointer forms: asynchronous on the instance stream, no host sync.
 * `produced` is decided on the host from the frame count alone (E0). */
int vs_stab_push_dev(vs_stab* s, const void* d_data, int w, int h, size_t stride,
                     int fmt, void* d_out, size_t out_stride, int* produced);
/* n consecutive pushes of one geometry in one call: the j-th result that becomes due goes to d_outs[j]; *produced = how many did */
int vs_stab_push_dev_n(vs_stab* s, const void* const* d_frames, int n, int w, int h, size_t stride, int fmt,
                       void* const* d_outs, size_t out_stride, int* produced);
int vs_stab_flush_dev(vs_stab* s, void* d_out, size_t out_stride, int* produced);
int vs_stab_sync(vs_stab* s);
/* size of the frames stabilize() returns for w x h input (crop/border rules,
 * Stabilizer.cpp:981-990,1108-1127) */
int vs_stab_out_size(const vs_stab* s, int w, int h, int* out_w, int* out_h);
/* size of the frame the LAST successful push/flush produced.  Equals
 * vs_stab_out_size() except for the final frame of a flush when a border pad
 * is configured: the reference returns that frame unpadded (Stabilizer.cpp:
 * 774-780); it is then stored top-left in `out`, the rest zero. */
int vs_stab_last_out_dims(const vs_stab* s, int* w, int* h);
int vs_stab_get_counters(vs_stab* s, vs_counters* out);      /* synchronises  */
int vs_stab_get_debug(vs_stab* s, vs_debug_frame* out);      /* synchronises  */
/* enableVirtualCanvas, state after the last output: {canvas w, canvas h, canvas scale (float bits), empty regions,
 * regions filled from the temporal buffer, temporal index of the last fill or -1, window x, window y}
 * (Stabilizer.cpp:2083-2088, 2232-2241, 2115-2132).  Zeros when the canvas is off. */
int vs_stab_canvas_info(const vs_stab* s, int32_t info[8]);
/* copies the debug arrays of the last push: any pointer may be NULL.
 * prev/curr: n_prev * 2 floats; status: n_prev bytes; inliers: n_valid bytes;
 * detected: n_detected * 2 floats; gray: analysis image (aw*ah bytes). */
int vs_stab_get_debug_arrays(vs_stab* s, float* prev_pts, float* curr_pts,
                             uint8_t* status, uint8_t* inliers,
                             float* detected_pts, uint8_t* gray, int* aw, int* ah);
const char* vs_stab_last_error(const vs_stab* s);
void*       vs_stab_stream(vs_stab* s);    /* hipStream_t of the instance     */
/* Host pipeline for vs_stab_push / vs_stab_flush (replaces the synchronous upload - compute - download of the reference's
 * GPU branch, /root/reference/src/Stabilizer.cpp:1021-1031): a call returns the frame the call BEFORE it computed - one
 * more call of latency than vs::Stabilizer::stabilize(): clamp(smoothingRadius,5,35) empty results instead of one less -
 * while its own frame is uploaded; the analysis and the warp of that frame then run behind the caller's back.  Same
 * frames in the same order; vs_stab_flush first hands out the frame that is still held.  Off by default.  Choose while no
 * frame is queued. */
int vs_stab_set_host_pipeline(vs_stab* s, int enable);
/* Page-locked host memory for frames handed to vs_stab_push / vs_stab_flush and the other host entry points: transfers
 * from and to such buffers are DMA transfers of their own (pageable memory is staged by the runtime, about half the
 * rate). */
int  vs_host_alloc(void** p, size_t bytes);
void vs_host_free(void* p);
/* The same for memory the caller already owns (a cv::Mat's buffer): page-locks it in place / lets it go again.  The memory
 * must be unregistered before it is freed. */
int  vs_host_register(void* p, size_t bytes);
int  vs_host_unregister(void* p);
/* Deferred output for vs_stab_push_dev / vs_stab_flush_dev (batch / file-to-file use): the
 * warps of up to `frames` (1..32) consecutive results are issued as ONE kernel launch, each
 * result into the d_out its push named.  Results are complete after vs_stab_sync(); with
 * frames > 1 every push must be given its own d_out until then.  frames = 1 (default):
 * every push issues its own warp.  The host entry points (vs_stab_push / vs_stab_flush)
 * always deliver their result before returning. */
int vs_stab_set_warp_batch(vs_stab* s, int frames);
/* Batch mode for vs_stab_push_dev / vs_stab_flush_dev: the analysis of `frames` (1..64)
 * consecutive pushes - goodFeaturesToTrack, calcOpticalFlowPyrLK and the RANSAC
 * hypothesis scoring, all latency-bound on one frame - runs as ONE launch per stage over
 * the whole group; the ordered part (hypothesis selection + trajectory append, smoothing)
 * stays per frame, and the warps go out together as with vs_stab_set_warp_batch(frames)
 * (at most 32 frames per warp launch: a batch of 64 is two launches back to back).
 * Results are bit-identical to frames = 1 and complete after vs_stab_sync(); every push must
 * be given its own d_out until then.  (The warps of a batch are queued behind the analysis of the
 * batch after the next one, so that a batch's ordered part runs beside the warps of the batch before
 * it; up to two batches' warps are pending between syncs, and vs_stab_sync, vs_stab_flush_dev and
 * vs_stab_clean issue all of them, oldest first.  With frames copied in - zero-copy off - a stream
 * holds up to 35 + 3 x frames of them: its queue ring has 160 slots, 256 for frames > 32.)  Must be chosen before the first frame (or after
 * vs_stab_clean).  BGR8, GRAY8, NV12, P010, I420 and I010 / I012 frames; border padding and crop-and-zoom (BGR8;
 * crop-and-zoom also on YUV streams that opted in, vs_stab_set_yuv_crop_zoom) run batched too; the "fade" border, the virtual canvas and
 * adaptive smoothing keep the per-frame path (each of their outputs depends on the one
 * before it or on a host decision).  Instances of one device share its HIP streams and
 * are to be driven from ONE host thread. */
int vs_stab_set_batch(vs_stab* s, int frames);
/* Zero-copy input for vs_stab_push_dev: the frame is read where the caller put it (decoder
 * surface pool, resident clip) instead of being copied into the instance's queue - the
 * reference aliases the caller's cv::Mat the same way (Stabilizer.cpp:376).  The buffer
 * must stay valid and unchanged until the result of the same push count has been produced
 * (clamp(smoothingRadius,5,35) further pushes plus three times the batch depth: the warps of a
 * batch are issued with the batch after the next one; a vs_stab_sync issues everything that is
 * pending) and vs_stab_sync has returned, or the queue has been drained with vs_stab_flush_dev.  Rows may be padded (decoder pitch); all frames in flight
 * share one pitch, which may change only while nothing is queued.  The frame queue must be
 * empty when the mode is switched. */
int vs_stab_set_zero_copy(vs_stab* s, int enable);
/* Decoder hand-off (the step in front of the path: the reference's capture strings end in
 * `nvv4l2decoder ! nvvidconv ! BGR`, src/CamCap.cpp:49-52,66-72).  Hardware decoders export
 * NV12 surfaces as a Y plane and an interleaved UV plane with a common pitch, the UV plane
 * `uv_offset` bytes behind the Y pointer (rocDecode: pitch * aligned surface height; VA-API:
 * offsets[1]) - not as one block of h*3/2 rows.  Sets that offset for the frames given to
 * vs_stab_push_dev (`in`) and for the surfaces it fills (`out`); 0 = contiguous (h * pitch).
 * With zero-copy input the stabilizer then reads decoder surfaces and writes encoder surfaces
 * in place: no repacking blit on either side.  The frame queue must be empty. */
/* P010 surfaces take the same call: the offsets are in bytes and must be even. */
int vs_stab_set_nv12_layout(vs_stab* s, size_t in_uv_offset, size_t out_uv_offset);
/* The same for I420 surfaces (vs_pixfmt_planar): where the U and the V plane start, in bytes behind the Y pointer, and the
 * pitch of their rows - for the frames given to vs_stab_push_dev in zero-copy or copy-in mode (`in`) and for the device
 * surfaces it fills (`out`), independently.  0 = the default of that field: c_pitch = stride / 2, u_off = h * stride,
 * v_off = u_off + (h/2) * c_pitch (with the u_off and c_pitch in force).  A chroma pitch below w/2 is VS_ERR_INVALID_ARG (here
 * when the geometry is known, else at the next push).  YV12: swap the two offsets.  The frame queue must be empty.
 * I010 / I012 surfaces (vs_pixfmt_planar16) take the same call: offsets and pitch in bytes and even, the pitch at least w bytes.
 * Planar 4:2:2 / 4:4:4 surfaces (vs_pixfmt_planar4xx) take it too, the defaults being those of the format: c_pitch = stride >> sx,
 * v_off = u_off + h * c_pitch; the chroma pitch at least one chroma row's bytes; everything even for the 16-bit formats. */
int vs_stab_set_i420_layout(vs_stab* s, size_t in_u_off, size_t in_v_off, size_t in_c_pitch, size_t out_u_off, size_t out_v_off,
                            size_t out_c_pitch);
/* Crop-and-zoom on YUV streams - the reference's shipped settings, crop_n_zoom with border_size 30 (examples/config.yaml:68-69:
 * warp, cut the border off, resize back to the frame's size, Stabilizer.cpp:1108-1124), on NV12, P010 and the three-plane formats
 * (I420 / YV12, I010, I012, I422, I444, I210, I212, I410, I412).  Off by default: such a stream is VS_ERR_UNSUPPORTED as ever, and
 * allocates and launches exactly what it did.  The reference has no YUV path, so what the mode does is a DEFINITION of this
 * library, which a caller opts into with this call (enable != 0; the frame queue must be empty).  With the mode on,
 * crop_n_zoom != 0, border_size = b > 0, w - 2b > 0 and h - 2b > 0, every plane of a surface is processed on its own:
 *  (a) warp: exactly as the stream warps the plane without a border (BORDER_CONSTANT 0, the same matrices), into a scratch surface;
 *  (b) crop: (b, b, w - 2b, h - 2b) for Y and (b >> sx, b >> sy, (w - 2b) >> sx, (h - 2b) >> sy) for U, V or the interleaved UV
 *      plane.  b must be a multiple of 2^sx and 2^sy - even for every subsampled format, anything for 4:4:4 -, so the chroma
 *      rectangle is exactly the luma rectangle's; an odd b on a subsampled format is VS_ERR_INVALID_ARG with a text that names the
 *      format;
 *  (c) resize: cv::resize(crop, plane size, INTER_LINEAR) into the plane of the result, which has the size of the input plane.  The
 *      taps clamp to the crop, not to the plane: a sample outside the rectangle never enters a result (a cv::Mat ROI).
 *      Coordinates (float)((d + 0.5) * scale - 0.5) with scale = 1 / ((double)dst / src), as cv::resize computes it; coefficients
 *      a0, a1 (columns) and b0, b1 (rows) of 11 bits, rounded and saturated to int16; from the first column whose right tap would
 *      leave the crop on, the sample itself times 2048.
 *      8-bit planes: OpenCV's CV_8U arithmetic (cn 1; cn 2 for the UV plane of NV12) - h = v0 * a0 + v1 * a1 per tap row, result
 *      (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.
 *      16-bit planes: the same coordinates, coefficients and edge rule; the blend is the exact integer S = sum of v_ij * a_i * b_j
 *      over the four taps with ONE rounding, half to even: min(65535, (S + 2^21 - 1 + ((S >> 22) & 1)) >> 22) - in the spirit of
 *      the 16-bit warp blend, and NOT OpenCV's CV_16U resize, which blends with float coefficients.  Nothing depends on the bit
 *      depth or on where the value sits in the word (P010: high bits, I010: low bits).
 * w - 2b <= 0 or h - 2b <= 0: the frame is only warped, as for BGR8.  The last frame of a flush comes back unwarped and uncropped.
 * Analysis, trajectory and warp matrix do not depend on border_size or crop_n_zoom: the debug values are those of the same stream
 * with border_size = 0, bit for bit.  Border pad (crop_n_zoom = 0; a switch of its own, vs_stab_set_yuv_border_pad), the fade border (likewise: vs_stab_set_yuv_fade) and the virtual canvas stay refused on YUV
 * streams, with their texts; GRAY8 is not touched by the mode.  Zero-copy input, the decoder layouts (vs_stab_set_nv12_layout,
 * vs_stab_set_i420_layout) and the host entry points work as without the mode; in batch mode the warps of a launch (<= 32
 * surfaces) fill scratch surfaces and ONE launch behind them resizes all their planes. */
int vs_stab_set_yuv_crop_zoom(vs_stab* s, int enable);
/* Border pad on YUV streams - the reference's other border mode, crop_n_zoom = 0 with border_size = b > 0 and borderType black,
 * reflect, reflect101, replicate or wrap (Stabilizer.cpp:981-990: the frame gets a border of b pixels, the padded frame is warped, the
 * result has (w + 2b) x (h + 2b) pixels; the only mode that keeps every input pixel), on NV12, P010 and the three-plane formats.  Off
 * by default: such a stream is VS_ERR_UNSUPPORTED as ever, and allocates and launches exactly what it did.  The reference has no YUV
 * path, so what the mode does is a DEFINITION of this library, which a caller opts into with this call (enable != 0; the frame queue
 * must be empty).  It is independent of vs_stab_set_yuv_crop_zoom.  With the mode on, crop_n_zoom == 0, border_size = b > 0 and
 * border_type VS_BORDER_BLACK .. VS_BORDER_WRAP, every plane of a surface is processed on its own:
 *  (a) pad: cv::copyMakeBorder per plane.  Y gets b columns and rows on every side, U and V (b >> sx) columns and (b >> sy) rows,
 *      the interleaved UV plane of NV12 / P010 the same in (U, V) pairs.  b must be a multiple of 2^sx and 2^sy - even for every
 *      subsampled format, anything for 4:4:4; an odd b on a subsampled format is VS_ERR_INVALID_ARG with a text that names the
 *      format.  VS_BORDER_BLACK writes the plane's fill sample (below) where the reference writes 0; the other four modes index
 *      the plane itself by cv::borderInterpolate, reflections that fold more than once (a chroma plane smaller than its border)
 *      included.
 *  (b) warp: the padded surface of (w + 2b) x (h + 2b) is warped exactly as the stream warps a surface of that size under the same
 *      matrices (Y under M, chroma under the stream's chroma matrix) but with BORDER_REPLICATE: a tap outside the padded plane
 *      takes the nearest edge sample, each tap by itself (8-bit: the arithmetic of vs_op_warp_affine_ex; 16-bit: P010's blend).
 *      NOT BORDER_CONSTANT 0 as for BGR8: zero samples are not a colour in YUV - (0, 0, 0) is saturated green - whereas the edge
 *      of a padded plane is its border.  With VS_BORDER_BLACK the whole surround of the picture is therefore exactly the fill
 *      colour; with VS_BORDER_REPLICATE the result is the replicate-warp of the frame on a larger canvas.
 * fill: the samples of the three planes as they lie in memory (reserved = 0); NULL = limited-range video black of the format
 * (vs_yuv_video_black: Y = 16 << (bits - 8), U = V = 128 << (bits - 8); P010: in the high bits, 0x1000 and 0x8000).  A value above
 * 255 on an 8-bit format is VS_ERR_INVALID_ARG, here when the format is known, else at the next push.
 * The result has (w + 2b) x (h + 2b) pixels (vs_stab_last_out_dims): out_stride must hold a padded row, default plane offsets and
 * the default chroma pitch are those of a packed surface of the padded size, an explicit output layout (vs_stab_set_nv12_layout,
 * vs_stab_set_i420_layout) describes the padded surface, and an explicit output chroma pitch below a padded chroma row is
 * VS_ERR_INVALID_ARG.  The last frame of a flush has no transform: it comes back unpadded, w x h, with the default offsets of
 * that size at out_stride (vs_stab_last_out_dims reports (w, h)); nothing else of the output is written.  Analysis, trajectory,
 * matrices and debug records do not depend on border_size: they are those of the stream with border_size = 0, bit for bit.
 * The fade border (unless the stream opts in: vs_stab_set_yuv_fade) and the virtual canvas stay refused on YUV streams, with their texts; GRAY8 and the interleaved formats are
 * not touched.  Zero-copy input, the decoder layouts and the host entry points work as without the mode; in batch mode ONE launch
 * in front of each warp launch (<= 32 surfaces) pads all their planes. */
typedef struct vs_yuv_fill { uint16_t y, u, v, reserved; } vs_yuv_fill;   /* samples as they lie in memory */
int vs_stab_set_yuv_border_pad(vs_stab* s, int enable, const vs_yuv_fill* fill);
/* Limited-range video black of a YUV format, as above.  Host only; VS_ERR_INVALID_ARG for a format without chroma planes. */
int vs_yuv_video_black(int fmt, vs_yuv_fill* out);
/* The fade border on YUV streams - the reference's third border mode, borderType "fade" (Stabilizer.cpp:914-978, 1069-1106: the
 * padded frame is blended with a history of earlier results before the warp, and the history takes a tenth of the result after
 * it), on NV12, P010 and the three-plane formats, at 8, 10 and 12 bits.  Off by default: such a stream is VS_ERR_UNSUPPORTED as
 * ever, with the same text, and allocates and launches nothing.  The reference has no YUV path, so what the mode does is a
 * DEFINITION of this library, which a caller opts into with this call (enable != 0; the frame queue must be empty).  It is
 * independent of vs_stab_set_yuv_crop_zoom and vs_stab_set_yuv_border_pad, which go on governing crop_n_zoom and the five modes of
 * cv::copyMakeBorder.  With the mode on, crop_n_zoom == 0, border_size = b > 0, border_type == VS_BORDER_FADE and the virtual
 * canvas off, every plane of a surface is processed on its own, the interleaved UV plane in (U, V) pairs:
 *  (a) pad: as border pad on YUV with VS_BORDER_BLACK.  Y gets b columns and rows on every side, chroma (b >> sx) columns and
 *      (b >> sy) rows; the border holds the plane's fill sample.  b must be a multiple of 2^sx and 2^sy: an odd b on a subsampled
 *      format is VS_ERR_INVALID_ARG with a text that names the format.
 *  (b) history: one surface of the padded size per plane, which the library owns, in a layout of its own.  The first padded frame
 *      IS the history, and the count is then 0 - also after any change of geometry or format, and after any accepted call of this
 *      setter.  The history outlives vs_stab_clean (borderHistory_ outlives Stabilizer::clean()).
 *  (c) blend: alpha = fade_alpha * (count / fade_duration) in float while count < fade_duration (the count then goes up by one),
 *      fade_alpha afterwards; beta = 1.0f - alpha: exactly the BGR8 stream's.  Every sample of the padded plane (the reference's
 *      mask is all 255): v = fmaf(hist, alpha, fl32(frame * beta)), rounded half to even, saturated to 0 .. 255 (8-bit samples) or
 *      0 .. 65535 (16-bit) - cv::addWeighted.  Nothing depends on the bit depth or on where the value sits in the word.  (Weights
 *      outside [0, 1] - a fade_alpha outside it - are VS_ERR_INVALID_ARG at the first blend.)
 *  (d) warp: the blended padded surface is warped exactly as border pad on YUV warps its padded surface: the same matrices,
 *      BORDER_REPLICATE, a result of (w + 2b) x (h + 2b).  Output layout rules, out_stride, the output chroma-pitch refusals and
 *      vs_stab_last_out_dims are those of border pad.
 *  (e) update: history = (T)((1.0f - 0.1f) * history + 0.1f * result): two float products, one float sum, a truncation, for
 *      every sample of every plane (T: uint8_t or uint16_t).
 * fill: as for vs_stab_set_yuv_border_pad; NULL = vs_yuv_video_black of the format; a sample above 255 on an 8-bit format is
 * VS_ERR_INVALID_ARG, here when the format is known, else at the next push.
 * The last frame of a flush has no transform: it comes back unpadded, as with border pad, and leaves history and count alone.
 * Analysis, trajectory, matrices and debug records are those of the stream with border_size = 0, bit for bit.  The fade keeps the
 * per-frame path, as for BGR8: a stream with vs_stab_set_batch(n) runs per frame and gives the same bytes; vs_batch_create goes on
 * refusing the fade.  The virtual canvas stays refused on YUV streams.  Zero-copy input, the decoder layouts and the host entry
 * points work as with border pad.  Three launches per frame: blend (pad and blend fused), warp, update. */
int vs_stab_set_yuv_fade(vs_stab* s, int enable, const vs_yuv_fill* fill);
/* Edge fill on YUV streams - a constant-colour warp border.  A YUV stream warps its planes with BORDER_CONSTANT 0, and zero samples
 * are not a colour in YUV: (0, 0, 0) is saturated green.  The most common stream - output at the input's size, border_size = 0, the
 * picture sliding over its surround - therefore shows green wedges, and so does a crop-and-zoom stream whose correction exceeds
 * border_size (it warps the unpadded frame before it crops).  The reference has no YUV path, so what the mode does is a DEFINITION
 * of this library, which a caller opts into with this call (enable != 0; the frame queue must be empty).  Off by default: such a
 * stream allocates and launches exactly what it does without the call.  With the mode on, every warp of an UNPADDED YUV surface is
 *   cv::warpAffine(..., INTER_LINEAR, BORDER_CONSTANT, borderValue = fill)   per plane:
 * a tap outside the plane reads the plane's fill sample - on the interleaved UV plane of NV12 / P010 the (U, V) fill pair -, each
 * tap decided by itself.  Everything else is what the stream does without the mode: the same coordinates and tables, the 8-bit
 * arithmetic of vs_op_warp_affine_ex, P010's blend (one rounding, half to even) for 16-bit samples, Y under M and chroma under the
 * stream's chroma matrix.  fill (0, 0, 0) gives the bytes of the stream without the mode, bit for bit.
 * The mode applies to the plain stream (border_size == 0; a border_size without crop_n_zoom and without border pad or fade opted
 * in is refused as before) and to the warp into the scratch surface of a crop-and-zoom stream (vs_stab_set_yuv_crop_zoom), whose
 * crop is then taken from the fill-warped surface.  Border pad and fade (vs_stab_set_yuv_border_pad, vs_stab_set_yuv_fade) keep
 * their BORDER_REPLICATE warp of the padded surface: the mode is independent of them and does nothing there.
 * Analysis, trajectory, matrices and debug records, output size and layouts, and the last frame of a flush (copied with no
 * transform) do not depend on the mode, bit for bit.  GRAY8 and the interleaved formats are not touched.  Zero-copy input, the
 * decoder layouts, the host entry points and batch mode work as without the mode; no buffer and no launch is added.
 * fill: as for vs_stab_set_yuv_border_pad - the samples as they lie in memory, reserved = 0; NULL = vs_yuv_video_black of the
 * format; a sample above 255 on an 8-bit format is VS_ERR_INVALID_ARG, here when the format is known, else at the next push. */
int vs_stab_set_yuv_edge_fill(vs_stab* s, int enable, const vs_yuv_fill* fill);

/* ---- several streams of one device scheduled together (BASELINE configs[4]: 64 streams = 8 per GPU) ----------------------
 * The reference runs one Stabilizer per stream, each with its own cv::cuda::Stream objects (src/Stabilizer.cpp:102-104); here a
 * GROUP runs one schedule for all its streams: every step, the frames all members have queued go through ONE launch per stage
 * (one argument block per frame, whichever stream it belongs to), the ordered tails through one launch with a workgroup per
 * stream, the warps through launches of 32 frames.  Results are bit-identical to n_streams independent vs_stab instances.
 *   vs_batch_create      n_streams members with the same parameters, in batch mode with `frames_per_step` frames per stream and
 *                        step (1..64; n_streams x frames_per_step frames are analysed together: 8 x 8 fills the device like one
 *                        stream's batch of 64).  Adaptive smoothing, the fade border and the virtual canvas are per-stream
 *                        modes of vs_stab_* (their outputs depend on each other or on a host decision) and are refused here.
 *   vs_batch_create_params  the same with one parameter block per stream (params_per_stream[n_streams]).  The blocks may differ
 *                        in whatever does not shape a launch: smoothing radius and method, horizon lock, the drone filters'
 *                        settings, corner count and quality.  Frame geometry, analysis size (drone mode on or off for all),
 *                        pyramid depth, tracking window, RANSAC iteration count and the border / crop-and-zoom mode are common;
 *                        a step refuses members that disagree on them (VS_ERR_INVALID_ARG).
 * A standalone vs_stab instance in batch mode (vs_stab_set_batch) runs the same schedule as a group of one.
 *   vs_batch_push_dev    one frame per stream (d_frames[i] == NULL: none for stream i this time); device pointers, one geometry,
 *                        pitch and format for all; produced[i] = 1 when the push made an output of stream i due - it is complete
 *                        after vs_batch_sync, in d_outs[i].  A step runs when a member has frames_per_step frames queued.
 *                        A stream may get its first frame at any call, or never, and may stop early: the group takes its
 *                        launch shape from the first stream(s) to deliver frames, and a stream that joins later with another
 *                        geometry, pitch or launch shape is refused by the next step (VS_ERR_INVALID_ARG).
 *   vs_batch_flush_dev   drains the group, then the next queued frame of every stream (Stabilizer::flush); a stream that
 *                        never had a frame produces nothing.
 *   vs_batch_stream      the member instance i: for the per-stream getters (vs_stab_get_counters, vs_stab_get_debug, vs_stab_sync,
 *                        ...).  Its frames are pushed through the group only: vs_stab_push* / flush* / clean / set_* on a member
 *                        return VS_ERR_INVALID_ARG, vs_stab_destroy ignores it (the group owns its members).
 * One host thread drives a group (and all instances of a device). */
typedef struct vs_batch vs_batch;
int vs_batch_create(int device, int n_streams, const vs_params_c* params, int frames_per_step, vs_batch** out);
int vs_batch_create_params(int device, int n_streams, const vs_params_c* params_per_stream, int frames_per_step, vs_batch** out);
void vs_batch_destroy(vs_batch* b);
int vs_batch_streams(const vs_batch* b);
vs_stab* vs_batch_stream(vs_batch* b, int i);
int vs_batch_set_zero_copy(vs_batch* b, int enable);
int vs_batch_set_nv12_layout(vs_batch* b, size_t in_uv_offset, size_t out_uv_offset);
int vs_batch_set_i420_layout(vs_batch* b, size_t in_u_off, size_t in_v_off, size_t in_c_pitch, size_t out_u_off, size_t out_v_off,
                             size_t out_c_pitch);
/* vs_stab_set_yuv_crop_zoom for every member (the members of a group must agree on the mode; a step refuses those that do not) */
int vs_batch_set_yuv_crop_zoom(vs_batch* b, int enable);
/* vs_stab_set_yuv_border_pad for every member (the members of a group must agree on the mode and the fill) */
int vs_batch_set_yuv_border_pad(vs_batch* b, int enable, const vs_yuv_fill* fill);
/* vs_stab_set_yuv_edge_fill for every member (the members of a group must agree on the mode and the resolved fill: one warp launch
 * serves the frames of all of them) */
int vs_batch_set_yuv_edge_fill(vs_batch* b, int enable, const vs_yuv_fill* fill);
int vs_batch_push_dev(vs_batch* b, const void* const* d_frames, int w, int h, size_t stride, int fmt, void* const* d_outs,
                      size_t out_stride, int* produced);
int vs_batch_flush_dev(vs_batch* b, void* const* d_outs, size_t out_stride, int* produced);
int vs_batch_sync(vs_batch* b);
const char* vs_batch_last_error(const vs_batch* b);

/* Per-stage device timing with HIP events recorded on the instance stream
 * (SURVEY.md section 5 "Tracing").  mode 0 = off, 1 = warp stage only,
 * 2 = every stage, 3 = warp stage and the coordinate tables of batched warps.
 * vs_stab_get_stage_times() synchronises, adds the elapsed
 * time of every event pair recorded since the last call into total_ms[stage]
 * / launches[stage] (arrays of VS_STAGE_COUNT) and resets.  A vs_batch books
 * the stages of its steps on ONE member: the lowest-numbered member that had
 * frames queued when the group's first step ran (member 0 unless it started
 * late); its profiling mode decides what is recorded.  The
 * getter on a member that never had a frame reports zero. */
enum {
    VS_STAGE_COPY_IN = 0,   /* frame into the queue ring                       */
    VS_STAGE_GRAY = 1,      /* resize + BGR2GRAY                               */
    VS_STAGE_PYRAMID = 2,   /* pyrDown + Scharr                                */
    VS_STAGE_LK = 3,
    VS_STAGE_RANSAC = 4,    /* compaction + score + select/refine              */
    VS_STAGE_TRAJ = 5,      /* trajectory append + emit                        */
    VS_STAGE_GFTT = 6,
    VS_STAGE_WARP = 7,      /* warpAffine kernel(s) only                       */
    VS_STAGE_WARP_TABLES = 8, /* batch mode: coordinate tables of a batch's warps (queued behind the batch tail) */
    VS_STAGE_COUNT = 9
};
int vs_stab_set_profiling(vs_stab* s, int mode);
int vs_stab_get_stage_times(vs_stab* s, double* total_ms, int64_t* launches);

/* ---- device memory helpers (so callers need no HIP headers) --------------- */
int vs_dev_set_device(int device);          /* device used by the vs_dev_* / vs_op_* calls of this thread */
int vs_dev_malloc(void** d_ptr, size_t bytes);
int vs_dev_free(void* d_ptr);
int vs_dev_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int vs_dev_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int vs_dev_memset(void* d_dst, int value, size_t bytes);
int vs_dev_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
int vs_dev_sync(void);
/* Bandwidth yardstick for roofline reports: GB/s (read + written bytes) of a plain device copy of `bytes` bytes - 16 bytes
 * per lane, streaming stores - timed with HIP events around `iters` back-to-back launches that walk through buffers of
 * together more than 512 MB, so no launch finds its input in the Infinity Cache. */
int vs_dev_copy_rate(size_t bytes, int iters, double* gbytes_per_s);
const char* vs_last_error(void);           /* thread-local, op-level calls    */

/* ---- stage operators on device buffers (stream = hipStream_t or NULL) ------
 * Each one is the device counterpart of one OpenCV call made by
 * src/Stabilizer.cpp; the file:line of that call is cited per function.     */

/* cv::warpAffine(src,dst,T,size,INTER_LINEAR,BORDER_CONSTANT) -
 * Stabilizer.cpp:1056-1060.  M = forward 2x3 float matrix as the reference
 * builds it (:902-908).  `batch` frames of identical geometry, frame b at
 * d_src + b*src_frame_bytes with matrix M + 6*b.  cn = 3 (BGR8, RGB8), 4 (BGRA8,
 * RGBA8: every channel warped alike) or 1. */
int vs_op_warp_affine(const void* d_src, size_t src_stride, size_t src_frame_bytes,
                      void* d_dst, size_t dst_stride, size_t dst_frame_bytes,
                      int w, int h, int cn, const float* M, int batch, void* stream);
/* NV12 surface: Y plane warped with M, interleaved UV plane at half
 * resolution with the translation halved. */
int vs_op_warp_affine_nv12(const void* d_src, size_t src_stride, void* d_dst,
                           size_t dst_stride, int w, int h, const float* M,
                           int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                           void* stream);
/* P010 surface (vs_pixfmt16): the 16-bit luma plane warped with M, the interleaved 16-bit chroma plane at half resolution
 * with the translation halved; blend rounded half to even (see vs_pixfmt16).  Strides and frame distances in BYTES, all
 * even, as the pointers. */
int vs_op_warp_affine_p010(const void* d_src, size_t src_stride, void* d_dst,
                           size_t dst_stride, int w, int h, const float* M,
                           int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                           void* stream);
/* I420 / YV12 surface (vs_pixfmt_planar): the Y plane warped with M, the U and the V plane - w/2 x h/2, one channel each -
 * with the translation halved; all three planes of up to 32 surfaces in one launch.  Surface b at d_src + b * src_frame_bytes
 * with matrix M + 6 * b.  *_u_off / *_v_off: bytes from a surface's Y pointer to its U / V plane, *_c_pitch: pitch of the chroma
 * rows; 0 = the packed default of that field (vs_stab_set_i420_layout).  border: VS_BORDER_BLACK or VS_BORDER_REPLICATE. */
int vs_op_warp_affine_i420(const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch,
                           void* d_dst, size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch,
                           int w, int h, const float* M, int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                           int border, void* stream);
/* I010 / I012 surface (vs_pixfmt_planar16): the same three planes with 16-bit samples, one call for either depth (the warp does
 * not depend on it).  Strides, offsets and frame distances in bytes and even; a default chroma pitch needs a stride that is a
 * multiple of 4.  The blend is that of vs_op_warp_affine_p010. */
int vs_op_warp_affine_i010(const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch,
                           void* d_dst, size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch,
                           int w, int h, const float* M, int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                           int border, void* stream);
/* Any planar surface: fmt = VS_FMT_I420 (7) ... VS_FMT_I412 (15); the arguments of vs_op_warp_affine_i010 behind it.  Y under M, U and V
 * - (w >> sx) x (h >> sy), one channel each - under Mc = S^-1 M S (vs_pixfmt_planar4xx); both borders; all three planes of up to 32
 * surfaces in one launch.  For fmt 7 ... 9 the result is that of vs_op_warp_affine_i420 / vs_op_warp_affine_i010. */
int vs_op_warp_affine_planar(int fmt, const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch,
                             void* d_dst, size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch,
                             int w, int h, const float* M, int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                             int border, void* stream);
/* The warp of edge fill on YUV streams (vs_stab_set_yuv_edge_fill) as an operator: cv::warpAffine(..., INTER_LINEAR, BORDER_CONSTANT,
 * borderValue = fill) per plane.  The arguments of vs_op_warp_affine_planar, with the fill where that takes a border.  fmt: a planar
 * format, or VS_FMT_NV12 / VS_FMT_P010 - src_u_off / dst_u_off then name the interleaved UV plane (0 = behind the h luma rows), which
 * is warped in (U, V) pairs under the matrix with the halved translation, and the V offsets and chroma pitches are ignored.  fill:
 * samples as they lie in memory, reserved = 0; NULL = vs_yuv_video_black(fmt); a sample above 255 on an 8-bit format is
 * VS_ERR_INVALID_ARG.  (0, 0, 0) gives the bytes of VS_BORDER_BLACK.  Host matrices; up to 32 surfaces per launch, all planes of a
 * launch in one grid.  Every argument is checked on the host before anything is launched; the format, the fill and null arguments
 * are refused even without a device. */
int vs_op_warp_affine_yuv_fill(int fmt, const void* d_src, size_t src_stride, size_t src_u_off, size_t src_v_off, size_t src_c_pitch,
                               void* d_dst, size_t dst_stride, size_t dst_u_off, size_t dst_v_off, size_t dst_c_pitch,
                               int w, int h, const float* M, int batch, size_t src_frame_bytes, size_t dst_frame_bytes,
                               const vs_yuv_fill* fill, void* stream);
/* std::cos / std::sin / std::atan2 on float as the reference calls them (Stabilizer.cpp:662, 902-908, 1689: the host libm's
 * cosf / sinf / atan2f), evaluated by the DEVICE build of the library's restatement: the sum over i in [start, start + count) of
 * a 64-bit mix of (i, bits of f(argument i)) - fn 0 cosf, 1 sinf, 2 atanf: argument i = the float with bit pattern (uint32_t)i;
 * fn 3 atan2f: pair i of a fixed generator.  tests/test_libm.py compares it with the same sum over the host libm's values. */
int vs_op_libm_checksum(int fn, uint64_t start, uint64_t count, uint64_t* result);

/* Test hook: the library's trajectory kernels driven with given models instead of a RANSAC result; no arithmetic of its own.
 * Stream s has n_push[s] pushes (frames 1 .. n_push[s]; frame 0 only enters the queue), push i with the refined model
 * models[s] + 6 i and kinds[s][i] = 1 (model), 0 (estimation failed: the identity) or -1 (nothing to track: no estimate).
 * form 0, per frame (n_streams == 1): traj_append_device per push through a one-lane kernel, then the per-frame emit kernel for a
 *   due release.  dbg_out[s] receives the record after every push.
 * form 1, batch: steps of steps[k % n_steps] (1 .. 64) pushes per stream through the ordered tail kernel, one workgroup per
 *   stream, and the release kernel where the library runs releases apart (every smoother but Kalman).  dbg_out[s] receives the
 *   record after every step the stream took part in.  Adaptive smoothing has no batch form (VS_ERR_UNSUPPORTED).
 * Which push releases which frame is the stabilizer's own rule.  After the last push the queue is flushed through the per-frame
 * emit kernel, as vs_stab_flush_dev does; every flushed frame appends its record to dbg_out[s] too.
 * rel_out[s] receives every release in order (push = -1: flush).  has_M: M (frame matrix, chroma matrix) is valid - in batch
 * form only for the last release of a step; Minv (the two inverse maps) always is.
 * Capacity: dbg_out[s] 2 * n_push[s] + 2 records, rel_out[s] n_push[s] + 1. */
typedef struct vs_traj_release {
    int32_t push, idx, n_seen, has_M;
    float   M[12];
    double  Minv[12];
} vs_traj_release;
int vs_op_trajectory(const vs_params_c* params, int n_streams, const double* const* models, const int32_t* const* kinds,
                     const int32_t* n_push, int form, const int32_t* steps, int n_steps, vs_debug_frame* const* dbg_out,
                     int32_t* n_dbg, vs_traj_release* const* rel_out, int32_t* n_rel);
/* cv::resize(INTER_LINEAR) + cv::cvtColor(BGR2GRAY) - Stabilizer.cpp:304-305,
 * 448-450.  fmt BGR8 / BGRA8 / RGBA8 / RGB8 (resize per channel, then gray from
 * B, G, R; alpha ignored), GRAY8 / NV12 (luma plane resize), P010 (resize of the luma
 * samples' high bytes; the result is an 8-bit gray image), I010 / I012 (resize of
 * min(sample >> 2, 255) / min(sample >> 4, 255) of the luma samples). */
int vs_op_resize_gray(const void* d_src, size_t src_stride, int sw, int sh, int fmt,
                      void* d_dst, size_t dst_stride, int dw, int dh, void* stream);
/* cv::pyrDown as used inside calcOpticalFlowPyrLK - Stabilizer.cpp:611 */
int vs_op_pyr_down(const void* d_src, size_t src_stride, int sw, int sh,
                   void* d_dst, size_t dst_stride, void* stream);
/* Scharr derivative image (int16, interleaved dx,dy) of calcOpticalFlowPyrLK */
int vs_op_scharr(const void* d_src, size_t src_stride, int w, int h,
                 void* d_dst /* int16[h][w][2] */, void* stream);
/* One pyramid level as batch mode builds it: the Scharr derivatives of `items` images (w x h, src_frame_bytes apart) and, when
 * d_next != NULL, their pyrDown ((w+1)/2 x (h+1)/2, next_frame_bytes apart) from one staged read of each image. */
int vs_op_pyr_level(const void* d_src, size_t src_stride, size_t src_frame_bytes, int w, int h, void* d_der /* int16[h][w][2] per image */,
                    void* d_next, size_t next_stride, size_t next_frame_bytes, int items, void* stream);
/* cv::calcOpticalFlowPyrLK(prev,next,prevPts,nextPts,status,err,win,maxLevel,
 * TermCriteria(COUNT+EPS,iters,eps)) - Stabilizer.cpp:611-619 */
int vs_op_pyr_lk(const void* d_prev, const void* d_next, size_t stride, int w, int h,
                 const float* d_prev_pts, int n, float* d_next_pts,
                 uint8_t* d_status, float* d_err,
                 int win, int max_level, int max_iters, double eps, void* stream);
/* cv::goodFeaturesToTrack(gray,corners,maxCorners,quality,minDistance,noArray(),
 * blockSize) - Stabilizer.cpp:354-358,740-744.  d_pts: maxCorners*2 floats,
 * d_count: one int32.  d_eig (optional, w*h floats) receives the min-eigen map. */
int vs_op_gftt(const void* d_gray, size_t stride, int w, int h, int max_corners,
               double quality, double min_distance, int block_size,
               float* d_pts, int32_t* d_count, float* d_eig, void* stream);
/* cv::estimateAffinePartial2D(from,to,noArray(),RANSAC,thr,maxIters) -
 * Stabilizer.cpp:647-649.  d_model: 6 doubles (or NaN when no model),
 * d_inliers: n bytes, d_info: int32[4] = {ok, best_iter, iters_run, n_inliers}. */
int vs_op_estimate_affine_partial2d(const float* d_from, const float* d_to, int n,
                                    double thr, int max_iters, double* d_model,
                                    uint8_t* d_inliers, int32_t* d_info, void* stream);

/* ---- roll correction: vs::RollCorrection (RollCorrection.h:12-50, RollCorrection.cpp:16-155) ---- */
/* RollCorrection::Parameters defaults, RollCorrection.h:16-38 */
void vs_roll_params_default(vs_roll_params_c* p);
/* The function-static sSmoothedAngle / sFirstCall (RollCorrection.cpp:13-14) become
 * per-object state. */
int vs_roll_create(const vs_roll_params_c* params, int device, vs_roll** out);
void vs_roll_destroy(vs_roll* r);
const char* vs_roll_last_error(const vs_roll* r);
/* Parameters travel with every autoCorrectRoll call while the smoothed angle persists
 * (RollCorrection.cpp:16-19): replaces the parameters, keeps the state. */
int vs_roll_set_params(vs_roll* r, const vs_roll_params_c* params);
/* cv::Mat RollCorrection::autoCorrectRoll(const cv::Mat&, const Parameters&),
 * RollCorrection.cpp:16-155.  BGR8 in, BGR8 out of the same size; synchronous. */
int vs_roll_correct(vs_roll* r, const uint8_t* data, int w, int h, size_t stride,
                    uint8_t* out, size_t out_stride);
/* Same with frames in HBM; the warp is left in flight on the object's stream
 * (vs_roll_sync to wait). */
int vs_roll_correct_dev(vs_roll* r, const void* d_data, int w, int h, size_t stride,
                        void* d_out, size_t out_stride);
int vs_roll_sync(vs_roll* r);
/* autoCorrectRoll for an NV12 surface in HBM (BASELINE configs[2]: decoder surfaces), ASYNCHRONOUS.  The reference has no NV12
 * path; defined as the BGR operator's geometry applied per plane: the line search (resize x scale_factor, Canny, HoughLines,
 * RollCorrection.cpp:35-119) runs on the luma plane (a gray picture: no cvtColor), the rotation about the picture centre
 * (:141-149, BORDER_REPLICATE) is applied to the luma plane and, with the translation halved, to the half-size interleaved
 * chroma plane.  uv_offset / out_uv_offset: where the chroma plane starts (0 = h * pitch).  The call hands the frame over and
 * returns (it waits only when 128 frames are pending): eight consecutive frames form a batch whose line searches a worker
 * thread (five of them; environment VS_ROLL_WORKERS: 1 .. 8) queues as ONE launch per stage on its own stream; when the batch's results (24 bytes per frame) have arrived the
 * smoothed angle advances - in call order, on the host - and the rotations are queued.  Results are complete after
 * vs_roll_sync (which closes an incomplete batch); surfaces and result buffers must stay untouched until then.
 * vs_roll_get_state (after vs_roll_sync) reports the last frame. */
int vs_roll_correct_nv12_dev(vs_roll* r, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset,
                             void* d_out, size_t out_pitch, size_t out_uv_offset);
/* n surfaces of one layout, in call order (n calls of the above in one) */
int vs_roll_correct_nv12_dev_n(vs_roll* r, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                               size_t pitch, size_t uv_offset, size_t out_pitch, size_t out_uv_offset);
/* The same for P010 surfaces (vs_pixfmt16: the definitions are there).  pitch, out_pitch >= 2 * w; pointers, pitches and offsets
 * in bytes and even (VS_ERR_INVALID_ARG otherwise).  Batches of eight, the worker threads, VS_ROLL_WORKERS, vs_roll_sync and
 * vs_roll_get_state as for NV12.  One object may receive NV12 and P010 calls: a change of sample size closes the pending batch,
 * exactly as a change of geometry does, and the smoothed angle - per-object state - carries across. */
int vs_roll_correct_p010_dev(vs_roll* r, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset,
                             void* d_out, size_t out_pitch, size_t out_uv_offset);
int vs_roll_correct_p010_dev_n(vs_roll* r, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                               size_t pitch, size_t uv_offset, size_t out_pitch, size_t out_uv_offset);
/* Where the three planes of a planar surface (VS_FMT_I420, VS_FMT_I010, VS_FMT_I012; VS_FMT_I422 ... VS_FMT_I412) lie, in BYTES: rows
 * of `pitch` bytes of Y at the surface pointer; U and V rows `c_pitch` bytes apart, the planes u_off / v_off bytes behind the surface
 * pointer.  0 means the packed default for c_pitch (pitch >> sx: pitch / 2, for 4:4:4 pitch), u_off (behind the Y rows) and v_off
 * (behind the h >> sy rows of U) - the fields of
 * vs_stab_set_i420_layout.  YV12: give both offsets, V first.  The roll and zoom entry points take one such struct for the surface
 * and one for the result (a small POD by pointer, read during the call - not the eight plain size_t arguments the two layouts would
 * otherwise be; vs_stab_set_i420_layout keeps its six plain arguments, its pitches travel with every push). */
typedef struct vs_i420_layout {
    size_t pitch;             /* bytes per Y row */
    size_t c_pitch;           /* bytes per U / V row; 0 = pitch / 2 (4:4:4 formats: pitch) */
    size_t u_off, v_off;      /* bytes from the surface pointer to the U / V plane; 0 = packed behind the plane before */
} vs_i420_layout;
/* autoCorrectRoll for planar 4:2:0 surfaces in HBM, ASYNCHRONOUS: vs_roll_correct_nv12_dev for fmt = VS_FMT_I420 (YV12 through the
 * offsets), VS_FMT_I010 or VS_FMT_I012 (definitions: vs_pixfmt_planar, vs_pixfmt_planar16).  w and h even; for the 16-bit formats
 * pointers, pitches and offsets even and the chroma pitch at least w bytes, for I420 at least w / 2; with c_pitch = 0 the pitch must
 * be even (16-bit: a multiple of 4); the planes of a layout may not overlap.  Violations: VS_ERR_INVALID_ARG with a text that names the
 * format (vs_roll_last_error).  Y, U and V of a batch's surfaces are rotated by ONE launch when the batch's results share a
 * layout.  Batches of eight, worker threads, VS_ROLL_WORKERS, vs_roll_sync and vs_roll_get_state as for NV12.  One object may
 * receive NV12, P010 and planar calls in any order: a change of format or of layout closes the pending batch exactly as a change
 * of geometry does, the smoothed angle carries across.
 * fmt may also be a 4:2:2 / 4:4:4 format - VS_FMT_I422, I444, I210, I212, I410, I412 (definitions: vs_pixfmt_planar4xx): w and h even
 * all the same; a chroma plane holds h >> sy rows of w >> sx samples, so a chroma pitch holds at least (w >> sx) samples, the default
 * chroma pitch is pitch >> sx (4:2:2: the pitch even, 16-bit a multiple of 4; 4:4:4: any pitch of whole samples) and U and V, in either
 * order, lie behind the luma rows (h >> sy) * c_pitch bytes apart at least; the texts name the format.  NV12, P010 and any other
 * value: VS_ERR_INVALID_ARG, the text names the three-plane formats. */
int vs_roll_correct_i420_dev(vs_roll* r, int fmt, const void* d_surface, int w, int h, const vs_i420_layout* in,
                             void* d_out, const vs_i420_layout* out);
int vs_roll_correct_i420_dev_n(vs_roll* r, int fmt, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                               const vs_i420_layout* in, const vs_i420_layout* out);
/* The same for an interleaved colour frame in HBM, ASYNCHRONOUS with the semantics of vs_roll_correct_nv12_dev (batches of eight,
 * worker threads, vs_roll_sync, vs_roll_get_state after it): fmt is VS_FMT_BGR8, VS_FMT_RGB8, VS_FMT_BGRA8 or VS_FMT_RGBA8, the frame
 * one plane of w x h pixels (w, h >= 1: no evenness rule, there is no chroma plane) with rows of `stride` bytes.
 *  - analysis: resize + BGR2GRAY reads B, G, R at the format's positions; the fourth channel never enters.  For BGR8 angle, state and
 *    pixels are those of vs_roll_correct_dev on the same frames, bit for bit; for the other formats the angle is that of the frame's BGR
 *    permutation.
 *  - pixels: every channel, the fourth included, goes through cv::warpAffine's arithmetic as a channel of its own, under
 *    getRotationMatrix2D((w / 2.0f, h / 2.0f), smoothed, 1) with BORDER_REPLICATE.
 * Colour frames, NV12, P010 and planar surfaces may alternate on one object in any order: a change of format, pixel size, geometry or
 * stride closes the pending batch, the smoothed angle carries across; the synchronous vs_roll_correct_dev syncs what is in flight first.
 * Refused before any device call with VS_ERR_INVALID_ARG and a text (vs_roll_last_error) that names the call and the four formats: any
 * other fmt (GRAY8, NV12, P010, planar, out of range), stride or out_stride below w * cn, null pointers, w or h < 1, n < 1. */
int vs_roll_correct_rgb_dev(vs_roll* r, int fmt, const void* d_frame, int w, int h, size_t stride, void* d_out, size_t out_stride);
int vs_roll_correct_rgb_dev_n(vs_roll* r, int fmt, const void* const* d_frames, void* const* d_outs, int n, int w, int h,
                              size_t stride, size_t out_stride);
/* smoothed angle (sSmoothedAngle), the angle detected on the last frame, lines found / used */
int vs_roll_get_state(const vs_roll* r, double* smoothed_deg, double* detected_deg,
                      int* n_lines, int* n_used);
/* cv::Canny(gray, edges, low, high, 3, false) - RollCorrection.cpp:54-61 (there cv::cuda) */
int vs_op_canny(const void* d_gray, size_t stride, int w, int h, double low, double high,
                void* d_edges, size_t edges_stride, void* stream);
/* cv::HoughLines(edges, lines, rho, theta, threshold) - RollCorrection.cpp:66-73.
 * d_lines: max_lines (rho,theta) float pairs in OpenCV order (votes descending),
 * d_count: one int32.
 * At most 8192 lines: when more than 8192 accumulator cells are peaks, the 8192 that cv::HoughLines
 * would list first are kept, in that order (votes descending, ties by ascending accumulator index),
 * and *d_count is min(8192, max_lines).  The roll stage (vs_roll_*) takes its angle statistics over
 * those 8192 and reports n_lines = 8192.  Either way the result is a function of the input alone.
 * Such a frame takes a second round of launches and one more wait of the host (the exact selection). */
int vs_op_hough_lines(const void* d_edges, size_t stride, int w, int h, float rho, float theta,
                      int threshold, float* d_lines, int max_lines, int32_t* d_count, void* stream);
/* cv::warpAffine(src, dst, M(2x3 double, forward), dsize, INTER_LINEAR, border) -
 * RollCorrection.cpp:146-149 (BORDER_REPLICATE there).  border: VS_BORDER_BLACK | VS_BORDER_REPLICATE */
int vs_op_warp_affine_ex(const void* d_src, size_t src_stride, int sw, int sh, void* d_dst,
                         size_t dst_stride, int dw, int dh, int cn, const double* M, int border,
                         void* stream);
/* cv::warpAffine on a plane of 16-bit samples: cn 1 or 2 (the planes of a P010 surface), a destination size of its own, double
 * forward matrix, VS_BORDER_BLACK | VS_BORDER_REPLICATE, P010's blend (vs_pixfmt16).  Strides in bytes; pointers and strides
 * must be even (VS_ERR_INVALID_ARG).  The 16-bit counterpart of vs_op_warp_affine_ex. */
int vs_op_warp_affine16_ex(const void* d_src, size_t src_stride, int sw, int sh, void* d_dst,
                           size_t dst_stride, int dw, int dh, int cn, const double* M, int border,
                           void* stream);

/* ---- auto zoom/crop: vs::AutoZoomCrop (AutoZoomCrop.h:7-17, AutoZoomCrop.cpp:102-283) ---- */
typedef struct vs_azc vs_azc;
int vs_azc_create(int device, vs_azc** out);
void vs_azc_destroy(vs_azc* a);
const char* vs_azc_last_error(const vs_azc* a);
/* cv::Mat AutoZoomCrop::autoZoomCrop(const cv::Mat& corrected, double marginPercent)
 * (marginPercent is ignored by the reference, AutoZoomCrop.cpp:102).  BGR8 (cn 3) or gray
 * (cn 1).  `out` must hold max(w*h, 640*360)*cn bytes and receives packed rows; the
 * result is 640x360 (ow x oh after vs_azc_set_output_size, here and below), or the unchanged w x h frame on the reference's fall-back paths
 * (no contour :149-152, empty crop :238-249).  Synchronous. */
int vs_azc_apply(vs_azc* a, const uint8_t* data, int w, int h, size_t stride, int cn,
                 uint8_t* out, int* out_w, int* out_h);
/* Same with the frame in HBM; out_stride >= max(w,640)*cn.  The scaled crop is left in
 * flight on the object's stream (vs_azc_sync). */
int vs_azc_apply_dev(vs_azc* a, const void* d_data, int w, int h, size_t stride, int cn,
                     void* d_out, size_t out_stride, int* out_w, int* out_h);
int vs_azc_sync(vs_azc* a);
/* autoZoomCrop for an NV12 surface in HBM, ASYNCHRONOUS (the BGR operator's geometry per plane: content mask from the luma
 * plane, gray > 1; the crop rectangle as it is for the luma plane and halved (x/2, y/2, max(1, w/2), max(1, h/2)) for the
 * half-size interleaved chroma plane; each plane scaled to its share of 640 x 360 by the reference's scale matrix,
 * AutoZoomCrop.cpp:246-270).  d_out receives 640 x 360 (chroma 320 x 180 at out_uv_offset) or, on the fall-back paths, the
 * unchanged w x h surface: out_pitch >= max(w, 640), out_uv_offset >= max(h, 360) * out_pitch.  The call hands the frame over
 * and returns a ticket; eight consecutive frames of one geometry form a batch whose mask kernels are one launch each and
 * whose bit masks reach the host with one copy; the contour logic runs on the object's worker threads (it is host work in the
 * reference too, :141-147), a frame each; the worker that finishes a batch's last contour queues the crop-and-scale of the
 * batch as one launch.  vs_azc_result(ticket) waits for that frame's host part and tells what came out, vs_azc_sync completes
 * the pixels (both close an incomplete batch).  Four batches in flight, twelve worker threads (environment VS_AZC_WORKERS:
 * 1 .. 16), results of the last 1024 tickets kept. */
int vs_azc_apply_nv12_dev(vs_azc* a, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset,
                          void* d_out, size_t out_pitch, size_t out_uv_offset, int64_t* ticket);
int vs_azc_apply_nv12_dev_n(vs_azc* a, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                            size_t pitch, size_t uv_offset, size_t out_pitch, size_t out_uv_offset, int64_t* tickets);
/* The same for P010 surfaces (vs_pixfmt16: the definitions are there).  pitch >= 2 * w, out_pitch >= 2 * max(w, 640),
 * out_uv_offset >= max(h, 360) * out_pitch; pointers, pitches and offsets in bytes and even (VS_ERR_INVALID_ARG otherwise).
 * Batches, worker threads, VS_AZC_WORKERS, tickets, vs_azc_result, vs_azc_worker_times and vs_azc_sync as for NV12; one object
 * may receive NV12 and P010 calls, a change of sample size closes the pending batch. */
int vs_azc_apply_p010_dev(vs_azc* a, const void* d_surface, int w, int h, size_t pitch, size_t uv_offset,
                          void* d_out, size_t out_pitch, size_t out_uv_offset, int64_t* ticket);
int vs_azc_apply_p010_dev_n(vs_azc* a, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                            size_t pitch, size_t uv_offset, size_t out_pitch, size_t out_uv_offset, int64_t* tickets);
/* The same for planar 4:2:0 surfaces: fmt = VS_FMT_I420 (YV12 through the offsets), VS_FMT_I010 or VS_FMT_I012; layouts and their
 * rules as for vs_roll_correct_i420_dev.  d_out receives Y 640 x 360, U and V 320 x 180 each - or the unchanged surface - with the
 * planes where `out` puts them whichever size comes out, so `out` describes a surface of max(w, 640) x max(h, 360): pitch >=
 * max(w, 640) samples, u_off >= max(h, 360) * pitch, v_off >= u_off + max(h, 360) / 2 * c_pitch (or U behind V), and its zero
 * fields default to the packed layout of that size.  The three planes of a batch's surfaces are cropped and scaled by ONE launch.
 * Tickets, vs_azc_result, batches, worker threads and vs_azc_sync as for NV12; NV12, P010 and planar calls may alternate.
 * fmt may also be a 4:2:2 / 4:4:4 format (vs_pixfmt_planar4xx): U and V come out at (640 >> sx) x (360 >> sy), `out` holds
 * max(h, 360) >> sy chroma rows of max(w, 640) >> sx samples, and a fall-back surface comes back with its planes at their own sizes. */
int vs_azc_apply_i420_dev(vs_azc* a, int fmt, const void* d_surface, int w, int h, const vs_i420_layout* in,
                          void* d_out, const vs_i420_layout* out, int64_t* ticket);
int vs_azc_apply_i420_dev_n(vs_azc* a, int fmt, const void* const* d_surfaces, void* const* d_outs, int n, int w, int h,
                            const vs_i420_layout* in, const vs_i420_layout* out, int64_t* tickets);
/* The same for an interleaved colour frame in HBM, ASYNCHRONOUS with the semantics of vs_azc_apply_nv12_dev (batches of eight, worker
 * threads, tickets, vs_azc_result, vs_azc_sync): fmt is VS_FMT_BGR8, VS_FMT_RGB8, VS_FMT_BGRA8 or VS_FMT_RGBA8, the frame one plane of
 * w x h pixels (w, h >= 1) with rows of `stride` bytes.
 *  - analysis: the content mask is BGR2GRAY > 1 on B, G, R at the format's positions; the fourth channel never enters.  For BGR8
 *    info8 and pixels are those of vs_azc_apply_dev on the same frame; for the other formats info8 and the rectangle are those of the
 *    frame's BGR permutation.
 *  - pixels: the crop scaled to the object's output size by the reference's CV_32F scale matrix, every channel - the fourth too - as a
 *    channel of its own, BORDER_CONSTANT 0 on the crop (a fourth channel is 0 there as well, as in the stabilizer's BGRA warp).
 *  - fall-back paths (no contour, empty crop): the frame comes back unchanged, all channels, w x h.
 * vs_azc_set_output_size applies as everywhere: out_stride >= max(w, ow) * cn, and d_out holds max(h, oh) rows.
 * Refused before any device call with VS_ERR_INVALID_ARG and a text (vs_azc_last_error) that names the call and the four formats: any
 * other fmt, stride below w * cn, out_stride too small, null pointers, w or h < 1, n < 1. */
int vs_azc_apply_rgb_dev(vs_azc* a, int fmt, const void* d_frame, int w, int h, size_t stride, void* d_out, size_t out_stride,
                         int64_t* ticket);
int vs_azc_apply_rgb_dev_n(vs_azc* a, int fmt, const void* const* d_frames, void* const* d_outs, int n, int w, int h, size_t stride,
                           size_t out_stride, int64_t* tickets);
int vs_azc_result(vs_azc* a, int64_t ticket, int* out_w, int* out_h, int32_t* info8);
/* The output size of the crop-and-scale: ow x oh wherever the comments above say 640 x 360 (the reference hard-codes its author's
 * frame size, AutoZoomCrop.cpp:246-261; the stage means "crop the black corners and zoom back to the frame").  A new object has
 * (640, 360).  (0, 0) = the size of the surface handed over: every result is w x h.  Otherwise both values even and in 2 .. 8192;
 * anything else is VS_ERR_INVALID_ARG with a text in vs_azc_last_error.  The setting is the object's and every entry point obeys it:
 * luma / BGR / gray scaled by [(float)((double)ow / cw), 0, 0; 0, (float)((double)oh / ch), 0] to ow x oh, the chroma planes of the
 * 4:2:0 surfaces by [(float)((double)(ow / 2) / uw), 0, 0; 0, (float)((double)(oh / 2) / uh), 0] to (ow / 2) x (oh / 2) (planar 4:2:2 /
 * 4:4:4: ow >> sx and oh >> sy in place of the halves); buffer and
 * layout rules read max(w, ow) and max(h, oh).  The crop rectangle, info8, the mask and the contours do not depend on it; on the
 * fall-back paths the surface comes back unchanged, w x h.  It applies to frames handed over after the call: like a change of
 * geometry it closes the pending batch, and tickets already issued keep the size they were issued under. */
int vs_azc_set_output_size(vs_azc* a, int out_w, int out_h);
int vs_azc_get_output_size(const vs_azc* a, int* out_w, int* out_h);
/* The stage's crop-and-scale as an operator (the call the stage itself makes for a batch): n <= 24 jobs of one sample size (1 or 2
 * bytes; cn 1 or 2), src = the crop's first sample, each crop scaled to dw x dh by the matrix above (INTER_LINEAR, BORDER_CONSTANT 0:
 * a tap outside the sw x sh crop is 0 even where the plane has samples there; 8-bit arithmetic of vs_op_warp_affine_ex, 16-bit
 * P010's blend).  Sizes 1 .. 32767, strides in bytes, reserved = 0; 16-bit pointers and strides even.
 * path 0: as the stage chooses per job - a job whose output tiles' source boxes fit the staging area (every zoom-in, downscales by
 * less than 1.19 across and 1.4 down) goes to the staged kernel, the others to the direct one: one launch per class;
 * path 1: every job through the direct kernel.  Both give the same bytes. */
typedef struct vs_scale_job { const void* src; size_t src_stride; int32_t sw, sh;
                              void* dst; size_t dst_stride; int32_t dw, dh; int32_t cn, reserved; } vs_scale_job;
int vs_op_scale_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int path, void* stream);
/* host only, needs no device: staged[i] = 1 where path 0 sends job i to the staged kernel */
int vs_op_scale_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int32_t* staged);
/* The same two for crops of interleaved colour frames (the call a batch of vs_azc_apply_rgb_dev makes): 8-bit samples, cn 3 or 4 - a
 * call may mix them -, every channel a channel of its own; the staging rule is that of vs_op_scale_jobs (a staged pixel is one dword
 * whatever its size).  vs_op_scale_jobs itself keeps refusing cn 3 and 4. */
int vs_op_scale_jobs_rgb(const vs_scale_job* jobs, int n, int path, void* stream);       /* 8-bit, cn 3 or 4 */
int vs_op_scale_jobs_rgb_plan(const vs_scale_job* jobs, int n, int32_t* staged);              /* host only */
/* The zoom of crop-and-zoom on YUV surfaces as an operator (the call a stream with vs_stab_set_yuv_crop_zoom makes behind its
 * warps): n = 1 .. 96 jobs of one sample size (1 or 2 bytes; 32 surfaces of up to three planes) in ONE launch, cn 1 and 2 mixed.
 * src = the crop's first sample, sw x sh the crop, dw x dh the destination, reserved = 0; the result is cv::resize(crop, (dw, dh),
 * INTER_LINEAR) as vs_stab_set_yuv_crop_zoom defines it for that sample size - taps clamp to the crop; no byte outside the crop is
 * read, none outside dw x dh written.  Sizes 1 .. 32767, strides in bytes; 16-bit pointers and strides even.  dw >= sw and
 * dh >= sh: anything else is VS_ERR_UNSUPPORTED (this operator is the zoom-in of crop-and-zoom, not a general resize; unlike
 * vs_op_scale_jobs, which is cv::warpAffine arithmetic).  Refusals are decided before any device call, with a text in
 * vs_last_error that names the call and the job.  Asynchronous on `stream`. */
int vs_op_resize_jobs(const vs_scale_job* jobs, int n, int sample_bytes, void* stream);
/* The pad of border pad on YUV surfaces as an operator (the call a stream with vs_stab_set_yuv_border_pad makes in front of its
 * warps): n = 1 .. 96 jobs of one sample size (1 or 2 bytes; 32 surfaces of up to three planes) in ONE launch, cn 1 and 2 mixed.
 * A job pads the sw x sh samples (of cn channels) at src to (sw + 2 bx) x (sh + 2 by) at dst: cv::copyMakeBorder with
 * border = VS_BORDER_BLACK .. VS_BORDER_WRAP, where VS_BORDER_BLACK writes fill[channel] instead of 0; bx = by = 0 copies.
 * bx, by >= 0, padded sizes 1 .. 32767, strides in bytes and below 2^32, reserved = 0; 16-bit pointers and strides even; a fill above 255 with
 * 8-bit samples is refused; source and destination must not overlap.  No byte outside the source plane is read, none outside
 * the padded plane written.  Refusals (VS_ERR_INVALID_ARG) are decided before any device call, with a text in vs_last_error that
 * names the call and the job.  Asynchronous on `stream`. */
typedef struct vs_pad_job { const void* src; size_t src_stride; int32_t sw, sh;      /* samples of cn channels */
                            void* dst; size_t dst_stride; int32_t bx, by;            /* dst is (sw + 2bx) x (sh + 2by) */
                            int32_t cn, border; uint16_t fill[2]; int32_t reserved; } vs_pad_job;
int vs_op_pad_jobs(const vs_pad_job* jobs, int n, int sample_bytes, void* stream);
/* The two launches of the fade border on YUV surfaces as operators (what a stream with vs_stab_set_yuv_fade queues around its
 * warp): n = 1 .. 32 jobs of one sample size (1 or 2 bytes) in ONE launch, cn 1 and 2 mixed; a job is one plane.
 * vs_op_fade_blend_jobs - pad and blend fused: dst, (sw + 2 bx) x (sh + 2 by) samples of cn channels, = addWeighted(hist, alpha,
 * padded, beta) where padded is src (sw x sh) with a border of fill[channel]: v = fmaf(hist, alpha, fl32(padded * beta)), rounded
 * half to even, saturated to the sample.  hist has the padded size; src, hist and dst have their own pitches.  One alpha and one
 * beta serve the launch, both in [0, 1].
 * vs_op_fade_update_jobs: hist = (T)((1.0f - 0.1f) * hist + 0.1f * res), in place, over w x h samples of cn channels.
 * Sizes at least 1, bx, by >= 0, padded sizes at most 32767, strides in bytes, at least a row and below 2^32, reserved = 0; 16-bit
 * pointers and strides even; a fill above 255 with 8-bit samples is refused; dst must not overlap src or hist, nor hist res.  No
 * byte outside the source, history and result planes is read, none outside the destination (history) plane written.  Refusals
 * (VS_ERR_INVALID_ARG) are decided before any device call, with a text in vs_last_error that names the call and the job.
 * Asynchronous on `stream`. */
typedef struct vs_fade_job { const void* src; size_t src_stride; int32_t sw, sh;      /* samples of cn channels */
                             const void* hist; size_t hist_stride;                    /* (sw + 2bx) x (sh + 2by), as dst */
                             void* dst; size_t dst_stride; int32_t bx, by;
                             uint16_t fill[2]; int32_t cn; int64_t reserved; } vs_fade_job;
typedef struct vs_fade_update_job { void* hist; size_t hist_stride; const void* res; size_t res_stride;
                                    int32_t w, h, cn, reserved; } vs_fade_update_job;
int vs_op_fade_blend_jobs(const vs_fade_job* jobs, int n, int sample_bytes, float alpha, float beta, void* stream);
int vs_op_fade_update_jobs(const vs_fade_update_job* jobs, int n, int sample_bytes, void* stream);
/* Diagnostics of the asynchronous path: out9 = {frames through the worker threads; seconds, summed over the threads: without a
 * frame to work on, waiting for the masks of the batches on their way (one worker at a time does), in the contour logic, queueing
 * launches and publishing; batches; seconds, summed over the batches: from a batch's launches to the arrival of its masks on the
 * host, from there to its crop-and-scale launch; seconds the caller waited for a free batch slot}. */
int vs_azc_worker_times(vs_azc* a, double* out9);
/* info8 = {n_contours, contour_points, crop_x, crop_y, crop_w, crop_h, iterations, cropped} */
int vs_azc_get_info(const vs_azc* a, int32_t* info8);
/* cvtColor + threshold(gray,1,255,BINARY) + morphologyEx(MORPH_CLOSE, 5x5 ellipse) -
 * AutoZoomCrop.cpp:111-139 (there cv::cuda) */
int vs_op_content_mask(const void* d_src, size_t stride, int w, int h, int cn, void* d_mask,
                       size_t mask_stride, void* stream);
/* Host part of the stage: findContours(EXTERNAL, SIMPLE) -> largest contour -> filled mask ->
 * interior rectangle -> aspect fix (AutoZoomCrop.cpp:141-228) on a HOST mask (the reference
 * also runs this on the CPU, :141-147).  filled_out (optional, w*h bytes) receives the
 * drawContours(FILLED) mask.  Needs no device. */
int vs_azc_crop_from_mask(const uint8_t* mask, int w, int h, size_t stride, int32_t* info8,
                          uint8_t* filled_out);
/* cv::boundingRect of every contour cv::findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) returns, in the order of
 * that vector: the region list of the virtual canvas (Stabilizer.cpp:2232-2241).  HOST mask; xywh receives up to
 * max_boxes rectangles, *n_boxes the number found.  Needs no device. */
int vs_op_external_boxes(const uint8_t* mask, int w, int h, size_t stride, int32_t* xywh, int max_boxes,
                         int32_t* n_boxes);

/* ---- the compositing stages as operators (the calls the stream itself makes; tests/compref.py states what they compute) ---- */
/* cv::copyMakeBorder (Stabilizer.cpp:981-990): w x h pixels of cn channels (1, 3 or 4) to (w + 2b) x (h + 2b), b >= 0 (b = 0
 * copies), border = VS_BORDER_BLACK .. VS_BORDER_WRAP (VS_BORDER_FADE is no copyMakeBorder mode: VS_ERR_INVALID_ARG).  Pitches in
 * bytes, at least a row each.  Asynchronous on `stream`. */
int vs_op_copy_make_border(const void* d_src, size_t src_stride, int w, int h, int cn, void* d_dst, size_t dst_stride, int b,
                           int border, void* stream);
/* The fade blend (Stabilizer.cpp:914-978): frame = cv::addWeighted(history, alpha, frame, beta, 0) on 8-bit samples, in place,
 * = fma(a, alpha, fl(b * beta)) in float, rounded half to even, saturated.  alpha, beta in [0, 1].  The kernel works on words of
 * four samples: both buffers are 4-byte aligned and hold `bytes` rounded up to a multiple of 4, and the samples of that last
 * word are blended like the rest.  Asynchronous on `stream`. */
int vs_op_fade_blend(const void* d_hist, void* d_frame, size_t bytes, float alpha, float beta, void* stream);
/* The fade history's update (Stabilizer.cpp:1086-1100): history = (uchar)((1 - 0.1f) * history + 0.1f * stabilized), in float,
 * truncated.  The history is packed (rows of row_bytes), `d_stab` has pitch stab_stride >= row_bytes; the kernel works on single
 * samples, so no size is rounded and nothing outside a row's row_bytes is written.  Asynchronous on `stream`. */
int vs_op_fade_update(void* d_hist, const void* d_stab, size_t stab_stride, int row_bytes, int rows, void* stream);
/* The virtual canvas of a BGR8 stream (Stabilizer.cpp:2066-2443) with a given correction in place of the trajectory kernel's.
 * The object holds what the stream's canvas holds (temporal buffer, scale, canvas size) and a stream of its own.  apply: d_frame
 * w x h at `pitch`, t = the correction (dx, dy, da) and transforms = the n >= 0 past transforms (n x 3, read when the adaptive
 * scale is chosen), both HOST floats; the call builds the device trajectory ring the scale kernel reads (n may exceed the ring),
 * writes the w x h result to d_out and is synchronous.  info8 (optional) as vs_stab_canvas_info.  The canvas rules of
 * vs_stab_create hold for `params`; a frame for which a scale the call can choose (the factor, or min / max when adaptive) gives
 * a canvas outside 1..65535 x 1..32767 is VS_ERR_UNSUPPORTED.  Every refusal happens before anything is launched. */
typedef struct vs_canvas_op vs_canvas_op;
int vs_op_canvas_create(vs_canvas_op** out);
int vs_op_canvas_apply(vs_canvas_op* c, const vs_params_c* params, const void* d_frame, size_t pitch, int w, int h, const float* t,
                       const float* transforms, int n, void* d_out, size_t out_pitch, int32_t* info8);
int vs_op_canvas_info(const vs_canvas_op* c, int32_t info[8]);
void vs_op_canvas_destroy(vs_canvas_op* c);

/* ---- colour conversion between YUV surfaces and interleaved 8-bit RGB in HBM (tests/cvtref.py states what they compute) ----
 * The bridge between the decoder / encoder surfaces and the stages that take interleaved colour (the enhancer, border pad,
 * crop-and-zoom, fade, the virtual canvas, the C++ classes): what the reference does with nvvidconv in front of its pipeline
 * (src/CamCap.cpp:49-52,66-72) and with cv::cvtColor(COLOR_BGR2YUV_I420) plus a byte loop on the host behind it
 * (examples/JetsonEncoder.cpp:199-241).
 *
 * yuv_fmt: any non-interleaved format - VS_FMT_NV12, VS_FMT_P010, VS_FMT_I420 (YV12 through the offsets), VS_FMT_I010, VS_FMT_I012,
 * VS_FMT_I422, VS_FMT_I444, VS_FMT_I210, VS_FMT_I212, VS_FMT_I410, VS_FMT_I412; its chroma planes have (w >> sx) x (h >> sy) samples.
 * rgb_fmt: VS_FMT_BGR8, VS_FMT_RGB8, VS_FMT_BGRA8 or VS_FMT_RGBA8; alpha is written as 255 and ignored on input.
 * n = 1 .. 32 surfaces of one geometry and layout are converted in ONE launch, asynchronous on `stream`; d_surfaces and d_rgb are
 * HOST arrays of n device pointers, read during the call.
 * Layout of the YUV side: struct vs_i420_layout with its defaults per format (c_pitch 0 = pitch >> sx, u_off 0 = behind the h luma
 * rows, v_off 0 = behind U).  NV12 / P010: u_off is the offset of the interleaved (U, V) plane (0 = h * pitch), v_off must be 0 and
 * c_pitch 0 or equal to pitch.  rgb_stride: bytes per row of the RGB side, at least w * 3 (w * 4 with alpha).
 *
 * Definition: ITU-R BT.601 limited range in the fixed-point arithmetic of OpenCV 4.x (imgproc/src/color_yuv.simd.hpp), the path of
 * COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420 and COLOR_BGR2YUV_I420.  All arithmetic in 32-bit integers, >> an arithmetic shift,
 * sat = clamp to 0 .. 255, H = 1 << 19.
 *   YUV -> RGB, pixel (x, y) with the chroma sample at (x >> sx, y >> sy), nearest, no interpolation:
 *     Y' = max(0, Y - 16) * 1220542;  u = U - 128;  v = V - 128
 *     R = sat((Y' + H + 1673527 * v) >> 20)
 *     G = sat((Y' + H - 852492 * v - 409993 * u) >> 20)
 *     B = sat((Y' + H + 2116026 * u) >> 20)
 *   RGB -> YUV: Y for every pixel; U and V from the ONE pixel at (cx << sx, cy << sy), the top-left of its block, no averaging
 *   (that is what OpenCV does):
 *     Y = sat((269484 * R + 528482 * G + 102760 * B + H + (16 << 20)) >> 20)
 *     U = sat((-155188 * R - 305135 * G + 460324 * B + H + (128 << 20)) >> 20)
 *     V = sat((460324 * R - 385875 * G - 74448 * B + H + (128 << 20)) >> 20)
 *   16-bit samples are read as the byte their analysis uses - P010: sample >> 8; the low-bit formats: min(sample >> (bits - 8), 255) -
 *   and written as byte << 8 (P010) or byte << (bits - 8).  OpenCV has no code for these samples, nor for planar 4:2:2 / 4:4:4:
 *   there the formulas above with the format's (sx, sy) ARE the definition.
 * Refusals (VS_ERR_INVALID_ARG, vs_last_error names the format), all decided before any device call: a null pointer; n outside
 * 1 .. 32; w not a multiple of 1 << sx or h not one of 1 << sy (or a size above 65536); a pitch below a row's bytes; rgb_stride
 * < w * cn; an odd pointer, pitch or offset of a 16-bit format; with c_pitch = 0 and sx = 1 an odd pitch (16-bit: one that is no
 * multiple of 4); planes of a layout that overlap; a format of the wrong family on either side.  Valid arguments on a machine without
 * a device: VS_ERR_NO_DEVICE.  Nothing outside a row's w samples is written (padding and gaps between planes keep their bytes). */
int vs_op_cvt_yuv_to_rgb(int yuv_fmt, const void* const* d_surfaces, const vs_i420_layout* in, int rgb_fmt, void* const* d_rgb,
                         size_t rgb_stride, int n, int w, int h, void* stream);
int vs_op_cvt_rgb_to_yuv(int rgb_fmt, const void* const* d_rgb, size_t rgb_stride, int yuv_fmt, void* const* d_surfaces,
                         const vs_i420_layout* out, int n, int w, int h, void* stream);

/* ---- the colour space of a conversion: matrix, range, and how RGB -> YUV takes the chroma of a block ----------------------------
 * The two calls above speak BT.601 limited range with the top-left pixel of a block as its chroma.  Decoder surfaces of 1280 x 720
 * and above are BT.709 (HEVC / AV1 1080p, 2160p) or BT.2020 (UHD, 10-bit masters); MJPEG cameras and screen capture are full range.
 * A descriptor names the space; a null pointer and the all-zero struct both mean what the calls above compute, bit for bit. */
enum vs_cvt_matrix { VS_CVT_MATRIX_BT601 = 0, VS_CVT_MATRIX_BT709 = 1, VS_CVT_MATRIX_BT2020 = 2 };   /* BT.2020 non-constant luminance */
enum vs_cvt_range  { VS_CVT_RANGE_LIMITED = 0, VS_CVT_RANGE_FULL = 1 };
enum vs_cvt_chroma { VS_CVT_CHROMA_TOPLEFT = 0, VS_CVT_CHROMA_MEAN = 1 };                            /* RGB -> YUV only */
typedef struct vs_cvt_colorimetry { int32_t matrix, range, chroma_down, reserved; } vs_cvt_colorimetry;  /* reserved must be 0 */
/* Definition.  The shape is the one stated above: 32-bit integers, >> an arithmetic shift, sat = clamp to 0 .. 255, H = 1 << 19,
 * the chroma sample at (x >> sx, y >> sy) on the way up (nearest), the same byte view of 16-bit samples.  With fifteen integers
 * y_off, CY, RV, GV, GU, BU, YR, YG, YB, UR, UG, UB, VR, VG, VB:
 *   YUV -> RGB:  Y' = max(0, Y - y_off) * CY;  u = U - 128;  v = V - 128
 *                R = sat((Y' + H + RV*v) >> 20)   G = sat((Y' + H - GV*v - GU*u) >> 20)   B = sat((Y' + H + BU*u) >> 20)
 *   RGB -> YUV:  Y = sat((YR*R + YG*G + YB*B + H + (y_off << 20)) >> 20)
 *                U = sat((UR*R + UG*G + UB*B + H + (128 << 20)) >> 20)      V likewise with VR, VG, VB
 * (BT.601, limited): the integers are OpenCV's, those written out above - they are not derived, so the default cannot move.
 * The other five combinations: from the standard's Kr, Kb (Kg = 1 - Kr - Kb) in exact rational arithmetic, each value scaled by
 * 2^20 and rounded half away from zero:
 *   scales    ys = 219/255, cs = 224/255, y_off = 16 in limited range; ys = cs = 1, y_off = 0 in full range
 *   YUV->RGB  CY = 1/ys, RV = 2(1-Kr)/cs, BU = 2(1-Kb)/cs, GV = 2(1-Kr)*Kr/Kg/cs, GU = 2(1-Kb)*Kb/Kg/cs
 *   luma      YR, YG, YB = Kr*ys, Kg*ys, Kb*ys
 *   U         UR = -Kr/(2(1-Kb))*cs, UG = -Kg/(2(1-Kb))*cs, UB = cs/2
 *   V         VR = cs/2, VG = -Kg/(2(1-Kr))*cs, VB = -Kb/(2(1-Kr))*cs
 *   Kr, Kb    BT.601 0.299, 0.114;  BT.709 0.2126, 0.0722;  BT.2020 0.2627, 0.0593
 * Mean chroma (VS_CVT_CHROMA_MEAN, RGB -> YUV; luma is unchanged): with s = sx + sy and SR, SG, SB the sums of R, G, B over the
 * (1 << sx) x (1 << sy) pixels of a chroma block,
 *   U = sat((UR*SR + UG*SG + UB*SB + (H << s) + (128 << (20 + s))) >> (20 + s))      V likewise
 * For 4:4:4 that is the top-left rule.  The sample sits at the block centre; left-sited filters and interpolation on the way up
 * are not built.  Nothing overflows 32 bits: the largest intermediate is 2^30 (mean chroma, full range, s = 2).
 * chroma_down is IGNORED by the YUV -> RGB direction (any value of the enum is accepted there and changes nothing).
 *
 * vs_op_cvt_yuv_to_rgb_cs / vs_op_cvt_rgb_to_yuv_cs: the calls above with the descriptor in front of `stream`; the same refusals,
 * the same one launch for n = 1 .. 32; the calls above are these with cs = NULL.  Further refusals, VS_ERR_INVALID_ARG with a
 * text in vs_last_error that names the call and the field, decided before any device call (so a bad descriptor on a machine
 * without a device gives VS_ERR_INVALID_ARG, not VS_ERR_NO_DEVICE, and the refused call writes and queues nothing): matrix, range
 * or chroma_down outside its enum; reserved != 0. */
int vs_op_cvt_yuv_to_rgb_cs(int yuv_fmt, const void* const* d_surfaces, const vs_i420_layout* in, int rgb_fmt, void* const* d_rgb,
                            size_t rgb_stride, int n, int w, int h, const vs_cvt_colorimetry* cs, void* stream);
int vs_op_cvt_rgb_to_yuv_cs(int rgb_fmt, const void* const* d_rgb, size_t rgb_stride, int yuv_fmt, void* const* d_surfaces,
                            const vs_i420_layout* out, int n, int w, int h, const vs_cvt_colorimetry* cs, void* stream);
/* Host only, needs no device: the integers the kernels use for a descriptor (NULL = the default), in the order
 * y_off, CY, RV, GV, GU, BU, YR, YG, YB, UR, UG, UB, VR, VG, VB, 0.  VS_ERR_INVALID_ARG for a bad descriptor or a null `out`. */
int vs_cvt_coefficients(const vs_cvt_colorimetry* cs, int32_t out[16]);
/* Host only: the common convention for video whose container carries no tag - h > 576: BT.709 limited, otherwise BT.601 limited;
 * never BT.2020, never full range; chroma_down = VS_CVT_CHROMA_TOPLEFT.  A convenience for the caller: the library itself never
 * guesses. */
void vs_cvt_colorimetry_guess(int w, int h, vs_cvt_colorimetry* out);

/* ---- conversion between YUV surface formats in HBM (tests/yuvref.py states what it computes) -------------------------------------
 * Every stage returns the format it was given; what follows the library often takes another one - a hardware encoder NV12 and
 * P010, x264 and libvpx I420 - and a software decoder delivers I420 / I010 / I210 where a hardware path delivers NV12 / P010.  The
 * reference bridges this on the host (videoconvert ! video/x-raw,format=NV12, examples/vs.cpp:298, src/RTSPServer.cpp:85).  This
 * call does it on the device without a colour matrix and without an RGB frame: samples keep every bit the destination can hold.
 *
 * vs_op_cvt_yuv_to_yuv converts n = 1 .. 32 surfaces of one geometry from src_fmt in layout `in` to dst_fmt in layout `out`, in ONE
 * launch, asynchronous on `stream`; d_src and d_dst are HOST arrays of n device pointers, read during the call.  src_fmt and
 * dst_fmt: any of the eleven non-interleaved formats (VS_FMT_NV12, VS_FMT_P010, VS_FMT_I420 ... VS_FMT_I412) in any pairing; the same
 * format twice is a repack to another pitch or plane order (I420 <-> YV12 by swapping u_off and v_off).  Layouts, their defaults and
 * their rules are those of vs_op_cvt_yuv_to_rgb, on both sides.  desc: NULL and the all-zero struct mean the same - truncate,
 * top-left.
 *
 * Definition: exact integer arithmetic in two steps.
 *  Step 1, depth, per sample and on every plane.  A format holds values of b bits: 8-bit formats b = 8; the low-bit formats b = 10
 *  or 12, the value in the low bits; P010 b = 16 - the whole word, its most significant bits meaningful (P012 / P016 content passes
 *  through, as everywhere in this header).  d = b_in - b_out.
 *    d = 0: the word is unchanged (out-of-range high bits of a low-bit format are copied, not clamped).
 *    otherwise v = sample, for a low-bit source v = min(sample, 2^b_in - 1), and
 *    d < 0: out = v << -d
 *    d > 0, VS_YUV_DEPTH_TRUNCATE: out = v >> d
 *    d > 0, VS_YUV_DEPTH_ROUND:    out = min((v + (1 << (d - 1))) >> d, 2^b_out - 1)
 *  Truncation is the default because it gives the byte that the analysis and vs_op_cvt_yuv_to_rgb read: P010 -> NV12 is sample >> 8,
 *  I010 -> I420 is min(sample >> 2, 255).  Going up in depth and coming back down is the identity under either rule.
 *  Step 2, chroma siting, on the step-1 values of U and V, with (sx, sy) of each side (the format set only ever moves both axes
 *  the same way).
 *    same shifts: copy.
 *    down, dsx = sx_out - sx_in, dsy = sy_out - sy_in, s = dsx + dsy > 0:
 *      VS_CVT_CHROMA_TOPLEFT: the sample at (cx << dsx, cy << dsy)
 *      VS_CVT_CHROMA_MEAN:    (sum of the (1 << dsx) x (1 << dsy) block + (1 << (s - 1))) >> s; the largest intermediate is 4 * 65535 + 2
 *    up, usx = sx_in - sx_out, usy = sy_in - sy_out: the sample at (cx >> usx, cy >> usy), nearest.  Interpolating filters and
 *    left-sited down-filters are not built, as in the colour conversion.
 *  NV12 / P010 interleave (U, V) pairs, the three-plane formats do not: that is layout only.
 * Refusals (VS_ERR_INVALID_ARG, decided before any device call; vs_last_error names the call, the side - "source" / "destination" -
 * and the format): everything vs_op_cvt_yuv_to_rgb refuses about a YUV side, for either side - so w must be a multiple of
 * 1 << max(sx_in, sx_out) and h of 1 << max(sy_in, sy_out); d_src[i] == d_dst[j] for any i, j (surfaces may not overlap; equal
 * pointers are the part that can be checked); a descriptor field outside its enum; a reserved field that is not 0.  Valid arguments
 * on a machine without a device: VS_ERR_NO_DEVICE.  Nothing outside a row's samples is written (padding and gaps keep their bytes). */
enum vs_yuv_depth_down { VS_YUV_DEPTH_TRUNCATE = 0, VS_YUV_DEPTH_ROUND = 1 };
typedef struct vs_yuv_cvt_desc { int32_t depth_down;      /* vs_yuv_depth_down */
                                 int32_t chroma_down;     /* vs_cvt_chroma: TOPLEFT / MEAN */
                                 int32_t reserved[2];     /* must be 0 */ } vs_yuv_cvt_desc;
int vs_op_cvt_yuv_to_yuv(int src_fmt, const void* const* d_src, const vs_i420_layout* in,
                         int dst_fmt, void* const* d_dst, const vs_i420_layout* out,
                         int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream);
/* Host only, needs no device: the layout of a w x h surface of `fmt` with every default filled in (*resolved: for NV12 / P010
 * c_pitch = pitch, u_off = the interleaved plane, v_off = 0 - a layout the conversions accept as it is), and the number of bytes
 * from the surface pointer to the end of its last sample (*bytes) - what a caller allocates for a format it did not hold before.
 * lay == NULL: all defaults at the tight pitch (w samples).  resolved and bytes may each be NULL.  Refuses exactly what
 * vs_op_cvt_yuv_to_rgb refuses about a format, a size and a layout (VS_ERR_INVALID_ARG, the text in vs_last_error). */
int vs_yuv_surface_layout(int fmt, int w, int h, const vs_i420_layout* lay, vs_i420_layout* resolved, size_t* bytes);

/* ---- packed 4:2:2 capture formats <-> YUV surfaces in HBM (tests/packedref.py states what they compute) ----------------------------
 * Capture sources deliver none of the surface formats: SDI / HDMI cards UYVY and, at ten bits, v210; UVC cameras and V4L2 devices
 * YUY2 (YUYV); some hardware paths Y210.  These two calls are the conversion in front of a stage (capture -> NV12 / P010 / I422 ...)
 * and behind one (-> UYVY / v210 for playout), on the device.  The packed formats have an enum of their own: they are NOT VS_FMT_*
 * values, and no stream, stage or other operator takes them.
 *
 * vs_op_cvt_packed_to_yuv converts n = 1 .. 32 packed frames of w x h pixels, rows src_pitch bytes apart, to n surfaces of dst_fmt
 * in layout `out`; vs_op_cvt_yuv_to_packed n surfaces of src_fmt in layout `in` to n packed frames, rows dst_pitch bytes apart.  ONE
 * launch each, asynchronous on `stream`; d_src and d_dst are HOST arrays of n device pointers, read during the call.  The surface
 * side: any of the eleven non-interleaved formats; its layouts, defaults and rules are those of vs_op_cvt_yuv_to_yuv.  A packed
 * pitch of 0 is the format's default.  desc: NULL and the all-zero struct mean the same - truncate, top-left.
 *
 * Memory of the packed side: words are little-endian, a row starts at ptr + y * pitch, w is even.
 *  VS_PACKED_YUY2, VS_PACKED_UYVY, VS_PACKED_YVYU: 8-bit samples, two pixels in 4 bytes: Y0 U Y1 V, U Y0 V Y1, Y0 V Y1 U.  Row bytes
 *   2 w, which is the default pitch; any pitch >= the row bytes and any pointer.
 *  VS_PACKED_Y210: the YUY2 layout with 16-bit words.  The value is the whole word, its most significant bits meaningful, exactly
 *   as for P010 (Y216 content passes through).  Row bytes 4 w, the default pitch; pointer and pitch must be even.
 *  VS_PACKED_V210: a group of 16 bytes holds 6 pixels as four 32-bit words of three 10-bit fields, at bits 0-9, 10-19 and 20-29:
 *     w0 = Cb0 | Y0 << 10 | Cr0 << 20      w1 = Y1 | Cb1 << 10 | Y2 << 20
 *     w2 = Cr1 | Y3 << 10 | Cb2 << 20      w3 = Y4 | Cr2 << 10 | Y5 << 20
 *   Row bytes 16 * ceil(w / 6): a partial last group is still 16 bytes of the row; any even w is taken.  The default pitch is the
 *   format's convention, 128 * ceil(w / 48); pointer and pitch must be multiples of 4.  Reading: bits 30-31 and the fields of
 *   pixels >= w are ignored.  Writing: bits 30-31 are 0, and the fields of pixels >= w in the last group are 0.
 *   (Y = 0x040 .. 0x045, Cb = 0x200, 0x201, 0x202, Cr = 0x300, 0x301, 0x302 are 0x30010200, 0x04280441, 0x20210F01, 0x045C0844.)
 *
 * Definition: the two steps of vs_op_cvt_yuv_to_yuv, word for word, with the packed side a 4:2:2 format, (sx, sy) = (1, 0), that
 * holds values of b = 8 bits (the three 8-bit orders), b = 16 (Y210: the whole word, like P010) or b = 10 (v210).  Step 1, depth:
 * truncate, or round with saturation; step 2, chroma siting: top-left or the block mean going down (a 4:2:0 destination, a 4:4:4
 * source), nearest going up.  One addition, to step 1: a v210 field holds ten bits, so a v210 destination takes min(value, 1023) -
 * also when d = 0 and a low-bit source (I010, I210, I410) carries out-of-range high bits, which the surface formats copy.  SDI-illegal codes
 * (0 - 3, 1020 - 1023) are not clamped: the calls move samples, they do not legalise them.  So, bit for bit,
 *   YUY2 / UYVY / YVYU -> X is vs_op_cvt_yuv_to_yuv(I422 -> X) on the de-interleaved planes, v210 -> X is (I210 -> X).
 * Refusals (VS_ERR_INVALID_ARG, decided before any device call; vs_last_error names the call, the side - "source" / "destination" -
 * and the format): everything vs_op_cvt_yuv_to_yuv refuses about the surface side (so h must be even for a 4:2:0 format);
 * packed_fmt outside the enum; an odd w; a packed pitch below the row bytes; a packed pitch or pointer that breaks the alignment
 * above; a NULL pointer; d_src[i] == d_dst[j] for any i, j; n outside 1 .. 32; a descriptor field outside its enum; a reserved
 * field that is not 0.  Valid arguments on a machine without a device: VS_ERR_NO_DEVICE.  Nothing outside a row's bytes is written
 * on either side: pitch padding, gaps between planes and the bytes behind the last row keep their contents.
 * Not built: packed formats as stream or stage formats, or in the colour conversions and the enhancer's YUV calls (two calls chain
 * through a surface format); packed 4:4:4 (AYUV, VUYA, Y410); semi-planar 4:2:2 / 4:4:4; big-endian samples; interlaced fields;
 * interpolating chroma filters; SDI range legalisation. */
enum vs_packed_fmt { VS_PACKED_YUY2 = 0, VS_PACKED_UYVY = 1, VS_PACKED_YVYU = 2, VS_PACKED_Y210 = 3, VS_PACKED_V210 = 4 };
int vs_op_cvt_packed_to_yuv(int packed_fmt, const void* const* d_src, size_t src_pitch,
                            int dst_fmt, void* const* d_dst, const vs_i420_layout* out,
                            int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream);
int vs_op_cvt_yuv_to_packed(int src_fmt, const void* const* d_src, const vs_i420_layout* in,
                            int packed_fmt, void* const* d_dst, size_t dst_pitch,
                            int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream);
/* Host only, needs no device: the bytes of a row of a w x h packed frame (*row_bytes), its pitch (*resolved_pitch: `pitch`, or the
 * format's default for 0) and the number of bytes from the frame pointer to the end of its last row's bytes (*bytes =
 * (h - 1) * pitch + row bytes).  Each result may be NULL.  Refuses exactly what the two calls refuse about a packed format, a size
 * and a pitch (VS_ERR_INVALID_ARG, the text in vs_last_error). */
int vs_packed_layout(int packed_fmt, int w, int h, size_t pitch, size_t* row_bytes, size_t* resolved_pitch, size_t* bytes);

/* ---- resize to an output size: INTER_LINEAR and INTER_LANCZOS4 ----------------------------------------------------------------
 * A stream in border-pad or fade mode returns surfaces of (w + 2b) x (h + 2b); the reference's shipped main resizes what the
 * stabilizer returns to the frame size in front of its encoder - cv::resize(..., INTER_LANCZOS4) in processing mode
 * (examples/vs.cpp:651-652), INTER_LINEAR in passthrough mode and for a camera of another size (:541, :638; vsg.cpp:255).  These
 * calls do it on the device, in any ratio, up or down: sw x sh -> dw x dh.  (vs_op_resize_jobs is the zoom-in of crop-and-zoom only,
 * vs_op_scale_jobs is cv::warpAffine arithmetic with a constant-0 border and two taps whatever the ratio.)
 *
 * Definition (tests/resizeref.py states it in numpy and `math`).  Per axis src -> dst and destination index d:
 *   scale = 1.0 / ((double)dst / src), f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f = f - (float)s in float32.
 * VS_INTERP_LINEAR is cv::resize(INTER_LINEAR) as vs_stab_set_yuv_crop_zoom defines it, for any ratio: columns follow the edge rule
 *   (s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; from the first column whose second tap would leave the source on, the
 *   result of the horizontal pass is the sample x 2048), rows keep their coefficients and clamp both tap rows; coefficients
 *   saturate_cast<short>((1 - f) * 2048.f) and (f * 2048.f); 8-bit vertical pass (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2,
 *   16-bit the exact sum with ONE rounding half to even at bit 22.  The exact 2 : 1 case (sw == 2 dw and sh == 2 dh) is the 2 x 2
 *   mean (s00 + s01 + s10 + s11 + 2) >> 2 at both depths (cv::resize reroutes it to INTER_AREA).  For dw >= sw and dh >= sh the
 *   result equals vs_op_resize_jobs' bit for bit.
 * VS_INTERP_LANCZOS4 is cv::resize(INTER_LANCZOS4) for CV_8U: neither s nor f is clamped; eight taps at clamp(s - 3 + k, 0, src - 1),
 *   k = 0 .. 7, on both axes; their weights are interpolateLanczos4's - f < FLT_EPSILON: (0,0,0,1,0,0,0,0); otherwise with
 *   cs = {{1,0},{-r,-r},{0,1},{r,-r},{-1,0},{r,r},{0,-1},{-r,r}}, r = 0.70710678118654752440084436210485, y0 = -(f + 3) * pi / 4,
 *   s0 = sin(y0), c0 = cos(y0) in double: w[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)), y = -(f + 3 - i) * pi / 4; the
 *   float running sum of the w[i]; w[i] *= 1.f / sum - and the coefficient of a tap is saturate_cast<short>(w[i] * 2048.f).  The eight
 *   coefficients are NOT renormalised (their sum ranges from 2045 to 2051: a flat 255 area may come out as 254).
 *   out = clamp((S + 2^21) >> 22, 0, max_value), S = the exact integer sum over the 64 taps, arithmetic shift.  16-bit samples: the
 *   same coefficients and sums with S in 64 bits - a definition of this library (OpenCV's CV_16U path has float coefficients).
 *   The kernel is not widened for downscales, as in OpenCV: a strong downscale aliases.
 *   Over a dense scan of f the positive coefficients of an axis sum to at most 2780 and the negative ones to at most 732, so on
 *   8-bit planes |S| <= 255 * 2780^2 < 2^31 - 2^21.
 * The same size in and out is the identity at either interpolation.  max_value: every result is clamped to 0 .. max_value, 0 = the
 * sample type's maximum.
 * Coefficients are built on the host from the double sin / cos of the C library (never a device libm); the kernels read them as
 * tables from device memory: one table per (src, dst, interp, axis), built once, uploaded and cached per device (64 MiB of tables
 * per device; when they are full the device is drained before places are given out anew).  A CALL THAT MEETS A NEW AXIS MAY BLOCK
 * WHILE ITS TABLE IS UPLOADED; later calls only launch.  A single call whose distinct tables exceed the 64 MiB is VS_ERR_CAPACITY.
 *
 * vs_op_resample_jobs - plane jobs: n = 1 .. 96 jobs of one sample size (1 or 2 bytes) in ONE launch per path class; vs_scale_job
 *   as it is: src = the plane's first sample, sw x sh -> dw x dh, sizes 1 .. 32767, strides in bytes, reserved = 0; cn 1 .. 4 with
 *   8-bit samples, cn 1 .. 2 with 16-bit samples (every channel a channel of its own), mixed freely; 16-bit pointers and strides even.
 *   path 0: the staged kernel where the source box of every tile (256 bytes x 16 rows of destination) fits the staging area (40
 *   rows of 570 bytes: every upscale, downscales to about 2 : 1), the direct kernel otherwise; the exact 2 : 1 LINEAR mean needs no
 *   staging and rides in the staged launch.  path 1: every job through the direct kernel.  Both give the same bytes.
 *   vs_op_resample_jobs_plan (host only, needs no device): staged[i] = 1 where path 0 sends job i into the staged launch.
 * vs_op_resize_yuv - n = 1 .. 32 surfaces of one geometry, any of the eleven YUV surface formats, all planes of all surfaces
 *   through the job launch above (path 0).  Layouts and their rules are those of vs_op_cvt_yuv_to_yuv, per side.  A chroma plane is
 *   a plane of its own, (sw >> sx) x (sh >> sy) -> (dw >> sx) x (dh >> sy) with its own scale, resized about its centre; the
 *   interleaved UV plane of NV12 / P010 goes as cn 2.  sw, sh, dw, dh: multiples of the format's subsampling, 1 .. 32767.
 *   max_value: with LANCZOS4 (1 << bits) - 1 for the low-bit formats (I010, I012, I210, I212, I410, I412), else the type's maximum.
 * vs_op_resize_rgb - VS_FMT_BGR8 / RGB8 / BGRA8 / RGBA8 / GRAY8, n = 1 .. 32: the reference's own case (a BGR cv::Mat).  Alpha and
 *   the fourth channel are channels like the others.
 * d_src and d_dst are HOST arrays of n device pointers, read during the call.
 * Refusals: all decided before any device call, VS_ERR_INVALID_ARG with a text in vs_last_error that names the call, the job or
 * side, and the format: everything vs_op_resize_jobs and vs_op_cvt_yuv_to_yuv refuse about jobs, formats, sizes, layouts, parity
 * and counts (but no ratio is refused), and interp or path outside its enum; max_value below 0 or above the sample type's
 * maximum; cn outside the ranges above; reserved != 0; a destination that overlaps its source (surfaces: d_src[i] == d_dst[j], the
 * part that can be checked).  Valid arguments without a device: VS_ERR_NO_DEVICE.  No byte outside a job's sw x sh samples is
 * read, none outside dw x dh written.  Asynchronous on `stream`.
 * Not built: cubic, nearest, a widened (antialiased) Lanczos or linear kernel - for decimation there is the area-averaging
 * downscale below; packed capture formats; chroma-siting-aware resampling; a stream or stage that emits another size by itself. */
enum vs_interp { VS_INTERP_LINEAR = 0, VS_INTERP_LANCZOS4 = 1 };
int vs_op_resample_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int interp,
                        int max_value, int path, void* stream);
int vs_op_resample_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int interp, int32_t* staged);
int vs_op_resize_yuv(int fmt, const void* const* d_src, const vs_i420_layout* in, int sw, int sh,
                     void* const* d_dst, const vs_i420_layout* out, int dw, int dh,
                     int n, int interp, void* stream);
int vs_op_resize_rgb(int fmt, const void* const* d_src, size_t src_stride, int sw, int sh,
                     void* const* d_dst, size_t dst_stride, int dw, int dh,
                     int n, int interp, void* stream);
/* Host only, needs no device: the table of one axis src -> dst (1 .. 32767 each).  K = 2 (LINEAR) or 8 (LANCZOS4);
 * idx[d * K + k] = the source index of tap k of destination index d, already clamped; coef[d * K + k] = its 11-bit coefficient.
 * axis 0 = columns, 1 = rows (they differ for LINEAR: the edge rule above is the columns').  idx and coef hold dst * K entries. */
int vs_resize_axis_table(int src, int dst, int interp, int axis, int32_t* idx, int16_t* coef);

/* ---- area-averaging downscale: cv::resize(INTER_AREA) for dw <= sw and dh <= sh ----------------------------------------------
 * cv::resize(..., INTER_AREA) is what OpenCV's documentation names for decimation: every source sample of a destination sample's
 * cell enters the result, so 2160p -> 720p, 1080p -> 720p or the (w + 2b) x (h + 2b) surface of a pad or fade stream brought down to
 * a proxy size do not alias the way a point-sampled LINEAR or LANCZOS4 downscale does.  These calls do it on the device for
 * dw <= sw and dh <= sh, on every surface the resize calls above take.  enum vs_interp and the resize calls are unchanged (interp
 * = 2 stays refused there); the feature has entry points of its own.
 *
 * Definition (tests/arearef.py states it in numpy and `math`).  Per axis scale = 1.0 / ((double)dst / src) in IEEE doubles and
 * i = rint(scale); the axis is INTEGER when |scale - i| < DBL_EPSILON (every k d -> d is).  A job has one of three classes:
 * Class 2, the 2 x 2 mean - both axes integer with i = 2: (s00 + s01 + s10 + s11 + 2) >> 2 at both depths and every cn, byte for
 *   byte what VS_INTERP_LINEAR gives for the same job.  It is OpenCV's SIMD path for cn 1, 3 and 4; for cn 2 OpenCV's scalar path
 *   rounds ties to even, and + 2 >> 2 there is this library's choice (docs/opencv_semantics.md).
 * Class 1, integer box - both axes integer otherwise (the same size included: the identity): S = the exact integer sum of the
 *   ix x iy samples, out = rint_half_even((float)S * (1.f / (ix * iy))) - one float32 product, then saturate_cast's rounding.
 *   OpenCV bit for bit on 8-bit planes; on 16-bit planes wherever OpenCV's float running sum is exact (S < 2^24: any area up to 256
 *   at the full 16-bit range).  Beyond that the exact sum is this library's definition.
 * Class 0, general - every other job; a job with one integer and one fractional axis is general on BOTH axes.  Per axis the taps of
 *   destination index d follow computeResizeAreaTab: f1 = d * scale, f2 = f1 + scale, cw = min(scale, src - f1), s1 = ceil(f1),
 *   s2 = min(floor(f2), src - 1), s1 = min(s1, s2); then, in this order,
 *     (s1 - 1, (float)((s1 - f1) / cw))                        if s1 - f1 > 1e-3
 *     (sx, (float)(1.0 / cw))                                  for sx = s1 .. s2 - 1
 *     (s2, (float)(min(min(f2 - s2, 1.0), cw) / cw))           if f2 - s2 > 1e-3
 *   The taps of an index are contiguous, at least one, and all middle weights are equal (tests/test_area_cpu.py checks it over
 *   several hundred pairs), so an axis entry is first, count and three weights: tap 0 takes w_first, tap count - 1 takes w_last
 *   when count > 1, every other tap w_mid - vs_area_axis_table's output and the device's table, four dwords per destination index
 *   whatever the ratio.  Accumulation is in float32, every product and every sum rounded on its own, NOTHING fused:
 *     for each tap row sy, ascending: buf = 0, then buf += (float)S[sx] * alpha over the column taps, ascending;
 *     first tap row of a destination row: sum = beta * buf; later tap rows: sum += beta * buf;
 *     out = clamp(rint_half_even(sum), 0, max_value).
 *   This is OpenCV's order of operations; whether an OpenCV build fuses the vertical multiply-add depends on its SIMD baseline, and
 *   the unfused form is this library's definition (docs/opencv_semantics.md).  The 1e-3 thresholds are OpenCV's: they drop
 *   slivers, and the weights of an index then sum to as little as 0.99902 per axis, so a flat 16-bit area can come out a few codes
 *   low at awkward ratios.  That is INTER_AREA, not a defect to repair here.
 * max_value: every result is clamped to 0 .. max_value, 0 = the sample type's maximum, as in vs_op_resample_jobs.
 * The tables are built on the host in doubles (no FMA contraction), one per (src, dst), and live in the resize's table arena under
 * a key of their own: A CALL THAT MEETS A NEW AXIS MAY BLOCK WHILE ITS TABLE IS UPLOADED; VS_ERR_CAPACITY as above.  Classes 1 and
 * 2 need no table.
 *
 * vs_op_area_jobs - plane jobs as in vs_op_resample_jobs: n = 1 .. 96 jobs of one sample size in ONE launch, whatever their classes;
 *   cn 1 .. 4 with 8-bit samples, 1 .. 2 with 16-bit samples.  One kernel body, hence no path argument.
 *   vs_op_area_jobs_plan (host only, needs no device): cls[i] = the class of job i.
 * vs_op_area_yuv - n = 1 .. 32 surfaces of one geometry, any of the eleven YUV surface formats, layouts and plane rules as in
 *   vs_op_resize_yuv: every chroma plane a plane of its own with its own ratio (and class), the UV plane of NV12 / P010 as cn 2.
 *   max_value is (1 << bits) - 1 for the low-bit formats (I010, I012, I210, I212, I410, I412), else the type's maximum.
 * vs_op_area_rgb - VS_FMT_BGR8 / RGB8 / BGRA8 / RGBA8 / GRAY8, n = 1 .. 32.
 * Refusals: everything the resize calls refuse about jobs, formats, sizes, strides, layouts, parity, overlap, reserved and counts,
 * VS_ERR_INVALID_ARG with a text that names the call, the job or side, and the format, decided before any device call.  One more:
 * dw > sw or dh > sh on a job or surface is VS_ERR_UNSUPPORTED, and the text says so (the same size is accepted).  Valid arguments
 * without a device: VS_ERR_NO_DEVICE.  No byte outside a job's sw x sh samples is read, none outside dw x dh written.
 * Asynchronous on `stream`.
 * Not built: cv::resize's emulation of INTER_AREA for upscales (a variant of bilinear); cubic and nearest; a widened Lanczos;
 * chroma-siting-aware resampling; routing the zoom/crop stage's 640 x 360 output through this kernel; packed capture formats. */
int vs_op_area_jobs(const vs_scale_job* jobs, int n, int sample_bytes, int max_value, void* stream);
int vs_op_area_jobs_plan(const vs_scale_job* jobs, int n, int sample_bytes, int32_t* cls);
int vs_op_area_yuv(int fmt, const void* const* d_src, const vs_i420_layout* in, int sw, int sh,
                   void* const* d_dst, const vs_i420_layout* out, int dw, int dh, int n, void* stream);
int vs_op_area_rgb(int fmt, const void* const* d_src, size_t src_stride, int sw, int sh,
                   void* const* d_dst, size_t dst_stride, int dw, int dh, int n, void* stream);
/* Host only, needs no device: the table of one axis src -> dst, 1 <= dst <= src <= 32767 (dst > src: VS_ERR_UNSUPPORTED).  Each
 * array holds dst entries: the taps of destination index d are the count[d] source samples from first[d] on; tap 0 weighs
 * w_first[d], tap count[d] - 1 (count[d] > 1) w_last[d], every other tap w_mid[d]. */
int vs_area_axis_table(int src, int dst, int32_t* first, int32_t* count,
                       float* w_first, float* w_mid, float* w_last);

/* ---- interlaced sources: deinterlace (linear, yadif) and re-weave (tests/deintref.py states what they compute) ----------------
 * A woven interlaced frame (1080i from an SDI card) cannot be stabilized: the analysis sees combing as texture and the warp
 * rotates the two fields into each other.  These calls turn frames of two fields into progressive frames at single or double rate
 * in HBM, and weave pairs of progressive frames back into interlaced ones.
 *
 * DEFINITION.  The reference project has no deinterlacer, so this is a definition of this library.  It is modelled on the widely
 * used yadif filter and pinned to no other implementation.
 *
 * A plane has h rows of w pixels of cn channels, 8- or 16-bit samples.  Every channel is treated on its own: x +- j below means
 * the same channel of the pixel j pixels away.  Plane row y belongs to field y & 1; this holds for every plane by its own row
 * index, and so for the chroma planes of 4:2:0 as well.  Inputs are three frames P (previous), C (current) and N (next), all
 * read-only, and two job fields:
 *   keep   in {0, 1}: rows with (y & 1) == keep are copied from C.
 *   second in {0, 1}: 0 - this output is the first field in time of frame C and the temporal pair is (A, B) = (P, C);
 *                     1 - the second field, (A, B) = (C, N).
 * A NULL P or N stands for C (the first and the last frame of a stream).
 * For a missing row y: up = y > 0 ? y - 1 : y + 1 and dn = y + 1 < h ? y + 1 : y - 1.  Requires h >= 2.
 *
 * VS_DEINT_LINEAR uses C only and ignores `second`:  out = (C[up][x] + C[dn][x] + 1) >> 1.
 *
 * VS_DEINT_YADIF, in plain integer arithmetic (the largest sum is 3 x 65535: everything fits 32 bits):
 *
 *   c = C[up][x];  e = C[dn][x];  d = (A[y][x] + B[y][x]) >> 1
 *   td0 = |A[y][x] - B[y][x]|
 *   td1 = (|P[up][x] - c| + |P[dn][x] - e|) >> 1
 *   td2 = (|N[up][x] - c| + |N[dn][x] - e|) >> 1
 *   diff = max(td0 >> 1, td1, td2)
 *   sp = (c + e) >> 1
 *   if 3 <= x < w - 3:                           edge-directed search; no pixel of a plane with w < 7 has one
 *       best = |C[up][x-1] - C[dn][x-1]| + |c - e| + |C[up][x+1] - C[dn][x+1]| - 1
 *       score(j) = |C[up][x-1+j] - C[dn][x-1-j]| + |C[up][x+j] - C[dn][x-j]| + |C[up][x+1+j] - C[dn][x+1-j]|
 *       for g in (-1, +1), in this order:
 *           if score(g) < best:  best = score(g); sp = (C[up][x+g] + C[dn][x-g]) >> 1
 *               if score(2g) < best:  best = score(2g); sp = (C[up][x+2g] + C[dn][x-2g]) >> 1      only after g itself won
 *   if not (y == 1 or y + 2 == h):               spatial interlacing check; upp / dnn lie inside the plane exactly then
 *       upp = y + 2 (up - y);  dnn = y + 2 (dn - y)
 *       b = (A[upp][x] + B[upp][x]) >> 1;  f = (A[dnn][x] + B[dnn][x]) >> 1
 *       mx = max(d - e, d - c, min(b - c, f - e));  mn = min(d - e, d - c, max(b - c, f - e))
 *       diff = max(diff, mn, -mx)
 *   out = sp > d + diff ? d + diff : sp < d - diff ? d - diff : sp
 *
 * The result lies between sp and d, so it never leaves the sample range; nothing depends on the bit depth or on where the value
 * sits in the word (P010 and the low-bit formats alike).
 *
 * WEAVE is the inverse step: from two progressive frames F (first in time) and S, destination row y is F's row y where
 * (y & 1) == (tff ? 0 : 1), and S's row y otherwise.  A copy.  Because kept rows are copies,
 * weave(deint first field, deint second field) of one frame gives the frame back.
 *
 * vs_op_deint_jobs - n = 1 .. 96 plane jobs of one sample size (1 or 2 bytes) in ONE launch; cn 1 .. 4 with 8-bit samples, 1 .. 2
 *   with 16-bit samples, mixed freely; w 1 .. 32767, h 2 .. 32767; mode a vs_deint_mode.  prev or next NULL stands for cur (its
 *   stride is then not looked at).
 * vs_op_deint_yuv - n = 1 .. 16 frames of one geometry, any of the eleven YUV surface formats, all planes of all frames and both
 *   fields in one launch; the interleaved UV plane of NV12 / P010 goes as cn 2.  Layouts and plane rules as in vs_op_resize_yuv:
 *   `in` describes d_prev, d_cur and d_next, `out` d_first and d_second.  d_first[i] receives keep = tff ? 0 : 1, second = 0;
 *   d_second[i] the other field with second = 1.  d_second == NULL: single rate, first fields only.  d_prev / d_next may be NULL
 *   as arrays or hold NULL entries.  In a batch of consecutive frames prev[i] = cur[i - 1] and next[i] = cur[i + 1].  w and h are
 *   multiples of the format's subsampling, and every plane has at least 2 rows.
 * vs_op_interlace_yuv - the weave of n = 1 .. 32 pairs of surfaces, one launch.
 * Refusals are decided before any device call and are VS_ERR_INVALID_ARG with a text that names the call, the job or side, and
 * the format: counts, sizes, strides that do not hold a row, 16-bit parity, reserved; keep / second / tff / mode outside their
 * values; h < 2; a destination that overlaps any source of any job of the call, or another destination.  Sources may alias each
 * other freely.  Valid arguments without a device: VS_ERR_NO_DEVICE.  No byte outside w x h of a destination is written, none
 * outside w x h of a source read.  Asynchronous on `stream`.
 * Not built: bwdif and other filters, field-rate motion search, 3:2 pulldown / telecine detection, the packed capture formats as
 * direct inputs (vs_op_cvt_packed_to_yuv stays a call in front), a stream that deinterlaces by itself, the C++ classes. */
typedef enum vs_deint_mode { VS_DEINT_LINEAR = 0, VS_DEINT_YADIF = 1 } vs_deint_mode;
typedef struct vs_deint_job { const void* prev; size_t prev_stride; const void* cur; size_t cur_stride;
                              const void* next; size_t next_stride; void* dst; size_t dst_stride;
                              int32_t w, h, cn, keep, second, reserved; } vs_deint_job;
int vs_op_deint_jobs(const vs_deint_job* jobs, int n, int sample_bytes, int mode, void* stream);
int vs_op_deint_yuv(int fmt, const void* const* d_prev, const void* const* d_cur, const void* const* d_next,
                    const vs_i420_layout* in, int w, int h, void* const* d_first, void* const* d_second,
                    const vs_i420_layout* out, int tff, int mode, int n, void* stream);
int vs_op_interlace_yuv(int fmt, const void* const* d_first, const void* const* d_second, const vs_i420_layout* in,
                        int w, int h, void* const* d_dst, const vs_i420_layout* out, int tff, int n, void* stream);

/* ---- image enhancer: vs::Enhancer (Enhancer.h:10-60, Enhancer.cpp:138-239) ------------ */
/* Enhancer::Parameters defaults, Enhancer.h:12-43 */
void vs_enh_params_default(vs_enh_params_c* p);
/* enhanceImage is a static function without state (Enhancer.cpp:138); the object only owns
 * the device tables, scratch frames and the stream the work is queued on. */
int vs_enh_create(int device, vs_enh** out);
void vs_enh_destroy(vs_enh* e);
const char* vs_enh_last_error(const vs_enh* e);
/* cv::Mat Enhancer::enhanceImage(const cv::Mat& input, const Parameters&), Enhancer.cpp:138-239.
 * BGR8 in, BGR8 out of the same size; synchronous.  Stage order: params->use_cuda = 0 the CPU
 * branch (:142-181: white balance, brightness/contrast, CLAHE, vibrance, unsharp, gamma),
 * 1 the CUDA branch (:183-233: brightness/contrast, unsharp, white balance, vibrance, CLAHE,
 * gamma; fastNlMeansDenoisingColored, :165-169, follows the unsharp mask in both); each stage
 * computes what the CPU OpenCV primitive computes. */
int vs_enh_apply(vs_enh* e, const vs_enh_params_c* params, const uint8_t* data, int w, int h,
                 size_t stride, uint8_t* out, size_t out_stride);
/* Same with frames in HBM (d_out must not alias d_data); left in flight on the object's
 * stream (vs_enh_sync to wait). */
int vs_enh_apply_dev(vs_enh* e, const vs_enh_params_c* params, const void* d_data, int w, int h,
                     size_t stride, void* d_out, size_t out_stride);
/* n frames of one geometry; one launch per pass over all frames when the stage list has no
 * per-frame statistic or multi-pass stage (no white balance / CLAHE / denoise), frame by
 * frame otherwise. */
int vs_enh_apply_batch_dev(vs_enh* e, const vs_enh_params_c* params, const void* const* d_frames,
                           void* const* d_outs, int n, int w, int h, size_t stride,
                           size_t out_stride);
/* The enhancer on one YUV surface in HBM (yuv_fmt, layouts and their rules as for vs_op_cvt_yuv_to_rgb).  The result is BY DEFINITION
 * the composition of three calls: vs_op_cvt_yuv_to_rgb_cs(..., VS_FMT_BGR8) into the object's scratch (rows padded to a multiple of 4
 * bytes), the stages of vs_enh_apply_dev, vs_op_cvt_rgb_to_yuv_cs into d_out - both with the object's colorimetry
 * (vs_enh_set_yuv_colorimetry; none set: the default, BT.601 limited range and top-left chroma).  All three run on the object's stream and are left in
 * flight (vs_enh_sync).  d_out may be d_surface.  The two conversions are lossy - limited range, chroma decimated to one sample per
 * block, the low bits of 16-bit samples dropped - so an enhancer with neutral settings does NOT return the surface bit for bit.
 * Refusals: those of the two operators and of vs_enh_apply_dev, with the text in vs_enh_last_error.  (The batch form, with a fused
 * single pass where the stage list allows one: vs_enh_apply_yuv_batch_dev.) */
int vs_enh_apply_yuv_dev(vs_enh* e, const vs_enh_params_c* params, int yuv_fmt, const void* d_surface,
                         const vs_i420_layout* in, void* d_out, const vs_i420_layout* out, int w, int h);
/* n = 1 .. 32 surfaces of one format, geometry and layout (one `in` for every source, one `out` for every destination): the result
 * of n calls of vs_enh_apply_yuv_dev, byte for byte - that composition of three calls stays the definition.  Where the stage list
 * comes to ONE pass over the frame - table stages (brightness / contrast, gamma), optionally vibrance, or the unsharp mask with
 * tables in front of and behind it; no white balance, CLAHE or denoiser - all n surfaces go through ONE launch that reads the
 * YUV samples, converts them on the way in, runs the pass and converts the results back on the way out: no BGR8 frame in between.
 * Every other stage list runs surface by surface through the three calls.  d_outs[i] may be d_surfaces[i] (in place; the unsharp
 * pass then takes the three calls, since a tile reads its neighbours' samples); ANY OTHER overlap between an output and an input
 * of the same call - two entries that share bytes, an output inside another surface's planes - is the caller's error and gives
 * undefined bytes.  Left in flight on the object's stream (vs_enh_sync).  Refusals: VS_ERR_INVALID_ARG with a text in
 * vs_enh_last_error that names this call and the format, for what vs_op_cvt_yuv_to_rgb refuses about either side (n outside
 * 1 .. 32, a null entry, geometry, pitches, 16-bit alignment, overlapping planes, a format that is no YUV surface format); the
 * code vs_enh_apply_dev gives for a stage list it refuses (blur_sigma, clahe_tile_grid_size).  All of them are decided before any
 * device call: a refused call writes nothing and queues nothing. */
int vs_enh_apply_yuv_batch_dev(vs_enh* e, const vs_enh_params_c* params, int yuv_fmt, const void* const* d_surfaces,
                               const vs_i420_layout* in, void* const* d_outs, const vs_i420_layout* out, int n, int w, int h);
/* how many surfaces of the last vs_enh_apply_yuv_batch_dev call went through the fused launch (0: the three-call path) */
int vs_enh_last_fused(const vs_enh* e);
/* Host only, needs no device: 1 if a vs_enh_apply_yuv_batch_dev call with these parameters would take the fused launch (in_place: some
 * d_outs[i] is d_surfaces[i]), 0 if the three-call path, < 0 a refusal: minus the vs_status the call would return
 * (-VS_ERR_INVALID_ARG: null params, not a YUV surface format, blur_sigma; -VS_ERR_UNSUPPORTED: clahe_tile_grid_size, a blur
 * of more than 33 taps). */
int vs_enh_yuv_plan(const vs_enh_params_c* params, int yuv_fmt, int in_place);
/* The colour space of the object's YUV calls - a setting of the object, NULL = the default (BT.601 limited, top-left chroma).
 * vs_enh_apply_yuv_dev and vs_enh_apply_yuv_batch_dev use it for BOTH of their conversions: the definition of vs_enh_apply_yuv_dev
 * stays the composition of three calls, now vs_op_cvt_yuv_to_rgb_cs and vs_op_cvt_rgb_to_yuv_cs with this descriptor, and the fused
 * launch is taken for exactly the stage lists for which it is taken with the default (vs_enh_yuv_plan does not depend on the
 * descriptor).  Refusals as for vs_op_cvt_yuv_to_rgb_cs: VS_ERR_INVALID_ARG with a text in vs_last_error and vs_enh_last_error that
 * names this call and the field; a refused call leaves the setting as it was.  Needs no device call. */
int vs_enh_set_yuv_colorimetry(vs_enh* e, const vs_cvt_colorimetry* cs);
int vs_enh_sync(vs_enh* e);
/* passes over the frame (kernel launches that read it) the last apply needed */
int vs_enh_last_passes(const vs_enh* e);
/* cv::cvtColor on packed 8-bit 3-channel pixels (Enhancer.cpp:43,56,61,68), on the object's stream */
enum vs_cvt_code { VS_CVT_BGR2HSV = 0, VS_CVT_HSV2BGR = 1, VS_CVT_BGR2LAB = 2, VS_CVT_LAB2BGR = 3 };
int vs_enh_cvt_color(vs_enh* e, int code, const void* d_src, void* d_dst, size_t npix);
/* cv::GaussianBlur(src, dst, Size(0,0), sigma) on BGR8 (Enhancer.cpp:160-161), on the object's stream */
int vs_enh_gaussian_blur(vs_enh* e, const void* d_src, size_t stride, int w, int h, double sigma,
                         void* d_dst, size_t dstride);

/* ------------------------------------------------------------------ config layer (host only, no device)
 * The YAML the reference's example mains read through cv::FileStorage and the key -> parameter mapping each of
 * them repeats (examples/config.yaml:1-159; examples/vs.cpp:50-168; examples/vsg.cpp:1007-1112), plus the
 * st_mtime test of their hot reload (vs.cpp:199-200,381-394).  Scalars and `>>` conversions follow OpenCV's YAML
 * reader (see csrc/config.cpp for the rules restated).  Key paths are section names joined by '.',
 * e.g. "stabilizer.smoothing_radius". */
typedef struct vs_config vs_config;

typedef enum vs_config_kind_e {
    VS_CFG_NONE = 0,      /* absent, or an empty value */
    VS_CFG_INT = 1,
    VS_CFG_REAL = 2,
    VS_CFG_STRING = 3,
    VS_CFG_MAP = 4,
    VS_CFG_SEQ = 5
} vs_config_kind_e;

/* VS_ERR_INVALID_ARG when the file cannot be read or is malformed (vs_last_error names the line). */
int vs_config_open(const char* path, vs_config** out);
int vs_config_parse(const char* text, size_t len, vs_config** out);
void vs_config_close(vs_config* c);
int vs_config_kind(const vs_config* c, const char* key_path);
int vs_config_size(const vs_config* c, const char* key_path);      /* entries of a map / sequence, 1 for a scalar */
/* `node >> value` of cv::FileNode: an absent key gives 0 / 0.0 / "", a value of the wrong kind INT_MAX / DBL_MAX /
 * FLT_MAX / "", a real read as int is rounded half to even. */
int vs_config_get_int(const vs_config* c, const char* key_path, int32_t* v);
int vs_config_get_double(const vs_config* c, const char* key_path, double* v);
int vs_config_get_float(const vs_config* c, const char* key_path, float* v);
int vs_config_get_string(const vs_config* c, const char* key_path, char* buf, size_t cap);
int vs_config_seq_get_double(const vs_config* c, const char* key_path, int index, double* v);
/* The sections of config.yaml into the flat parameter structs (struct_size must be set; start from
 * vs_*_params_default).  An absent section leaves *p alone and reports *present = 0 (the mains test
 * `!node.empty()`).  zero_missing = 1 is the reference to the letter: every key the mains read is assigned, an
 * absent one as 0 / "" (that is what `node["k"] >> field` does); 0 keeps the field's value for absent keys. */
int vs_config_read_stab(const vs_config* c, const char* section, int zero_missing, vs_params_c* p, int* present);
int vs_config_read_roll(const vs_config* c, const char* section, int zero_missing, vs_roll_params_c* p, int* present);
int vs_config_read_enh(const vs_config* c, const char* section, int zero_missing, vs_enh_params_c* p, int* present);
int vs_config_mtime(const char* path, int64_t* mtime);

#ifdef __cplusplus
}
#endif
#endif /* VS_STAB_H */
