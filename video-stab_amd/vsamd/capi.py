"""ctypes binding of the product C-ABI (include/vs_stab.h, libvideo-stab.so).

This is plumbing for tests/bench: every call goes straight into the HIP
library.  There is no Python or CPU fallback - if the library is missing, or
no GPU is usable, calls raise.
"""
import collections
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "csrc", "libvideo-stab.so")

u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)

# The pixel formats, one record each: the columns of the C table (csrc/pixfmt.h), which tests/test_pixfmt_table_cpu.py holds this
# one to.  kind: 0 one plane of interleaved channels, 1 luma + interleaved (U, V) plane (NV12, P010), 2 three planes.  cn: bytes per
# pixel of the first plane; a chroma plane has (w >> sx) x (h >> sy) samples; gray_source: the format the gray kernels are asked for.
#
# A colour format's frames are (h, w, channels) arrays.  The others are (rows, w) arrays, uint8 or uint16: h rows of luma, then
# NV12 / P010: h / 2 rows of interleaved (U, V) pairs (P010: the ten significant bits at the top of each sample);
# three planes: the U plane and the V plane, (h >> sy) rows of (w >> sx) samples each, the value in the low bits (I420: synth.nv12_to_i420;
# I010 / I012: synth.p010_to_i010; 4:2:2 and 4:4:4: synth.yuv_pack, synth.bgr_to_planar).  YV12 and padded chroma rows are layouts
# of a packed frame (set_i420_layout, in bytes).
PixFmt = collections.namedtuple("PixFmt", "fmt name text kind cn sample_bytes bits sx sy gray_source border_modes")
KIND_INTERLEAVED, KIND_LUMA_UV, KIND_THREE_PLANES = range(3)
PIXFMTS = (
    PixFmt(0, "BGR8", "BGR8", KIND_INTERLEAVED, 3, 1, 8, 0, 0, 0, True),
    PixFmt(1, "NV12", "NV12", KIND_LUMA_UV, 1, 1, 8, 1, 1, 2, False),
    PixFmt(2, "GRAY8", "GRAY8", KIND_INTERLEAVED, 1, 1, 8, 0, 0, 2, False),
    PixFmt(3, "BGRA8", "BGRA8", KIND_INTERLEAVED, 4, 1, 8, 0, 0, 3, True),
    PixFmt(4, "RGBA8", "RGBA8", KIND_INTERLEAVED, 4, 1, 8, 0, 0, 4, True),
    PixFmt(5, "RGB8", "RGB8", KIND_INTERLEAVED, 3, 1, 8, 0, 0, 5, True),
    PixFmt(6, "P010", "P010", KIND_LUMA_UV, 2, 2, 10, 1, 1, 6, False),
    PixFmt(7, "I420", "I420", KIND_THREE_PLANES, 1, 1, 8, 1, 1, 2, False),
    PixFmt(8, "I010", "I010 / I012", KIND_THREE_PLANES, 2, 2, 10, 1, 1, 8, False),       # yuv420p10le
    PixFmt(9, "I012", "I010 / I012", KIND_THREE_PLANES, 2, 2, 12, 1, 1, 9, False),       # yuv420p12le
    PixFmt(10, "I422", "I422", KIND_THREE_PLANES, 1, 1, 8, 1, 0, 2, False),              # yuv422p
    PixFmt(11, "I444", "I444", KIND_THREE_PLANES, 1, 1, 8, 0, 0, 2, False),              # yuv444p
    PixFmt(12, "I210", "I210", KIND_THREE_PLANES, 2, 2, 10, 1, 0, 12, False),            # yuv422p10le
    PixFmt(13, "I212", "I212", KIND_THREE_PLANES, 2, 2, 12, 1, 0, 13, False),            # yuv422p12le
    PixFmt(14, "I410", "I410", KIND_THREE_PLANES, 2, 2, 10, 0, 0, 14, False),            # yuv444p10le
    PixFmt(15, "I412", "I412", KIND_THREE_PLANES, 2, 2, 12, 0, 0, 15, False),            # yuv444p12le
)
PIXFMT = {f.fmt: f for f in PIXFMTS}
PIXFMT_BY_NAME = {f.name: f for f in PIXFMTS}
globals().update({"FMT_" + f.name: f.fmt for f in PIXFMTS})        # FMT_BGR8 ... FMT_I412

# the names the tests and synth.py use, read from the table
FMT_CHANNELS = {f.fmt: f.cn for f in PIXFMTS if f.sample_bytes == 1 and f.kind != KIND_THREE_PLANES}   # 8-bit: bytes per pixel of the first plane
FMT_SAMPLE_BYTES = {f.fmt: f.sample_bytes for f in PIXFMTS if f.kind == KIND_LUMA_UV and f.sample_bytes == 2}      # P010
FMT_CHROMA_SHIFTS = {f.fmt: (f.sx, f.sy) for f in PIXFMTS if f.kind == KIND_THREE_PLANES}
FMT_PLANAR_BITS = {f.fmt: f.bits for f in PIXFMTS if f.kind == KIND_THREE_PLANES}


def fmt_px_bytes(fmt):
    """Bytes per pixel of a format's (first) plane."""
    return PIXFMT[fmt].cn


def fmt_dtype(fmt):
    return np.uint16 if PIXFMT[fmt].sample_bytes == 2 else np.uint8


def fmt_two_planes(fmt):
    return PIXFMT[fmt].kind == KIND_LUMA_UV


def fmt_420(fmt):
    """A frame array of this format has h * 3 / 2 rows: h of luma, h / 2 of subsampled chroma."""
    f = PIXFMT[fmt]
    return f.kind != KIND_INTERLEAVED and f.sy == 1


def fmt_frame_rows(fmt, h):
    """Rows of a packed frame array of h picture rows (its columns: w)."""
    f = PIXFMT[fmt]
    if f.kind == KIND_THREE_PLANES and not f.sy:
        return h + (2 * h >> f.sx)
    return h * 3 // 2 if fmt_420(fmt) else h


def fmt_picture_rows(fmt, rows):
    """The picture's rows of a packed frame array with `rows` rows: the inverse of fmt_frame_rows."""
    f = PIXFMT[fmt]
    if f.kind == KIND_THREE_PLANES and not f.sy:
        return rows // (1 + (2 >> f.sx))
    return rows * 2 // 3 if fmt_420(fmt) else rows


BORDER_BLACK, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_WRAP, BORDER_FADE = range(6)
SMOOTH_BOX, SMOOTH_GAUSSIAN, SMOOTH_KALMAN = range(3)
STAGE_WARP, STAGE_WARP_TABLES, STAGE_COUNT = 7, 8, 9      # vs_stab.h VS_STAGE_*


class VsParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("logging", C.c_int32), ("smoothing_radius", C.c_int32),
        ("max_corners", C.c_int32), ("quality_level", C.c_double), ("min_distance", C.c_double),
        ("block_size", C.c_int32), ("border_type", C.c_int32), ("border_size", C.c_int32),
        ("crop_n_zoom", C.c_int32), ("smoothing_method", C.c_int32), ("horizon_lock", C.c_int32),
        ("gaussian_sigma", C.c_double), ("adaptive_smoothing", C.c_int32),
        ("min_smoothing_radius", C.c_int32), ("max_smoothing_radius", C.c_int32),
        ("fade_alpha", C.c_float), ("fade_duration", C.c_int32), ("enable_virtual_canvas", C.c_int32),
        ("drone_high_freq_mode", C.c_int32), ("hf_shake_px", C.c_float),
        ("hf_analysis_max_width", C.c_int32), ("hf_rot_lp_alpha", C.c_float),
        ("enable_conditional_clahe", C.c_int32), ("hf_dead_zone_threshold", C.c_float),
        ("hf_freeze_duration", C.c_int32), ("hf_motion_accumulator_decay", C.c_float),
        ("lk_win_size", C.c_int32), ("lk_max_level", C.c_int32), ("lk_max_iters", C.c_int32),
        ("lk_epsilon", C.c_double), ("ransac_max_iters", C.c_int32), ("ransac_threshold", C.c_double),
        ("canvas_scale_factor", C.c_float), ("temporal_buffer_size", C.c_int32), ("canvas_blend_weight", C.c_float),
        ("adaptive_canvas_size", C.c_int32), ("max_canvas_scale", C.c_float), ("min_canvas_scale", C.c_float),
        ("edge_blend_radius", C.c_int32), ("reserved", C.c_int32 * 1),
    ]


class VsCounters(C.Structure):
    _fields_ = [
        ("frames_in", C.c_uint64), ("frames_out", C.c_uint64), ("detections", C.c_uint64),
        ("last_features", C.c_int32), ("last_tracked", C.c_int32), ("last_inliers", C.c_int32),
        ("last_candidates", C.c_int32), ("gftt_overflow", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class VsDebugFrame(C.Structure):
    _fields_ = [
        ("n_prev", C.c_int32), ("n_valid", C.c_int32), ("ransac_best_iter", C.c_int32),
        ("ransac_iters_run", C.c_int32), ("n_inliers", C.c_int32), ("detected", C.c_int32),
        ("n_detected", C.c_int32), ("box_radius", C.c_int32), ("intent", C.c_int32),
        ("out_index", C.c_int32), ("transform", C.c_float * 3), ("smoothed", C.c_float * 3),
        ("warp_matrix", C.c_float * 6), ("model", C.c_double * 6),
    ]


class VsTrajRelease(C.Structure):
    """vs_traj_release (include/vs_stab.h)"""
    _fields_ = [("push", C.c_int32), ("idx", C.c_int32), ("n_seen", C.c_int32), ("has_M", C.c_int32),
                ("M", C.c_float * 12), ("Minv", C.c_double * 12)]


class VsRollParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("canny_aperture", C.c_int32), ("scale_factor", C.c_double),
        ("canny_threshold_low", C.c_double), ("canny_threshold_high", C.c_double),
        ("hough_rho", C.c_float), ("hough_theta", C.c_float), ("hough_threshold", C.c_int32),
        ("reserved0", C.c_int32), ("angle_filter_min", C.c_double), ("angle_filter_max", C.c_double),
        ("angle_smoothing_alpha", C.c_double), ("angle_decay", C.c_double), ("max_angle_change_deg", C.c_double),
    ]


class VsEnhParams(C.Structure):
    """vs_enh_params_c (include/vs_stab.h): flat mirror of vs::Enhancer::Parameters."""
    _fields_ = [
        ("struct_size", C.c_int32), ("brightness", C.c_float), ("contrast", C.c_float),
        ("enable_white_balance", C.c_int32), ("wb_strength", C.c_float),
        ("enable_vibrance", C.c_int32), ("vibrance_strength", C.c_float),
        ("enable_unsharp", C.c_int32), ("sharpness", C.c_float), ("blur_sigma", C.c_float),
        ("enable_clahe", C.c_int32), ("clahe_clip_limit", C.c_float), ("clahe_tile_grid_size", C.c_int32),
        ("enable_denoise", C.c_int32), ("denoise_strength", C.c_float), ("gamma", C.c_float),
        ("use_cuda", C.c_int32), ("reserved0", C.c_int32),
    ]


class VsYuvFill(C.Structure):
    """struct vs_yuv_fill (include/vs_stab.h): the fill colour of border pad on YUV streams, samples as they lie in memory."""
    _fields_ = [("y", C.c_uint16), ("u", C.c_uint16), ("v", C.c_uint16), ("reserved", C.c_uint16)]


class VsPadJob(C.Structure):
    """struct vs_pad_job (include/vs_stab.h): one plane pad of vs_op_pad_jobs."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_size_t), ("sw", C.c_int32), ("sh", C.c_int32),
                ("dst", C.c_void_p), ("dst_stride", C.c_size_t), ("bx", C.c_int32), ("by", C.c_int32),
                ("cn", C.c_int32), ("border", C.c_int32), ("fill", C.c_uint16 * 2), ("reserved", C.c_int32)]


class VsFadeJob(C.Structure):
    """struct vs_fade_job (include/vs_stab.h): one plane of vs_op_fade_blend_jobs."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_size_t), ("sw", C.c_int32), ("sh", C.c_int32),
                ("hist", C.c_void_p), ("hist_stride", C.c_size_t),
                ("dst", C.c_void_p), ("dst_stride", C.c_size_t), ("bx", C.c_int32), ("by", C.c_int32),
                ("fill", C.c_uint16 * 2), ("cn", C.c_int32), ("reserved", C.c_int64)]


class VsFadeUpdateJob(C.Structure):
    """struct vs_fade_update_job (include/vs_stab.h): one plane of vs_op_fade_update_jobs."""
    _fields_ = [("hist", C.c_void_p), ("hist_stride", C.c_size_t), ("res", C.c_void_p), ("res_stride", C.c_size_t),
                ("w", C.c_int32), ("h", C.c_int32), ("cn", C.c_int32), ("reserved", C.c_int32)]


INTERP_LINEAR, INTERP_LANCZOS4 = 0, 1          # enum vs_interp


class VsScaleJob(C.Structure):
    """struct vs_scale_job (include/vs_stab.h): one crop-and-scale of vs_op_scale_jobs."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_size_t), ("sw", C.c_int32), ("sh", C.c_int32),
                ("dst", C.c_void_p), ("dst_stride", C.c_size_t), ("dw", C.c_int32), ("dh", C.c_int32),
                ("cn", C.c_int32), ("reserved", C.c_int32)]


DEINT_LINEAR, DEINT_YADIF = 0, 1               # enum vs_deint_mode


class VsDeintJob(C.Structure):
    """struct vs_deint_job (include/vs_stab.h): one plane of vs_op_deint_jobs."""
    _fields_ = [("prev", C.c_void_p), ("prev_stride", C.c_size_t), ("cur", C.c_void_p), ("cur_stride", C.c_size_t),
                ("next", C.c_void_p), ("next_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_stride", C.c_size_t),
                ("w", C.c_int32), ("h", C.c_int32), ("cn", C.c_int32), ("keep", C.c_int32), ("second", C.c_int32), ("reserved", C.c_int32)]


class VsError(RuntimeError):
    pass


def _p(a, t):
    return a.ctypes.data_as(t)


class DevBuf:
    """A device allocation owned through vs_dev_malloc/vs_dev_free."""

    def __init__(self, vs, nbytes):
        self.vs = vs
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        vs.check(vs.lib.vs_dev_malloc(C.byref(p), max(self.nbytes, 16)))
        self.ptr = p.value

    @classmethod
    def from_array(cls, vs, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(vs, arr.nbytes)
        b.upload(arr)
        return b

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= max(self.nbytes, 16)
        self.vs.check(self.vs.lib.vs_dev_memcpy_h2d(C.c_void_p(self.ptr + offset), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, shape, dtype, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= max(self.nbytes, 16)
        self.vs.check(self.vs.lib.vs_dev_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + offset), out.nbytes))
        return out

    def zero(self):
        self.vs.check(self.vs.lib.vs_dev_memset(C.c_void_p(self.ptr), 0, max(self.nbytes, 16)))

    def free(self):
        if self.ptr:
            self.vs.lib.vs_dev_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CanvasOp:
    """vs_op_canvas_*: the stream's virtual canvas driven with a given correction."""

    def __init__(self, vs):
        self.vs = vs
        h = C.c_void_p()
        vs.check(vs.lib.vs_op_canvas_create(C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.vs.lib.vs_op_canvas_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, params, frame, t, transforms=None, pitch=None):
        """frame (h, w, 3) uint8 -> (output (h, w, 3), info8).  pitch: a row pitch of its own for the device frame."""
        frame = np.ascontiguousarray(frame, np.uint8)
        h, w = frame.shape[:2]
        pitch = pitch or w * 3
        rows = np.full((h, pitch), 0xA5, np.uint8)
        rows[:, :w * 3] = frame.reshape(h, w * 3)
        t = np.ascontiguousarray(t, np.float32).reshape(3)
        tr = np.ascontiguousarray(transforms if transforms is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3)
        d_in = DevBuf.from_array(self.vs, rows)
        d_out = DevBuf(self.vs, w * h * 3)
        info = np.zeros(8, np.int32)
        self.vs.check(self.vs.lib.vs_op_canvas_apply(self.h, C.byref(params), d_in.ptr, pitch, w, h, _p(t, f32p),
                                                     _p(tr, f32p) if len(tr) else None, len(tr), d_out.ptr, w * 3, _p(info, i32p)))
        return d_out.download((h, w, 3), np.uint8), info


class HostBuf:
    """Page-locked host memory (vs_host_alloc) as a numpy array: frames that the host entry points move by DMA."""

    def __init__(self, vs, shape, dtype=np.uint8):
        self.vs = vs
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        vs.check(vs.lib.vs_host_alloc(C.byref(p), max(n, 1)))
        self.ptr = p.value
        self.array = np.frombuffer((C.c_uint8 * max(n, 1)).from_address(self.ptr), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            self.vs.lib.vs_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class VsLib:
    def __init__(self, lib):
        self.lib = lib
        L = lib
        vp = C.c_void_p
        L.vs_abi_version.restype = C.c_int
        try:
            L.vs_build_tag.restype = C.c_char_p
        except AttributeError:      # a library of an earlier build (A/B measurements)
            pass
        L.vs_build_info.restype = C.c_char_p
        L.vs_device_count.restype = C.c_int
        L.vs_params_default.argtypes = [C.POINTER(VsParams)]
        L.vs_status_string.restype = C.c_char_p
        L.vs_status_string.argtypes = [C.c_int]
        L.vs_last_error.restype = C.c_char_p
        L.vs_stab_create.argtypes = [C.POINTER(VsParams), C.c_int, C.POINTER(vp)]
        L.vs_stab_destroy.argtypes = [vp]
        L.vs_stab_clean.argtypes = [vp]
        L.vs_stab_push.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_int, u8p, C.c_size_t, i32p]
        L.vs_stab_flush.argtypes = [vp, u8p, C.c_size_t, i32p]
        L.vs_stab_push_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_size_t, i32p]
        L.vs_stab_flush_dev.argtypes = [vp, vp, C.c_size_t, i32p]
        L.vs_stab_sync.argtypes = [vp]
        L.vs_stab_out_size.argtypes = [vp, C.c_int, C.c_int, i32p, i32p]
        L.vs_stab_last_out_dims.argtypes = [vp, i32p, i32p]
        L.vs_stab_get_counters.argtypes = [vp, C.POINTER(VsCounters)]
        L.vs_stab_get_debug.argtypes = [vp, C.POINTER(VsDebugFrame)]
        L.vs_stab_canvas_info.argtypes = [vp, i32p]
        L.vs_stab_get_debug_arrays.argtypes = [vp, f32p, f32p, u8p, u8p, f32p, u8p, i32p, i32p]
        L.vs_stab_last_error.restype = C.c_char_p
        L.vs_stab_last_error.argtypes = [vp]
        L.vs_stab_stream.restype = vp
        L.vs_stab_stream.argtypes = [vp]
        L.vs_stab_set_warp_batch.argtypes = [vp, C.c_int]
        L.vs_stab_set_batch.argtypes = [vp, C.c_int]
        L.vs_stab_set_zero_copy.argtypes = [vp, C.c_int]
        L.vs_stab_set_nv12_layout.argtypes = [vp, C.c_size_t, C.c_size_t]
        L.vs_stab_set_i420_layout.argtypes = [vp] + [C.c_size_t] * 6
        L.vs_stab_set_profiling.argtypes = [vp, C.c_int]
        L.vs_stab_get_stage_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        try:
            L.vs_batch_create.argtypes = [C.c_int, C.c_int, C.POINTER(VsParams), C.c_int, C.POINTER(vp)]
            L.vs_batch_create_params.argtypes = [C.c_int, C.c_int, C.POINTER(VsParams), C.c_int, C.POINTER(vp)]
            L.vs_batch_destroy.argtypes = [vp]
            L.vs_batch_destroy.restype = None
            L.vs_batch_streams.argtypes = [vp]
            L.vs_batch_stream.argtypes = [vp, C.c_int]
            L.vs_batch_stream.restype = vp
            L.vs_batch_set_zero_copy.argtypes = [vp, C.c_int]
            L.vs_batch_set_nv12_layout.argtypes = [vp, C.c_size_t, C.c_size_t]
            L.vs_batch_set_i420_layout.argtypes = [vp] + [C.c_size_t] * 6
            L.vs_batch_push_dev.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(vp), C.c_size_t, i32p]
            L.vs_batch_flush_dev.argtypes = [vp, C.POINTER(vp), C.c_size_t, i32p]
            L.vs_batch_sync.argtypes = [vp]
            L.vs_batch_last_error.argtypes = [vp]
            L.vs_batch_last_error.restype = C.c_char_p
        except AttributeError:      # a library of an earlier build (A/B measurements)
            pass
        L.vs_dev_set_device.argtypes = [C.c_int]
        L.vs_dev_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
        try:
            L.vs_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
            L.vs_host_free.argtypes = [vp]
            L.vs_host_free.restype = None
            L.vs_stab_set_host_pipeline.argtypes = [vp, C.c_int]
        except AttributeError:      # a library of an earlier build (A/B measurements)
            pass
        L.vs_dev_free.argtypes = [vp]
        L.vs_dev_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
        L.vs_dev_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
        L.vs_dev_memset.argtypes = [vp, C.c_int, C.c_size_t]
        L.vs_dev_memcpy_d2d.argtypes = [vp, vp, C.c_size_t]
        L.vs_dev_copy_rate.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_double)]
        L.vs_op_libm_checksum.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.vs_op_trajectory.argtypes = [C.POINTER(VsParams), C.c_int, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_int32)),
                                       C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.POINTER(VsDebugFrame)),
                                       C.POINTER(C.c_int32), C.POINTER(C.POINTER(VsTrajRelease)), C.POINTER(C.c_int32)]
        L.vs_op_warp_affine.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                        C.c_int, f32p, C.c_int, vp]
        L.vs_op_warp_affine_p010.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, C.c_size_t, vp]
        L.vs_op_warp_affine_nv12.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, f32p, C.c_int,
                                             C.c_size_t, C.c_size_t, vp]
        L.vs_op_warp_affine_i420.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                             C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.vs_op_warp_affine_i010.argtypes = L.vs_op_warp_affine_i420.argtypes
        L.vs_op_warp_affine_planar.argtypes = [C.c_int] + list(L.vs_op_warp_affine_i420.argtypes)
        L.vs_op_resize_gray.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, vp]
        L.vs_op_pyr_down.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, vp]
        L.vs_op_scharr.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, vp]
        L.vs_op_pyr_level.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.vs_op_pyr_lk.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp,
                                   C.c_int, C.c_int, C.c_int, C.c_double, vp]
        L.vs_op_gftt.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                 vp, vp, vp, vp]
        L.vs_op_estimate_affine_partial2d.argtypes = [vp, vp, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp]
        L.vs_roll_params_default.argtypes = [C.POINTER(VsRollParams)]
        L.vs_roll_params_default.restype = None
        L.vs_roll_create.argtypes = [C.POINTER(VsRollParams), C.c_int, C.POINTER(vp)]
        L.vs_roll_destroy.argtypes = [vp]
        L.vs_roll_destroy.restype = None
        L.vs_roll_last_error.argtypes = [vp]
        L.vs_roll_last_error.restype = C.c_char_p
        L.vs_roll_correct.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, u8p, C.c_size_t]
        L.vs_roll_correct_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]
        L.vs_roll_correct_nv12_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t]
        L.vs_roll_correct_nv12_dev_n.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
        L.vs_azc_apply_nv12_dev_n.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.POINTER(C.c_int64)]
        L.vs_stab_push_dev_n.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(vp), C.c_size_t, i32p]
        L.vs_azc_apply_nv12_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64)]
        L.vs_azc_result.argtypes = [vp, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), i32p]
        L.vs_roll_sync.argtypes = [vp]
        L.vs_roll_get_state.argtypes = [vp, f64p, f64p, i32p, i32p]
        L.vs_op_canny.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, vp, C.c_size_t, vp]
        L.vs_op_hough_lines.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp,
                                        C.c_int, vp, vp]
        L.vs_azc_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.vs_azc_destroy.argtypes = [vp]
        L.vs_azc_destroy.restype = None
        L.vs_azc_last_error.argtypes = [vp]
        L.vs_azc_last_error.restype = C.c_char_p
        L.vs_azc_apply.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_int, u8p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]
        L.vs_azc_apply_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_size_t,
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.vs_azc_sync.argtypes = [vp]
        L.vs_azc_worker_times.argtypes = [vp, C.POINTER(C.c_double)]
        L.vs_azc_get_info.argtypes = [vp, i32p]
        L.vs_op_content_mask.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]
        L.vs_azc_crop_from_mask.argtypes = [u8p, C.c_int, C.c_int, C.c_size_t, i32p, u8p]
        L.vs_op_external_boxes.argtypes = [u8p, C.c_int, C.c_int, C.c_size_t, i32p, C.c_int, i32p]
        cp = C.c_char_p
        L.vs_config_open.argtypes = [cp, C.POINTER(vp)]
        L.vs_config_parse.argtypes = [cp, C.c_size_t, C.POINTER(vp)]
        L.vs_config_close.argtypes = [vp]
        L.vs_config_close.restype = None
        L.vs_config_kind.argtypes = [vp, cp]
        L.vs_config_size.argtypes = [vp, cp]
        L.vs_config_get_int.argtypes = [vp, cp, i32p]
        L.vs_config_get_double.argtypes = [vp, cp, f64p]
        L.vs_config_get_float.argtypes = [vp, cp, C.POINTER(C.c_float)]
        L.vs_config_get_string.argtypes = [vp, cp, C.c_char_p, C.c_size_t]
        L.vs_config_seq_get_double.argtypes = [vp, cp, C.c_int, f64p]
        L.vs_config_read_stab.argtypes = [vp, cp, C.c_int, C.POINTER(VsParams), i32p]
        L.vs_config_read_roll.argtypes = [vp, cp, C.c_int, C.POINTER(VsRollParams), i32p]
        L.vs_config_read_enh.argtypes = [vp, cp, C.c_int, C.POINTER(VsEnhParams), i32p]
        L.vs_config_mtime.argtypes = [cp, C.POINTER(C.c_int64)]
        ep = C.POINTER(VsEnhParams)
        L.vs_enh_params_default.argtypes = [ep]
        L.vs_enh_params_default.restype = None
        L.vs_enh_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.vs_enh_destroy.argtypes = [vp]
        L.vs_enh_destroy.restype = None
        L.vs_enh_last_error.argtypes = [vp]
        L.vs_enh_last_error.restype = C.c_char_p
        L.vs_enh_apply.argtypes = [vp, ep, u8p, C.c_int, C.c_int, C.c_size_t, u8p, C.c_size_t]
        L.vs_enh_apply_dev.argtypes = [vp, ep, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]
        L.vs_enh_apply_batch_dev.argtypes = [vp, ep, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int,
                                             C.c_size_t, C.c_size_t]
        L.vs_enh_sync.argtypes = [vp]
        L.vs_enh_last_passes.argtypes = [vp]
        L.vs_enh_cvt_color.argtypes = [vp, C.c_int, vp, vp, C.c_size_t]
        L.vs_enh_gaussian_blur.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_double, vp, C.c_size_t]
        L.vs_op_warp_affine_ex.argtypes =[vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.c_int,
                                           C.c_int, f64p, C.c_int, vp]
        L.vs_op_warp_affine16_ex.argtypes = L.vs_op_warp_affine_ex.argtypes
        L.vs_roll_correct_p010_dev.argtypes = L.vs_roll_correct_nv12_dev.argtypes
        L.vs_roll_correct_p010_dev_n.argtypes = L.vs_roll_correct_nv12_dev_n.argtypes
        L.vs_azc_apply_p010_dev.argtypes = L.vs_azc_apply_nv12_dev.argtypes
        L.vs_azc_apply_p010_dev_n.argtypes = L.vs_azc_apply_nv12_dev_n.argtypes
        lp = C.POINTER(I420LayoutC)
        L.vs_roll_correct_i420_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, lp, vp, lp]
        L.vs_roll_correct_i420_dev_n.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, lp, lp]
        L.vs_azc_apply_i420_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, lp, vp, lp, C.POINTER(C.c_int64)]
        L.vs_azc_apply_i420_dev_n.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, lp, lp, C.POINTER(C.c_int64)]
        L.vs_azc_set_output_size.argtypes = [vp, C.c_int, C.c_int]
        L.vs_azc_get_output_size.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.vs_op_scale_jobs.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, C.c_int, vp]
        L.vs_op_scale_jobs_plan.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, i32p]
        L.vs_op_copy_make_border.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, vp]
        L.vs_op_fade_blend.argtypes = [vp, vp, C.c_size_t, C.c_float, C.c_float, vp]
        L.vs_op_fade_update.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp]
        L.vs_op_canvas_create.argtypes = [C.POINTER(vp)]
        L.vs_op_canvas_apply.argtypes = [vp, C.POINTER(VsParams), vp, C.c_size_t, C.c_int, C.c_int, f32p, f32p, C.c_int, vp, C.c_size_t, i32p]
        L.vs_op_canvas_info.argtypes = [vp, i32p]
        L.vs_op_canvas_destroy.argtypes = [vp]
        L.vs_op_canvas_destroy.restype = None
        try:
            L.vs_op_cvt_yuv_to_rgb.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_cvt_rgb_to_yuv.argtypes = [C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int, vp]
            L.vs_enh_apply_yuv_dev.argtypes = [vp, ep, C.c_int, vp, lp, vp, lp, C.c_int, C.c_int]
            L.vs_enh_apply_yuv_batch_dev.argtypes = [vp, ep, C.c_int, C.POINTER(vp), lp, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int]
            L.vs_enh_last_fused.argtypes = [vp]
            L.vs_enh_yuv_plan.argtypes = [ep, C.c_int, C.c_int]
            csp = C.POINTER(CvtColorimetry)
            L.vs_op_cvt_yuv_to_rgb_cs.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.c_int, csp, vp]
            L.vs_op_cvt_rgb_to_yuv_cs.argtypes = [C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int, csp, vp]
            L.vs_enh_set_yuv_colorimetry.argtypes = [vp, csp]
            L.vs_cvt_coefficients.argtypes = [csp, i32p]
            L.vs_cvt_colorimetry_guess.argtypes = [C.c_int, C.c_int, csp]
            L.vs_cvt_colorimetry_guess.restype = None
            L.vs_op_cvt_yuv_to_yuv.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(VsYuvCvtDesc), vp]
            L.vs_yuv_surface_layout.argtypes = [C.c_int, C.c_int, C.c_int, lp, lp, C.POINTER(C.c_size_t)]
            # packed 4:2:2 capture formats
            L.vs_op_cvt_packed_to_yuv.argtypes = [C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(VsYuvCvtDesc), vp]
            L.vs_op_cvt_yuv_to_packed.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(VsYuvCvtDesc), vp]
            L.vs_packed_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t] + [C.POINTER(C.c_size_t)] * 3
            # crop-and-zoom on YUV streams
            L.vs_stab_set_yuv_crop_zoom.argtypes = [vp, C.c_int]
            L.vs_batch_set_yuv_crop_zoom.argtypes = [vp, C.c_int]
            L.vs_op_resize_jobs.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, vp]
            # border pad on YUV streams
            L.vs_stab_set_yuv_border_pad.argtypes = [vp, C.c_int, C.POINTER(VsYuvFill)]
            L.vs_batch_set_yuv_border_pad.argtypes = [vp, C.c_int, C.POINTER(VsYuvFill)]
            L.vs_yuv_video_black.argtypes = [C.c_int, C.POINTER(VsYuvFill)]
            L.vs_op_pad_jobs.argtypes = [C.POINTER(VsPadJob), C.c_int, C.c_int, vp]
            # the fade border on YUV streams
            L.vs_stab_set_yuv_fade.argtypes = [vp, C.c_int, C.POINTER(VsYuvFill)]
            L.vs_op_fade_blend_jobs.argtypes = [C.POINTER(VsFadeJob), C.c_int, C.c_int, C.c_float, C.c_float, vp]
            L.vs_op_fade_update_jobs.argtypes = [C.POINTER(VsFadeUpdateJob), C.c_int, C.c_int, vp]
            # roll correction and auto zoom/crop on interleaved colour frames (BGR8, RGB8, BGRA8, RGBA8)
            L.vs_roll_correct_rgb_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t]
            L.vs_roll_correct_rgb_dev_n.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t]
            L.vs_azc_apply_rgb_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int64)]
            L.vs_azc_apply_rgb_dev_n.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                                 C.POINTER(C.c_int64)]
            L.vs_op_scale_jobs_rgb.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, vp]
            L.vs_op_scale_jobs_rgb_plan.argtypes = [C.POINTER(VsScaleJob), C.c_int, i32p]
            # resize to an output size
            L.vs_op_resample_jobs.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_resample_jobs_plan.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, C.c_int, i32p]
            L.vs_op_resize_yuv.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_resize_rgb.argtypes = [C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int,
                                           C.c_int, C.c_int, vp]
            L.vs_resize_axis_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.POINTER(C.c_int16)]
            # area-averaging downscale
            L.vs_op_area_jobs.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_area_jobs_plan.argtypes = [C.POINTER(VsScaleJob), C.c_int, C.c_int, i32p]
            L.vs_op_area_yuv.argtypes = [C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_area_rgb.argtypes = [C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.POINTER(vp), C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
            L.vs_area_axis_table.argtypes = [C.c_int, C.c_int, i32p, i32p, f32p, f32p, f32p]
            # interlaced sources
            L.vs_op_deint_jobs.argtypes = [C.POINTER(VsDeintJob), C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_deint_yuv.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), lp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), lp,
                                          C.c_int, C.c_int, C.c_int, vp]
            L.vs_op_interlace_yuv.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), lp, C.c_int, C.c_int, C.POINTER(vp), lp, C.c_int, C.c_int, vp]
            # edge fill on YUV streams
            L.vs_stab_set_yuv_edge_fill.argtypes = [vp, C.c_int, C.POINTER(VsYuvFill)]
            L.vs_batch_set_yuv_edge_fill.argtypes = [vp, C.c_int, C.POINTER(VsYuvFill)]
            L.vs_op_warp_affine_yuv_fill.argtypes = [C.c_int] + list(L.vs_op_warp_affine_i420.argtypes[:-2]) + [C.POINTER(VsYuvFill), vp]
        except AttributeError:      # a library of an earlier build (A/B measurements)
            pass

    # ---- helpers ----------------------------------------------------------
    def check(self, status, inst=None):
        if status != 0:
            msg = self.lib.vs_status_string(status).decode()
            detail = (self.lib.vs_stab_last_error(inst) if inst else self.lib.vs_last_error()) or b""
            raise VsError("%s: %s" % (msg, detail.decode()))

    def params(self, **kw):
        p = VsParams()
        self.lib.vs_params_default(C.byref(p))
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, v)
        return p

    def sync(self):
        self.check(self.lib.vs_dev_sync())

    # ---- stage operators, numpy in / numpy out (device round trip) ----------
    def trajectory(self, params, streams, steps=None):
        """vs_op_trajectory.  streams: [(models (n, 6) float64, kinds (n,) int32: 1 model, 0 failed, -1 nothing to track)];
        steps None: per-frame form (one stream), else the batch form with these step sizes in turn.
        -> per stream (records [VsDebugFrame], releases [VsTrajRelease])."""
        n = len(streams)
        mods = [np.ascontiguousarray(m, np.float64).reshape(-1, 6) for m, _ in streams]
        kinds = [np.ascontiguousarray(k, np.int32) for _, k in streams]
        npush = (C.c_int32 * n)(*[len(k) for k in kinds])
        dbg = [(VsDebugFrame * (2 * len(k) + 2))() for k in kinds]
        rel = [(VsTrajRelease * (len(k) + 1))() for k in kinds]
        n_dbg, n_rel = (C.c_int32 * n)(), (C.c_int32 * n)()
        mp = (C.POINTER(C.c_double) * n)(*[m.ctypes.data_as(C.POINTER(C.c_double)) for m in mods])
        kp = (C.POINTER(C.c_int32) * n)(*[k.ctypes.data_as(C.POINTER(C.c_int32)) for k in kinds])
        dp = (C.POINTER(VsDebugFrame) * n)(*[C.cast(d, C.POINTER(VsDebugFrame)) for d in dbg])
        rp = (C.POINTER(VsTrajRelease) * n)(*[C.cast(r, C.POINTER(VsTrajRelease)) for r in rel])
        st = (C.c_int32 * len(steps))(*steps) if steps else None
        self.check(self.lib.vs_op_trajectory(C.byref(params), n, mp, kp, npush, 0 if steps is None else 1, st, len(steps) if steps else 0,
                                             dp, n_dbg, rp, n_rel))
        return [(list(dbg[s][:n_dbg[s]]), list(rel[s][:n_rel[s]])) for s in range(n)]

    def warp_affine(self, img, M, batch=None):
        """img: (h,w[,3]) or (b,h,w,3) uint8; M: (6,) or (b,6).  batch=True / False settles what a 3-d array is: b planes of
        one channel, or one image of shape[2] channels."""
        img = np.ascontiguousarray(img)
        batched = img.ndim == 4 or (img.ndim == 3 and (img.shape[2] not in (1, 3) if batch is None else batch))
        if img.ndim == 2:
            b, (h, w), cn = 1, img.shape, 1
        elif img.ndim == 3 and not batched:
            b, (h, w, cn) = 1, img.shape
        elif img.ndim == 3:
            (b, h, w), cn = img.shape, 1
        else:
            b, h, w, cn = img.shape
        M = np.ascontiguousarray(M, np.float32).reshape(b, 6)
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        fb = h * w * cn
        self.check(self.lib.vs_op_warp_affine(d_in.ptr, w * cn, fb, d_out.ptr, w * cn, fb, w, h, cn,
                                              _p(M, f32p), b, None))
        self.sync()
        return d_out.download(img.shape, np.uint8)

    def warp_affine_nv12(self, img, w, h, M):
        """img: one NV12 surface (h * 3 / 2 rows of w bytes) and one matrix, or a stack of n surfaces and n matrices (launches
        of four and more surfaces warp both planes in one grid)."""
        img = np.ascontiguousarray(img)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        self.check(self.lib.vs_op_warp_affine_nv12(d_in.ptr, w, d_out.ptr, w, w, h, _p(M, f32p), n, fb, fb, None))
        self.sync()
        return d_out.download(img.shape, np.uint8)

    def warp_affine_p010(self, img, w, h, M):
        """img: one P010 surface (h * 3 / 2 rows of w uint16) and one matrix, or a stack of n surfaces and n matrices."""
        img = np.ascontiguousarray(img, np.uint16)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        self.check(self.lib.vs_op_warp_affine_p010(d_in.ptr, 2 * w, d_out.ptr, 2 * w, w, h, _p(M, f32p), n, fb, fb, None))
        self.sync()
        return d_out.download(img.shape, np.uint16)

    def warp_affine_i420(self, img, w, h, M, border=BORDER_BLACK):
        """img: one packed I420 surface (h * 3 / 2 rows of w bytes: Y, U plane, V plane) and one matrix, or a stack of n surfaces
        and n matrices; all three planes of up to 32 surfaces per launch."""
        img = np.ascontiguousarray(img, np.uint8)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        try:
            self.check(self.lib.vs_op_warp_affine_i420(d_in.ptr, w, 0, 0, 0, d_out.ptr, w, 0, 0, 0, w, h, _p(M, f32p), n, fb, fb, border, None))
            self.sync()
            return d_out.download(img.shape, np.uint8)
        finally:
            d_in.free(); d_out.free()

    def warp_affine_i010(self, img, w, h, M, border=BORDER_BLACK):
        """img: one packed I010 / I012 surface (h * 3 / 2 rows of w uint16: Y, U plane, V plane) and one matrix, or a stack of n
        surfaces and n matrices.  One call for both depths: the warp does not depend on the depth."""
        img = np.ascontiguousarray(img, np.uint16)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        try:
            self.check(self.lib.vs_op_warp_affine_i010(d_in.ptr, 2 * w, 0, 0, 0, d_out.ptr, 2 * w, 0, 0, 0, w, h, _p(M, f32p), n, fb, fb, border, None))
            self.sync()
            return d_out.download(img.shape, np.uint16)
        finally:
            d_in.free(); d_out.free()

    def warp_affine_planar(self, fmt, img, w, h, M, border=BORDER_BLACK):
        """img: one packed surface of a planar format (FMT_I420 ... FMT_I412: fmt_frame_rows(fmt, h) rows of w samples) and one
        matrix, or a stack of n surfaces and n matrices; all three planes of up to 32 surfaces per launch."""
        dt = fmt_dtype(fmt)
        img = np.ascontiguousarray(img, dt)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        sb = fmt_px_bytes(fmt)
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        try:
            self.check(self.lib.vs_op_warp_affine_planar(fmt, d_in.ptr, sb * w, 0, 0, 0, d_out.ptr, sb * w, 0, 0, 0, w, h, _p(M, f32p), n, fb, fb, border, None))
            self.sync()
            return d_out.download(img.shape, dt)
        finally:
            d_in.free(); d_out.free()

    def warp_affine_yuv_fill(self, fmt, img, w, h, M, fill=None):
        """vs_op_warp_affine_yuv_fill on packed surfaces of any YUV format (NV12, P010, I420 ... I412): one surface and one matrix,
        or a stack of n surfaces and n matrices.  fill: (y, u, v) samples as they lie in memory; None: the format's video black."""
        dt = fmt_dtype(fmt)
        img = np.ascontiguousarray(img, dt)
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 6)
        n = M.shape[0]
        fb = img.nbytes // n
        sb = img.itemsize
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, img.nbytes)
        try:
            self.check(self.lib.vs_op_warp_affine_yuv_fill(fmt, d_in.ptr, sb * w, 0, 0, 0, d_out.ptr, sb * w, 0, 0, 0, w, h, _p(M, f32p), n, fb, fb, c, None))
            self.sync()
            return d_out.download(img.shape, dt)
        finally:
            d_in.free(); d_out.free()

    def resize_gray(self, img, dw, dh, fmt=None):
        img = np.ascontiguousarray(img)
        if fmt is None:
            fmt = FMT_BGR8 if img.ndim == 3 else FMT_GRAY8
        w = img.shape[1]
        h = img.shape[0] if not fmt_two_planes(fmt) else img.shape[0] * 2 // 3
        cn = fmt_px_bytes(fmt)
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, dw * dh)
        self.check(self.lib.vs_op_resize_gray(d_in.ptr, w * cn, w, h, fmt, d_out.ptr, dw, dw, dh, None))
        self.sync()
        return d_out.download((dh, dw), np.uint8)

    def pyr_down(self, g):
        g = np.ascontiguousarray(g)
        h, w = g.shape
        dh, dw = (h + 1) // 2, (w + 1) // 2
        d_in = DevBuf.from_array(self, g)
        d_out = DevBuf(self, dw * dh)
        self.check(self.lib.vs_op_pyr_down(d_in.ptr, w, w, h, d_out.ptr, dw, None))
        self.sync()
        return d_out.download((dh, dw), np.uint8)

    def scharr(self, g):
        g = np.ascontiguousarray(g)
        h, w = g.shape
        d_in = DevBuf.from_array(self, g)
        d_out = DevBuf(self, h * w * 4)
        self.check(self.lib.vs_op_scharr(d_in.ptr, w, w, h, d_out.ptr, None))
        self.sync()
        return d_out.download((h, w, 2), np.int16)

    def pyr_level(self, g, down=True):
        """One pyramid level of batch mode: (derivatives int16 (h, w, 2), next level or None) of a gray image."""
        g = np.ascontiguousarray(g)
        h, w = g.shape
        dh, dw = (h + 1) // 2, (w + 1) // 2
        d_in = DevBuf.from_array(self, g)
        d_der = DevBuf(self, h * w * 4)
        d_next = DevBuf(self, dw * dh) if down else None
        self.check(self.lib.vs_op_pyr_level(d_in.ptr, w, w * h, w, h, d_der.ptr, d_next.ptr if down else None, dw, dw * dh, 1, None))
        self.sync()
        return d_der.download((h, w, 2), np.int16), (d_next.download((dh, dw), np.uint8) if down else None)

    def pyr_lk(self, prev, nxt, pts, win=15, max_level=2, iters=20, eps=0.03):
        prev = np.ascontiguousarray(prev)
        nxt = np.ascontiguousarray(nxt)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        h, w = prev.shape
        d_prev = DevBuf.from_array(self, prev)
        d_next = DevBuf.from_array(self, nxt)
        d_pts = DevBuf.from_array(self, pts)
        d_out = DevBuf(self, n * 8)
        d_st = DevBuf(self, n)
        d_err = DevBuf(self, n * 4)
        self.check(self.lib.vs_op_pyr_lk(d_prev.ptr, d_next.ptr, w, w, h, d_pts.ptr, n, d_out.ptr, d_st.ptr,
                                         d_err.ptr, win, max_level, iters, eps, None))
        self.sync()
        return (d_out.download((n, 2), np.float32), d_st.download((n,), np.uint8),
                d_err.download((n,), np.float32))

    def gftt(self, g, max_corners, quality, min_distance, block_size=3, want_eig=False):
        g = np.ascontiguousarray(g)
        h, w = g.shape
        d_in = DevBuf.from_array(self, g)
        d_pts = DevBuf(self, max(max_corners, 1) * 8)
        d_cnt = DevBuf(self, 16)
        d_eig = DevBuf(self, w * h * 4) if want_eig else None
        self.check(self.lib.vs_op_gftt(d_in.ptr, w, w, h, max_corners, quality, min_distance, block_size,
                                       d_pts.ptr, d_cnt.ptr, d_eig.ptr if d_eig else None, None))
        self.sync()
        n = int(d_cnt.download((1,), np.int32)[0])
        pts = d_pts.download((max(max_corners, 1), 2), np.float32)[:n].copy()
        if want_eig:
            return pts, d_eig.download((h, w), np.float32)
        return pts

    def estimate_affine_partial2d(self, a, b, thr=5.0, max_iters=500):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 2)
        n = a.shape[0]
        d_a = DevBuf.from_array(self, a)
        d_b = DevBuf.from_array(self, b)
        d_model = DevBuf(self, 48)
        d_inl = DevBuf(self, max(n, 1))
        d_info = DevBuf(self, 16)
        self.check(self.lib.vs_op_estimate_affine_partial2d(d_a.ptr, d_b.ptr, n, thr, max_iters, d_model.ptr,
                                                            d_inl.ptr, d_info.ptr, None))
        self.sync()
        info = d_info.download((4,), np.int32)
        return (int(info[0]), d_model.download((6,), np.float64), d_inl.download((max(n, 1),), np.uint8)[:n], info)

    def canny(self, g, low, high):
        g = np.ascontiguousarray(g)
        h, w = g.shape
        d_in = DevBuf.from_array(self, g)
        d_out = DevBuf(self, w * h)
        self.check(self.lib.vs_op_canny(d_in.ptr, w, w, h, low, high, d_out.ptr, w, None))
        self.sync()
        return d_out.download((h, w), np.uint8)

    def hough_lines(self, edges, rho, theta, threshold, max_lines=8192):
        edges = np.ascontiguousarray(edges)
        h, w = edges.shape
        d_in = DevBuf.from_array(self, edges)
        d_lines = DevBuf(self, max_lines * 8)
        d_cnt = DevBuf(self, 16)
        self.check(self.lib.vs_op_hough_lines(d_in.ptr, w, w, h, rho, theta, threshold, d_lines.ptr, max_lines,
                                              d_cnt.ptr, None))
        self.sync()
        n = int(d_cnt.download((1,), np.int32)[0])
        return d_lines.download((max_lines, 2), np.float32)[:n].copy()

    def warp_affine_ex(self, img, M, border=BORDER_BLACK, dsize=None):
        """cv::warpAffine with a double 2x3 forward matrix and a border mode."""
        img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        cn = 1 if img.ndim == 2 else img.shape[2]
        dw, dh = dsize if dsize else (w, h)
        M = np.ascontiguousarray(M, np.float64).reshape(6)
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, dw * dh * cn)
        self.check(self.lib.vs_op_warp_affine_ex(d_in.ptr, w * cn, w, h, d_out.ptr, dw * cn, dw, dh, cn,
                                                 _p(M, f64p), border, None))
        self.sync()
        return d_out.download((dh, dw) if img.ndim == 2 else (dh, dw, cn), np.uint8)

    def warp_affine16_ex(self, img, M, border=BORDER_BLACK, dsize=None):
        """cv::warpAffine on a plane of 16-bit samples, (h, w) or (h, w, 2) uint16, with P010's blend (vs_op_warp_affine16_ex)."""
        img = np.ascontiguousarray(img, np.uint16)
        h, w = img.shape[:2]
        cn = 1 if img.ndim == 2 else img.shape[2]
        dw, dh = dsize if dsize else (w, h)
        M = np.ascontiguousarray(M, np.float64).reshape(6)
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, dw * dh * cn * 2)
        self.check(self.lib.vs_op_warp_affine16_ex(d_in.ptr, w * cn * 2, w, h, d_out.ptr, dw * cn * 2, dw, dh, cn,
                                                   _p(M, f64p), border, None))
        self.sync()
        return d_out.download((dh, dw) if img.ndim == 2 else (dh, dw, cn), np.uint16)

    @staticmethod
    def _scale_job_array(jobs):
        arr = (VsScaleJob * max(1, len(jobs)))()
        for i, (src, src_stride, sw, sh, dst, dst_stride, dw, dh, cn) in enumerate(jobs):
            arr[i] = VsScaleJob(src, src_stride, sw, sh, dst, dst_stride, dw, dh, cn, 0)
        return arr

    def scale_jobs(self, jobs, sample_bytes=1, path=0, stream=None):
        """vs_op_scale_jobs: jobs = tuples (src, src_stride, sw, sh, dst, dst_stride, dw, dh, cn) of device addresses; asynchronous."""
        self.check(self.lib.vs_op_scale_jobs(self._scale_job_array(jobs), len(jobs), sample_bytes, path, stream))

    def resize_jobs(self, jobs, sample_bytes=1, stream=None):
        """vs_op_resize_jobs (the zoom of crop-and-zoom on YUV surfaces): 1 .. 96 jobs, tuples as for scale_jobs; asynchronous."""
        self.check(self.lib.vs_op_resize_jobs(self._scale_job_array(jobs), len(jobs), sample_bytes, stream))

    def resample_jobs(self, jobs, sample_bytes=1, interp=INTERP_LINEAR, max_value=0, path=0, stream=None):
        """vs_op_resample_jobs (resize to an output size, any ratio): 1 .. 96 jobs, tuples as for scale_jobs; asynchronous."""
        self.check(self.lib.vs_op_resample_jobs(self._scale_job_array(jobs), len(jobs), sample_bytes, interp, max_value, path, stream))

    def resample_jobs_plan(self, jobs, sample_bytes=1, interp=INTERP_LINEAR):
        """vs_op_resample_jobs_plan (no device needed): 1 per job that path 0 sends into the staged launch."""
        staged = np.zeros(max(1, len(jobs)), np.int32)
        self.check(self.lib.vs_op_resample_jobs_plan(self._scale_job_array(jobs), len(jobs), sample_bytes, interp, _p(staged, i32p)))
        return staged[:len(jobs)].copy()

    def resize_axis_table(self, src, dst, interp, axis):
        """vs_resize_axis_table (no device needed): (idx (dst, K) int32, coef (dst, K) int16), K = 2 (LINEAR) or 8 (LANCZOS4)."""
        k = 8 if interp == INTERP_LANCZOS4 else 2
        idx, coef = np.zeros((max(dst, 1), k), np.int32), np.zeros((max(dst, 1), k), np.int16)
        self.check(self.lib.vs_resize_axis_table(src, dst, interp, axis, _p(idx, i32p), coef.ctypes.data_as(C.POINTER(C.c_int16))))
        return idx, coef

    def resize_yuv(self, fmt, d_src, in_layout, sw, sh, d_dst, out_layout, dw, dh, interp=INTERP_LINEAR, stream=None):
        """vs_op_resize_yuv on surfaces in device memory: d_src, d_dst lists of device addresses, layouts (pitch[, c_pitch[, u_off[,
        v_off]]]) in bytes, 0 = the default of a field; asynchronous."""
        src, dst = (C.c_void_p * len(d_src))(*d_src), (C.c_void_p * len(d_dst))(*d_dst)
        self.check(self.lib.vs_op_resize_yuv(fmt, src, C.byref(I420LayoutC(*in_layout)), sw, sh, dst, C.byref(I420LayoutC(*out_layout)), dw, dh,
                                             len(d_src), interp, stream))

    def resize_rgb(self, fmt, d_src, src_stride, sw, sh, d_dst, dst_stride, dw, dh, interp=INTERP_LINEAR, stream=None):
        """vs_op_resize_rgb on BGR8 / RGB8 / BGRA8 / RGBA8 / GRAY8 frames in device memory (lists of device addresses); asynchronous."""
        src, dst = (C.c_void_p * len(d_src))(*d_src), (C.c_void_p * len(d_dst))(*d_dst)
        self.check(self.lib.vs_op_resize_rgb(fmt, src, src_stride, sw, sh, dst, dst_stride, dw, dh, len(d_src), interp, stream))

    def area_jobs(self, jobs, sample_bytes=1, max_value=0, stream=None):
        """vs_op_area_jobs (area-averaging downscale, dw <= sw and dh <= sh): 1 .. 96 jobs, tuples as for scale_jobs; asynchronous."""
        self.check(self.lib.vs_op_area_jobs(self._scale_job_array(jobs), len(jobs), sample_bytes, max_value, stream))

    def area_jobs_plan(self, jobs, sample_bytes=1):
        """vs_op_area_jobs_plan (no device needed): the class of every job - 2 the 2 x 2 mean, 1 integer box, 0 general."""
        cls = np.zeros(max(1, len(jobs)), np.int32)
        self.check(self.lib.vs_op_area_jobs_plan(self._scale_job_array(jobs), len(jobs), sample_bytes, _p(cls, i32p)))
        return cls[:len(jobs)].copy()

    def area_axis_table(self, src, dst):
        """vs_area_axis_table (no device needed): first, count (int32) and w_first, w_mid, w_last (float32), dst entries each."""
        n = max(dst, 1)
        first, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
        w = [np.zeros(n, np.float32) for _ in range(3)]
        self.check(self.lib.vs_area_axis_table(src, dst, _p(first, i32p), _p(count, i32p), *[_p(x, f32p) for x in w]))
        return (first, count) + tuple(w)

    def area_yuv(self, fmt, d_src, in_layout, sw, sh, d_dst, out_layout, dw, dh, stream=None):
        """vs_op_area_yuv on surfaces in device memory: arguments as for resize_yuv, without interp; asynchronous."""
        src, dst = (C.c_void_p * len(d_src))(*d_src), (C.c_void_p * len(d_dst))(*d_dst)
        self.check(self.lib.vs_op_area_yuv(fmt, src, C.byref(I420LayoutC(*in_layout)), sw, sh, dst, C.byref(I420LayoutC(*out_layout)), dw, dh,
                                           len(d_src), stream))

    def area_rgb(self, fmt, d_src, src_stride, sw, sh, d_dst, dst_stride, dw, dh, stream=None):
        """vs_op_area_rgb on BGR8 / RGB8 / BGRA8 / RGBA8 / GRAY8 frames in device memory (lists of device addresses); asynchronous."""
        src, dst = (C.c_void_p * len(d_src))(*d_src), (C.c_void_p * len(d_dst))(*d_dst)
        self.check(self.lib.vs_op_area_rgb(fmt, src, src_stride, sw, sh, dst, dst_stride, dw, dh, len(d_src), stream))

    def deint_jobs(self, jobs, sample_bytes=1, mode=DEINT_YADIF, stream=None):
        """vs_op_deint_jobs: 1 .. 96 plane jobs, tuples (prev, prev_stride, cur, cur_stride, next, next_stride, dst, dst_stride, w, h,
        cn, keep, second[, reserved]) of device addresses, prev / next None or 0 = the current frame; asynchronous."""
        arr = (VsDeintJob * max(1, len(jobs)))()
        for a, j in zip(arr, jobs):
            j = tuple(j) + (0,) * (14 - len(j))
            (a.prev, a.prev_stride, a.cur, a.cur_stride, a.next, a.next_stride, a.dst, a.dst_stride, a.w, a.h, a.cn, a.keep, a.second, a.reserved) = j
        self.check(self.lib.vs_op_deint_jobs(arr, len(jobs), sample_bytes, mode, stream))

    def deint_yuv(self, fmt, d_prev, d_cur, d_next, in_layout, w, h, d_first, d_second, out_layout, tff=1, mode=DEINT_YADIF, stream=None):
        """vs_op_deint_yuv on surfaces in device memory: lists of device addresses; d_prev / d_next None or lists that may hold None
        (the current frame stands in); d_second None = single rate; layouts as for resize_yuv; asynchronous."""
        def arr(v):
            return None if v is None else (C.c_void_p * len(v))(*v)
        self.check(self.lib.vs_op_deint_yuv(fmt, arr(d_prev), arr(d_cur), arr(d_next), C.byref(I420LayoutC(*in_layout)), w, h, arr(d_first), arr(d_second),
                                            C.byref(I420LayoutC(*out_layout)), tff, mode, len(d_cur), stream))

    def interlace_yuv(self, fmt, d_first, d_second, in_layout, w, h, d_dst, out_layout, tff=1, stream=None):
        """vs_op_interlace_yuv (the weave of pairs of progressive surfaces): lists of device addresses; asynchronous."""
        a, b, d = ((C.c_void_p * len(v))(*v) for v in (d_first, d_second, d_dst))
        self.check(self.lib.vs_op_interlace_yuv(fmt, a, b, C.byref(I420LayoutC(*in_layout)), w, h, d, C.byref(I420LayoutC(*out_layout)), tff, len(d_dst), stream))

    def pad_jobs(self, jobs, sample_bytes=1, stream=None):
        """vs_op_pad_jobs (the pad of border pad on YUV surfaces): 1 .. 96 jobs, tuples (src, src_stride, sw, sh, dst, dst_stride, bx,
        by, cn, border, (fill0, fill1)) of device addresses; asynchronous."""
        arr = (VsPadJob * max(1, len(jobs)))()
        for a, (src, ss, sw, sh, dst, ds, bx, by, cn, border, fill) in zip(arr, jobs):
            a.src, a.src_stride, a.sw, a.sh, a.dst, a.dst_stride, a.bx, a.by, a.cn, a.border = src, ss, sw, sh, dst, ds, bx, by, cn, border
            a.fill[0], a.fill[1] = fill
        self.check(self.lib.vs_op_pad_jobs(arr, len(jobs), sample_bytes, stream))

    def fade_blend_jobs(self, jobs, alpha, beta, sample_bytes=1, stream=None):
        """vs_op_fade_blend_jobs (pad and blend of the fade border on YUV surfaces): 1 .. 32 jobs, tuples (src, src_stride, sw, sh,
        hist, hist_stride, dst, dst_stride, bx, by, cn, (fill0, fill1)) of device addresses; asynchronous."""
        arr = (VsFadeJob * max(1, len(jobs)))()
        for a, (src, ss, sw, sh, hist, hs, dst, ds, bx, by, cn, fill) in zip(arr, jobs):
            a.src, a.src_stride, a.sw, a.sh, a.hist, a.hist_stride = src, ss, sw, sh, hist, hs
            a.dst, a.dst_stride, a.bx, a.by, a.cn = dst, ds, bx, by, cn
            a.fill[0], a.fill[1] = fill
        self.check(self.lib.vs_op_fade_blend_jobs(arr, len(jobs), sample_bytes, alpha, beta, stream))

    def fade_update_jobs(self, jobs, sample_bytes=1, stream=None):
        """vs_op_fade_update_jobs (the history update of the fade border on YUV surfaces): 1 .. 32 jobs, tuples (hist, hist_stride,
        res, res_stride, w, h, cn) of device addresses; asynchronous."""
        arr = (VsFadeUpdateJob * max(1, len(jobs)))()
        for a, (hist, hs, res, rs, w, h, cn) in zip(arr, jobs):
            a.hist, a.hist_stride, a.res, a.res_stride, a.w, a.h, a.cn = hist, hs, res, rs, w, h, cn
        self.check(self.lib.vs_op_fade_update_jobs(arr, len(jobs), sample_bytes, stream))

    def yuv_video_black(self, fmt):
        """vs_yuv_video_black (no device needed): (y, u, v) of limited-range black, samples as they lie in memory."""
        c = VsYuvFill()
        self.check(self.lib.vs_yuv_video_black(fmt, C.byref(c)))
        return c.y, c.u, c.v

    def scale_jobs_plan(self, jobs, sample_bytes=1):
        """vs_op_scale_jobs_plan (no device needed): 1 per job that path 0 sends to the staged kernel."""
        staged = np.zeros(max(1, len(jobs)), np.int32)
        self.check(self.lib.vs_op_scale_jobs_plan(self._scale_job_array(jobs), len(jobs), sample_bytes, _p(staged, i32p)))
        return staged[:len(jobs)].copy()

    def scale_jobs_rgb(self, jobs, path=0, stream=None):
        """vs_op_scale_jobs_rgb: crops of interleaved colour frames (8-bit, cn 3 or 4), tuples as for scale_jobs; asynchronous."""
        self.check(self.lib.vs_op_scale_jobs_rgb(self._scale_job_array(jobs), len(jobs), path, stream))

    def scale_jobs_rgb_plan(self, jobs):
        """vs_op_scale_jobs_rgb_plan (no device needed): 1 per job that path 0 sends to the staged kernel."""
        staged = np.zeros(max(1, len(jobs)), np.int32)
        self.check(self.lib.vs_op_scale_jobs_rgb_plan(self._scale_job_array(jobs), len(jobs), _p(staged, i32p)))
        return staged[:len(jobs)].copy()

    def copy_make_border(self, img, b, border, src_pitch=None):
        """vs_op_copy_make_border: img (h, w) or (h, w, cn); src_pitch: a source row pitch of its own, in bytes."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        cn = 1 if img.ndim == 2 else img.shape[2]
        pitch = src_pitch or w * cn
        rows = np.full((h, pitch), 0xA5, np.uint8)
        rows[:, :w * cn] = img.reshape(h, w * cn)
        ow, oh = w + 2 * b, h + 2 * b
        d_in = DevBuf.from_array(self, rows)
        d_out = DevBuf(self, ow * oh * cn)
        self.check(self.lib.vs_op_copy_make_border(d_in.ptr, pitch, w, h, cn, d_out.ptr, ow * cn, b, border, None))
        self.sync()
        return d_out.download((oh, ow) if img.ndim == 2 else (oh, ow, cn), np.uint8)

    def fade_blend(self, hist, frame, alpha, beta):
        """vs_op_fade_blend on two flat uint8 arrays of one size: the blended frame."""
        hist = np.ascontiguousarray(hist, np.uint8).reshape(-1)
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        assert hist.size == frame.size
        pad = (-hist.size) % 4
        d_h = DevBuf.from_array(self, np.concatenate([hist, np.zeros(pad, np.uint8)]))
        d_f = DevBuf.from_array(self, np.concatenate([frame, np.zeros(pad, np.uint8)]))
        self.check(self.lib.vs_op_fade_blend(d_h.ptr, d_f.ptr, hist.size, alpha, beta, None))
        self.sync()
        return d_f.download((hist.size,), np.uint8)

    def fade_update(self, hist, stab, row_bytes, rows):
        """vs_op_fade_update: hist a flat uint8 array of at least rows * row_bytes bytes (the whole array comes back, so that a
        guard behind the history can be checked), stab (rows, pitch) uint8 with pitch >= row_bytes."""
        hist = np.ascontiguousarray(hist, np.uint8).reshape(-1)
        stab = np.ascontiguousarray(stab, np.uint8)
        assert stab.shape[0] == rows and stab.shape[1] >= row_bytes and hist.size >= rows * row_bytes
        d_h = DevBuf.from_array(self, hist)
        d_s = DevBuf.from_array(self, stab)
        self.check(self.lib.vs_op_fade_update(d_h.ptr, d_s.ptr, stab.shape[1], row_bytes, rows, None))
        self.sync()
        return d_h.download((hist.size,), np.uint8)

    def cvt_coefficients(self, colorimetry=None):
        """vs_cvt_coefficients (host only): the sixteen integers of a descriptor - y_off, CY, RV, GV, GU, BU, YR, YG, YB, UR, UG, UB,
        VR, VG, VB, 0.  colorimetry: None, a CvtColorimetry or (matrix, range[, chroma_down[, reserved]])."""
        out = np.zeros(16, np.int32)
        self.check(self.lib.vs_cvt_coefficients(_cs_ref(colorimetry), _p(out, i32p)))
        return out

    def cvt_colorimetry_guess(self, w, h):
        """vs_cvt_colorimetry_guess (host only): the convention for untagged video -> CvtColorimetry."""
        cs = CvtColorimetry(-1, -1, -1, -1)
        self.lib.vs_cvt_colorimetry_guess(w, h, C.byref(cs))
        return cs

    def cvt_yuv_to_rgb(self, yuv_fmt, surfaces, w, h, rgb_fmt=FMT_BGR8, layout=None, rgb_stride=None, raw=False, fill=0xA5, colorimetry=None,
                       use_cs=False):
        """vs_op_cvt_yuv_to_rgb.  surfaces: one surface of w x h pixels or a list of up to 32, converted in one launch - packed frames
        ((rows, w) arrays of the format's dtype: synth.yuv_pack, synth.nv12_to_i420, the NV12 / P010 arrays) or flat buffers in
        `layout` = (pitch, c_pitch, u_off, v_off) in bytes, 0 = the default of a field (NV12 / P010: u_off = the interleaved plane).
        -> (h, w, cn) uint8 per surface; raw=True: the whole destination instead, h * rgb_stride + 16 bytes prefilled with `fill`.
        colorimetry: None (the entry point without a descriptor), a CvtColorimetry or (matrix, range[, chroma_down]) through
        vs_op_cvt_yuv_to_rgb_cs; use_cs=True: the _cs entry point with a null descriptor."""
        f, cn = PIXFMT[yuv_fmt], PIXFMT[rgb_fmt].cn
        srcs, single = _surface_list(surfaces)
        n = len(srcs)
        lay = I420LayoutC(*(layout or (f.sample_bytes * w, 0, 0, 0)))
        stride = rgb_stride or w * cn
        nbytes = h * stride + 16
        d_in = [DevBuf.from_array(self, s) for s in srcs]
        d_out = [DevBuf.from_array(self, np.full(nbytes, fill, np.uint8)) for _ in range(n)]
        try:
            if colorimetry is None and not use_cs:
                self.check(self.lib.vs_op_cvt_yuv_to_rgb(yuv_fmt, _ptr_array(d_in), C.byref(lay), rgb_fmt, _ptr_array(d_out), stride, n, w, h, None))
            else:
                self.check(self.lib.vs_op_cvt_yuv_to_rgb_cs(yuv_fmt, _ptr_array(d_in), C.byref(lay), rgb_fmt, _ptr_array(d_out), stride, n, w, h,
                                                            _cs_ref(colorimetry), None))
            self.sync()
            outs = [d.download((nbytes,), np.uint8) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()
        if not raw:
            outs = [o[:h * stride].reshape(h, stride)[:, :w * cn].reshape(h, w, cn).copy() for o in outs]
        return outs[0] if single else outs

    def cvt_rgb_to_yuv(self, frames, yuv_fmt, rgb_fmt=FMT_BGR8, layout=None, size=None, rgb_stride=None, raw=False, fill=0xA5, colorimetry=None,
                       use_cs=False):
        """vs_op_cvt_rgb_to_yuv.  frames: one (h, w, cn) uint8 frame or a list of up to 32 of one size, converted in one launch.
        -> per frame the packed surface ((rows, w) array of the format's dtype) or, with a `layout` (as above) and `size` in bytes, the
        flat buffer of that layout; raw=True: the whole destination as bytes instead, `size` + 16 of them prefilled with `fill`.
        colorimetry, use_cs: as for cvt_yuv_to_rgb (vs_op_cvt_rgb_to_yuv_cs)."""
        f = PIXFMT[yuv_fmt]
        single = isinstance(frames, np.ndarray) and frames.ndim == 3
        frames = [np.ascontiguousarray(x, np.uint8) for x in ([frames] if single else frames)]
        n = len(frames)
        h, w, cn = frames[0].shape
        stride = rgb_stride or w * cn
        lay = I420LayoutC(*(layout or (f.sample_bytes * w, 0, 0, 0)))
        size = size or yuv_surface_bytes(yuv_fmt, w, h, *(layout or ()))
        d_in = []
        for x in frames:
            rows = np.full((h, stride), fill, np.uint8)
            rows[:, :w * cn] = x.reshape(h, w * cn)
            d_in.append(DevBuf.from_array(self, rows))
        d_out = [DevBuf.from_array(self, np.full(size + 16, fill, np.uint8)) for _ in range(n)]
        try:
            if colorimetry is None and not use_cs:
                self.check(self.lib.vs_op_cvt_rgb_to_yuv(rgb_fmt, _ptr_array(d_in), stride, yuv_fmt, _ptr_array(d_out), C.byref(lay), n, w, h, None))
            else:
                self.check(self.lib.vs_op_cvt_rgb_to_yuv_cs(rgb_fmt, _ptr_array(d_in), stride, yuv_fmt, _ptr_array(d_out), C.byref(lay), n, w, h,
                                                            _cs_ref(colorimetry), None))
            self.sync()
            outs = [d.download((size + 16,), np.uint8) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()
        if not raw:
            outs = [o[:size].view(fmt_dtype(yuv_fmt)) for o in outs]
            if not layout:
                outs = [o.reshape(fmt_frame_rows(yuv_fmt, h), w) for o in outs]
        return outs[0] if single else outs

    def yuv_surface_layout(self, fmt, w, h, layout=None):
        """vs_yuv_surface_layout (host only): ((pitch, c_pitch, u_off, v_off), bytes) - the layout of a w x h surface with every default
        filled in and the bytes from the surface pointer to the end of its last sample.  layout: None (all defaults at the tight
        pitch) or (pitch[, c_pitch[, u_off[, v_off]]]) in bytes, 0 = the default of a field."""
        res, nbytes = I420LayoutC(), C.c_size_t()
        self.check(self.lib.vs_yuv_surface_layout(fmt, w, h, C.byref(I420LayoutC(*layout)) if layout else None, C.byref(res), C.byref(nbytes)))
        return (res.pitch, res.c_pitch, res.u_off, res.v_off), nbytes.value

    def cvt_yuv_to_yuv(self, src_fmt, surfaces, w, h, dst_fmt, in_layout=None, out_layout=None, desc=None, raw=False, fill=0xA5):
        """vs_op_cvt_yuv_to_yuv.  surfaces: one surface of w x h pixels or a list of up to 32, converted in one launch - packed frames
        or flat buffers in `in_layout`, as for cvt_yuv_to_rgb.  -> per surface the packed frame of dst_fmt ((rows, w) array of its
        dtype) or, with an `out_layout`, the flat array of that layout up to its last sample (vs_yuv_surface_layout); raw=True: the
        whole destination as bytes instead, those bytes + 16 prefilled with `fill`.  desc: None (a null descriptor), a VsYuvCvtDesc
        or (depth_down[, chroma_down]) - YUV_DEPTH_TRUNCATE / YUV_DEPTH_ROUND, CVT_CHROMA_TOPLEFT / CVT_CHROMA_MEAN."""
        fi, fo = PIXFMT[src_fmt], PIXFMT[dst_fmt]
        srcs, single = _surface_list(surfaces)
        n = len(srcs)
        lin = I420LayoutC(*(in_layout or (fi.sample_bytes * w, 0, 0, 0)))
        lout = I420LayoutC(*(out_layout or (fo.sample_bytes * w, 0, 0, 0)))
        _, size = self.yuv_surface_layout(dst_fmt, w, h, out_layout)
        d_in = [DevBuf.from_array(self, s) for s in srcs]
        d_out = [DevBuf.from_array(self, np.full(size + 16, fill, np.uint8)) for _ in range(n)]
        try:
            self.check(self.lib.vs_op_cvt_yuv_to_yuv(src_fmt, _ptr_array(d_in), C.byref(lin), dst_fmt, _ptr_array(d_out), C.byref(lout), n, w, h,
                                                     _yuv_desc_ref(desc), None))
            self.sync()
            outs = [d.download((size + 16,), np.uint8) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()
        if not raw:
            outs = [o[:size].view(fmt_dtype(dst_fmt)) for o in outs]
            if not out_layout:
                outs = [o.reshape(fmt_frame_rows(dst_fmt, h), w) for o in outs]
        return outs[0] if single else outs

    def packed_layout(self, packed_fmt, w, h, pitch=0):
        """vs_packed_layout (host only): (row_bytes, pitch, bytes) of a w x h frame of a PACKED_* format - the bytes of a row, the
        pitch (`pitch`, or the format's default for 0) and the bytes from the frame pointer to the end of the last row's bytes."""
        row, res, nbytes = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.check(self.lib.vs_packed_layout(packed_fmt, w, h, pitch, C.byref(row), C.byref(res), C.byref(nbytes)))
        return row.value, res.value, nbytes.value

    def cvt_packed_to_yuv(self, packed_fmt, frames, w, h, dst_fmt, pitch=0, out_layout=None, desc=None, raw=False, fill=0xA5):
        """vs_op_cvt_packed_to_yuv.  frames: one packed frame of w x h pixels or a list of up to 32, converted in one launch - arrays
        of any dtype whose bytes are the frame's, rows `pitch` bytes apart (0 = the format's default).  -> per frame what
        cvt_yuv_to_yuv gives for dst_fmt, out_layout and raw; desc as there."""
        fo = PIXFMT[dst_fmt]
        srcs, single = _surface_list(frames)
        n = len(srcs)
        lout = I420LayoutC(*(out_layout or (fo.sample_bytes * w, 0, 0, 0)))
        _, size = self.yuv_surface_layout(dst_fmt, w, h, out_layout)
        d_in = [DevBuf.from_array(self, s) for s in srcs]
        d_out = [DevBuf.from_array(self, np.full(size + 16, fill, np.uint8)) for _ in range(n)]
        try:
            self.check(self.lib.vs_op_cvt_packed_to_yuv(packed_fmt, _ptr_array(d_in), pitch, dst_fmt, _ptr_array(d_out), C.byref(lout), n, w, h,
                                                        _yuv_desc_ref(desc), None))
            self.sync()
            outs = [d.download((size + 16,), np.uint8) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()
        if not raw:
            outs = [o[:size].view(fmt_dtype(dst_fmt)) for o in outs]
            if not out_layout:
                outs = [o.reshape(fmt_frame_rows(dst_fmt, h), w) for o in outs]
        return outs[0] if single else outs

    def cvt_yuv_to_packed(self, src_fmt, surfaces, w, h, packed_fmt, in_layout=None, pitch=0, desc=None, raw=False, fill=0xA5):
        """vs_op_cvt_yuv_to_packed.  surfaces, in_layout, desc: as for cvt_yuv_to_yuv.  -> per surface the (h, row_bytes) uint8 rows
        of the packed frame, rows `pitch` bytes apart on the device (0 = the format's default); raw=True: the whole destination
        instead, the bytes of vs_packed_layout + 16 prefilled with `fill`."""
        fi = PIXFMT[src_fmt]
        srcs, single = _surface_list(surfaces)
        n = len(srcs)
        lin = I420LayoutC(*(in_layout or (fi.sample_bytes * w, 0, 0, 0)))
        row, res, size = self.packed_layout(packed_fmt, w, h, pitch)
        d_in = [DevBuf.from_array(self, s) for s in srcs]
        d_out = [DevBuf.from_array(self, np.full(size + 16, fill, np.uint8)) for _ in range(n)]
        try:
            self.check(self.lib.vs_op_cvt_yuv_to_packed(src_fmt, _ptr_array(d_in), C.byref(lin), packed_fmt, _ptr_array(d_out), pitch, n, w, h,
                                                        _yuv_desc_ref(desc), None))
            self.sync()
            outs = [d.download((size + 16,), np.uint8) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()
        if not raw:
            outs = [np.stack([o[y * res:y * res + row] for y in range(h)]) for o in outs]
        return outs[0] if single else outs

    def enh_yuv_plan(self, params, yuv_fmt, in_place=False):
        """vs_enh_yuv_plan (host only): 1 = Enhancer.apply_yuv_batch_dev would take the fused launch, 0 = the three calls per surface,
        < 0 = minus the status of the refusal.  params: VsEnhParams or None."""
        return self.lib.vs_enh_yuv_plan(C.byref(params) if params is not None else None, yuv_fmt, int(bool(in_place)))

    def canvas_op(self):
        return CanvasOp(self)

    def content_mask(self, img):
        img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        cn = 1 if img.ndim == 2 else 3
        d_in = DevBuf.from_array(self, img)
        d_out = DevBuf(self, w * h)
        self.check(self.lib.vs_op_content_mask(d_in.ptr, w * cn, w, h, cn, d_out.ptr, w, None))
        self.sync()
        return d_out.download((h, w), np.uint8)

    def azc_crop_from_mask(self, mask, want_filled=False):
        """Host logic of AutoZoomCrop (no device needed): info8 [, filled mask]."""
        mask = np.ascontiguousarray(mask)
        h, w = mask.shape
        info = np.zeros(8, np.int32)
        filled = np.empty((h, w), np.uint8) if want_filled else None
        self.check(self.lib.vs_azc_crop_from_mask(_p(mask, u8p), w, h, w, _p(info, i32p),
                                                  _p(filled, u8p) if want_filled else None))
        return (info, filled) if want_filled else info

    def external_boxes(self, mask):
        """Bounding rectangles (x, y, w, h) of the external contours of a host mask, in cv::findContours order."""
        mask = np.ascontiguousarray(mask)
        h, w = mask.shape
        cap = w * h // 2 + 4
        xywh = np.zeros((cap, 4), np.int32)
        n = C.c_int32()
        self.check(self.lib.vs_op_external_boxes(_p(mask, u8p), w, h, w, _p(xywh, i32p), cap, C.byref(n)))
        return xywh[:n.value].copy()

    def auto_zoom_crop(self, device=0):
        return AutoZoomCrop(self, device)

    def roll_params(self, **kw):
        p = VsRollParams()
        self.lib.vs_roll_params_default(C.byref(p))
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, v)
        return p

    def roll_correction(self, params=None, device=0):
        return RollCorrection(self, params or self.roll_params(), device)

    def batch(self, params, n_streams, frames_per_step, device=0):
        return Batch(self, params, n_streams, frames_per_step, device)

    def stabilizer(self, params, device=0):
        return Stabilizer(self, params, device)


class I420LayoutC(C.Structure):
    """struct vs_i420_layout: where the planes of a three-plane surface (I420 ... I412) lie, in bytes (0 = the packed default of a field)."""
    _fields_ = [("pitch", C.c_size_t), ("c_pitch", C.c_size_t), ("u_off", C.c_size_t), ("v_off", C.c_size_t)]


class CvtColorimetry(C.Structure):
    """struct vs_cvt_colorimetry: the colour space of a conversion (all zero = BT.601 limited, top-left chroma)."""
    _fields_ = [("matrix", C.c_int32), ("range", C.c_int32), ("chroma_down", C.c_int32), ("reserved", C.c_int32)]


CVT_MATRIX_BT601, CVT_MATRIX_BT709, CVT_MATRIX_BT2020 = 0, 1, 2
CVT_RANGE_LIMITED, CVT_RANGE_FULL = 0, 1
CVT_CHROMA_TOPLEFT, CVT_CHROMA_MEAN = 0, 1


def _cs_ref(colorimetry):
    """None -> a null pointer; a CvtColorimetry or a tuple of its leading fields -> a reference to the struct."""
    if colorimetry is None:
        return None
    if not isinstance(colorimetry, CvtColorimetry):
        colorimetry = CvtColorimetry(*colorimetry)
    return C.byref(colorimetry)


class VsYuvCvtDesc(C.Structure):
    """struct vs_yuv_cvt_desc: how vs_op_cvt_yuv_to_yuv goes down in depth and in chroma resolution (all zero = truncate, top-left)."""
    _fields_ = [("depth_down", C.c_int32), ("chroma_down", C.c_int32), ("reserved", C.c_int32 * 2)]


YUV_DEPTH_TRUNCATE, YUV_DEPTH_ROUND = 0, 1
# enum vs_packed_fmt: the packed 4:2:2 capture formats of cvt_packed_to_yuv / cvt_yuv_to_packed (not pixel formats of a stream)
PACKED_YUY2, PACKED_UYVY, PACKED_YVYU, PACKED_Y210, PACKED_V210 = range(5)
PACKED_BY_NAME = {"YUY2": PACKED_YUY2, "UYVY": PACKED_UYVY, "YVYU": PACKED_YVYU, "Y210": PACKED_Y210, "v210": PACKED_V210}


def _yuv_desc_ref(desc):
    """None -> a null pointer; a VsYuvCvtDesc or (depth_down[, chroma_down]) -> a reference to the struct."""
    if desc is None:
        return None
    if not isinstance(desc, VsYuvCvtDesc):
        desc = VsYuvCvtDesc(*desc)
    return C.byref(desc)


def i420_layout(pitch, c_pitch=0, u_off=0, v_off=0):
    return I420LayoutC(pitch, c_pitch, u_off, v_off)


def yuv_surface_bytes(fmt, w, h, pitch=0, c_pitch=0, u_off=0, v_off=0):
    """Bytes up to the end of the last plane of a YUV surface in a layout (bytes, 0 = the library's default of a field)."""
    f = PIXFMT[fmt]
    pitch = pitch or f.sample_bytes * w
    if f.kind == KIND_LUMA_UV:
        return (u_off or h * pitch) + (h >> 1) * pitch
    c_pitch = c_pitch or pitch >> f.sx
    u_off = u_off or h * pitch
    v_off = v_off or u_off + (h >> f.sy) * c_pitch
    return max(u_off, v_off) + (h >> f.sy) * c_pitch


def _surface_list(surfaces):
    """([contiguous arrays], single): one surface - a flat buffer or a (rows, w) frame - or a list / stack of them."""
    single = isinstance(surfaces, np.ndarray) and surfaces.ndim <= 2
    return [np.ascontiguousarray(s) for s in ([surfaces] if single else surfaces)], single


def _ptr_array(bufs):
    return (C.c_void_p * len(bufs))(*[C.c_void_p(b.ptr) for b in bufs])


class AutoZoomCrop:
    """C-ABI mirror of vs::AutoZoomCrop::autoZoomCrop (AutoZoomCrop.cpp:102-283)."""

    def __init__(self, vs, device=0):
        self.vs = vs
        self.lib = vs.lib
        h = C.c_void_p()
        vs.check(self.lib.vs_azc_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.vs_azc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        if status != 0:
            raise VsError("%s: %s" % (self.lib.vs_status_string(status).decode(),
                                      (self.lib.vs_azc_last_error(self.h) or b"").decode()))

    def set_output_size(self, out_w, out_h):
        """vs_azc_set_output_size: the size of every later result; (640, 360) on a new object, (0, 0) = the surface's own size."""
        self._check(self.lib.vs_azc_set_output_size(self.h, out_w, out_h))

    @property
    def output_size(self):
        ow, oh = C.c_int(), C.c_int()
        self._check(self.lib.vs_azc_get_output_size(self.h, C.byref(ow), C.byref(oh)))
        return ow.value, oh.value

    def apply(self, frame):
        frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        cn = 1 if frame.ndim == 2 else 3
        sw, sh = self.output_size
        buf = np.empty(max(w * h, (sw or w) * (sh or h)) * cn, np.uint8)
        ow, oh = C.c_int(), C.c_int()
        self._check(self.lib.vs_azc_apply(self.h, _p(frame, u8p), w, h, w * cn, cn, _p(buf, u8p),
                                          C.byref(ow), C.byref(oh)))
        shape = (oh.value, ow.value) if cn == 1 else (oh.value, ow.value, 3)
        return buf[:oh.value * ow.value * cn].reshape(shape).copy()

    def apply_nv12_dev(self, d_in, w, h, pitch, d_out, out_pitch, out_uv_offset, uv_offset=0):
        """Asynchronous (vs_azc_apply_nv12_dev): returns the ticket; result(ticket) tells what came out, sync() completes the pixels."""
        t = C.c_int64(-1)
        self._check(self.lib.vs_azc_apply_nv12_dev(self.h, d_in, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset, C.byref(t)))
        return t.value

    def apply_nv12_dev_n(self, d_ins, w, h, pitch, d_outs, out_pitch, out_uv_offset, uv_offset=0):
        """n surfaces in call order, one trip through the binding; returns the tickets."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        t = (C.c_int64 * n)()
        self._check(self.lib.vs_azc_apply_nv12_dev_n(self.h, a, b, n, w, h, pitch, uv_offset, out_pitch, out_uv_offset, t))
        return list(t)

    def apply_p010_dev(self, d_in, w, h, pitch, d_out, out_pitch, out_uv_offset, uv_offset=0):
        """apply_nv12_dev for a P010 surface (vs_azc_apply_p010_dev): pitches and offsets in bytes, even."""
        t = C.c_int64(-1)
        self._check(self.lib.vs_azc_apply_p010_dev(self.h, d_in, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset, C.byref(t)))
        return t.value

    def apply_p010_dev_n(self, d_ins, w, h, pitch, d_outs, out_pitch, out_uv_offset, uv_offset=0):
        """n P010 surfaces in call order, one trip through the binding; returns the tickets."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        t = (C.c_int64 * n)()
        self._check(self.lib.vs_azc_apply_p010_dev_n(self.h, a, b, n, w, h, pitch, uv_offset, out_pitch, out_uv_offset, t))
        return list(t)

    def apply_i420_dev(self, fmt, d_in, w, h, lin, d_out, lout):
        """apply_nv12_dev for a planar surface (vs_azc_apply_i420_dev): fmt any three-plane format (FMT_I420 ... FMT_I412), lin / lout:
        i420_layout()."""
        t = C.c_int64(-1)
        self._check(self.lib.vs_azc_apply_i420_dev(self.h, fmt, d_in, w, h, C.byref(lin), d_out, C.byref(lout), C.byref(t)))
        return t.value

    def apply_i420_dev_n(self, fmt, d_ins, w, h, lin, d_outs, lout):
        """n planar surfaces in call order, one trip through the binding; returns the tickets."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        t = (C.c_int64 * n)()
        self._check(self.lib.vs_azc_apply_i420_dev_n(self.h, fmt, a, b, n, w, h, C.byref(lin), C.byref(lout), t))
        return list(t)

    def apply_rgb_dev(self, fmt, d_in, w, h, stride, d_out, out_stride):
        """apply_nv12_dev for an interleaved colour frame (vs_azc_apply_rgb_dev): fmt FMT_BGR8, FMT_RGB8, FMT_BGRA8 or FMT_RGBA8."""
        t = C.c_int64(-1)
        self._check(self.lib.vs_azc_apply_rgb_dev(self.h, fmt, d_in, w, h, stride, d_out, out_stride, C.byref(t)))
        return t.value

    def apply_rgb_dev_n(self, fmt, d_ins, w, h, stride, d_outs, out_stride):
        """n colour frames in call order, one trip through the binding; returns the tickets."""
        n = len(d_ins)
        a = (C.c_void_p * max(1, n))(*d_ins)
        b = (C.c_void_p * max(1, n))(*d_outs)
        t = (C.c_int64 * max(1, n))()
        self._check(self.lib.vs_azc_apply_rgb_dev_n(self.h, fmt, a, b, n, w, h, stride, out_stride, t))
        return list(t)[:n]

    def result(self, ticket):
        ow, oh = C.c_int(), C.c_int()
        info = np.zeros(8, np.int32)
        self._check(self.lib.vs_azc_result(self.h, ticket, C.byref(ow), C.byref(oh), _p(info, i32p)))
        return ow.value, oh.value, info

    def apply_dev(self, d_in, w, h, stride, cn, d_out, out_stride):
        ow, oh = C.c_int(), C.c_int()
        self._check(self.lib.vs_azc_apply_dev(self.h, d_in, w, h, stride, cn, d_out, out_stride,
                                              C.byref(ow), C.byref(oh)))
        return ow.value, oh.value

    def sync(self):
        self._check(self.lib.vs_azc_sync(self.h))

    def worker_times(self):
        """(frames, s without a frame, s waiting for masks, s in the contour logic, s queueing / publishing - summed over the workers;
        batches, s from launches to masks, s from masks to the crop launch - summed over the batches; s the caller waited for a slot)"""
        out = (C.c_double * 9)()
        self._check(self.lib.vs_azc_worker_times(self.h, out))
        return tuple(out)

    def info(self):
        info = np.zeros(8, np.int32)
        self._check(self.lib.vs_azc_get_info(self.h, _p(info, i32p)))
        return info


class Config:
    """The config layer of the C ABI (vs_config_*): config.yaml of the reference's example mains, read with the
    conversions of cv::FileNode (examples/vs.cpp:50-168, examples/vsg.cpp:1007-1112).  Host only."""

    KINDS = ("none", "int", "real", "string", "map", "seq")

    def __init__(self, vs, path=None, text=None):
        self.vs = vs
        self.lib = vs.lib
        h = C.c_void_p()
        if path is not None:
            vs.check(self.lib.vs_config_open(os.fsencode(path), C.byref(h)))
        else:
            raw = text.encode() if isinstance(text, str) else bytes(text)
            vs.check(self.lib.vs_config_parse(raw, len(raw), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.vs_config_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kind(self, key):
        return self.KINDS[self.lib.vs_config_kind(self.h, key.encode())]

    def size(self, key):
        return self.lib.vs_config_size(self.h, key.encode())

    def get_int(self, key):
        v = C.c_int32()
        self.vs.check(self.lib.vs_config_get_int(self.h, key.encode(), C.byref(v)))
        return v.value

    def get_bool(self, key):
        return self.get_int(key) != 0

    def get_double(self, key):
        v = C.c_double()
        self.vs.check(self.lib.vs_config_get_double(self.h, key.encode(), C.byref(v)))
        return v.value

    def get_float(self, key):
        v = C.c_float()
        self.vs.check(self.lib.vs_config_get_float(self.h, key.encode(), C.byref(v)))
        return v.value

    def get_string(self, key):
        buf = C.create_string_buffer(4096)
        self.vs.check(self.lib.vs_config_get_string(self.h, key.encode(), buf, len(buf)))
        return buf.value.decode()

    def get_seq(self, key):
        out = []
        for i in range(self.size(key) if self.kind(key) == "seq" else 0):
            v = C.c_double()
            self.vs.check(self.lib.vs_config_seq_get_double(self.h, key.encode(), i, C.byref(v)))
            out.append(v.value)
        return out

    def _read(self, fn, p, section, zero_missing):
        present = C.c_int32()
        self.vs.check(fn(self.h, section.encode(), int(zero_missing), C.byref(p), C.byref(present)))
        return p, bool(present.value)

    def stab_params(self, section="stabilizer", zero_missing=False, base=None):
        return self._read(self.lib.vs_config_read_stab, base or self.vs.params(), section, zero_missing)

    def roll_params(self, section="roll_correction", zero_missing=False, base=None):
        return self._read(self.lib.vs_config_read_roll, base or self.vs.roll_params(), section, zero_missing)

    def enh_params(self, section="enhancer", zero_missing=False, base=None):
        return self._read(self.lib.vs_config_read_enh, base or Enhancer.default_params(self.vs), section, zero_missing)

    @staticmethod
    def mtime(vs, path):
        v = C.c_int64()
        vs.check(vs.lib.vs_config_mtime(os.fsencode(path), C.byref(v)))
        return v.value


class Enhancer:
    """C-ABI mirror of vs::Enhancer::enhanceImage (Enhancer.cpp:138-239)."""

    CVT = dict(bgr2hsv=0, hsv2bgr=1, bgr2lab=2, lab2bgr=3)

    def __init__(self, vs, device=0):
        self.vs = vs
        self.lib = vs.lib
        h = C.c_void_p()
        vs.check(self.lib.vs_enh_create(device, C.byref(h)))
        self.h = h

    @staticmethod
    def default_params(vs, **kw):
        p = VsEnhParams()
        vs.lib.vs_enh_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def close(self):
        if self.h:
            self.lib.vs_enh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        if status != 0:
            raise VsError("%s: %s" % (self.lib.vs_status_string(status).decode(),
                                      (self.lib.vs_enh_last_error(self.h) or b"").decode()))

    def apply(self, frame, params):
        frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        out = np.empty_like(frame)
        self._check(self.lib.vs_enh_apply(self.h, C.byref(params), _p(frame, u8p), w, h, w * 3, _p(out, u8p), w * 3))
        return out

    def apply_dev(self, params, d_in, w, h, stride, d_out, out_stride):
        self._check(self.lib.vs_enh_apply_dev(self.h, C.byref(params), d_in, w, h, stride, d_out, out_stride))

    def apply_yuv_dev(self, params, yuv_fmt, surface, w, h, layout=None, out_layout=None, out_size=None, in_place=False, fill=0xA5):
        """vs_enh_apply_yuv_dev on one surface: a packed frame or a flat buffer in `layout` (VsLib.cvt_yuv_to_rgb).  The result lies
        in `out_layout` (default: the source's) in a buffer of out_size bytes prefilled with `fill`, or - in_place - in the source's
        own device buffer.  -> the packed (rows, w) surface, or with a layout the flat buffer, in the format's dtype."""
        f = PIXFMT[yuv_fmt]
        src = np.ascontiguousarray(surface)
        out_layout = out_layout or layout
        lin = I420LayoutC(*(layout or (f.sample_bytes * w, 0, 0, 0)))
        lout = I420LayoutC(*(out_layout or (f.sample_bytes * w, 0, 0, 0)))
        size = src.nbytes if in_place else out_size or yuv_surface_bytes(yuv_fmt, w, h, *(out_layout or ()))
        d_in = DevBuf.from_array(self.vs, src)
        d_out = d_in if in_place else DevBuf.from_array(self.vs, np.full(size, fill, np.uint8))
        try:
            self._check(self.lib.vs_enh_apply_yuv_dev(self.h, C.byref(params), yuv_fmt, d_in.ptr, C.byref(lin), d_out.ptr, C.byref(lout), w, h))
            self.sync()
            out = d_out.download((size,), np.uint8).view(fmt_dtype(yuv_fmt))
        finally:
            d_in.free()
            d_out.free()
        return out if out_layout else out.reshape(fmt_frame_rows(yuv_fmt, h), w)

    def apply_yuv_batch_dev(self, params, yuv_fmt, surfaces, w, h, layout=None, out_layout=None, out_size=None, in_place=False, fill=0xA5,
                            raw=False):
        """vs_enh_apply_yuv_batch_dev on a list of up to 32 surfaces of one geometry (each as for apply_yuv_dev) -> a list: per surface
        the packed (rows, w) surface or, with a layout, the flat buffer, in the format's dtype.  raw=True: the whole destination as
        bytes instead - out_size + 16 of them prefilled with `fill` (in_place: the source's buffer and 16 bytes of `fill` behind it)."""
        f = PIXFMT[yuv_fmt]
        srcs = [np.ascontiguousarray(s) for s in surfaces]
        n = len(srcs)
        out_layout = out_layout or layout
        lin = I420LayoutC(*(layout or (f.sample_bytes * w, 0, 0, 0)))
        lout = I420LayoutC(*(out_layout or (f.sample_bytes * w, 0, 0, 0)))
        guard = np.full(16, fill, np.uint8)
        d_in = [DevBuf.from_array(self.vs, np.concatenate([s.reshape(-1).view(np.uint8), guard]) if in_place else s) for s in srcs]
        size = srcs[0].nbytes if in_place else out_size or yuv_surface_bytes(yuv_fmt, w, h, *(out_layout or ()))
        d_out = d_in if in_place else [DevBuf.from_array(self.vs, np.full(size + 16, fill, np.uint8)) for _ in range(n)]
        try:
            self._check(self.lib.vs_enh_apply_yuv_batch_dev(self.h, C.byref(params), yuv_fmt, _ptr_array(d_in), C.byref(lin), _ptr_array(d_out),
                                                            C.byref(lout), n, w, h))
            self.sync()
            outs = [d.download((size + 16,), np.uint8) for d in d_out]
        finally:
            for d in d_in + ([] if in_place else d_out):
                d.free()
        if not raw:
            outs = [o[:size].view(fmt_dtype(yuv_fmt)) for o in outs]
            if not out_layout:
                outs = [o.reshape(fmt_frame_rows(yuv_fmt, h), w) for o in outs]
        return outs

    def last_fused(self):
        return self.lib.vs_enh_last_fused(self.h)

    def set_yuv_colorimetry(self, colorimetry=None):
        """vs_enh_set_yuv_colorimetry: the colour space of apply_yuv_dev / apply_yuv_batch_dev; None = the default."""
        self._check(self.lib.vs_enh_set_yuv_colorimetry(self.h, _cs_ref(colorimetry)))

    def apply_batch_dev(self, params, d_ins, d_outs, w, h, stride, out_stride):
        n = len(d_ins)
        a = (C.c_void_p * n)(*[C.c_void_p(int(x)) for x in d_ins])
        b = (C.c_void_p * n)(*[C.c_void_p(int(x)) for x in d_outs])
        self._check(self.lib.vs_enh_apply_batch_dev(self.h, C.byref(params), a, b, n, w, h, stride, out_stride))

    def sync(self):
        self._check(self.lib.vs_enh_sync(self.h))

    def passes(self):
        return self.lib.vs_enh_last_passes(self.h)

    def cvt_color(self, code, px):
        """px: (n,3) uint8 host array -> converted (n,3) array (through device buffers)."""
        px = np.ascontiguousarray(px, np.uint8)
        n = px.shape[0]
        d_in, d_out = DevBuf(self.vs, n * 3), DevBuf(self.vs, n * 3)
        d_in.upload(px)
        self._check(self.lib.vs_enh_cvt_color(self.h, self.CVT[code], d_in.ptr, d_out.ptr, n))
        self.sync()
        return d_out.download((n, 3), np.uint8)

    def gaussian_blur(self, frame, sigma):
        frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        d_in, d_out = DevBuf(self.vs, frame.nbytes), DevBuf(self.vs, frame.nbytes)
        d_in.upload(frame)
        self._check(self.lib.vs_enh_gaussian_blur(self.h, d_in.ptr, w * 3, w, h, sigma, d_out.ptr, w * 3))
        self.sync()
        return d_out.download(frame.shape, np.uint8)


class RollCorrection:
    """C-ABI mirror of vs::RollCorrection::autoCorrectRoll (RollCorrection.cpp:16-155)."""

    def __init__(self, vs, params, device=0):
        self.vs = vs
        self.lib = vs.lib
        h = C.c_void_p()
        vs.check(self.lib.vs_roll_create(C.byref(params), device, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.vs_roll_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        if status != 0:
            raise VsError("%s: %s" % (self.lib.vs_status_string(status).decode(),
                                      (self.lib.vs_roll_last_error(self.h) or b"").decode()))

    def correct(self, frame):
        frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        out = np.empty_like(frame)
        self._check(self.lib.vs_roll_correct(self.h, _p(frame, u8p), w, h, w * 3, _p(out, u8p), w * 3))
        return out

    def correct_dev(self, d_in, w, h, stride, d_out, out_stride):
        self._check(self.lib.vs_roll_correct_dev(self.h, d_in, w, h, stride, d_out, out_stride))

    def correct_nv12_dev_n(self, d_ins, w, h, pitch, d_outs, out_pitch, uv_offset=0, out_uv_offset=0):
        """n surfaces in call order (lists of device pointers), one trip through the binding."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        self._check(self.lib.vs_roll_correct_nv12_dev_n(self.h, a, b, n, w, h, pitch, uv_offset, out_pitch, out_uv_offset))

    def correct_nv12_dev(self, d_in, w, h, pitch, d_out, out_pitch, uv_offset=0, out_uv_offset=0):
        """Asynchronous (vs_roll_correct_nv12_dev): the result is complete after sync()."""
        self._check(self.lib.vs_roll_correct_nv12_dev(self.h, d_in, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset))

    def correct_p010_dev_n(self, d_ins, w, h, pitch, d_outs, out_pitch, uv_offset=0, out_uv_offset=0):
        """n P010 surfaces in call order (lists of device pointers), one trip through the binding."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        self._check(self.lib.vs_roll_correct_p010_dev_n(self.h, a, b, n, w, h, pitch, uv_offset, out_pitch, out_uv_offset))

    def correct_p010_dev(self, d_in, w, h, pitch, d_out, out_pitch, uv_offset=0, out_uv_offset=0):
        """correct_nv12_dev for a P010 surface (vs_roll_correct_p010_dev): pitches and offsets in bytes, even."""
        self._check(self.lib.vs_roll_correct_p010_dev(self.h, d_in, w, h, pitch, uv_offset, d_out, out_pitch, out_uv_offset))

    def correct_i420_dev(self, fmt, d_in, w, h, lin, d_out, lout):
        """correct_nv12_dev for a planar surface (vs_roll_correct_i420_dev): fmt any three-plane format (FMT_I420 ... FMT_I412), lin / lout:
        i420_layout()."""
        self._check(self.lib.vs_roll_correct_i420_dev(self.h, fmt, d_in, w, h, C.byref(lin), d_out, C.byref(lout)))

    def correct_i420_dev_n(self, fmt, d_ins, w, h, lin, d_outs, lout):
        """n planar surfaces in call order (lists of device pointers), one trip through the binding."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        self._check(self.lib.vs_roll_correct_i420_dev_n(self.h, fmt, a, b, n, w, h, C.byref(lin), C.byref(lout)))

    def correct_rgb_dev(self, fmt, d_in, w, h, stride, d_out, out_stride):
        """correct_nv12_dev for an interleaved colour frame (vs_roll_correct_rgb_dev): fmt FMT_BGR8, FMT_RGB8, FMT_BGRA8 or FMT_RGBA8."""
        self._check(self.lib.vs_roll_correct_rgb_dev(self.h, fmt, d_in, w, h, stride, d_out, out_stride))

    def correct_rgb_dev_n(self, fmt, d_ins, w, h, stride, d_outs, out_stride):
        n = len(d_ins)
        a = (C.c_void_p * max(1, n))(*d_ins)
        b = (C.c_void_p * max(1, n))(*d_outs)
        self._check(self.lib.vs_roll_correct_rgb_dev_n(self.h, fmt, a, b, n, w, h, stride, out_stride))

    def sync(self):
        self._check(self.lib.vs_roll_sync(self.h))

    def state(self):
        s, d = C.c_double(), C.c_double()
        n, u = C.c_int32(), C.c_int32()
        self._check(self.lib.vs_roll_get_state(self.h, C.byref(s), C.byref(d), C.byref(n), C.byref(u)))
        return s.value, d.value, n.value, u.value


class Stabilizer:
    """One video stream: the C-ABI mirror of vs::Stabilizer (Stabilizer.h:177-198)."""

    def __init__(self, vs, params, device=0):
        self.vs = vs
        self.lib = vs.lib
        h = C.c_void_p()
        vs.check(self.lib.vs_stab_create(C.byref(params), device, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.vs_stab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _geom(self, frame, fmt):
        """(w, h, bytes per pixel of the first plane) of a frame array of format fmt."""
        w = frame.shape[1]
        return w, fmt_picture_rows(fmt, frame.shape[0]), fmt_px_bytes(fmt)

    def out_shape(self, w, h, fmt):
        ow, oh = C.c_int32(), C.c_int32()
        self.vs.check(self.lib.vs_stab_out_size(self.h, w, h, C.byref(ow), C.byref(oh)), self.h)
        if fmt in FMT_CHROMA_SHIFTS or fmt_420(fmt):
            return (fmt_frame_rows(fmt, oh.value), ow.value)
        if FMT_CHANNELS[fmt] > 1:
            return (oh.value, ow.value, FMT_CHANNELS[fmt])
        return (oh.value, ow.value)

    def push(self, frame, fmt=FMT_BGR8, out=None):
        """stabilize(frame): returns the stabilized frame or None (warm-up).  `out`: a caller's array for the result (for
        instance page-locked: HostBuf), else a new one."""
        frame = np.ascontiguousarray(frame)
        w, h, cn = self._geom(frame, fmt)
        if out is None:
            out = np.zeros(self.out_shape(w, h, fmt), fmt_dtype(fmt))
        produced = C.c_int32(0)
        self.vs.check(self.lib.vs_stab_push(self.h, _p(frame, u8p), w, h, w * cn, fmt, _p(out, u8p),
                                            out.shape[1] * cn, C.byref(produced)), self.h)
        return out if produced.value else None

    def flush(self, like, fmt=FMT_BGR8):
        w, h, cn = self._geom(like, fmt)
        out = np.zeros(self.out_shape(w, h, fmt), fmt_dtype(fmt))
        produced = C.c_int32(0)
        self.vs.check(self.lib.vs_stab_flush(self.h, _p(out, u8p), out.shape[1] * cn, C.byref(produced)), self.h)
        return out if produced.value else None

    def set_host_pipeline(self, on=True):
        self.vs.check(self.lib.vs_stab_set_host_pipeline(self.h, int(on)), self.h)

    def push_dev(self, d_in, w, h, stride, fmt, d_out, out_stride):
        produced = C.c_int32(0)
        self.vs.check(self.lib.vs_stab_push_dev(self.h, d_in, w, h, stride, fmt, d_out, out_stride,
                                                C.byref(produced)), self.h)
        return produced.value

    def push_dev_n(self, d_ins, w, h, stride, fmt, d_outs, out_stride):
        """len(d_ins) consecutive pushes in one call; the j-th result that becomes due goes to d_outs[j].  Returns how many did."""
        n = len(d_ins)
        a = (C.c_void_p * n)(*d_ins)
        b = (C.c_void_p * n)(*d_outs)
        produced = C.c_int32(0)
        self.vs.check(self.lib.vs_stab_push_dev_n(self.h, a, n, w, h, stride, fmt, b, out_stride, C.byref(produced)), self.h)
        return produced.value

    def flush_dev(self, d_out, out_stride):
        produced = C.c_int32(0)
        self.vs.check(self.lib.vs_stab_flush_dev(self.h, d_out, out_stride, C.byref(produced)), self.h)
        return produced.value

    def sync(self):
        self.vs.check(self.lib.vs_stab_sync(self.h), self.h)

    def clean(self):
        self.vs.check(self.lib.vs_stab_clean(self.h), self.h)

    def set_batch(self, frames):
        self.vs.check(self.lib.vs_stab_set_batch(self.h, int(frames)), self.h)

    def set_nv12_layout(self, in_uv_offset=0, out_uv_offset=0):
        self.vs.check(self.lib.vs_stab_set_nv12_layout(self.h, in_uv_offset, out_uv_offset), self.h)

    def set_i420_layout(self, in_u_off=0, in_v_off=0, in_c_pitch=0, out_u_off=0, out_v_off=0, out_c_pitch=0):
        """Plane offsets (bytes behind the Y pointer) and chroma pitch (bytes) of the I420 / I010 / I012 surfaces pushed / filled;
        0 = packed default."""
        self.vs.check(self.lib.vs_stab_set_i420_layout(self.h, in_u_off, in_v_off, in_c_pitch, out_u_off, out_v_off, out_c_pitch), self.h)

    def set_yuv_crop_zoom(self, on=True):
        """vs_stab_set_yuv_crop_zoom: crop_n_zoom with a border_size on NV12 / P010 / three-plane streams (off: refused)."""
        self.vs.check(self.lib.vs_stab_set_yuv_crop_zoom(self.h, int(on)), self.h)

    def set_yuv_border_pad(self, on=True, fill=None):
        """vs_stab_set_yuv_border_pad: border_size without crop_n_zoom on NV12 / P010 / three-plane streams (off: refused).
        fill: (y, u, v) samples as they lie in memory; None: the format's video black."""
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        self.vs.check(self.lib.vs_stab_set_yuv_border_pad(self.h, int(on), c), self.h)

    def set_yuv_edge_fill(self, on=True, fill=None):
        """vs_stab_set_yuv_edge_fill: the warps of the stream's unpadded YUV surfaces read a colour outside the picture instead of 0
        (green).  fill: (y, u, v) samples as they lie in memory; None: the format's video black."""
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        self.vs.check(self.lib.vs_stab_set_yuv_edge_fill(self.h, int(on), c), self.h)

    def set_yuv_fade(self, on=True, fill=None):
        """vs_stab_set_yuv_fade: border_size with borderType "fade" on NV12 / P010 / three-plane streams (off: refused).
        fill: (y, u, v) samples as they lie in memory; None: the format's video black.  Every accepted call drops the history."""
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        self.vs.check(self.lib.vs_stab_set_yuv_fade(self.h, int(on), c), self.h)

    def set_zero_copy(self, on=True):
        self.vs.check(self.lib.vs_stab_set_zero_copy(self.h, int(on)), self.h)

    def set_warp_batch(self, frames):
        self.vs.check(self.lib.vs_stab_set_warp_batch(self.h, int(frames)), self.h)

    def set_profiling(self, mode):
        self.vs.check(self.lib.vs_stab_set_profiling(self.h, int(mode)), self.h)

    def stage_times(self):
        """(total_ms[STAGE_COUNT], launches[STAGE_COUNT]) accumulated since the last call (synchronises)."""
        ms = (C.c_double * STAGE_COUNT)()
        n = (C.c_int64 * STAGE_COUNT)()
        self.vs.check(self.lib.vs_stab_get_stage_times(self.h, ms, n), self.h)
        return list(ms), list(n)

    def counters(self):
        c = VsCounters()
        self.vs.check(self.lib.vs_stab_get_counters(self.h, C.byref(c)), self.h)
        return c

    def debug(self):
        d = VsDebugFrame()
        self.vs.check(self.lib.vs_stab_get_debug(self.h, C.byref(d)), self.h)
        return d

    def canvas_info(self):
        info = np.zeros(8, np.int32)
        self.vs.check(self.lib.vs_stab_canvas_info(self.h, info.ctypes.data_as(C.POINTER(C.c_int32))), self.h)
        return info

    def debug_arrays(self):
        d = self.debug()
        prev = np.zeros((max(d.n_prev, 1), 2), np.float32)
        cur = np.zeros((max(d.n_prev, 1), 2), np.float32)
        st = np.zeros(max(d.n_prev, 1), np.uint8)
        inl = np.zeros(max(d.n_valid, 1), np.uint8)
        det = np.zeros((max(d.n_detected, 1), 2), np.float32)
        aw, ah = C.c_int32(), C.c_int32()
        # the analysis size first (drone mode can analyse images larger than any fixed buffer), then the arrays
        self.vs.check(self.lib.vs_stab_get_debug_arrays(self.h, None, None, None, None, None, None,
                                                        C.byref(aw), C.byref(ah)), self.h)
        gray = np.zeros(max(aw.value * ah.value, 1), np.uint8)
        self.vs.check(self.lib.vs_stab_get_debug_arrays(self.h, _p(prev, f32p), _p(cur, f32p), _p(st, u8p),
                                                        _p(inl, u8p), _p(det, f32p), _p(gray, u8p),
                                                        C.byref(aw), C.byref(ah)), self.h)
        return dict(prev=prev[:d.n_prev], curr=cur[:d.n_prev], status=st[:d.n_prev], inliers=inl[:d.n_valid],
                    detected=det[:d.n_detected] if d.detected else det[:0],
                    gray=gray[:aw.value * ah.value].reshape(ah.value, aw.value))


class Batch:
    """vs_batch: n_streams streams of one device scheduled together (one launch per stage over the frames of all of them)."""

    def __init__(self, vs, params, n_streams, frames_per_step, device=0):
        """params: one VsParams for all streams, or a list of n_streams of them (vs_batch_create_params)."""
        self.vs, self.lib, self.n = vs, vs.lib, n_streams
        h = C.c_void_p()
        if isinstance(params, (list, tuple)):
            assert len(params) == n_streams
            arr = (VsParams * n_streams)(*params)
            vs.check(self.lib.vs_batch_create_params(device, n_streams, arr, frames_per_step, C.byref(h)))
        else:
            vs.check(self.lib.vs_batch_create(device, n_streams, C.byref(params), frames_per_step, C.byref(h)))
        self.h = h
        self._produced = (C.c_int32 * n_streams)()

    def _check(self, status):
        if status != 0:
            msg = self.lib.vs_status_string(status).decode()
            raise VsError("%s: %s" % (msg, (self.lib.vs_batch_last_error(self.h) or b"").decode()))

    def close(self):
        if self.h:
            self.lib.vs_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self, i):
        """Member i as a Stabilizer view (getters only; it is not closed through the view)."""
        s = Stabilizer.__new__(Stabilizer)
        s.vs, s.lib = self.vs, self.lib
        s.h = C.c_void_p(self.lib.vs_batch_stream(self.h, i))
        s.close = lambda: None
        return s

    def set_zero_copy(self, on=True):
        self._check(self.lib.vs_batch_set_zero_copy(self.h, int(on)))

    def set_nv12_layout(self, in_uv_offset=0, out_uv_offset=0):
        self._check(self.lib.vs_batch_set_nv12_layout(self.h, in_uv_offset, out_uv_offset))

    def set_i420_layout(self, in_u_off=0, in_v_off=0, in_c_pitch=0, out_u_off=0, out_v_off=0, out_c_pitch=0):
        self._check(self.lib.vs_batch_set_i420_layout(self.h, in_u_off, in_v_off, in_c_pitch, out_u_off, out_v_off, out_c_pitch))

    def set_yuv_crop_zoom(self, on=True):
        self._check(self.lib.vs_batch_set_yuv_crop_zoom(self.h, int(on)))

    def set_yuv_border_pad(self, on=True, fill=None):
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        self._check(self.lib.vs_batch_set_yuv_border_pad(self.h, int(on), c))

    def set_yuv_edge_fill(self, on=True, fill=None):
        c = C.byref(VsYuvFill(*fill, 0)) if fill is not None else None
        self._check(self.lib.vs_batch_set_yuv_edge_fill(self.h, int(on), c))

    def push_dev(self, d_frames, w, h, stride, fmt, d_outs, out_stride):
        """d_frames / d_outs: one device pointer per stream (None: no frame for that stream).  Returns produced[]."""
        fr = (C.c_void_p * self.n)(*[C.c_void_p(p) if p else None for p in d_frames])
        ou = (C.c_void_p * self.n)(*[C.c_void_p(p) if p else None for p in d_outs])
        self._check(self.lib.vs_batch_push_dev(self.h, fr, w, h, stride, fmt, ou, out_stride, self._produced))
        return list(self._produced)

    def pointer_array(self, ptrs):
        """A reusable argument of push_dev_arrays: one device pointer per stream."""
        return (C.c_void_p * self.n)(*[C.c_void_p(p) if p else None for p in ptrs])

    def push_dev_arrays(self, fr, w, h, stride, fmt, ou, out_stride):
        """push_dev with prepared pointer arrays (pointer_array): no per-call marshalling."""
        self._check(self.lib.vs_batch_push_dev(self.h, fr, w, h, stride, fmt, ou, out_stride, self._produced))

    def flush_dev(self, d_outs, out_stride):
        ou = (C.c_void_p * self.n)(*[C.c_void_p(p) if p else None for p in d_outs])
        self._check(self.lib.vs_batch_flush_dev(self.h, ou, out_stride, self._produced))
        return list(self._produced)

    def sync(self):
        self._check(self.lib.vs_batch_sync(self.h))


_cached = None


def load(path=None):
    """Load libvideo-stab.so; raises if it has not been built (no fallback)."""
    global _cached
    if _cached is None:
        # (VS_LAB=1 VS_LIB_PATH=...: a measurement build of the library, scratch/blend_lab.sh)
        path = path or (os.environ.get("VS_LIB_PATH") if os.environ.get("VS_LAB") == "1" else None) or LIB_PATH
        if not os.path.exists(path):
            raise VsError("libvideo-stab.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _cached = VsLib(C.CDLL(path))
    return _cached
