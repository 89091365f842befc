// The compositing stages as operators (include/vs_stab.h): vs_op_copy_make_border, vs_op_fade_blend, vs_op_fade_update, the
// vs_op_canvas_* object and the colour conversions vs_op_cvt_yuv_to_rgb[_cs] / vs_op_cvt_rgb_to_yuv[_cs], with the integers of
// their colour spaces (cvt_resolve, vs_cvt_coefficients, vs_cvt_colorimetry_guess), and the conversion between YUV surface formats
// vs_op_cvt_yuv_to_yuv with vs_yuv_surface_layout, and between them and the packed 4:2:2 capture formats: vs_op_cvt_packed_to_yuv,
// vs_op_cvt_yuv_to_packed with vs_packed_layout.  Nothing is computed here: each
// entry checks its arguments and calls what the pipeline calls (launch_make_border, launch_fade_blend, launch_fade_update of
// k_traj.hip; canvas_apply of k_canvas.hip; launch_cvt_* of k_cvt.hip; launch_cvt_yuv_to_yuv of k_yuvcvt.hip;
// launch_cvt_packed_to_yuv, launch_cvt_yuv_to_packed of k_yuvpacked.hip).
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cvt_px.h"
#include "stab_internal.h"

using namespace vsd;

namespace {

int refuse(int code, const char* why) {
    set_last_error(why);
    return code;
}

// The RGB side of a conversion: the format, the n pointers, the pitch.
int cvt_check_rgb(const char* call, int rgb_fmt, const void* const* rgb, size_t rgb_stride, int n, int w, const PixFmt** rf, std::string* msg) {
    const PixFmt* f = pixfmt(rgb_fmt);
    auto fail = [&](const std::string& what) { *msg = std::string(call) + ": " + what; return (int)VS_ERR_INVALID_ARG; };
    if (!f || !f->border_modes)       // the interleaved colour formats: BGR8, BGRA8, RGBA8, RGB8
        return fail((f ? std::string(f->name) : "format " + std::to_string(rgb_fmt)) + " is not an interleaved colour format (BGR8, RGB8, BGRA8, RGBA8)");
    if (!rgb) return fail(std::string(f->name) + ": null pointer");
    for (int k = 0; k < n; k++)
        if (!rgb[k]) return fail(std::string(f->name) + ": null pointer");
    if (rgb_stride < (size_t)w * f->cn) return fail(std::string(f->name) + ": the pitch must hold a row of the picture");
    *rf = f;
    return VS_OK;
}

// The packed 4:2:2 capture formats (enum vs_packed_fmt), one row per value: what include/vs_stab.h says of each.
struct PackedFmt {
    const char* name;
    int kind;           // PackedKind
    uint32_t sel;       // 8-bit orders: where Y0, U, Y1, V lie in a macropixel, a byte each
    int bits;           // of a value: 8; Y210 the whole word; v210 ten
    int align;          // what pointers and pitches must be multiples of
    const char* align_text;
    size_t row_bytes(int w) const { return kind == PACKED_V210 ? 16 * (((size_t)w + 5) / 6) : (size_t)w * (kind == PACKED_16 ? 4 : 2); }
    size_t default_pitch(int w) const { return kind == PACKED_V210 ? 128 * (((size_t)w + 47) / 48) : row_bytes(w); }
};
const PackedFmt PACKED_FMTS[] = {
    {"YUY2", PACKED_8, 0x03020100u, 8, 1, ""},
    {"UYVY", PACKED_8, 0x02030001u, 8, 1, ""},
    {"YVYU", PACKED_8, 0x01020300u, 8, 1, ""},
    {"Y210", PACKED_16, 0u, 16, 2, ": pointers and the pitch must be even (16-bit words)"},
    {"v210", PACKED_V210, 0u, 10, 4, ": pointers and the pitch must be multiples of 4 (32-bit words)"},
};

// The packed side of a conversion: the format, the geometry, the n pointers, the pitch (0 = the format's default; resolved into
// *pitch).  call: the entry point and the side, as for cvt_check_yuv.
int cvt_check_packed(const char* call, int packed_fmt, const void* const* ptrs, int n, int w, int h, size_t* pitch, const PackedFmt** pf, std::string* msg) {
    auto fail = [&](const std::string& what) { *msg = std::string(call) + ": " + what; return (int)VS_ERR_INVALID_ARG; };
    if (packed_fmt < VS_PACKED_YUY2 || packed_fmt > VS_PACKED_V210)
        return fail("packed format " + std::to_string(packed_fmt) + " is not a vs_packed_fmt (YUY2, UYVY, YVYU, Y210, v210)");
    const PackedFmt& f = PACKED_FMTS[packed_fmt];
    const std::string name = f.name;
    if (n < 1 || n > CVT_MAX_SURFACES) return fail(name + ": n must be 1 .. 32 surfaces");
    if (!ptrs) return fail(name + ": null pointer");
    uintptr_t ptr_bits = 0;
    for (int k = 0; k < n; k++) {
        if (!ptrs[k]) return fail(name + ": null pointer");
        ptr_bits |= (uintptr_t)ptrs[k];
    }
    if (w < 1 || h < 1 || w > 65536 || h > 65536) return fail(name + ": size out of range");
    if (w & 1) return fail(name + ": w must be even (two pixels share a chroma pair)");
    if (!*pitch) *pitch = f.default_pitch(w);
    if (*pitch < f.row_bytes(w)) return fail(name + ": the pitch must hold a row of the picture (" + std::to_string(f.row_bytes(w)) + " bytes)");
    if ((ptr_bits | *pitch) & (size_t)(f.align - 1)) return fail(name + f.align_text);
    *pf = &f;
    return VS_OK;
}

// What vs_op_cvt_yuv_to_yuv refuses about its descriptor, in its words.  pair: the call and both formats.
int cvt_check_yuv_desc(const std::string& pair, const vs_yuv_cvt_desc* desc, std::string* msg) {
    auto bad = [&](const char* field, int32_t v, const char* want) {
        *msg = pair + "descriptor: " + field + " = " + std::to_string(v) + " " + want;
        return (int)VS_ERR_INVALID_ARG;
    };
    if (desc->depth_down < VS_YUV_DEPTH_TRUNCATE || desc->depth_down > VS_YUV_DEPTH_ROUND)
        return bad("depth_down", desc->depth_down, "is not a vs_yuv_depth_down (0, 1)");
    if (desc->chroma_down < VS_CVT_CHROMA_TOPLEFT || desc->chroma_down > VS_CVT_CHROMA_MEAN)
        return bad("chroma_down", desc->chroma_down, "is not a vs_cvt_chroma (0, 1)");
    for (int k = 0; k < 2; k++)
        if (desc->reserved[k] != 0) return bad(k ? "reserved[1]" : "reserved[0]", desc->reserved[k], "must be 0");
    return VS_OK;
}

// ... and about its pointers: no source is a destination
int cvt_check_distinct(const std::string& pair, const void* const* d_src, void* const* d_dst, int n, std::string* msg) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
            if (d_src[i] == d_dst[j]) {
                *msg = pair + "source surface " + std::to_string(i) + " is destination surface " + std::to_string(j) + " (surfaces may not overlap)";
                return (int)VS_ERR_INVALID_ARG;
            }
    return VS_OK;
}

// The depth step between a packed format and a surface format.  A v210 field holds ten bits: a 10-bit low-bit source, whose word
// is otherwise copied, clamps to them.
YuvDepth packed_depth(const PackedFmt& pf, const PixFmt& f, bool to_packed, bool round) {
    if (!to_packed) return yuv_depth_bits(pf.bits, false, yuv_value_bits(f), round);
    YuvDepth k = yuv_depth_bits(yuv_value_bits(f), yuv_low_bit(f), pf.bits, round);
    if (pf.kind == PACKED_V210) k.in_max = std::min(k.in_max, yuv_low_bit(f) ? (1u << f.bits) - 1u : 0xffffu);
    return k;
}

}  // namespace

namespace vsd {

// The fifteen integers per (matrix, range), in the order of vs_cvt_coefficients.  (BT.601, limited): OpenCV's, not derived - they
// are cvt_coef_default() of cvt_px.h, and the zeros here are never read.  The other five: the rule of include/vs_stab.h - from Kr, Kb in exact rational arithmetic, scaled by 2^20, rounded half away from
// zero; tests/test_cvt_colorimetry_cpu.py recomputes them with fractions.Fraction and holds this table to the rule.
static const int32_t CVT_TABLE[3][2][15] = {
    {{0},
     {0, 1048576, 1470104, 748826, 360853, 1858077, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}},
    {{16, 1220945, 1879825, 558796, 223607, 2215014, 191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230},
     {0, 1048576, 1651297, 490864, 196424, 1945738, 222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074}},
    {{16, 1220945, 1760217, 682019, 196426, 2245811, 236572, 610567, 53402, -128614, -331937, 460551, 460551, -423510, -37041},
     {0, 1048576, 1546230, 599107, 172546, 1972791, 275461, 710935, 62181, -146413, -377875, 524288, 524288, -482120, -42168}},
};

int cvt_resolve(const char* call, const vs_cvt_colorimetry* cs, CvtCoef* k, std::string* msg) {
    static const vs_cvt_colorimetry dflt = {VS_CVT_MATRIX_BT601, VS_CVT_RANGE_LIMITED, VS_CVT_CHROMA_TOPLEFT, 0};
    if (!cs) cs = &dflt;
    auto fail = [&](const char* field, int32_t v, const char* want) {
        *msg = std::string(call) + ": colorimetry: " + field + " = " + std::to_string(v) + " " + want;
        return (int)VS_ERR_INVALID_ARG;
    };
    if (cs->matrix < VS_CVT_MATRIX_BT601 || cs->matrix > VS_CVT_MATRIX_BT2020) return fail("matrix", cs->matrix, "is not a vs_cvt_matrix (0 .. 2)");
    if (cs->range < VS_CVT_RANGE_LIMITED || cs->range > VS_CVT_RANGE_FULL) return fail("range", cs->range, "is not a vs_cvt_range (0, 1)");
    if (cs->chroma_down < VS_CVT_CHROMA_TOPLEFT || cs->chroma_down > VS_CVT_CHROMA_MEAN)
        return fail("chroma_down", cs->chroma_down, "is not a vs_cvt_chroma (0, 1)");
    if (cs->reserved != 0) return fail("reserved", cs->reserved, "must be 0");
    static_assert(sizeof(CvtCoef) == 16 * sizeof(int32_t) && offsetof(CvtCoef, mean) == 15 * sizeof(int32_t), "fifteen integers and the chroma rule");
    *k = cvt_coef_default();
    if (cs->matrix != VS_CVT_MATRIX_BT601 || cs->range != VS_CVT_RANGE_LIMITED)
        memcpy(k, CVT_TABLE[cs->matrix][cs->range], 15 * sizeof(int32_t));
    k->mean = cs->chroma_down == VS_CVT_CHROMA_MEAN;
    return VS_OK;
}

int cvt_check_yuv(const char* call, int yuv_fmt, const void* const* surfaces, int n, const vs_i420_layout* lay, int w, int h, I420Layout* l,
                  std::string* msg) {
    const PixFmt* f = pixfmt(yuv_fmt);
    auto fail = [&](const std::string& what) { *msg = std::string(call) + ": " + what; return (int)VS_ERR_INVALID_ARG; };
    if (!f || f->kind == PIX_INTERLEAVED)
        return fail((f ? std::string(f->name) : "format " + std::to_string(yuv_fmt)) + " is not a YUV surface format (NV12, P010, I420 ... I412)");
    const std::string name = f->name;
    if (n < 1 || n > CVT_MAX_SURFACES) return fail(name + ": n must be 1 .. 32 surfaces");
    if (!surfaces || !lay) return fail(name + ": null pointer");
    uintptr_t ptr_bits = 0;
    for (int k = 0; k < n; k++) {
        if (!surfaces[k]) return fail(name + ": null pointer");
        ptr_bits |= (uintptr_t)surfaces[k];
    }
    const int sb = f->sample_bytes;
    if (w < 1 || h < 1 || w > 65536 || h > 65536) return fail(name + ": size out of range");
    if ((w & ((1 << f->sx) - 1)) || (h & ((1 << f->sy) - 1))) return fail(name + (f->sy ? ": w and h must be even" : ": w must be even"));
    if (lay->pitch < (size_t)w * sb) return fail(name + ": the pitch must hold a row of the picture");
    if (sb == 2 && ((ptr_bits | lay->pitch | lay->c_pitch | lay->u_off | lay->v_off) & 1))
        return fail(name + ": pointers, pitches and plane offsets must be even (16-bit samples)");
    const size_t rows = (size_t)h, crows = (size_t)(h >> f->sy), crow_bytes = f->chroma_row_bytes(w) * (f->luma_uv() ? 2 : 1);
    if (f->luma_uv()) {
        if (lay->v_off) return fail(name + ": v_off must be 0 (U and V share one interleaved plane, at u_off)");
        if (lay->c_pitch && lay->c_pitch != lay->pitch) return fail(name + ": c_pitch must be 0 or the pitch (the interleaved plane has the luma pitch)");
        l->pitch = l->cpitch = lay->pitch;
        l->u = lay->u_off ? lay->u_off : rows * lay->pitch;
        l->v = l->u;
    } else {
        if (!lay->c_pitch && f->sx && (lay->pitch & (size_t)(2 * sb - 1)))
            return fail(name + (sb == 2 ? ": the default chroma pitch needs a pitch that is a multiple of 4" : ": the default chroma pitch needs an even pitch"));
        *l = i420_layout(lay->pitch, h, lay->u_off, lay->v_off, lay->c_pitch, f->sx, f->sy);
        if (l->cpitch < crow_bytes) return fail(name + ": the chroma pitch must hold a chroma row");
    }
    // the bytes a plane's samples span: every row but the last in full, the last up to its last sample
    const size_t y_end = (rows - 1) * l->pitch + (size_t)w * sb, c_span = (crows - 1) * l->cpitch + crow_bytes;
    if (l->u < y_end || (!f->luma_uv() && l->v < y_end)) return fail(name + ": the chroma planes must start behind the luma rows");
    if (!f->luma_uv() && std::max(l->u, l->v) < std::min(l->u, l->v) + c_span) return fail(name + ": the U and V planes overlap");
    return VS_OK;
}

}  // namespace vsd

struct vs_canvas_op {
    Canvas* canvas = nullptr;
    hipStream_t st = nullptr;
    TrajState* d_traj = nullptr;
    float* d_t = nullptr;
    TrajState h_traj;
};

extern "C" {

int vs_op_copy_make_border(const void* d_src, size_t src_stride, int w, int h, int cn, void* d_dst, size_t dst_stride, int b, int border,
                           void* stream) {
    if (!d_src || !d_dst) return refuse(VS_ERR_INVALID_ARG, "vs_op_copy_make_border: null pointer");
    if (cn != 1 && cn != 3 && cn != 4) return refuse(VS_ERR_INVALID_ARG, "vs_op_copy_make_border: cn must be 1, 3 or 4");
    if (w < 1 || h < 1 || w > 32767 || h > 32767 || b < 0 || b > 8192) return refuse(VS_ERR_INVALID_ARG, "vs_op_copy_make_border: size out of range");
    if (border < VS_BORDER_BLACK || border > VS_BORDER_WRAP) return refuse(VS_ERR_INVALID_ARG, "vs_op_copy_make_border: not a copyMakeBorder mode");
    if (src_stride < (size_t)w * cn || dst_stride < (size_t)(w + 2 * b) * cn) return refuse(VS_ERR_INVALID_ARG, "vs_op_copy_make_border: pitch below a row");
    VS_TRY(ensure_device());
    return launch_make_border((const uint8_t*)d_src, src_stride, w, h, cn, (uint8_t*)d_dst, dst_stride, b, border, (hipStream_t)stream);
}

int vs_op_fade_blend(const void* d_hist, void* d_frame, size_t bytes, float alpha, float beta, void* stream) {
    if (!d_hist || !d_frame) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_blend: null pointer");
    if (bytes < 1 || bytes > ((size_t)1 << 31)) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_blend: size out of range");
    if (((uintptr_t)d_hist | (uintptr_t)d_frame) & 3) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_blend: buffers must be 4-byte aligned");
    if (!(alpha >= 0.0f && alpha <= 1.0f && beta >= 0.0f && beta <= 1.0f)) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_blend: weights must be in [0,1]");
    VS_TRY(ensure_device());
    return launch_fade_blend((const uint8_t*)d_hist, (uint8_t*)d_frame, (bytes + 3) & ~(size_t)3, alpha, beta, (hipStream_t)stream);
}

int vs_op_fade_update(void* d_hist, const void* d_stab, size_t stab_stride, int row_bytes, int rows, void* stream) {
    if (!d_hist || !d_stab) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_update: null pointer");
    if (row_bytes < 1 || rows < 1 || rows > 65535) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_update: size out of range");
    if (stab_stride < (size_t)row_bytes) return refuse(VS_ERR_INVALID_ARG, "vs_op_fade_update: pitch below a row");
    VS_TRY(ensure_device());
    return launch_fade_update((uint8_t*)d_hist, (const uint8_t*)d_stab, stab_stride, row_bytes, rows, (hipStream_t)stream);
}

int vs_op_cvt_yuv_to_rgb_cs(int yuv_fmt, const void* const* d_surfaces, const vs_i420_layout* in, int rgb_fmt, void* const* d_rgb, size_t rgb_stride,
                            int n, int w, int h, const vs_cvt_colorimetry* cs, void* stream) {
    static const char call[] = "vs_op_cvt_yuv_to_rgb";       // refusals name the operator, with or without _cs
    I420Layout l;
    const PixFmt* rf = nullptr;
    CvtCoef k;
    std::string msg;
    if (cvt_check_yuv(call, yuv_fmt, d_surfaces, n, in, w, h, &l, &msg) != VS_OK || cvt_check_rgb(call, rgb_fmt, d_rgb, rgb_stride, n, w, &rf, &msg) != VS_OK ||
        cvt_resolve(call, cs, &k, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    VS_TRY(ensure_device());
    return launch_cvt_yuv_to_rgb(*pixfmt(yuv_fmt), d_surfaces, l, *rf, d_rgb, rgb_stride, n, w, h, k, (hipStream_t)stream);
}

int vs_op_cvt_rgb_to_yuv_cs(int rgb_fmt, const void* const* d_rgb, size_t rgb_stride, int yuv_fmt, void* const* d_surfaces, const vs_i420_layout* out,
                            int n, int w, int h, const vs_cvt_colorimetry* cs, void* stream) {
    static const char call[] = "vs_op_cvt_rgb_to_yuv";
    I420Layout l;
    const PixFmt* rf = nullptr;
    CvtCoef k;
    std::string msg;
    if (cvt_check_yuv(call, yuv_fmt, d_surfaces, n, out, w, h, &l, &msg) != VS_OK || cvt_check_rgb(call, rgb_fmt, d_rgb, rgb_stride, n, w, &rf, &msg) != VS_OK ||
        cvt_resolve(call, cs, &k, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    VS_TRY(ensure_device());
    return launch_cvt_rgb_to_yuv(*rf, d_rgb, rgb_stride, *pixfmt(yuv_fmt), d_surfaces, l, n, w, h, k, (hipStream_t)stream);
}

int vs_op_cvt_yuv_to_rgb(int yuv_fmt, const void* const* d_surfaces, const vs_i420_layout* in, int rgb_fmt, void* const* d_rgb, size_t rgb_stride,
                         int n, int w, int h, void* stream) {
    return vs_op_cvt_yuv_to_rgb_cs(yuv_fmt, d_surfaces, in, rgb_fmt, d_rgb, rgb_stride, n, w, h, nullptr, stream);
}

int vs_op_cvt_rgb_to_yuv(int rgb_fmt, const void* const* d_rgb, size_t rgb_stride, int yuv_fmt, void* const* d_surfaces, const vs_i420_layout* out,
                         int n, int w, int h, void* stream) {
    return vs_op_cvt_rgb_to_yuv_cs(rgb_fmt, d_rgb, rgb_stride, yuv_fmt, d_surfaces, out, n, w, h, nullptr, stream);
}

int vs_op_cvt_yuv_to_yuv(int src_fmt, const void* const* d_src, const vs_i420_layout* in, int dst_fmt, void* const* d_dst, const vs_i420_layout* out,
                         int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream) {
    static const char call[] = "vs_op_cvt_yuv_to_yuv";
    static const vs_yuv_cvt_desc dflt = {VS_YUV_DEPTH_TRUNCATE, VS_CVT_CHROMA_TOPLEFT, {0, 0}};
    I420Layout li, lo;
    std::string msg;
    // each side by the rules of the colour conversions; w and h are then multiples of 1 << sx, 1 << sy of the coarser side as well
    if (cvt_check_yuv("vs_op_cvt_yuv_to_yuv: source", src_fmt, d_src, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_yuv("vs_op_cvt_yuv_to_yuv: destination", dst_fmt, d_dst, n, out, w, h, &lo, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    const PixFmt &sf = *pixfmt(src_fmt), &df = *pixfmt(dst_fmt);
    const std::string pair = std::string(call) + ": source " + sf.name + ", destination " + df.name + ": ";
    if (!desc) desc = &dflt;
    if (cvt_check_distinct(pair, d_src, d_dst, n, &msg) != VS_OK || cvt_check_yuv_desc(pair, desc, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    VS_TRY(ensure_device());
    return launch_cvt_yuv_to_yuv(sf, d_src, li, df, d_dst, lo, n, w, h, yuv_depth(sf, df, desc->depth_down == VS_YUV_DEPTH_ROUND),
                                 desc->chroma_down == VS_CVT_CHROMA_MEAN, (hipStream_t)stream);
}

int vs_op_cvt_packed_to_yuv(int packed_fmt, const void* const* d_src, size_t src_pitch, int dst_fmt, void* const* d_dst, const vs_i420_layout* out,
                            int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream) {
    static const char call[] = "vs_op_cvt_packed_to_yuv";
    static const vs_yuv_cvt_desc dflt = {VS_YUV_DEPTH_TRUNCATE, VS_CVT_CHROMA_TOPLEFT, {0, 0}};
    const PackedFmt* pf = nullptr;
    I420Layout lo;
    std::string msg;
    if (cvt_check_packed("vs_op_cvt_packed_to_yuv: source", packed_fmt, d_src, n, w, h, &src_pitch, &pf, &msg) != VS_OK ||
        cvt_check_yuv("vs_op_cvt_packed_to_yuv: destination", dst_fmt, d_dst, n, out, w, h, &lo, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    const PixFmt& df = *pixfmt(dst_fmt);
    const std::string pair = std::string(call) + ": source " + pf->name + ", destination " + df.name + ": ";
    if (!desc) desc = &dflt;
    if (cvt_check_distinct(pair, d_src, d_dst, n, &msg) != VS_OK || cvt_check_yuv_desc(pair, desc, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    VS_TRY(ensure_device());
    return launch_cvt_packed_to_yuv(pf->kind, pf->sel, d_src, src_pitch, df, d_dst, lo, n, w, h,
                                    packed_depth(*pf, df, false, desc->depth_down == VS_YUV_DEPTH_ROUND), desc->chroma_down == VS_CVT_CHROMA_MEAN,
                                    (hipStream_t)stream);
}

int vs_op_cvt_yuv_to_packed(int src_fmt, const void* const* d_src, const vs_i420_layout* in, int packed_fmt, void* const* d_dst, size_t dst_pitch,
                            int n, int w, int h, const vs_yuv_cvt_desc* desc, void* stream) {
    static const char call[] = "vs_op_cvt_yuv_to_packed";
    static const vs_yuv_cvt_desc dflt = {VS_YUV_DEPTH_TRUNCATE, VS_CVT_CHROMA_TOPLEFT, {0, 0}};
    const PackedFmt* pf = nullptr;
    I420Layout li;
    std::string msg;
    if (cvt_check_yuv("vs_op_cvt_yuv_to_packed: source", src_fmt, d_src, n, in, w, h, &li, &msg) != VS_OK ||
        cvt_check_packed("vs_op_cvt_yuv_to_packed: destination", packed_fmt, d_dst, n, w, h, &dst_pitch, &pf, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    const PixFmt& sf = *pixfmt(src_fmt);
    const std::string pair = std::string(call) + ": source " + sf.name + ", destination " + pf->name + ": ";
    if (!desc) desc = &dflt;
    if (cvt_check_distinct(pair, d_src, d_dst, n, &msg) != VS_OK || cvt_check_yuv_desc(pair, desc, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    VS_TRY(ensure_device());
    return launch_cvt_yuv_to_packed(sf, d_src, li, pf->kind, pf->sel, d_dst, dst_pitch, n, w, h,
                                    packed_depth(*pf, sf, true, desc->depth_down == VS_YUV_DEPTH_ROUND), desc->chroma_down == VS_CVT_CHROMA_MEAN,
                                    (hipStream_t)stream);
}

int vs_packed_layout(int packed_fmt, int w, int h, size_t pitch, size_t* row_bytes, size_t* resolved_pitch, size_t* bytes) {
    // the rules are those of a conversion's side, asked about one surface at an address that no rule objects to
    static const void* const aligned_surface[1] = {(const void*)(uintptr_t)4096};
    const PackedFmt* pf = nullptr;
    std::string msg;
    if (cvt_check_packed("vs_packed_layout", packed_fmt, aligned_surface, 1, w, h, &pitch, &pf, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    if (row_bytes) *row_bytes = pf->row_bytes(w);
    if (resolved_pitch) *resolved_pitch = pitch;
    if (bytes) *bytes = (size_t)(h - 1) * pitch + pf->row_bytes(w);
    return VS_OK;
}

int vs_yuv_surface_layout(int fmt, int w, int h, const vs_i420_layout* lay, vs_i420_layout* resolved, size_t* bytes) {
    const PixFmt* f = pixfmt(fmt);
    vs_i420_layout tight = {0, 0, 0, 0};
    if (!lay && f && w > 0) {
        tight.pitch = (size_t)w * f->sample_bytes;
        lay = &tight;
    }
    // the rules are those of a conversion's side, asked about one surface at an address that no rule objects to
    static const void* const aligned_surface[1] = {(const void*)(uintptr_t)4096};
    I420Layout l;
    std::string msg;
    if (cvt_check_yuv("vs_yuv_surface_layout", fmt, aligned_surface, 1, lay ? lay : &tight, w, h, &l, &msg) != VS_OK)
        return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    if (resolved) {
        resolved->pitch = l.pitch;
        resolved->c_pitch = l.cpitch;
        resolved->u_off = l.u;
        resolved->v_off = f->luma_uv() ? 0 : l.v;       // NV12 / P010: one interleaved plane, at u_off
    }
    if (bytes) {
        const size_t crow_bytes = f->chroma_row_bytes(w) * (f->luma_uv() ? 2 : 1);
        *bytes = std::max(l.u, l.v) + (size_t)((h >> f->sy) - 1) * l.cpitch + crow_bytes;
    }
    return VS_OK;
}

int vs_cvt_coefficients(const vs_cvt_colorimetry* cs, int32_t out[16]) {
    if (!out) return refuse(VS_ERR_INVALID_ARG, "vs_cvt_coefficients: null pointer");
    CvtCoef k;
    std::string msg;
    if (cvt_resolve("vs_cvt_coefficients", cs, &k, &msg) != VS_OK) return refuse(VS_ERR_INVALID_ARG, msg.c_str());
    memcpy(out, &k, 15 * sizeof(int32_t));
    out[15] = 0;
    return VS_OK;
}

void vs_cvt_colorimetry_guess(int w, int h, vs_cvt_colorimetry* out) {
    (void)w;                          // the convention goes by the height alone
    if (!out) return;
    out->matrix = h > 576 ? VS_CVT_MATRIX_BT709 : VS_CVT_MATRIX_BT601;
    out->range = VS_CVT_RANGE_LIMITED;
    out->chroma_down = VS_CVT_CHROMA_TOPLEFT;
    out->reserved = 0;
}

int vs_op_canvas_create(vs_canvas_op** out) {
    if (!out) return refuse(VS_ERR_INVALID_ARG, "vs_op_canvas_create: null pointer");
    *out = nullptr;
    VS_TRY(ensure_device());
    vs_canvas_op* c = new (std::nothrow) vs_canvas_op();
    if (!c) return refuse(VS_ERR_HIP, "out of host memory");
    c->canvas = canvas_new();
    hipError_t e = c->canvas ? hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_traj, sizeof(TrajState));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_t, 4 * sizeof(float));
    if (e != hipSuccess) { set_last_error(hipGetErrorString(e)); vs_op_canvas_destroy(c); return VS_ERR_HIP; }
    *out = c;
    return VS_OK;
}

void vs_op_canvas_destroy(vs_canvas_op* c) {
    if (!c) return;
    if (c->st) (void)hipStreamSynchronize(c->st);
    canvas_delete(c->canvas);
    if (c->d_traj) (void)hipFree(c->d_traj);
    if (c->d_t) (void)hipFree(c->d_t);
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

int vs_op_canvas_info(const vs_canvas_op* c, int32_t info[8]) {
    if (!c || !info) return refuse(VS_ERR_INVALID_ARG, "vs_op_canvas_info: null pointer");
    canvas_info(c->canvas, info);
    return VS_OK;
}

int vs_op_canvas_apply(vs_canvas_op* c, const vs_params_c* params, const void* d_frame, size_t pitch, int w, int h, const float* t,
                       const float* transforms, int n, void* d_out, size_t out_pitch, int32_t* info8) {
    if (!c || !params || !d_frame || !t || !d_out || (n > 0 && !transforms)) return refuse(VS_ERR_INVALID_ARG, "vs_op_canvas_apply: null pointer");
    if (params->struct_size != (int32_t)sizeof(vs_params_c)) return refuse(VS_ERR_INVALID_ARG, "params: struct_size mismatch");
    if (w < 1 || h < 1 || w > 32767 || h > 32767 || n < 0) return refuse(VS_ERR_INVALID_ARG, "vs_op_canvas_apply: size out of range");
    if (pitch < (size_t)w * 3 || out_pitch < (size_t)w * 3) return refuse(VS_ERR_INVALID_ARG, "vs_op_canvas_apply: pitch below a row");
    const vs_params_c& p = *params;
    // the canvas rules of vs_stab_create (check_params)
    if (p.temporal_buffer_size < 0 || p.temporal_buffer_size > 256) return refuse(VS_ERR_INVALID_ARG, "temporalBufferSize must be in [0,256]");
    if (!(p.canvas_blend_weight >= 0.0f && p.canvas_blend_weight <= 1.0f)) return refuse(VS_ERR_UNSUPPORTED, "canvasBlendWeight must be in [0,1]");
    if (!(p.canvas_scale_factor > 0.0f && p.canvas_scale_factor <= 16.0f) || !(p.min_canvas_scale > 0.0f) || !(p.max_canvas_scale <= 16.0f))
        return refuse(VS_ERR_INVALID_ARG, "canvas scale factors must be in (0,16]");
    // every scale the call can choose: the factor as given, or (adaptive, :2281-2314) a value clamped to [min, max]
    const float scales[3] = {p.canvas_scale_factor, p.adaptive_canvas_size ? p.min_canvas_scale : p.canvas_scale_factor,
                             p.adaptive_canvas_size ? p.max_canvas_scale : p.canvas_scale_factor};
    for (float s : scales) {
        const float fw = w * s, fh = h * s;
        if (!(fw >= 1.0f && fw <= 65535.0f && fh >= 1.0f && fh <= 32767.0f))
            return refuse(VS_ERR_UNSUPPORTED, "virtual canvas: canvas size out of range (1..65535 x 1..32767)");
    }
    // the trajectory state as canvas_motion_kernel reads it: n, and the last TRAJ_RING transforms in their ring slots
    memset(&c->h_traj, 0, sizeof c->h_traj);
    c->h_traj.n = n;
    for (int i = n > TRAJ_RING ? n - TRAJ_RING : 0; i < n; i++) memcpy(c->h_traj.transforms[i & (TRAJ_RING - 1)], transforms + 3 * (size_t)i, 3 * sizeof(float));
    VS_HIP_TRY(hipMemcpyAsync(c->d_traj, &c->h_traj, sizeof(TrajState), hipMemcpyHostToDevice, c->st));
    VS_HIP_TRY(hipMemcpyAsync(c->d_t, t, 3 * sizeof(float), hipMemcpyHostToDevice, c->st));
    VS_HIP_TRY(hipStreamSynchronize(c->st));         // (the host copies above were read from pageable memory)
    const int rc = canvas_apply(c->canvas, p, (const uint8_t*)d_frame, pitch, w, h, c->d_t, c->d_traj, (uint8_t*)d_out, out_pitch, c->st);
    VS_HIP_TRY(hipStreamSynchronize(c->st));
    if (rc == VS_OK && info8) canvas_info(c->canvas, info8);
    return rc;
}

}  // extern "C"
