// What the host code knows about the pixel formats (VS_FMT_*), in one table, and what a stream refuses about a frame, a surface
// or a layout, in one statement of the rules.  Plain C++ over integers: no HIP, no stream object - tests/cpp/pixfmt_check.cpp
// compiles this header alone and holds the rules to the recorded answers of the library (tests/golden/stream_refusals.json).
// Adding a format: DESIGN.md, "adding a pixel format".
#ifndef VS_PIXFMT_H
#define VS_PIXFMT_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <utility>

#include "../../include/vs_stab.h"

namespace vsd {

// How the samples of a frame lie: one plane of interleaved channels (BGR8 ... GRAY8); a luma plane and ONE plane of interleaved
// (U, V) pairs at the luma pitch (NV12, P010); a luma plane and a U and a V plane with a pitch of their own (I420 ... I412).
enum PixKind { PIX_INTERLEAVED, PIX_LUMA_UV, PIX_THREE_PLANES };

struct PixFmt {
    int fmt;
    const char* name;
    const char* text;       // as the stream's messages name it (the two 4:2:0 16-bit formats have always been named together)
    PixKind kind;
    int cn;                 // bytes per pixel of the first plane
    int sample_bytes;
    int bits;               // of a sample's value (P010: in the high bits; the three-plane 16-bit formats: in the low bits)
    int sx, sy;             // a chroma plane has (w >> sx) x (h >> sy) samples; 0, 0 where there is none
    int gray_source;        // the format the gray kernels are asked for: the Y plane of an 8-bit frame is a GRAY8 image
    bool border_modes;      // border, crop and fade work per byte of an interleaved colour frame

    bool luma_uv() const { return kind == PIX_LUMA_UV; }
    bool three_planes() const { return kind == PIX_THREE_PLANES; }
    bool planar_420() const { return three_planes() && sy; }                    // the three-plane 4:2:0 formats
    bool default_chroma_pitch_is_half() const { return three_planes() && sx; }
    // rows of `pitch` bytes of a whole (packed) frame: the h luma rows and the chroma rows behind them
    int rows(int h) const { return three_planes() ? h + (2 * (h >> sy) >> sx) : luma_uv() ? h * 3 / 2 : h; }
    size_t chroma_row_bytes(int w) const { return (size_t)(w >> sx) * (size_t)sample_bytes; }
    int lo16_shift() const { return three_planes() && sample_bytes == 2 ? bits - 8 : 0; }     // luma byte = min(sample >> shift, 255)
};

// One row per format, in the order of the enum values.
constexpr PixFmt PIXFMTS[] = {
    {VS_FMT_BGR8, "BGR8", "BGR8", PIX_INTERLEAVED, 3, 1, 8, 0, 0, VS_FMT_BGR8, true},
    {VS_FMT_NV12, "NV12", "NV12", PIX_LUMA_UV, 1, 1, 8, 1, 1, VS_FMT_GRAY8, false},
    {VS_FMT_GRAY8, "GRAY8", "GRAY8", PIX_INTERLEAVED, 1, 1, 8, 0, 0, VS_FMT_GRAY8, false},
    {VS_FMT_BGRA8, "BGRA8", "BGRA8", PIX_INTERLEAVED, 4, 1, 8, 0, 0, VS_FMT_BGRA8, true},
    {VS_FMT_RGBA8, "RGBA8", "RGBA8", PIX_INTERLEAVED, 4, 1, 8, 0, 0, VS_FMT_RGBA8, true},
    {VS_FMT_RGB8, "RGB8", "RGB8", PIX_INTERLEAVED, 3, 1, 8, 0, 0, VS_FMT_RGB8, true},
    {VS_FMT_P010, "P010", "P010", PIX_LUMA_UV, 2, 2, 10, 1, 1, VS_FMT_P010, false},
    {VS_FMT_I420, "I420", "I420", PIX_THREE_PLANES, 1, 1, 8, 1, 1, VS_FMT_GRAY8, false},
    {VS_FMT_I010, "I010", "I010 / I012", PIX_THREE_PLANES, 2, 2, 10, 1, 1, VS_FMT_I010, false},
    {VS_FMT_I012, "I012", "I010 / I012", PIX_THREE_PLANES, 2, 2, 12, 1, 1, VS_FMT_I012, false},
    {VS_FMT_I422, "I422", "I422", PIX_THREE_PLANES, 1, 1, 8, 1, 0, VS_FMT_GRAY8, false},
    {VS_FMT_I444, "I444", "I444", PIX_THREE_PLANES, 1, 1, 8, 0, 0, VS_FMT_GRAY8, false},
    {VS_FMT_I210, "I210", "I210", PIX_THREE_PLANES, 2, 2, 10, 1, 0, VS_FMT_I210, false},
    {VS_FMT_I212, "I212", "I212", PIX_THREE_PLANES, 2, 2, 12, 1, 0, VS_FMT_I212, false},
    {VS_FMT_I410, "I410", "I410", PIX_THREE_PLANES, 2, 2, 10, 0, 0, VS_FMT_I410, false},
    {VS_FMT_I412, "I412", "I412", PIX_THREE_PLANES, 2, 2, 12, 0, 0, VS_FMT_I412, false},
};
constexpr int N_PIXFMTS = (int)(sizeof PIXFMTS / sizeof PIXFMTS[0]);
constexpr bool pixfmts_in_enum_order(int i = 0) { return i == N_PIXFMTS || (PIXFMTS[i].fmt == i && pixfmts_in_enum_order(i + 1)); }
static_assert(pixfmts_in_enum_order(), "PIXFMTS[v] must be the row of the format with value v");

inline const PixFmt* pixfmt(int fmt) { return fmt >= 0 && fmt < N_PIXFMTS ? &PIXFMTS[fmt] : nullptr; }     // nullptr: not a format

// Where the chroma of a caller's surfaces lies, for one direction (the frames pushed, or the surfaces filled): bytes behind the
// surface pointer, 0 = the packed default of the field.  uv_off: the (U, V) plane of NV12 / P010 (vs_stab_set_nv12_layout);
// u_off, v_off, c_pitch: the planes of the three-plane formats and the pitch of their rows (vs_stab_set_i420_layout).  The two
// setters are independent, so the fields do not alias.
struct ChromaLayout {
    size_t uv_off = 0, u_off = 0, v_off = 0, c_pitch = 0;
    bool operator==(const ChromaLayout& o) const { return uv_off == o.uv_off && u_off == o.u_off && v_off == o.v_off && c_pitch == o.c_pitch; }
    size_t planar_bits() const { return u_off | v_off | c_pitch; }
};

// ---- what a stream refuses -------------------------------------------------------------------------------------------------
// rc VS_OK: accepted.  The texts are those the library has always given, byte for byte (INTEGRATION.md and vs_stab.h
// quote several); where families of formats were worded differently the branch says so.
struct Refusal {
    int rc = VS_OK;
    std::string text;
};
inline Refusal refuse(int rc, std::string text) { return Refusal{rc, std::move(text)}; }

// "I420 needs", "I010 / I012 need"
inline std::string fmt_needs(const PixFmt& f) { return std::string(f.text) + (strchr(f.text, '/') ? " need" : " needs"); }
// the formats whose messages name them where those of NV12 and GRAY8 do not (historical wording)
inline bool fmt_named_in_mode_texts(const PixFmt& f) { return f.three_planes() || f.sample_bytes == 2; }
// 16-bit samples: a pitch in bytes holds whole samples, and with the default chroma pitch - half of it - so does that
inline bool bad_pitch16(const PixFmt& f, size_t pitch, size_t c_pitch) { return (pitch & 1) || (!c_pitch && f.sx && (pitch & 3)); }
inline const char* half_pitch_clause(const PixFmt& f) { return f.sx ? " (16-bit samples; a default chroma pitch is half the pitch)" : " (16-bit samples)"; }

// An explicit chroma pitch (of either direction) must hold a chroma row.  `where`: "" or the setter's name and ": ".
inline Refusal check_chroma_pitch(const PixFmt& f, int w, size_t in_c_pitch, size_t out_c_pitch, const char* where) {
    const size_t crow = f.chroma_row_bytes(w);
    if (!((in_c_pitch && in_c_pitch < crow) || (out_c_pitch && out_c_pitch < crow))) return Refusal();
    // historical wording: three phrasings of the one rule, by the family the format came in with
    const std::string head = std::string(where) + f.text;
    if (f.sy) return refuse(VS_ERR_INVALID_ARG, head + (f.sample_bytes == 1 ? ": the chroma pitch must be at least w / 2" : ": the chroma pitch must be at least w bytes"));
    return refuse(VS_ERR_INVALID_ARG, head + ": the chroma pitch must hold a chroma row (" + std::to_string(crow) + " bytes)");
}

// The input side of a push, before the stream allocates: geometry, pitch, the stored layouts, the border modes.  f: pixfmt(fmt).
// yuv_crop_zoom: the stream has crop-and-zoom on YUV surfaces turned on (vs_stab_set_yuv_crop_zoom) AND its parameters ask for
// crop_n_zoom; 0 (the default) gives the answers of a stream without the mode.
// yuv_border_pad: the stream has border pad on YUV surfaces turned on (vs_stab_set_yuv_border_pad) AND its parameters ask for a
// pad (no crop_n_zoom, a border type of cv::copyMakeBorder - not the fade); 0 (the default) likewise.  The result then has
// (w + 2 border_size) x (h + 2 border_size) pixels, and an explicit output chroma pitch must hold a chroma row of that.
// yuv_fade: the stream has the fade border on YUV surfaces turned on (vs_stab_set_yuv_fade) AND its parameters ask for the fade (no
// crop_n_zoom, border_type VS_BORDER_FADE); 0 (the default) likewise.  The result is padded as with yuv_border_pad.
inline Refusal check_input(const PixFmt* f, int w, int h, size_t pitch, const ChromaLayout& in, const ChromaLayout& out, int border_size,
                           int yuv_crop_zoom = 0, int yuv_border_pad = 0, int yuv_fade = 0) {
    if (w <= 0 || h <= 0 || !f) return refuse(VS_ERR_INVALID_ARG, "push: bad geometry/format");
    if ((f->sx && (w & 1)) || (f->sy && (h & 1))) return refuse(VS_ERR_INVALID_ARG, fmt_needs(*f) + (f->sy ? " even w,h" : " an even w"));
    if (f->luma_uv() && f->sample_bytes == 2 && ((pitch | in.uv_off | out.uv_off) & 1))
        return refuse(VS_ERR_INVALID_ARG, fmt_needs(*f) + " even pitches and plane offsets (16-bit samples)");
    if (f->three_planes()) {
        if (f->sample_bytes == 1 && f->sx && (pitch & 1)) return refuse(VS_ERR_INVALID_ARG, fmt_needs(*f) + " an even pitch (the default chroma pitch is half of it)");
        if (f->sample_bytes == 2 && (bad_pitch16(*f, pitch, in.c_pitch) || ((in.planar_bits() | out.planar_bits()) & 1)))
            return refuse(VS_ERR_INVALID_ARG, fmt_needs(*f) + " even pitches and plane offsets" + half_pitch_clause(*f));
        const Refusal r = check_chroma_pitch(*f, w, in.c_pitch, out.c_pitch, "");
        if (r.rc != VS_OK) return r;
    }
    // the YUV mode that acts on the border, in the words of its texts; crop-and-zoom keeps the frame's size, the other two pad the result
    const char* const mode = yuv_crop_zoom ? "crop-and-zoom on " : yuv_border_pad ? "border pad on " : yuv_fade ? "fade on " : nullptr;
    if (border_size > 0 && mode && f->kind != PIX_INTERLEAVED) {
        // the crop / the border of a chroma plane is the luma one's: (b >> sx, b >> sy) must be exact
        if (border_size & ((1 << (f->sx > f->sy ? f->sx : f->sy)) - 1))
            return refuse(VS_ERR_INVALID_ARG, std::string(mode) + f->name + " needs an even border_size (the chroma planes are subsampled: their " +
                                                  (yuv_crop_zoom ? "crop starts at border_size / 2)" : "border is border_size / 2)"));
        if (!yuv_crop_zoom && f->three_planes() && out.c_pitch && out.c_pitch < f->chroma_row_bytes(w + 2 * border_size))
            return refuse(VS_ERR_INVALID_ARG, std::string(mode) + f->name + ": the output chroma pitch must hold a padded chroma row (" +
                                                  std::to_string(f->chroma_row_bytes(w + 2 * border_size)) + " bytes)");
    } else if (border_size > 0 && !f->border_modes) {
        // historical wording: two texts (the formats that came later name the fade mode and themselves)
        if (fmt_named_in_mode_texts(*f))
            return refuse(VS_ERR_UNSUPPORTED, std::string("border/crop/fade modes need a colour format (BGR8, BGRA8, RGBA8, RGB8), not ") + f->text);
        return refuse(VS_ERR_UNSUPPORTED, "border/crop modes need a colour format (BGR8, BGRA8, RGBA8, RGB8)");
    }
    if (pitch < (size_t)w * f->cn) return refuse(VS_ERR_INVALID_ARG, "push: stride < row bytes");
    return Refusal();
}

// Limited-range video black of a YUV format, samples as they lie in memory (vs_yuv_video_black): Y = 16 and U = V = 128 at the
// format's depth; P010 keeps its bits at the top of the word.
inline vs_yuv_fill yuv_video_black(const PixFmt& f) {
    const int sh = f.luma_uv() && f.sample_bytes == 2 ? 8 : f.bits - 8;
    return vs_yuv_fill{(uint16_t)(16 << sh), (uint16_t)(128 << sh), (uint16_t)(128 << sh), 0};
}
// A fill colour of border pad (or, with the setter's name given, of the fade) on a YUV stream: 8-bit formats hold 8-bit samples
inline Refusal check_yuv_fill(const PixFmt& f, const vs_yuv_fill& c, const char* setter = "vs_stab_set_yuv_border_pad") {
    if (f.sample_bytes == 1 && (c.y > 255 || c.u > 255 || c.v > 255))
        return refuse(VS_ERR_INVALID_ARG, std::string(setter) + ": a fill sample above 255 on " + f.name + " (8-bit samples)");
    return Refusal();
}

// ... and what allocation refuses once the analysis size is known: the virtual canvas
// (the reference's cvtColor(BGR2GRAY) of the canvas, Stabilizer.cpp:2225, throws on anything but three channels)
inline Refusal check_canvas(const PixFmt& f, bool canvas_on) {
    if (!canvas_on || f.fmt == VS_FMT_BGR8) return Refusal();
    return refuse(VS_ERR_UNSUPPORTED, std::string("enableVirtualCanvas needs a BGR8 stream") + (fmt_named_in_mode_texts(f) ? std::string(" (not ") + f.text + ")" : ""));
}

// A surface handed to an entry point, after the input side: the low bits of its pointer(s), its pitch, the stored chroma pitch
// that goes with it.  device_surface: the caller's device memory; false: the host entry points - pointers are not looked at
// (ptr_bits 0) and the frame has the packed default layout at its pitch (c_pitch 0).
inline Refusal check_surface(const PixFmt& f, bool device_surface, uintptr_t ptr_bits, size_t pitch, size_t c_pitch) {
    if (f.luma_uv() && f.sample_bytes == 2 && device_surface && ((ptr_bits | pitch) & 1))
        return refuse(VS_ERR_INVALID_ARG, fmt_needs(f) + " even surface pointers and pitches (16-bit samples)");
    if (f.three_planes() && f.sample_bytes == 1 && f.sx && (pitch & 1))
        return refuse(VS_ERR_INVALID_ARG, fmt_needs(f) + " an even output pitch (the default chroma pitch is half of it)");
    if (f.three_planes() && f.sample_bytes == 2 && ((ptr_bits & 1) || bad_pitch16(f, pitch, c_pitch)))
        return refuse(VS_ERR_INVALID_ARG, fmt_needs(f) + " even surface pointers and pitches" + half_pitch_clause(f));
    return Refusal();
}

// A host frame that is about to be delivered: the caller's buffer must be there and hold a row.  call: "push" / "flush".
inline Refusal check_host_out(const char* call, bool have_out, size_t out_pitch, size_t row_bytes) {
    if (have_out && out_pitch >= row_bytes) return Refusal();
    return refuse(VS_ERR_INVALID_ARG, std::string(call) + ": output buffer/stride too small");
}

// The layout setters once the geometry is known (before that, the next push checks what they stored).
inline Refusal check_set_nv12_layout(const PixFmt& f, size_t in_uv_off, size_t out_uv_off) {
    if (f.luma_uv() && f.sample_bytes == 2 && ((in_uv_off | out_uv_off) & 1))
        return refuse(VS_ERR_INVALID_ARG, "vs_stab_set_nv12_layout: " + fmt_needs(f) + " even plane offsets (16-bit samples)");
    return Refusal();
}
inline Refusal check_set_i420_layout(const PixFmt& f, int w, const ChromaLayout& in, const ChromaLayout& out) {
    if (!f.three_planes()) return Refusal();
    // historical wording: "plane offsets and pitches" here, "pitches and plane offsets" in a push
    if (f.sample_bytes == 2 && ((in.planar_bits() | out.planar_bits()) & 1))
        return refuse(VS_ERR_INVALID_ARG, "vs_stab_set_i420_layout: " + fmt_needs(f) + " even plane offsets and pitches (16-bit samples)");
    return check_chroma_pitch(f, w, in.c_pitch, out.c_pitch, "vs_stab_set_i420_layout: ");
}

}  // namespace vsd
#endif
