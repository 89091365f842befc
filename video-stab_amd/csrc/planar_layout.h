// Where the planes of a surface lie - the three-plane layout of the launchers (VS_FMT_I420 ... VS_FMT_I412) and the plane list of
// any format that the stream, the batch schedule and the roll and zoom/crop stages walk -, the frame record of those two stages,
// and what they refuse about a three-plane surface.  Plain C++ over integers like pixfmt.h: no HIP, no object -
// tests/cpp/planar_layout_check.cpp, planes_check.cpp and stage_frame_check.cpp compile this header alone and ask it without a device.
#ifndef VS_PLANAR_LAYOUT_H
#define VS_PLANAR_LAYOUT_H

#include <algorithm>
#include <string>

#include "pixfmt.h"

namespace vsd {

// Where the planes of a surface lie: rows of `pitch` bytes of luma at the surface pointer, the U and V planes (h >> sy rows of
// w >> sx samples, `cpitch` bytes apart) u and v bytes behind it.  One layout for all source surfaces of a call, one for all destinations.
struct I420Layout { size_t pitch, cpitch, u, v; };
// The layout a caller describes with 0 = default per field: chroma pitch = pitch >> sx, U behind the h luma rows, V behind U.
inline I420Layout i420_layout(size_t pitch, int h, size_t u_off, size_t v_off, size_t c_pitch, int sx = 1, int sy = 1) {
    I420Layout l;
    l.pitch = pitch;
    l.cpitch = c_pitch ? c_pitch : pitch >> sx;
    l.u = u_off ? u_off : (size_t)h * pitch;
    l.v = v_off ? v_off : l.u + (size_t)(h >> sy) * l.cpitch;
    return l;
}

// ---- the plane list: where every plane of a surface lies, stated once for the stream and the batch schedule (stab_internal.h)
// One plane: `off` bytes behind the surface pointer, rows of `pitch` bytes, w x h pixels of cn channels (an interleaved (U, V)
// pair is one pixel of two channels), subsampled by (sx, sy) against luma - which is also what a luma border or crop shifts by.
struct Plane {
    size_t off, pitch;
    int w, h, cn, sx, sy;
};
// A surface: luma and the UV plane (NV12, P010), luma, U and V (I420 ... I412), or the one plane of an interleaved format.
struct Planes {
    int n = 0, sample_bytes = 1;
    Plane p[3] = {};
    const Plane& operator[](int k) const { return p[k]; }
    size_t row_bytes(int k) const { return (size_t)p[k].w * p[k].cn * sample_bytes; }
    I420Layout i420() const { return I420Layout{p[0].pitch, p[1].pitch, p[1].off, p[2].off}; }      // (three planes)
};
// The planes of a w x h surface of format f at `pitch`; c: the caller's chroma layout, 0 = the packed default per field (chroma
// behind the h luma rows; three planes: i420_layout).
inline Planes planes(const PixFmt& f, int w, int h, size_t pitch, const ChromaLayout& c = ChromaLayout()) {
    Planes P;
    P.sample_bytes = f.sample_bytes;
    P.n = f.three_planes() ? 3 : f.luma_uv() ? 2 : 1;
    P.p[0] = Plane{0, pitch, w, h, P.n == 1 ? f.cn : 1, 0, 0};
    if (f.luma_uv()) P.p[1] = Plane{c.uv_off ? c.uv_off : (size_t)h * pitch, pitch, w >> f.sx, h >> f.sy, 2, f.sx, f.sy};
    if (f.three_planes()) {
        const I420Layout l = i420_layout(pitch, h, c.u_off, c.v_off, c.c_pitch, f.sx, f.sy);
        P.p[1] = Plane{l.u, l.cpitch, w >> f.sx, h >> f.sy, 1, f.sx, f.sy};
        P.p[2] = Plane{l.v, l.cpitch, w >> f.sx, h >> f.sy, 1, f.sx, f.sy};
    }
    return P;
}
// Channel ch of the fill sample of plane k: {y, 0}; {u, v} for the UV plane; {u, 0} and {v, 0} for planes of their own
inline uint16_t plane_fill(const vs_yuv_fill& c, const Planes& P, int k, int ch) {
    if (P[k].cn == 2) return ch ? c.v : c.u;
    return ch ? 0 : k == 0 ? c.y : k == 1 ? c.u : c.v;
}

// The inverse of Planes::i420(): the planes of a three-plane surface whose layout has been resolved (planar_layout_check)
inline Planes planes(const PixFmt& f, int w, int h, const I420Layout& l) { return planes(f, w, h, l.pitch, ChromaLayout{0, l.u, l.v, l.cpitch}); }
// Offsets and pitches of all planes agree: one launch can take both surfaces
inline bool same_layout(const Planes& a, const Planes& b) {
    if (a.n != b.n) return false;
    for (int k = 0; k < a.n; k++)
        if (a[k].off != b[k].off || a[k].pitch != b[k].pitch) return false;
    return true;
}

// ---- k_roll.hip, k_azc.hip: a frame handed to the stages around the stabilizer, whatever its format - w x h pixels of format *pf
// at src with planes S, the result at dst with planes D (the zoom stage: laid out for the larger of the frame and its output size)
struct StageFrame {
    const PixFmt* pf;
    int w, h;
    const uint8_t* src;
    uint8_t* dst;
    Planes S, D;
};
// The zoom stage's crop (cx, cy, cw, ch) of the picture as plane p sees it, and the size of p's share of an ow x oh result
struct PlaneRect { int x, y, w, h; };
inline PlaneRect plane_crop(const Plane& p, int cx, int cy, int cw, int ch) {
    return PlaneRect{cx >> p.sx, cy >> p.sy, std::max(1, cw >> p.sx), std::max(1, ch >> p.sy)};
}
inline PlaneRect plane_result(const Plane& p, int ow, int oh) { return PlaneRect{0, 0, ow >> p.sx, oh >> p.sy}; }
// ... and where the crop's first sample lies behind the surface pointer
inline size_t plane_crop_offset(const Planes& P, int k, const PlaneRect& r) {
    return P[k].off + (size_t)r.y * P[k].pitch + (size_t)r.x * P[k].cn * P.sample_bytes;
}

// ---- k_roll.hip, k_azc.hip: three-plane surfaces (VS_FMT_I420 ... VS_FMT_I412) of the stages around the stabilizer
// The geometry and layout rules of a planar surface handed to the roll / zoom stages (those vs_stab enforces).  need_w / need_h: the
// samples per row and the rows the layout must hold - the picture's, or for the zoom stage's result the larger of the picture's and
// the stage's output size (640 x 360 unless vs_azc_set_output_size said otherwise).  Fills *l with the defaults resolved, or *msg with a text that names the stage and the format.
// (sx, sy): the format's chroma shifts - a chroma plane holds need_h >> sy rows of need_w >> sx samples, the default chroma pitch is
// pitch >> sx.  The texts of the 4:2:0 formats are those they have always had; 4:2:2 and 4:4:4 word the chroma pitch as the stream does.
inline int planar_layout_check(int fmt, const void* ptr, int w, int h, const vs_i420_layout* in, int need_w, int need_h, const char* stage,
                               I420Layout* l, std::string* msg) {
    const PixFmt& f = *pixfmt(fmt);
    const int sb = f.sample_bytes, sx = f.sx, sy = f.sy;
    const char* name = f.name;
    auto fail = [&](const std::string& what) { *msg = std::string(stage) + ": " + name + ": " + what; return (int)VS_ERR_INVALID_ARG; };
    if ((w & 1) || (h & 1) || w < 2 || h < 2) return fail("w and h must be even");
    if (!in || in->pitch < (size_t)need_w * sb) return fail("the pitch must hold a row of the picture");
    if (sb == 2 && (((uintptr_t)ptr | in->pitch | in->c_pitch | in->u_off | in->v_off) & 1)) return fail("pointers, pitches and plane offsets must be even (16-bit samples)");
    if (!in->c_pitch && (in->pitch & (size_t)((sb << sx) - 1))) return fail(sb == 2 ? "the default chroma pitch needs a pitch that is a multiple of 4" : "the default chroma pitch needs an even pitch");
    *l = i420_layout(in->pitch, need_h, in->u_off, in->v_off, in->c_pitch, sx, sy);
    const size_t crow = (size_t)(need_w >> sx) * sb;
    if (l->cpitch < crow) {
        if (sy) return fail(sb == 2 ? "the chroma pitch must be at least w bytes" : "the chroma pitch must be at least w / 2");
        return fail("the chroma pitch must hold a chroma row (" + std::to_string(crow) + " bytes)");
    }
    if (l->u < (size_t)need_h * l->pitch || l->v < (size_t)need_h * l->pitch) return fail("the chroma planes must start behind the luma rows");
    const size_t cb = (size_t)(need_h >> sy) * l->cpitch, lo = std::min(l->u, l->v), hi = std::max(l->u, l->v);
    if (hi < lo + cb) return fail("the U and V planes overlap");
    return VS_OK;
}

}  // namespace vsd
#endif
