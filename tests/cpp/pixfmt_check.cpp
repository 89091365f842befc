// The format table and the refusal rules of video-stab_amd/csrc/pixfmt.h on their own: no HIP, no stream, no device.
//
//   pixfmt_check table     the table as JSON (tests/test_pixfmt_table_cpu.py compares it with vsamd/capi.py and vs_stab.h)
//   pixfmt_check cases     reads the case lines of tests/refusal_cases.py (line()) on stdin and prints, per case,
//                          "<id>\t<code>\t<text>": what the rules answer when they are asked in the entry point's order
//                          (tests/test_stream_refusals_cpu.py compares with tests/golden/stream_refusals.json)
//
// g++ -std=c++17 -I include tests/cpp/pixfmt_check.cpp
#include <cstdio>
#include <iostream>
#include <sstream>

#include "../../video-stab_amd/csrc/pixfmt.h"

using namespace vsd;

namespace {

int print_table() {
    printf("[\n");
    for (int i = 0; i < N_PIXFMTS; i++) {
        const PixFmt& f = PIXFMTS[i];
        printf(" {\"fmt\": %d, \"name\": \"%s\", \"text\": \"%s\", \"kind\": %d, \"cn\": %d, \"sample_bytes\": %d, \"bits\": %d, \"sx\": %d, \"sy\": %d, "
               "\"gray_source\": %d, \"border_modes\": %s, \"rows_of_48\": %d, \"chroma_row_bytes_of_64\": %zu, \"lo16_shift\": %d, "
               "\"default_chroma_pitch_is_half\": %s}%s\n",
               f.fmt, f.name, f.text, (int)f.kind, f.cn, f.sample_bytes, f.bits, f.sx, f.sy, f.gray_source, f.border_modes ? "true" : "false", f.rows(48),
               f.chroma_row_bytes(64), f.lo16_shift(), f.default_chroma_pitch_is_half() ? "true" : "false", i + 1 < N_PIXFMTS ? "," : "");
    }
    printf("]\n");
    return 0;
}

struct Case {
    std::string id;
    long long fmt, entry, w, h, pitch, border, crop, fade, canvas, batch, pipe, zc, nv12[2], i420[6], data_odd, out_odd, out_pitch, setter[6];
};
enum { PUSH_DEV, FLUSH_DEV, PUSH, FLUSH, SET_I420, SET_NV12, PROBE };

// The first push of a stream, as vs_stab_push_dev / vs_stab_push ask: the input side, the allocation, the surfaces.
Refusal first_push(const Case& c, bool host, int w, int h, size_t pitch, unsigned data_odd, unsigned out_odd, size_t out_pitch, const ChromaLayout& in,
                   const ChromaLayout& out) {
    const PixFmt* f = pixfmt((int)c.fmt);
    Refusal r = check_input(f, w, h, pitch, in, out, (int)c.border);
    if (r.rc != VS_OK) return r;
    r = check_canvas(*f, c.canvas && !c.crop);
    if (r.rc != VS_OK) return r;
    if (!host) return check_surface(*f, true, data_odd | out_odd, out_pitch, out.c_pitch);
    r = check_surface(*f, false, 0, pitch, 0);
    if (r.rc != VS_OK) return r;
    return check_surface(*f, false, 0, out_pitch, 0);      // (nothing is delivered by a first push: the buffer's size is not looked at)
}

Refusal answer(const Case& c) {
    ChromaLayout in, out;
    in.uv_off = c.nv12[0]; out.uv_off = c.nv12[1];
    in.u_off = c.i420[0]; in.v_off = c.i420[1]; in.c_pitch = c.i420[2];
    out.u_off = c.i420[3]; out.v_off = c.i420[4]; out.c_pitch = c.i420[5];
    const PixFmt* f = pixfmt((int)c.fmt);
    if (c.entry == PUSH_DEV || c.entry == PUSH)
        return first_push(c, c.entry == PUSH, (int)c.w, (int)c.h, (size_t)c.pitch, (unsigned)c.data_odd, (unsigned)c.out_odd, (size_t)c.out_pitch, in, out);
    if (!f) return refuse(-1, "pixfmt_check: this entry needs a known format");
    // the calls before the one under test: a tight 64 x 48 frame, which must be accepted
    const size_t tight = (size_t)64 * f->cn;
    Refusal r = first_push(c, c.entry == FLUSH, 64, 48, tight, 0, 0, tight, in, out);
    if (r.rc != VS_OK) return refuse(-1, "pixfmt_check: the push before the call under test is refused: " + r.text);
    switch (c.entry) {
        case FLUSH_DEV: return check_surface(*f, true, (unsigned)c.out_odd, (size_t)c.out_pitch, out.c_pitch);
        case FLUSH:
            r = check_host_out("flush", true, (size_t)c.out_pitch, tight);
            return r.rc != VS_OK ? r : check_surface(*f, false, 0, (size_t)c.out_pitch, 0);
        case SET_I420: {
            ChromaLayout a, b;
            a.u_off = c.setter[0]; a.v_off = c.setter[1]; a.c_pitch = c.setter[2];
            b.u_off = c.setter[3]; b.v_off = c.setter[4]; b.c_pitch = c.setter[5];
            return check_set_i420_layout(*f, 64, a, b);
        }
        case SET_NV12: return check_set_nv12_layout(*f, (size_t)c.setter[0], (size_t)c.setter[1]);
        default: return refuse(-1, "pixfmt_check: a stateful case needs a stream");
    }
}

int run_cases() {
    std::string ln;
    while (std::getline(std::cin, ln)) {
        if (ln.empty()) continue;
        std::istringstream is(ln);
        Case c;
        is >> c.id >> c.fmt >> c.entry >> c.w >> c.h >> c.pitch >> c.border >> c.crop >> c.fade >> c.canvas >> c.batch >> c.pipe >> c.zc >> c.nv12[0] >> c.nv12[1];
        for (auto& v : c.i420) is >> v;
        is >> c.data_odd >> c.out_odd >> c.out_pitch;
        for (auto& v : c.setter) is >> v;
        if (!is) { fprintf(stderr, "pixfmt_check: bad case line: %s\n", ln.c_str()); return 2; }
        const Refusal r = answer(c);
        printf("%s\t%d\t%s\n", c.id.c_str(), r.rc, r.text.c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table") return print_table();
    if (mode == "cases") return run_cases();
    fprintf(stderr, "usage: pixfmt_check table | cases < lines\n");
    return 2;
}
