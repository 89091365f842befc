// The input rules of a stream (video-stab_amd/csrc/pixfmt.h, check_input) with border pad on YUV surfaces turned on or off: plain
// host code, no HIP, no device.  Reads one case per line - fmt w h pitch border_size crop_n_zoom canvas fade cz_mode pad_mode
// out_c_pitch, integers - and prints per case "rc|text|rc|text|y|u|v": the answer with the stream's modes as given (the last two
// arguments of check_input as the stream passes them: cz_mode && crop_n_zoom, and pad_mode && !crop_n_zoom && !fade; then
// check_canvas, as the first allocation asks), the answer with both arguments left at their defaults, and the format's video black
// (0|0|0 where there is none) (tests/test_yuv_border_pad_cpu.py).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../video-stab_amd/csrc/pixfmt.h"

using namespace vsd;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        long long fmt, w, h, pitch, border, crop, canvas, fade, cz, pad, ocp;
        if (!(in >> fmt >> w >> h >> pitch >> border >> crop >> canvas >> fade >> cz >> pad >> ocp)) {
            std::printf("-1|unreadable case|-1|unreadable case|0|0|0\n");
            continue;
        }
        const PixFmt* f = pixfmt((int)fmt);
        ChromaLayout out;
        out.c_pitch = (size_t)ocp;
        Refusal a = check_input(f, (int)w, (int)h, (size_t)pitch, ChromaLayout(), out, (int)border, cz && crop, pad && !crop && !fade);
        if (a.rc == VS_OK && f) a = check_canvas(*f, canvas && !crop);
        Refusal d = check_input(f, (int)w, (int)h, (size_t)pitch, ChromaLayout(), out, (int)border);
        if (d.rc == VS_OK && f) d = check_canvas(*f, canvas && !crop);
        vs_yuv_fill k = {0, 0, 0, 0};
        if (f && f->kind != PIX_INTERLEAVED) k = yuv_video_black(*f);
        std::printf("%d|%s|%d|%s|%d|%d|%d\n", a.rc, a.text.c_str(), d.rc, d.text.c_str(), (int)k.y, (int)k.u, (int)k.v);
    }
    return 0;
}
