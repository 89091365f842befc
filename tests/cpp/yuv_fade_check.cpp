// The input rules of a stream (video-stab_amd/csrc/pixfmt.h, check_input) with the fade border on YUV surfaces turned on or off:
// plain host code, no HIP, no device.  Reads one case per line - fmt w h pitch border_size crop_n_zoom canvas fade pad_mode
// fade_mode out_c_pitch, integers - and prints per case "rc|text|rc|text": the answer with the stream's modes as given (the last
// two arguments of check_input as the stream passes them: pad_mode && !crop_n_zoom && !fade, and fade_mode && !crop_n_zoom && fade;
// then check_canvas, as the first allocation asks) and the answer with both arguments left at their defaults
// (tests/test_yuv_fade_cpu.py).  The layouts of the operators' job structs are part of the ABI: asserted here as a C++ compiler
// sees the public header.
#include <cstddef>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../video-stab_amd/csrc/pixfmt.h"

using namespace vsd;

static_assert(sizeof(vs_fade_job) == 80 && offsetof(vs_fade_job, hist) == 24 && offsetof(vs_fade_job, dst) == 40 && offsetof(vs_fade_job, fill) == 64 &&
                  offsetof(vs_fade_job, cn) == 68 && offsetof(vs_fade_job, reserved) == 72,
              "struct vs_fade_job");
static_assert(sizeof(vs_fade_update_job) == 48 && offsetof(vs_fade_update_job, res) == 16 && offsetof(vs_fade_update_job, w) == 32 &&
                  offsetof(vs_fade_update_job, reserved) == 44,
              "struct vs_fade_update_job");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        long long fmt, w, h, pitch, border, crop, canvas, fade, pad, fm, ocp;
        if (!(in >> fmt >> w >> h >> pitch >> border >> crop >> canvas >> fade >> pad >> fm >> ocp)) {
            std::printf("-1|unreadable case|-1|unreadable case\n");
            continue;
        }
        const PixFmt* f = pixfmt((int)fmt);
        ChromaLayout out;
        out.c_pitch = (size_t)ocp;
        Refusal a = check_input(f, (int)w, (int)h, (size_t)pitch, ChromaLayout(), out, (int)border, 0, pad && !crop && !fade, fm && !crop && fade);
        if (a.rc == VS_OK && f) a = check_canvas(*f, canvas && !crop);
        Refusal d = check_input(f, (int)w, (int)h, (size_t)pitch, ChromaLayout(), out, (int)border);
        if (d.rc == VS_OK && f) d = check_canvas(*f, canvas && !crop);
        std::printf("%d|%s|%d|%s\n", a.rc, a.text.c_str(), d.rc, d.text.c_str());
    }
    return 0;
}
