// The layout rules of the roll and zoom/crop stages' three-plane surfaces (video-stab_amd/csrc/planar_layout.h) on their own: plain
// host code, no HIP, no device.  Reads one case per line - fmt ptr w h pitch c_pitch u_off v_off need_w need_h, integers - and prints
// per case "rc|text" for a refusal or "0|pitch cpitch u v" for the resolved layout (tests/planar_layout_prog.py).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../video-stab_amd/csrc/planar_layout.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        long long fmt, ptr, w, h, pitch, c_pitch, u_off, v_off, need_w, need_h;
        if (!(in >> fmt >> ptr >> w >> h >> pitch >> c_pitch >> u_off >> v_off >> need_w >> need_h)) {
            std::printf("-1|unreadable case\n");
            continue;
        }
        const vsd::PixFmt* f = vsd::pixfmt((int)fmt);
        if (!f || !f->three_planes()) {
            std::printf("-1|not a three-plane format\n");
            continue;
        }
        vs_i420_layout lay;
        lay.pitch = (size_t)pitch; lay.c_pitch = (size_t)c_pitch; lay.u_off = (size_t)u_off; lay.v_off = (size_t)v_off;
        vsd::I420Layout l;
        std::string msg;
        const int rc = vsd::planar_layout_check((int)fmt, (const void*)(uintptr_t)ptr, (int)w, (int)h, &lay, (int)need_w, (int)need_h, "stage", &l, &msg);
        if (rc != VS_OK) std::printf("%d|%s\n", rc, msg.c_str());
        else std::printf("0|%zu %zu %zu %zu\n", l.pitch, l.cpitch, l.u, l.v);
    }
    return 0;
}
