// The plane list of a YUV surface (video-stab_amd/csrc/planar_layout.h: planes()) on its own: plain host code, no HIP, no device.
// Reads one case per line - fmt w h pitch uv_off u_off v_off c_pitch, integers (an offset or chroma pitch of 0: the default) - and
// prints per case "n sample_bytes" and, behind a '|' each, every plane's "off pitch w h cn sx sy row_bytes"; for a three-plane
// format then the I420Layout derived from the list and the one i420_layout computes, "pitch cpitch u v" each
// (tests/planes_prog.py).
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
        long long fmt, w, h, pitch, uv_off, u_off, v_off, c_pitch;
        if (!(in >> fmt >> w >> h >> pitch >> uv_off >> u_off >> v_off >> c_pitch)) {
            std::printf("-1 unreadable case\n");
            continue;
        }
        const vsd::PixFmt* f = vsd::pixfmt((int)fmt);
        if (!f) {
            std::printf("-1 not a format\n");
            continue;
        }
        vsd::ChromaLayout c;
        c.uv_off = (size_t)uv_off; c.u_off = (size_t)u_off; c.v_off = (size_t)v_off; c.c_pitch = (size_t)c_pitch;
        const vsd::Planes P = vsd::planes(*f, (int)w, (int)h, (size_t)pitch, c);
        std::printf("%d %d", P.n, P.sample_bytes);
        for (int k = 0; k < P.n; k++)
            std::printf("|%zu %zu %d %d %d %d %d %zu", P[k].off, P[k].pitch, P[k].w, P[k].h, P[k].cn, P[k].sx, P[k].sy, P.row_bytes(k));
        if (f->three_planes()) {
            const vsd::I420Layout a = P.i420(), b = vsd::i420_layout((size_t)pitch, (int)h, c.u_off, c.v_off, c.c_pitch, f->sx, f->sy);
            std::printf("|%zu %zu %zu %zu|%zu %zu %zu %zu", a.pitch, a.cpitch, a.u, a.v, b.pitch, b.cpitch, b.u, b.v);
        }
        std::printf("\n");
    }
    return 0;
}
