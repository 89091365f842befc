// The axis tables of the area-averaging downscale on their own: video-stab_amd/csrc/resize_tables.h, nothing else of the library.
// stdin: lines "src dst" (dst <= src); stdout per line: "src dst integer i", then dst lines "first count w_first w_mid w_last" with
// the weights as the 8 hex digits of their float bits.
// tests/test_area_cpu.py compares the output with tests/arearef.py; `make asan` runs it under the sanitizers.
#include "../../video-stab_amd/csrc/resize_tables.h"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main() {
    int src, dst;
    while (std::scanf("%d %d", &src, &dst) == 2) {
        if (dst < 1 || src > 32767 || dst > src) {
            std::fprintf(stderr, "bad line: %d %d\n", src, dst);
            return 2;
        }
        std::vector<int32_t> first(dst), count(dst);
        std::vector<float> wf(dst), wm(dst), wl(dst);
        vsd::rs_area_axis_table(src, dst, first.data(), count.data(), wf.data(), wm.data(), wl.data());
        int i = 0;
        const bool integer = vsd::rs_area_integer(src, dst, &i);
        std::printf("%d %d %d %d\n", src, dst, integer ? 1 : 0, i);
        for (int d = 0; d < dst; d++) std::printf("%d %d %08x %08x %08x\n", (int)first[d], (int)count[d], bits(wf[d]), bits(wm[d]), bits(wl[d]));
    }
    return 0;
}
