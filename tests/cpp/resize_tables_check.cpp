// The axis tables of the resize to an output size on their own: video-stab_amd/csrc/resize_tables.h, nothing else of the library.
// stdin: lines "src dst interp axis"; stdout per line: "src dst interp axis K", then dst lines of K indices and K coefficients.
// tests/test_resize_cpu.py compares the output with tests/resizeref.py; `make asan` runs it under the sanitizers.
#include "../../video-stab_amd/csrc/resize_tables.h"

#include <cstdio>
#include <vector>

int main() {
    int src, dst, interp, axis;
    while (std::scanf("%d %d %d %d", &src, &dst, &interp, &axis) == 4) {
        if (src < 1 || dst < 1 || src > 32767 || dst > 32767 || (interp != vsd::RS_LINEAR && interp != vsd::RS_LANCZOS4) || (axis != 0 && axis != 1)) {
            std::fprintf(stderr, "bad line: %d %d %d %d\n", src, dst, interp, axis);
            return 2;
        }
        const int k = vsd::rs_taps(interp);
        std::vector<int32_t> idx((size_t)dst * k);
        std::vector<int16_t> coef((size_t)dst * k);
        vsd::rs_axis_table(src, dst, interp, axis, idx.data(), coef.data());
        std::printf("%d %d %d %d %d\n", src, dst, interp, axis, k);
        for (int d = 0; d < dst; d++) {
            for (int t = 0; t < k; t++) std::printf("%d ", (int)idx[(size_t)d * k + t]);
            for (int t = 0; t < k; t++) std::printf("%d%c", (int)coef[(size_t)d * k + t], t + 1 < k ? ' ' : '\n');
        }
    }
    return 0;
}
