// vs::Stabilizer fed with four-channel (BGRA) Mats: argv[1] frames of a moving pattern whose fourth byte is a copy of B go
// through the class, and the same frames as BGR through the C ABI (vs_stab_push, VS_FMT_BGR8) with the same settings.
// Every result of the class must be a four-channel Mat whose B, G, R equal the C ABI's result and whose fourth byte equals
// its own B (the fourth channel is warped like the others).  Prints "<results> ok" or the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "video/Stabilizer.h"
#include "vs_stab.h"

static void make_frames(int w, int h, int k, cv::Mat &bgra, std::vector<unsigned char> &bgr) {
    bgra = cv::Mat(h, w, CV_MAKETYPE(CV_8U, 4));
    bgr.assign((size_t)w * h * 3, 0);
    for (int y = 0; y < h; y++) {
        unsigned char *p = bgra.ptr(y);
        for (int x = 0; x < w; x++) {
            const int u = x + 2 * k, v = y + (k % 3);
            const unsigned char c = (unsigned char)((((u / 24) + (v / 24)) & 1) ? 200 : 50);
            const unsigned char px[3] = {c, (unsigned char)(c / 2 + ((u * 7 + v * 3) & 31)), (unsigned char)(255 - c)};
            for (int i = 0; i < 3; i++) p[4 * x + i] = bgr[((size_t)y * w + x) * 3 + i] = px[i];
            p[4 * x + 3] = px[0];
        }
    }
}

static int compare(const cv::Mat &m, const std::vector<unsigned char> &ref, int w, int h, int idx) {
    if (m.type() != CV_MAKETYPE(CV_8U, 4) || m.rows != h || m.cols != w) {
        std::printf("result %d: type %d, %d x %d\n", idx, m.type(), m.cols, m.rows);
        return 1;
    }
    for (int y = 0; y < h; y++) {
        const unsigned char *p = m.ptr(y);
        for (int x = 0; x < w; x++)
            for (int i = 0; i < 4; i++) {
                const unsigned char want = ref[((size_t)y * w + x) * 3 + (i == 3 ? 0 : i)];
                if (p[4 * x + i] != want) {
                    std::printf("result %d: (%d, %d) channel %d: %d, want %d\n", idx, x, y, i, p[4 * x + i], want);
                    return 1;
                }
            }
    }
    return 0;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 40, w = 320, h = 240;
    vs::Stabilizer::Parameters sp;
    sp.smoothingRadius = 20;
    sp.borderType = "black";
    sp.logging = false;
    vs::Stabilizer stab(sp);

    vs_params_c c;
    vs_params_default(&c);
    c.smoothing_radius = 20;
    vs_stab *ref = nullptr;
    if (vs_stab_create(&c, 0, &ref) != VS_OK) { std::printf("vs_stab_create failed\n"); return 1; }

    std::vector<unsigned char> bgr, out((size_t)w * h * 3);
    int results = 0;
    for (int k = 0; k < n; k++) {
        cv::Mat f;
        make_frames(w, h, k, f, bgr);
        const cv::Mat got = stab.stabilize(f);
        int produced = 0;
        if (vs_stab_push(ref, bgr.data(), w, h, (size_t)w * 3, VS_FMT_BGR8, out.data(), (size_t)w * 3, &produced) != VS_OK) {
            std::printf("vs_stab_push: %s\n", vs_stab_last_error(ref));
            return 1;
        }
        if (got.empty() != !produced) { std::printf("frame %d: class %s a result, C ABI %s\n", k, got.empty() ? "without" : "with", produced ? "with" : "without"); return 1; }
        if (produced && compare(got, out, w, h, results++)) return 1;
    }
    for (;;) {
        const cv::Mat got = stab.flush();
        int produced = 0;
        if (vs_stab_flush(ref, out.data(), (size_t)w * 3, &produced) != VS_OK) return 1;
        if (got.empty() != !produced) { std::printf("flush: class and C ABI disagree\n"); return 1; }
        if (!produced) break;
        if (compare(got, out, w, h, results++)) return 1;
    }
    vs_stab_destroy(ref);
    std::printf("%d ok\n", results);
    return results == n ? 0 : 1;
}
