// libm_check [cos|sin|atan|atan2] : the product's restatements of glibc's cosf / sinf / atan2f (video-stab_amd/csrc/vs_libm.h,
// host build) against the host's own libm.  cos / sin / atan: every float; atan2: 2^30 random bit patterns + 2^30 pairs shaped like
// the stabilizer's (x near 1, y small; pixel translations).  Prints "<name> <values> <mismatches>" per function; exit code 1 on
// any mismatch.  Built and run by tests/test_libm.py.
//
// Two modes that do not depend on the host's float libm, so they hold on every host:
// libm_check ulp : the host build against (float)f((double)x), the double libm's value rounded once - cos / sin / atan on every
//   float, atan2 on 2^26 pairs of each of the two shapes above.  Prints "<name> <values> <over_1_ulp> <not_correctly_rounded>";
//   exit code 1 if any value is more than 1 ulp away.
// libm_check checksum <fn> <start> <count> : vs_op_libm_checksum's sum (include/vs_stab.h) computed from the host build of
//   vs_libm.h instead of the device build; prints the sum in decimal.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../video-stab_amd/csrc/vs_libm.h"

using vslibm::f2u;
using vslibm::u2f;

static inline uint64_t rng(uint64_t& s) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1DULL; }
static bool same(float a, float b) { return f2u(a) == f2u(b) || (a != a && b != b); }

// vs_op_libm_checksum's mix and atan2f argument pairs (the definition of k_traj.hip's libm_checksum_kernel)
static inline uint64_t mix(uint64_t i, uint32_t bits) {
    uint64_t z = (i * 0x9E3779B97F4A7C15ull) ^ (uint64_t)bits;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline void pair_of(uint64_t i, float* y, float* x) {
    const uint64_t v = mix(i, 0x5EEDu);
    if (i & 1) { *y = u2f((uint32_t)v); *x = u2f((uint32_t)(v >> 32)); return; }
    float xx = 0.9f + 0.2f * ((float)(v & 0xFFFFFFu) / 16777216.0f);
    float yy = ((float)((v >> 24) & 0xFFFFFFu) / 16777216.0f - 0.5f) * (((v >> 48) & 1) ? 0.5f : 0.02f);
    if ((v >> 49) & 1) { xx = (xx - 1.0f) * 200.0f; yy *= 100.0f; }
    *y = yy; *x = xx;
}

static int checksum_mode(int fn, uint64_t start, uint64_t count, int NT) {
    std::vector<uint64_t> part((size_t)NT, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t] {
        uint64_t acc = 0;
        for (uint64_t i = (uint64_t)t; i < count; i += (uint64_t)NT) {
            const uint64_t idx = start + i;
            float r;
            if (fn == 3) { float y, x; pair_of(idx, &y, &x); r = vslibm::atan2f_ref(y, x); }
            else {
                const float x = u2f((uint32_t)idx);
                r = fn == 0 ? vslibm::cosf_ref(x) : (fn == 1 ? vslibm::sinf_ref(x) : vslibm::atanf_ref(x));
            }
            acc += mix(idx, r != r ? 0x7FC00000u : f2u(r));
        }
        part[(size_t)t] = acc;
    });
    for (auto& x : th) x.join();
    uint64_t h = 0;
    for (uint64_t p : part) h += p;
    printf("%llu\n", (unsigned long long)h);
    return 0;
}

// distance in ulps between two floats (the bit patterns mapped to a monotonic integer line); NaN against NaN is 0
static uint64_t ulps(float a, float b) {
    if (a != a || b != b) return (a != a && b != b) ? 0 : ~0ull;
    auto key = [](float f) { const uint32_t u = f2u(f); return (int64_t)((u & 0x80000000u) ? -(int64_t)(u & 0x7FFFFFFFu) : (int64_t)u); };
    const int64_t d = key(a) - key(b);
    return (uint64_t)(d < 0 ? -d : d);
}

static int ulp_mode(int NT) {
    std::atomic<long> over[4] = {{0}, {0}, {0}, {0}}, inexact[4] = {{0}, {0}, {0}, {0}};
    const long npairs = 1l << 26;
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t] {
        long o[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
        auto count = [&](int k, float got, float want) {
            const uint64_t d = ulps(got, want);
            if (d > 1) o[k]++;
            if (d != 0) e[k]++;
        };
        for (uint64_t u = (uint64_t)t; u < (1ull << 32); u += (uint64_t)NT) {
            const float x = u2f((uint32_t)u);
            const double xd = (double)x;
            count(0, vslibm::cosf_ref(x), (float)cos(xd));
            count(1, vslibm::sinf_ref(x), (float)sin(xd));
            count(2, vslibm::atanf_ref(x), (float)atan(xd));
        }
        for (long i = t; i < 2 * npairs; i += NT) {
            float y, x;
            pair_of((uint64_t)i, &y, &x);
            count(3, vslibm::atan2f_ref(y, x), (float)atan2((double)y, (double)x));
        }
        for (int k = 0; k < 4; k++) { over[k] += o[k]; inexact[k] += e[k]; }
    });
    for (auto& x : th) x.join();
    const char* names[4] = {"cosf", "sinf", "atanf", "atan2f"};
    long total = 0;
    for (int k = 0; k < 4; k++) {
        printf("%s %s %ld %ld\n", names[k], k < 3 ? "4294967296" : "134217728", over[k].load(), inexact[k].load());
        total += over[k].load();
    }
    return total ? 1 : 0;
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "all";
    {
        int NT = (int)std::thread::hardware_concurrency();
        if (NT < 1) NT = 1;
        if (NT > 16) NT = 16;
        if (!strcmp(what, "ulp")) return ulp_mode(NT);
        if (!strcmp(what, "checksum")) {
            if (argc != 5) { fprintf(stderr, "usage: libm_check checksum <fn> <start> <count>\n"); return 2; }
            return checksum_mode(atoi(argv[2]), strtoull(argv[3], nullptr, 0), strtoull(argv[4], nullptr, 0), NT);
        }
    }
    // "quick": every 256th float and 2^22 pairs - the sanitizer run of `make asan`
    const bool quick = !strcmp(what, "quick");
    if (quick) what = "all";
    const uint64_t fstep = quick ? 256 : 1;
    int NT = (int)std::thread::hardware_concurrency();
    if (NT < 1) NT = 1;
    if (NT > 16) NT = 16;
    std::atomic<long> bad[4] = {{0}, {0}, {0}, {0}};
    const bool all = !strcmp(what, "all");
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t] {
        long b[4] = {0, 0, 0, 0};
        const bool dc = all || !strcmp(what, "cos"), ds = all || !strcmp(what, "sin"), da = all || !strcmp(what, "atan");
        if (dc || ds || da)
            for (uint64_t u = (uint64_t)t * fstep; u < (1ull << 32); u += (uint64_t)NT * fstep) {
                volatile float x = u2f((uint32_t)u);
                if (dc && !same(cosf(x), vslibm::cosf_ref(x))) b[0]++;
                if (ds && !same(sinf(x), vslibm::sinf_ref(x))) b[1]++;
                if (da && !same(atanf(x), vslibm::atanf_ref(x))) b[2]++;
            }
        if (all || !strcmp(what, "atan2")) {
            uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1);
            const long n = (quick ? (1l << 21) : (1l << 30)) / NT;
            for (long i = 0; i < n; i++) {
                const uint64_t v = rng(s);
                volatile float y = u2f((uint32_t)v), x = u2f((uint32_t)(v >> 32));
                if (!same(atan2f(y, x), vslibm::atan2f_ref(y, x))) b[3]++;
            }
            for (long i = 0; i < n; i++) {
                const uint64_t v = rng(s);
                float xx = 0.9f + 0.2f * ((v & 0xFFFFFF) / 16777216.0f), yy = (((v >> 24) & 0xFFFFFF) / 16777216.0f - 0.5f) * (((v >> 48) & 1) ? 0.5f : 0.02f);
                if ((v >> 49) & 1) { xx = (xx - 1.0f) * 200.0f; yy *= 100.0f; }
                volatile float y = yy, x = xx;
                if (!same(atan2f(y, x), vslibm::atan2f_ref(y, x))) b[3]++;
            }
        }
        for (int i = 0; i < 4; i++) bad[i] += b[i];
    });
    for (auto& x : th) x.join();
    const char* names[4] = {"cosf", "sinf", "atanf", "atan2f"};
    long total = 0;
    for (int i = 0; i < 4; i++) {
        const bool ran = all || !strcmp(what, i == 0 ? "cos" : i == 1 ? "sin" : i == 2 ? "atan" : "atan2");
        if (ran) printf("%s %s %ld\n", names[i], quick ? "sampled" : (i < 3 ? "4294967296" : "2147483648"), bad[i].load());
        total += bad[i].load();
    }
    return total ? 1 : 0;
}
