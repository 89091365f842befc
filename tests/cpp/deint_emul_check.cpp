// The deinterlace / weave kernel of csrc/k_deint.hip run on the host, lane by lane, against a per-pixel loop written from the
// definition in include/vs_stab.h - so that AddressSanitizer sees every load and store of the kernel body (`make asan-host`).
// The kernel has no barrier and no LDS, so calling its body once per (workgroup, wave, lane) in any order is what the device does.
// Every plane is an allocation of exactly (h - 1) * stride + row bytes at an odd offset: a byte read outside w x h of a source or
// written outside w x h of the destination is a sanitizer report or a difference.
//
//   clang++ -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I include -I <rocm>/include -I video-stab_amd/csrc \
//       tests/cpp/deint_emul_check.cpp -o deint_emul_check && ./deint_emul_check
//
// Needs clang (the kernel uses ext_vector_type and __builtin_nontemporal_store); no GPU, no HIP runtime library.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

// ---- what the device compiler provides ------------------------------------------------------------------------------------
#ifndef __launch_bounds__
#define __launch_bounds__(...)
#endif
struct EmIdx { unsigned x, y, z; };
static EmIdx threadIdx, blockIdx;
using std::max;
using std::min;
namespace vsd {
inline uint32_t xcd_seq(uint32_t lin, uint32_t n) {            // vs_common.h's, which is device-only there
    const uint32_t c = lin & 7u, k = lin >> 3, q = n >> 3, r = n & 7u;
    return c * q + (c < r ? c : r) + k;
}
}  // namespace vsd
static long em_lanes = 0;
template <class K, class A>
void em_launch(K kernel, dim3 grid, dim3 block, const A& args) {
    for (unsigned b = 0; b < grid.x; b++)
        for (unsigned ty = 0; ty < block.y; ty++)
            for (unsigned tx = 0; tx < block.x; tx++) {
                blockIdx = {b, 0, 0};
                threadIdx = {tx, ty, 0};
                kernel(args);
                em_lanes++;
            }
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, st, args) em_launch([](const auto& a) { kernel(a); }, grid, block, args)
#define hipGetLastError() hipSuccess

#include "../../video-stab_amd/csrc/k_deint.hip"

// ---- what the rest of the library provides ----------------------------------------------------------------------------------
static std::string em_error;
namespace vsd {
void set_last_error(const std::string& msg) { em_error = msg; }
const char* get_last_error() { return em_error.c_str(); }
int ensure_device() { return VS_OK; }
int cvt_check_yuv(const char*, int, const void* const*, int, const vs_i420_layout*, int, int, I420Layout*, std::string*) { return VS_ERR_INVALID_ARG; }
}  // namespace vsd
extern "C" const char* hipGetErrorString(hipError_t) { return "hip"; }

// ---- the definition, pixel by pixel -------------------------------------------------------------------------------------------
template <class T>
struct EmPlane {
    int w, h, cn;
    size_t stride;                 // bytes
    std::vector<uint8_t> mem;      // exactly the plane's span behind `off` bytes
    size_t off;
    uint8_t* base() { return mem.data() + off; }
    T& at(int y, int i) { return *reinterpret_cast<T*>(base() + (size_t)y * stride + (size_t)i * sizeof(T)); }
};
template <class T>
EmPlane<T> make_plane(int w, int h, int cn, size_t pad, std::mt19937& rng, int bits) {
    EmPlane<T> p{w, h, cn, (size_t)w * cn * sizeof(T) + pad * sizeof(T), {}, sizeof(T) == 1 ? 3u : 2u};
    p.mem.resize(p.off + (size_t)(h - 1) * p.stride + (size_t)w * cn * sizeof(T));
    for (auto& b : p.mem) b = (uint8_t)rng();
    if (bits < 16 && sizeof(T) == 2)
        for (int y = 0; y < h; y++)
            for (int i = 0; i < w * cn; i++) p.at(y, i) &= (T)((1u << bits) - 1u);
    return p;
}

template <class T>
int ref_sample(EmPlane<T>& P, EmPlane<T>& C, EmPlane<T>& N, int y, int i, int second, int mode) {
    const int h = C.h, w = C.w, cn = C.cn, x = i / cn;
    const int up = y > 0 ? y - 1 : y + 1, dn = y + 1 < h ? y + 1 : y - 1;
    const int c = C.at(up, i), e = C.at(dn, i);
    if (mode == VS_DEINT_LINEAR) return (c + e + 1) >> 1;
    EmPlane<T>& A = second ? C : P;
    EmPlane<T>& B = second ? N : C;
    const int d = (A.at(y, i) + B.at(y, i)) >> 1;
    const int td0 = std::abs((int)A.at(y, i) - (int)B.at(y, i));
    const int td1 = (std::abs((int)P.at(up, i) - c) + std::abs((int)P.at(dn, i) - e)) >> 1;
    const int td2 = (std::abs((int)N.at(up, i) - c) + std::abs((int)N.at(dn, i) - e)) >> 1;
    int diff = std::max({td0 >> 1, td1, td2});
    int sp = (c + e) >> 1;
    if (x >= 3 && x < w - 3) {
        auto score = [&](int j) {
            int s = 0;
            for (int k = -1; k <= 1; k++) s += std::abs((int)C.at(up, i + (k + j) * cn) - (int)C.at(dn, i + (k - j) * cn));
            return s;
        };
        int best = score(0) - 1;
        for (int g = -1; g <= 1; g += 2)
            if (score(g) < best) {
                best = score(g);
                sp = (C.at(up, i + g * cn) + C.at(dn, i - g * cn)) >> 1;
                if (score(2 * g) < best) {
                    best = score(2 * g);
                    sp = (C.at(up, i + 2 * g * cn) + C.at(dn, i - 2 * g * cn)) >> 1;
                }
            }
    }
    if (!(y == 1 || y + 2 == h)) {
        const int upp = y + 2 * (up - y), dnn = y + 2 * (dn - y);
        const int b = (A.at(upp, i) + B.at(upp, i)) >> 1, f = (A.at(dnn, i) + B.at(dnn, i)) >> 1;
        const int mx = std::max({d - e, d - c, std::min(b - c, f - e)}), mn = std::min({d - e, d - c, std::max(b - c, f - e)});
        diff = std::max({diff, mn, -mx});
    }
    return sp > d + diff ? d + diff : sp < d - diff ? d - diff : sp;
}

static long failures = 0, checked = 0;

// One launch of the jobs of `shapes` (w, h, cn), every (keep, second) or the weave, against the loop
template <class T>
void run(const std::vector<std::array<int, 3>>& shapes, int mode, int bits, unsigned seed, int nulls) {
    std::mt19937 rng(seed);
    struct Case { EmPlane<T> P, C, N, D, want; int keep, second; };
    std::vector<Case> cases;
    for (const auto& s : shapes)
        for (int ks = 0; ks < (mode == 2 ? 2 : 4); ks++) {
            Case q{make_plane<T>(s[0], s[1], s[2], 1, rng, bits), make_plane<T>(s[0], s[1], s[2], 3, rng, bits), make_plane<T>(s[0], s[1], s[2], 0, rng, bits),
                   make_plane<T>(s[0], s[1], s[2], 5, rng, bits), {}, ks & 1, ks >> 1};
            cases.push_back(std::move(q));
        }
    std::vector<vs_deint_job> jobs;
    for (Case& q : cases) {
        const bool np = nulls & 1, nn = (nulls & 2) && mode != 2;
        EmPlane<T>& P = np ? q.C : q.P;
        EmPlane<T>& N = nn ? q.C : q.N;
        q.want = q.D;                                                   // bytes between the rows stay what they were
        for (int y = 0; y < q.C.h; y++)
            for (int i = 0; i < q.C.w * q.C.cn; i++)
                q.want.at(y, i) = mode == 2 ? ((y & 1) == q.keep ? q.C.at(y, i) : N.at(y, i))
                                            : (y & 1) == q.keep ? q.C.at(y, i) : (T)ref_sample(P, q.C, N, y, i, q.second, mode);
        jobs.push_back(vs_deint_job{np ? nullptr : q.P.base(), q.P.stride, q.C.base(), q.C.stride, nn ? nullptr : q.N.base(), q.N.stride, q.D.base(), q.D.stride,
                                    q.C.w, q.C.h, q.C.cn, q.keep, q.second, 0});
    }
    for (size_t at = 0; at < jobs.size(); at += 96) {
        const int n = (int)std::min<size_t>(96, jobs.size() - at);
        const int rc = vsd::launch_deint("deint_emul_check", jobs.data() + at, n, (int)sizeof(T), mode, nullptr);
        if (rc != VS_OK) { std::printf("launch refused: %s\n", em_error.c_str()); failures++; return; }
    }
    for (Case& q : cases) {
        checked++;
        if (q.D.mem != q.want.mem) {
            failures++;
            size_t k = 0;
            while (q.D.mem[k] == q.want.mem[k]) k++;
            const size_t rel = k - q.D.off;
            if (failures < 20)
                std::printf("DIFFERS: u%d cn %d %d x %d mode %d keep %d second %d nulls %d: first at row %zu byte %zu: got %d want %d\n", (int)sizeof(T) * 8, q.C.cn, q.C.w,
                            q.C.h, mode, q.keep, q.second, nulls, rel / q.D.stride, rel % q.D.stride, q.D.mem[k], q.want.mem[k]);
        }
    }
}

int main() {
    // widths on both sides of 3 + 3 pixels, of a lane's 16 bytes, of the tile's 256 bytes and of two tiles; heights 2 .. 7 and on
    // both sides of a strip (16 rows), of a wave's strips and of the tile (256 rows)
    const int ws[] = {1, 2, 5, 6, 7, 8, 15, 16, 17, 31, 33, 63, 65, 127, 128, 129, 255, 256, 257, 515};
    const int hs[] = {2, 3, 4, 5, 6, 7, 15, 16, 17, 18, 31, 33, 63, 65, 255, 256, 257, 258};
    unsigned seed = 1;
    for (int mode = 0; mode <= 2; mode++)
        for (int cn = 1; cn <= 4; cn++) {
            std::vector<std::array<int, 3>> wide, tall;
            for (int w : ws) wide.push_back({w, 2 + (w % 9), cn});
            for (int h : hs) tall.push_back({h < 100 ? 7 + h : 9, h, cn});
            for (int nulls = 0; nulls < 4; nulls++) {
                run<uint8_t>(wide, mode, 8, seed++, nulls);
                run<uint8_t>(tall, mode, 8, seed++, nulls);
                if (cn <= 2) {
                    run<uint16_t>(wide, mode, 16, seed++, nulls);
                    run<uint16_t>(tall, mode, nulls & 1 ? 10 : 16, seed++, nulls);
                }
            }
        }
    std::printf("deint_emul_check: %ld planes, %ld lanes run, %ld differ\n", checked, em_lanes, failures);
    return failures ? 1 : 0;
}
