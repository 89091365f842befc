// The per-axis tables of the resize to an output size (k_resize.hip; vs_op_resample_jobs, vs_op_resize_yuv, vs_op_resize_rgb):
// for every destination index of one axis the source indices of its K taps, already clamped into the source, and their 11-bit
// coefficients.  K = 2: cv::resize(INTER_LINEAR) as oracle/vso_resize_linear_u8 restates it; K = 8: cv::resize(INTER_LANCZOS4) for
// CV_8U.  The definition is in include/vs_stab.h and tests/resizeref.py states it in numpy and `math`.
//
// Host only, standard headers only: tests/cpp/resize_tables_check.cpp compiles this header alone.  The coefficients come from the
// host's double sin / cos, built without FMA contraction; no device libm ever computes them - the kernels read these tables from
// device memory.
#ifndef VS_RESIZE_TABLES_H
#define VS_RESIZE_TABLES_H

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace vsd {

constexpr int RS_LINEAR = 0, RS_LANCZOS4 = 1;        // enum vs_interp
constexpr int RS_COEF = 2048;                        // INTER_RESIZE_COEF_SCALE
inline int rs_taps(int interp) { return interp == RS_LANCZOS4 ? 8 : 2; }

// saturate_cast<short>(v): rounded to nearest even, saturated
inline int16_t rs_sat_short(float v) {
    const long r = std::lrintf(v);
    return (int16_t)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// The source coordinate of destination index d: the sample index (not clamped) and f in [0, 1)
inline int rs_coord(int d, double scale, float* f) {
    const float v = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)std::floor(v);
    *f = v - (float)s;
    return s;
}
inline double rs_scale(int src, int dst) { return 1.0 / ((double)dst / (double)src); }

// interpolateLanczos4: the eight weights of f, not renormalised after the conversion to 11 bits
inline void rs_lanczos4(float f, int16_t* coef) {
    static const double r = 0.70710678118654752440084436210485, pi = 3.1415926535897932384626433832795;
    static const double cs[8][2] = {{1, 0}, {-r, -r}, {0, 1}, {r, -r}, {-1, 0}, {r, r}, {0, -1}, {-r, r}};
    float w[8];
    if (f < FLT_EPSILON) {
        for (int i = 0; i < 8; i++) w[i] = 0.f;
        w[3] = 1.f;
    } else {
        float sum = 0.f;
        const double y0 = -((double)f + 3.0) * pi * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
        for (int i = 0; i < 8; i++) {
            const double y = -((double)f + 3.0 - (double)i) * pi * 0.25;
            w[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
            sum += w[i];
        }
        sum = 1.f / sum;
        for (int i = 0; i < 8; i++) w[i] *= sum;
    }
    for (int i = 0; i < 8; i++) coef[i] = rs_sat_short(w[i] * (float)RS_COEF);
}

// The table of one axis src -> dst (1 .. 32767 each): idx[d * K + k] and coef[d * K + k], K = rs_taps(interp).
// axis 0 = columns, 1 = rows.  They differ for RS_LINEAR only: columns follow HResizeLinear's edge rule (s < 0: the first sample;
// from the first column whose second tap would leave the source on: the sample itself times 2048), rows keep their coefficients
// and clamp both tap rows.  RS_LANCZOS4 clamps neither s nor f; its taps s - 3 .. s + 4 clamp into the source.
inline void rs_axis_table(int src, int dst, int interp, int axis, int32_t* idx, int16_t* coef) {
    const double scale = rs_scale(src, dst);
    auto clamp = [&](int v) { return v < 0 ? 0 : v > src - 1 ? src - 1 : v; };
    for (int d = 0; d < dst; d++) {
        float f;
        int s = rs_coord(d, scale, &f);
        if (interp == RS_LANCZOS4) {
            rs_lanczos4(f, coef + (size_t)d * 8);
            for (int k = 0; k < 8; k++) idx[(size_t)d * 8 + k] = clamp(s - 3 + k);
            continue;
        }
        int32_t* ix = idx + (size_t)d * 2;
        int16_t* cf = coef + (size_t)d * 2;
        if (axis == 0) {
            bool edge = false;
            if (s < 0) { f = 0.f; s = 0; }
            if (s + 1 >= src) {
                edge = true;
                if (s >= src - 1) { f = 0.f; s = src - 1; }
            }
            ix[0] = s;
            ix[1] = edge ? s : s + 1;
            cf[0] = edge ? (int16_t)RS_COEF : rs_sat_short((1.f - f) * (float)RS_COEF);
            cf[1] = edge ? (int16_t)0 : rs_sat_short(f * (float)RS_COEF);
        } else {
            ix[0] = clamp(s);
            ix[1] = clamp(s + 1);
            cf[0] = rs_sat_short((1.f - f) * (float)RS_COEF);
            cf[1] = rs_sat_short(f * (float)RS_COEF);
        }
    }
}

// ---- area-averaging downscale (vs_op_area_jobs, vs_op_area_yuv, vs_op_area_rgb): cv::resize(INTER_AREA) for dst <= src --------
// The definition is in include/vs_stab.h and tests/arearef.py states it in numpy and `math`; tests/cpp/area_tables_check.cpp
// compiles this part alone.  RS_AREA is the arena's key for these tables in k_resize.hip, not a vs_interp.
constexpr int RS_AREA = 2;

// An axis is integer when scale = 1 / (dst / src) lies within DBL_EPSILON of rint(scale); *i = that integer (then src == i * dst)
inline bool rs_area_integer(int src, int dst, int* i) {
    const double scale = rs_scale(src, dst);
    const long r = std::lrint(scale);
    *i = (int)r;
    return std::fabs(scale - (double)r) < DBL_EPSILON;
}

// The class of a job: 2 = the 2 x 2 mean, 1 = integer box (ix x iy), 0 = general (both axes through the tables)
inline int rs_area_class(int sw, int sh, int dw, int dh, int* ix, int* iy) {
    const bool x = rs_area_integer(sw, dw, ix), y = rs_area_integer(sh, dh, iy);
    if (!x || !y) return 0;
    return *ix == 2 && *iy == 2 ? 2 : 1;
}

// computeResizeAreaTab for one axis src -> dst, 1 <= dst <= src <= 32767.  The taps of destination index d are the `count[d]`
// source samples from first[d] on; tap 0 weighs w_first[d], tap count - 1 (count > 1) w_last[d], every other tap w_mid[d].
// (count == 1: w_last = w_first.  w_mid is 1 / cellWidth whether or not a tap takes it.)
inline void rs_area_axis_table(int src, int dst, int32_t* first, int32_t* count, float* w_first, float* w_mid, float* w_last) {
    const double scale = rs_scale(src, dst);
    for (int d = 0; d < dst; d++) {
        const double f1 = (double)d * scale, f2 = f1 + scale;
        const double cw = std::min(scale, (double)src - f1);
        int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
        s2 = std::min(s2, src - 1);
        s1 = std::min(s1, s2);
        const float mid = (float)(1.0 / cw);
        int n = 0, lo = s1;
        float wf = mid, wl = mid;
        if ((double)s1 - f1 > 1e-3) {
            lo = s1 - 1;
            wf = (float)(((double)s1 - f1) / cw);
            n = 1;
        }
        n += s2 - s1;
        if (f2 - (double)s2 > 1e-3) {
            wl = (float)(std::min(std::min(f2 - (double)s2, 1.0), cw) / cw);
            if (n == 0) { lo = s2; wf = wl; }
            n++;
        }
        first[d] = lo; count[d] = n;
        w_first[d] = wf; w_mid[d] = mid; w_last[d] = n > 1 ? wl : wf;
    }
}

}  // namespace vsd
#endif
