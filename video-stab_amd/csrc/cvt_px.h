// The per-pixel arithmetic of the colour conversion between YUV samples and 8-bit R, G, B (include/vs_stab.h: the 20-bit fixed
// point of OpenCV's COLOR_YUV2BGR_NV12 / _I420 and COLOR_BGR2YUV_I420, with the fifteen integers of a colour space - BT.601,
// BT.709 or BT.2020, limited or full range; tests/cvtref.py and tests/cvtref_cs.py state it in numpy).  The one place the
// formulas and the clamp rules are written down on the device: k_cvt.hip (the two operators) and k_enhance.hip (the enhancer's
// YUV form) both include it.  The integers come from the host (cvt_resolve, comp_op.cpp) as a kernel argument: wave-uniform, so
// every multiply takes a scalar operand where it took a literal (plain 32-bit multiplies: the 24-bit form measured no faster).
#ifndef VS_CVT_PX_H
#define VS_CVT_PX_H

#include <hip/hip_runtime.h>

namespace vsd {

// The integers of one vs_cvt_colorimetry, in the order of vs_cvt_coefficients; mean: VS_CVT_CHROMA_MEAN (RGB -> YUV).
struct CvtCoef {
    int32_t y_off, cy, rv, gv, gu, bu, yr, yg, yb, ur, ug, ub, vr, vg, vb;
    int32_t mean;
};
// (BT.601, limited), top-left chroma: OpenCV's constants, the ones that are not derived from a rule - what a conversion without a
// descriptor computes with.  A function, so that device code folds the integers into its instructions.
__host__ __device__ constexpr CvtCoef cvt_coef_default() {
    return {16, 1220542, 1673527, 852492, 409993, 2116026, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448, 0};
}

__device__ __forceinline__ int cvt_sat8(int v) { return min(max(v, 0), 255); }

// a 16-bit sample as the byte the conversion reads (P010: shift 8; the low-bit formats: bits - 8, values beyond the range read
// as 255), and the sample written for a byte
__device__ __forceinline__ int cvt_sample_to_byte(int sample, int shift) { return min(sample >> shift, 255); }
__device__ __forceinline__ uint32_t cvt_byte_to_sample(uint32_t byte, int shift) { return byte << shift; }

// YUV -> RGB: the terms of one (U, V) sample, with the rounding half, then one luma sample against them
__device__ __forceinline__ void cvt_chroma_terms(const CvtCoef& k, int u, int v, int& ru, int& gu, int& bu) {
    const int uu = u - 128, vv = v - 128;
    ru = (1 << 19) + k.rv * vv;
    gu = (1 << 19) - k.gv * vv - k.gu * uu;
    bu = (1 << 19) + k.bu * uu;
}
__device__ __forceinline__ void cvt_yuv_px(const CvtCoef& k, int y, int ru, int gu, int bu, int& R, int& G, int& B) {
    const int yp = k.cy * max(0, y - k.y_off);
    R = cvt_sat8((yp + ru) >> 20);
    G = cvt_sat8((yp + gu) >> 20);
    B = cvt_sat8((yp + bu) >> 20);
}

// RGB -> YUV: luma of every pixel; U and V of the sums of R, G, B over the 1 << s pixels of a chroma block (s = 0: of ONE pixel -
// the top-left rule, and 4:4:4 under either rule)
__device__ __forceinline__ int cvt_luma(const CvtCoef& k, int R, int G, int B) {
    return cvt_sat8((k.yr * R + k.yg * G + k.yb * B + (1 << 19) + (k.y_off << 20)) >> 20);
}
__device__ __forceinline__ void cvt_chroma(const CvtCoef& k, int SR, int SG, int SB, int s, int& u, int& v) {
    const int bias = ((1 << 19) << s) + (128 << (20 + s));
    u = cvt_sat8((k.ur * SR + k.ug * SG + k.ub * SB + bias) >> (20 + s));
    v = cvt_sat8((k.vr * SR + k.vg * SG + k.vb * SB + bias) >> (20 + s));
}

}  // namespace vsd
#endif
