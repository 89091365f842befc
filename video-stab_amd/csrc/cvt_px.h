// The per-pixel arithmetic of the colour conversion between YUV samples and 8-bit R, G, B (include/vs_stab.h: ITU-R BT.601 limited
// range in the 20-bit fixed point of OpenCV's COLOR_YUV2BGR_NV12 / _I420 and COLOR_BGR2YUV_I420; tests/cvtref.py states it in
// numpy).  The one place the constants and the clamp rules are written down on the device: k_cvt.hip (the two operators) and
// k_enhance.hip (the enhancer's YUV form) both include it.
#ifndef VS_CVT_PX_H
#define VS_CVT_PX_H

#include <hip/hip_runtime.h>

namespace vsd {

__device__ __forceinline__ int cvt_sat8(int v) { return min(max(v, 0), 255); }

// a 16-bit sample as the byte the conversion reads (P010: shift 8; the low-bit formats: bits - 8, values beyond the range read
// as 255), and the sample written for a byte
__device__ __forceinline__ int cvt_sample_to_byte(int sample, int shift) { return min(sample >> shift, 255); }
__device__ __forceinline__ uint32_t cvt_byte_to_sample(uint32_t byte, int shift) { return byte << shift; }

// YUV -> RGB: the terms of one (U, V) sample, with the rounding half, then one luma sample against them
__device__ __forceinline__ void cvt_chroma_terms(int u, int v, int& ru, int& gu, int& bu) {
    const int uu = u - 128, vv = v - 128;
    ru = (1 << 19) + 1673527 * vv;
    gu = (1 << 19) - 852492 * vv - 409993 * uu;
    bu = (1 << 19) + 2116026 * uu;
}
__device__ __forceinline__ void cvt_yuv_px(int y, int ru, int gu, int bu, int& R, int& G, int& B) {
    const int yp = max(0, y - 16) * 1220542;
    R = cvt_sat8((yp + ru) >> 20);
    G = cvt_sat8((yp + gu) >> 20);
    B = cvt_sat8((yp + bu) >> 20);
}

// RGB -> YUV: luma of every pixel; U and V of the one pixel at the top-left of a chroma block (no averaging)
__device__ __forceinline__ int cvt_luma(int R, int G, int B) {
    return cvt_sat8((269484 * R + 528482 * G + 102760 * B + (1 << 19) + (16 << 20)) >> 20);
}
__device__ __forceinline__ void cvt_chroma(int R, int G, int B, int& u, int& v) {
    u = cvt_sat8((-155188 * R - 305135 * G + 460324 * B + (1 << 19) + (128 << 20)) >> 20);
    v = cvt_sat8((460324 * R - 385875 * G - 74448 * B + (1 << 19) + (128 << 20)) >> 20);
}

}  // namespace vsd
#endif
