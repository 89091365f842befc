// Device-resident trajectory state of one stream (vs::Stabilizer members
// transforms_, path_, drone-mode state; Stabilizer.h:311-371,418-429).
#ifndef VS_TRAJ_STATE_H
#define VS_TRAJ_STATE_H

#include <stdint.h>

namespace vsd {

constexpr int TRAJ_RING = 256;   // >= 35 (queue) + 50 (drone box radius) + 20, power of two
constexpr int GAUSS_MAX = 63;

struct TrajState {
    int n;                          // transforms_.size() == path_.size()
    float last_path[3];
    float transforms[TRAJ_RING][3];
    float path[TRAJ_RING][3];
    int smoothing_radius;           // params_.smoothingRadius (mutated by adaptSmoothingRadius)
    // incremental Kalman (x0,x1,P00,P01,P10,P11) per component
    float kal[3][6];
    int kal_n[3];
    float kal_last[3];
    // drone mode
    float hfMedian[2];
    float hfRotLP;
    int hfInDeadZone;
    int hfFreezeCounter;
    float hfAccum;
    int hfHistN;
    float hfHist[10][2];
};

struct TrajParams {
    int method;                     // vs_smoothing
    int horizon_lock;
    int drone;
    int adaptive, min_radius, max_radius;
    float hf_shake_px, hf_rot_lp_alpha, hf_dead_zone, hf_decay;
    int hf_freeze_duration;
    int gauss_ksize;
    float gauss_kernel[GAUSS_MAX];
    // The chroma matrix M[6..11] that goes with a frame matrix M: Mc = S^-1 M S for the subsampling S = diag(2^sx, 2^sy) of the
    // stream's chroma planes.  TRAJ_CHROMA_420 (0, what every two-plane and 4:2:0 format has): translation halved; 422: sx 1, sy 0;
    // 444: Mc = M.
    int chroma;
};
enum { TRAJ_CHROMA_420 = 0, TRAJ_CHROMA_422 = 1, TRAJ_CHROMA_444 = 2 };

}  // namespace vsd
#endif
