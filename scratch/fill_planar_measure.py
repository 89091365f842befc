"""The edge-fill operator on planar surfaces at 3840 x 2160 (profiles/r32_warp_bodies_bench_lines_ab.txt): vs_op_warp_affine_yuv_fill over
32 surfaces of I420, I422, I444, I010 and I210 - the warp_i420_fill_kernel instances of k_warp.hip - and of NV12 and P010
(warp_nv12_fill_kernel) beside them, under a stabilizer's maps: a fraction of a degree and a few pixels.  Windows of ITERS calls between
two device events on the null stream, REPS of them behind WARM warm-up calls; random content (the kernel's time does not depend on it).
  python scratch/fill_planar_measure.py [OUT.json]
To compare two builds, run it once per library (VS_LAB=1 VS_LIB_PATH=... for the other one), alternating.  One line per format on
stdout; OUT.json holds them all.  Fails without a device."""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

W, H, N, ITERS, REPS, WARM = 3840, 2160, 32, 10, 9, 40
vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("no device")
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
ev0, ev1 = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

def window(fn):
    assert hip.hipEventRecord(ev0, None) == 0
    for _ in range(ITERS):
        fn()
    assert hip.hipEventRecord(ev1, None) == 0
    assert hip.hipEventSynchronize(ev1) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
    return ms.value / ITERS

a = np.deg2rad(np.linspace(-0.6, 0.6, N))
M = np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a), np.linspace(-14.5, 12.25, N), np.sin(a), np.cos(a), np.linspace(9.75, -11.5, N)], axis=1), np.float32)
FORMATS = {"NV12": (capi.FMT_NV12, 1, 1, 1), "P010": (capi.FMT_P010, 1, 1, 2), "I420": (capi.FMT_I420, 1, 1, 1), "I422": (capi.FMT_I422, 1, 0, 1), "I444": (capi.FMT_I444, 0, 0, 1), "I010": (capi.FMT_I010, 1, 1, 2), "I210": (capi.FMT_I210, 1, 0, 2)}
rng = np.random.default_rng(7)
res = {"build": vs.lib.vs_build_tag().decode()}
for name, (fmt, sx, sy, sb) in FORMATS.items():
    fb = (W * H + 2 * (W >> sx) * (H >> sy)) * sb
    one = rng.integers(0, 256, fb, dtype=np.uint8)
    if sb == 2:
        one[1::2] &= 3                      # ten-bit samples
    d_in, d_out = capi.DevBuf(vs, fb * N), capi.DevBuf(vs, fb * N)
    for i in range(N):
        d_in.upload(np.roll(one, 2 * sb * i), i * fb)

    def fill():
        vs.check(vs.lib.vs_op_warp_affine_yuv_fill(fmt, d_in.ptr, W * sb, 0, 0, 0, d_out.ptr, W * sb, 0, 0, 0, W, H, capi._p(M, capi.f32p), N, fb, fb, None, None))
    for _ in range(WARM):
        fill()
    vs.sync()
    t = [window(fill) for _ in range(REPS)]
    res[name] = {"ms_per_call_median": statistics.median(t), "ms_windows": t}
    print(name, json.dumps(res[name]), flush=True)
    d_in.free(); d_out.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
