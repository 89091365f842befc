"""Edge fill on YUV surfaces at 3840 x 2160 (DESIGN section 8 "Edge fill on YUV", profiles/r29_yuvfill_*).

1. The operator: vs_op_warp_affine_yuv_fill over 32 surfaces (NV12, P010) next to the VS_BORDER_BLACK operator of the same surfaces
   and matrices (vs_op_warp_affine_nv12 / vs_op_warp_affine_p010): the same table launch and one warp launch each - the fill
   instance of the one-launch kernel against the zero instance.  Windows of ITERS calls between two device events on the null
   stream, after a warm-up, alternating, REPS of each.  The matrices are a stabilizer's: a fraction of a degree and a few pixels.
2. The stream: NV12 and P010 streams in batch mode (64 frames a step, zero-copy, frames resident in HBM) with the mode off and on,
   frames/s over STEPS steps after a warm-up, alternating in one process.
  python scratch/fill_measure.py OUT.json
A library of an earlier build (VS_LAB=1 VS_LIB_PATH=...: the parent commit's, for the baseline of the mode-off stream in the same
session) has no edge fill: the script then measures the zero operator and the mode-off streams alone.
One JSON line per case on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi, synth

W, H, N, ITERS, REPS, WARM = 3840, 2160, 32, 10, 5, 3
BT, NF, STEPS, SWARM = 64, 32, 4, 2

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("fill_measure: no device")
HAVE = hasattr(vs.lib, "vs_op_warp_affine_yuv_fill")
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


ev0, ev1 = C.c_void_p(), C.c_void_p()
hip_ok(hip.hipEventCreate(C.byref(ev0)))
hip_ok(hip.hipEventCreate(C.byref(ev1)))


def window(fn):
    """ms per call of fn over ITERS calls between two events on the null stream."""
    hip_ok(hip.hipEventRecord(ev0, None))
    for _ in range(ITERS):
        fn()
    hip_ok(hip.hipEventRecord(ev1, None))
    hip_ok(hip.hipEventSynchronize(ev1))
    ms = C.c_float()
    hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
    return ms.value / ITERS


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


# the clips: NV12 rendered on the device; P010 = its bytes in the high half of the samples
nv12 = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF, nv12=True)
fb8 = W * H * 3 // 2
p010 = capi.DevBuf(vs, 2 * fb8 * NF)
for i in range(NF):
    p010.upload((nv12.download((fb8,), np.uint8, i * fb8).astype(np.uint16) << 8) | 0x40, 2 * i * fb8)
CLIPS = {"NV12": (capi.FMT_NV12, nv12, 1), "P010": (capi.FMT_P010, p010, 2)}
res = []

# ---- 1. the operator -------------------------------------------------------------------------------------------------------------
a = np.deg2rad(np.linspace(-0.6, 0.6, N))
M = np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a), np.linspace(-14.5, 12.25, N), np.sin(a), np.cos(a), np.linspace(9.75, -11.5, N)], axis=1), np.float32)
for name, (fmt, clip, sb) in CLIPS.items():
    fb = fb8 * sb
    out = capi.DevBuf(vs, fb * N)
    zero_op = vs.lib.vs_op_warp_affine_nv12 if sb == 1 else vs.lib.vs_op_warp_affine_p010

    def black():
        vs.check(zero_op(clip.ptr, W * sb, out.ptr, W * sb, W, H, capi._p(M, capi.f32p), N, fb, fb, None))

    def fill():
        vs.check(vs.lib.vs_op_warp_affine_yuv_fill(fmt, clip.ptr, W * sb, 0, 0, 0, out.ptr, W * sb, 0, 0, 0, W, H, capi._p(M, capi.f32p), N, fb, fb, None, None))
    ops = {"black": black, "fill": fill} if HAVE else {"black": black}
    for fn in ops.values():
        for _ in range(WARM):
            fn()
    vs.sync()
    t = {k: [] for k in ops}
    for _ in range(REPS):
        for k, fn in ops.items():
            t[k].append(window(fn))
    r = {"what": "warp_op_%s" % name.lower(), "w": W, "h": H, "surfaces": N, "calls_per_window": ITERS, "bytes_read_plus_written_per_call": 2 * fb * N,
         "ms_per_call": {k: statistics.median(v) for k, v in t.items()}, "ms_windows": t, "spread": {k: spread(v) for k, v in t.items()}}
    if HAVE:
        r["fill_over_black"] = r["ms_per_call"]["fill"] / r["ms_per_call"]["black"]
    res.append(r)
    print(json.dumps(r), flush=True)
    out.free()


# ---- 2. the streams --------------------------------------------------------------------------------------------------------------
def stream(fmt, clip, fb, pitch, mode):
    s = vs.stabilizer(vs.params(max_corners=400))
    s.set_batch(BT)
    s.set_zero_copy(True)
    if mode:
        s.set_yuv_edge_fill(True)
    out = capi.DevBuf(vs, fb * BT * 2)
    state = {"i": 0, "k": 0}

    def steps(n):
        for _ in range(n * BT):
            i, k = state["i"], state["k"]
            state["k"] = (k + s.push_dev(clip.ptr + (i % NF) * fb, W, H, pitch, fmt, out.ptr + (k % (2 * BT)) * fb, pitch)) % (2 * BT)
            state["i"] = i + 1
        s.sync()
    return s, out, steps


for name, (fmt, clip, sb) in CLIPS.items():
    runs = {"off": stream(fmt, clip, fb8 * sb, W * sb, False)}
    if HAVE:
        runs["on"] = stream(fmt, clip, fb8 * sb, W * sb, True)
    times = {k: [] for k in runs}
    for _, _, steps in runs.values():
        steps(SWARM)
    for _ in range(REPS):
        for k, (_, _, steps) in runs.items():
            t0 = time.perf_counter()
            steps(STEPS)
            times[k].append(time.perf_counter() - t0)
    fps = {k: [STEPS * BT / x for x in v] for k, v in times.items()}
    r = {"what": "stream_batch64_%s" % name.lower(), "w": W, "h": H, "steps_per_window": STEPS, "frames_per_step": BT,
         "frames_per_s": {k: statistics.median(v) for k, v in fps.items()}, "frames_per_s_windows": fps, "spread": {k: spread(v) for k, v in fps.items()}}
    if HAVE:
        r["on_over_off_frames_per_s"] = r["frames_per_s"]["on"] / r["frames_per_s"]["off"]
    res.append(r)
    print(json.dumps(r), flush=True)
    for s, out, _ in runs.values():
        s.close(); out.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
