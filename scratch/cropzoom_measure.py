"""Crop-and-zoom on YUV surfaces at 3840 x 2160 with border_size 30 (DESIGN section 8 "Crop-and-zoom on YUV", profiles/cropzoom_*).

1. The k_cropzoom launch of 32 surfaces (vs_op_resize_jobs: 64 jobs for NV12 / P010, 96 for I420 / I210) next to hipMemcpyAsync
   device-to-device copies that read plus write the same number of bytes - read: the crops, written: the surfaces - in the same
   process.  Zoom and copy alternate, REPS windows of ITERS launches each, timed with device events on the null stream after a
   warm-up; every window moves more than the Infinity Cache holds.
2. Context: an NV12 stream in batch mode (32 frames a step, zero-copy, frames resident in HBM) with the mode on next to the same
   stream with border_size = 0, and the BGR8 crop-and-zoom stream of the same size (which resizes frame by frame), frames/s over
   STEPS steps after a warm-up, alternated.
  python scratch/cropzoom_measure.py OUT.json
One JSON line per case on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi, synth

W, H, B, N, ITERS, REPS, WARM = 3840, 2160, 30, 32, 20, 5, 3
FORMATS = ["NV12", "P010", "I420", "I210"]
PITCH_ALIGN = 256

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("cropzoom_measure: no device")
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
D2D = 3         # hipMemcpyDeviceToDevice


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


def pool(nbytes, fill):
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(N)]
    if fill:
        one = np.random.default_rng(nbytes % 9973).integers(0, 256, nbytes, np.uint8)
        for k, b in enumerate(bufs):
            b.upload(np.roll(one, 4099 * k))
    return bufs


def planes(name):
    """(plane w, plane h, cn, x, y of the crop, crop w, crop h) per plane of a W x H surface with border B."""
    f = capi.PIXFMT_BY_NAME[name]
    luma = (W, H, 1, B, B, W - 2 * B, H - 2 * B)
    cw, ch = W >> f.sx, H >> f.sy
    chroma = (cw, ch, 1, B >> f.sx, B >> f.sy, (W - 2 * B) >> f.sx, (H - 2 * B) >> f.sy)
    if name in ("NV12", "P010"):
        return f, [luma, chroma[:2] + (2,) + chroma[3:]]
    return f, [luma, chroma, chroma]


res = []
for name in FORMATS:
    f, pl = planes(name)
    sb = f.sample_bytes
    # scratch surfaces as the stream lays them out (rows of whole 256-byte lines, planes one behind the other); results packed
    offs_s, offs_d, ss, ds = [], [], 0, 0
    lp = -(-(W * sb) // PITCH_ALIGN) * PITCH_ALIGN
    for k, (pw, ph, cn, *_) in enumerate(pl):
        sp = lp if k == 0 or cn == 2 else lp >> f.sx       # (the interleaved plane has the luma pitch, a chroma plane pitch >> sx)
        offs_s.append((ss, sp)); ss += sp * ph
        offs_d.append((ds, pw * cn * sb)); ds += pw * cn * sb * ph
    d_src, d_dst = pool(ss, True), pool(ds, False)
    jobs = []
    for a, b in zip(d_src, d_dst):
        for (so, sp), (do, dp), (pw, ph, cn, x, y, cw, ch) in zip(offs_s, offs_d, pl):
            jobs.append((a.ptr + so + y * sp + x * cn * sb, sp, cw, ch, b.ptr + do, dp, pw, ph, cn))
    arr = vs._scale_job_array(jobs)
    read = sum(cw * ch * cn * sb for _, _, cn, _, _, cw, ch in pl)
    half = (read + ds) // 2 // 256 * 256                 # a copy of `half` bytes reads and writes read + written
    c_src, c_dst = pool(half, True), pool(half, False)

    def zoom():
        vs.check(vs.lib.vs_op_resize_jobs(arr, len(jobs), sb, None))

    def copy():
        for a, b in zip(c_src, c_dst):
            hip_ok(hip.hipMemcpyAsync(b.ptr, a.ptr, half, D2D, None))
    for _ in range(WARM):
        zoom()
        copy()
    vs.sync()
    t_z, t_c = [], []
    for _ in range(REPS):
        t_z.append(window(zoom))
        t_c.append(window(copy))
    moved = N * (read + ds)
    m_z, m_c = statistics.median(t_z), statistics.median(t_c)
    r = {"what": "cropzoom_" + name.lower(), "w": W, "h": H, "border": B, "surfaces": N, "jobs": len(jobs), "launches_per_window": ITERS,
         "bytes_read_plus_written_per_launch": moved, "zoom_ms_per_launch": m_z, "zoom_ms_windows": t_z, "zoom_gbytes_per_s": moved / m_z / 1e6,
         "copy_ms_same_bytes": m_c, "copy_ms_windows": t_c, "copy_gbytes_per_s": moved / m_c / 1e6, "zoom_over_copy": m_z / m_c}
    res.append(r)
    print(json.dumps(r), flush=True)
    for b in d_src + d_dst + c_src + c_dst:
        b.free()

# ---- context: streams in batch mode ----------------------------------------------------------------------------------------------
BT, NF, STEPS, SWARM = 32, 32, 6, 3


def stream(fmt, clip, fb, pitch, **params):
    s = vs.stabilizer(vs.params(max_corners=400, **params))
    s.set_batch(BT)
    s.set_zero_copy(True)
    if fmt == capi.FMT_NV12 and params.get("border_size"):
        s.set_yuv_crop_zoom(True)
    out = capi.DevBuf(vs, fb * BT * 2)
    state = {"i": 0, "k": 0}

    def steps(n):
        for _ in range(n * BT):
            i, k = state["i"], state["k"]
            state["k"] = (k + s.push_dev(clip.ptr + (i % NF) * fb, W, H, pitch, fmt, out.ptr + (k % (2 * BT)) * fb, pitch)) % (2 * BT)
            state["i"] = i + 1
        s.sync()
    return s, out, steps


nv12 = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF, nv12=True)
bgr = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF)
fb_nv, fb_bgr = W * H * 3 // 2, W * H * 3
runs = {"nv12_border0": stream(capi.FMT_NV12, nv12, fb_nv, W), "nv12_cropzoom_b30": stream(capi.FMT_NV12, nv12, fb_nv, W, border_size=B, crop_n_zoom=1),
        "bgr8_cropzoom_b30": stream(capi.FMT_BGR8, bgr, fb_bgr, 3 * W, border_size=B, crop_n_zoom=1)}
times = {k: [] for k in runs}
for k, (_, _, steps) in runs.items():
    steps(SWARM)
for _ in range(REPS):
    for k, (_, _, steps) in runs.items():
        t0 = time.perf_counter()
        steps(STEPS)
        times[k].append(time.perf_counter() - t0)
r = {"what": "streams_batch32", "w": W, "h": H, "border": B, "steps_per_window": STEPS, "frames_per_step": BT,
     "frames_per_s": {k: STEPS * BT / statistics.median(v) for k, v in times.items()},
     "frames_per_s_windows": {k: [STEPS * BT / t for t in v] for k, v in times.items()}}
res.append(r)
print(json.dumps(r), flush=True)
for s, out, _ in runs.values():
    s.close(); out.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
