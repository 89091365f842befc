"""Border pad on YUV surfaces at 3840 x 2160 with border_size 30 (DESIGN section 8 "Border pad on YUV", profiles/r25_yuvpad_*).

1. The k_yuvpad launch of 32 surfaces (vs_op_pad_jobs: 64 jobs for NV12 / P010, 96 for I210) with VS_BORDER_BLACK and
   VS_BORDER_REFLECT, sources in the stream's packed input layout, destinations in its scratch layout (rows of whole 256-byte
   lines).  The yardstick is vs_dev_copy_rate in the same process for the bytes the launch WRITES: a device copy of that many bytes
   reads and writes twice that, so copy_ms = 2 * written / rate.  Pad windows (ITERS launches between two device events on the null
   stream, after a warm-up) and yardstick calls alternate, REPS of each.
2. Context: an NV12 stream in batch mode (32 frames a step, zero-copy, frames resident in HBM) with the mode on next to the same
   stream with border_size = 0, and the BGR8 pad stream of the same clip, frames/s over STEPS steps after a warm-up, alternated.
  python scratch/pad_measure.py OUT.json
One JSON line per case on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi, synth

W, H, B, N, ITERS, REPS, WARM = 3840, 2160, 30, 32, 20, 5, 3
PW, PH = W + 2 * B, H + 2 * B
FORMATS = ["NV12", "P010", "I210"]
MODES = {"black": 0, "reflect": 1}
PITCH_ALIGN = 256

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("pad_measure: no device")
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


def copy_rate(nbytes):
    r = C.c_double()
    vs.check(vs.lib.vs_dev_copy_rate(nbytes, ITERS, C.byref(r)))
    return r.value


def pool(nbytes, fill):
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(N)]
    if fill:
        one = np.random.default_rng(nbytes % 9973).integers(0, 256, nbytes, np.uint8)
        for k, b in enumerate(bufs):
            b.upload(np.roll(one, 4099 * k))
    return bufs


def planes(name):
    """(plane w, plane h, cn, bx, by) per plane of a W x H surface with border B."""
    f = capi.PIXFMT_BY_NAME[name]
    luma = (W, H, 1, B, B)
    chroma = (W >> f.sx, H >> f.sy, 1, B >> f.sx, B >> f.sy)
    if name in ("NV12", "P010"):
        return f, [luma, chroma[:2] + (2,) + chroma[3:]]
    return f, [luma, chroma, chroma]


res = []
for name in FORMATS:
    f, pl = planes(name)
    sb = f.sample_bytes
    offs_s, offs_d, ss, ds = [], [], 0, 0
    lp = -(-(PW * sb) // PITCH_ALIGN) * PITCH_ALIGN
    for k, (pw, ph, cn, bx, by) in enumerate(pl):
        sp = W * sb if k == 0 or cn == 2 else (W * sb) >> f.sx
        dp = lp if k == 0 or cn == 2 else lp >> f.sx        # (the interleaved plane has the luma pitch, a chroma plane pitch >> sx)
        offs_s.append((ss, sp)); ss += sp * ph
        offs_d.append((ds, dp)); ds += dp * (ph + 2 * by)
    d_src, d_dst = pool(ss, True), pool(ds, False)
    read = sum(pw * ph * cn * sb for pw, ph, cn, _, _ in pl)
    written = sum((pw + 2 * bx) * (ph + 2 * by) * cn * sb for pw, ph, cn, bx, by in pl)
    for mname, mode in MODES.items():
        jobs = []
        for a, b in zip(d_src, d_dst):
            for (so, sp), (do, dp), (pw, ph, cn, bx, by) in zip(offs_s, offs_d, pl):
                jobs.append((a.ptr + so, sp, pw, ph, b.ptr + do, dp, bx, by, cn, mode, (16 << (8 * (sb - 1)), 128 << (8 * (sb - 1)))))
        arr = (capi.VsPadJob * len(jobs))()
        for a, (src, s_p, sw, sh, dst, d_p, bx, by, cn, border, fill) in zip(arr, jobs):
            a.src, a.src_stride, a.sw, a.sh, a.dst, a.dst_stride, a.bx, a.by, a.cn, a.border = src, s_p, sw, sh, dst, d_p, bx, by, cn, border
            a.fill[0], a.fill[1] = fill

        def pad():
            vs.check(vs.lib.vs_op_pad_jobs(arr, len(jobs), sb, None))
        for _ in range(WARM):
            pad()
        vs.sync()
        copy_rate(N * written)
        t_p, rates = [], []
        for _ in range(REPS):
            t_p.append(window(pad))
            rates.append(copy_rate(N * written))
        m_p, rate = statistics.median(t_p), statistics.median(rates)
        copy_ms = 2 * N * written / rate / 1e6
        r = {"what": "yuvpad_%s_%s" % (name.lower(), mname), "w": W, "h": H, "border": B, "surfaces": N, "jobs": len(jobs), "launches_per_window": ITERS,
             "bytes_read_per_launch": N * read, "bytes_written_per_launch": N * written, "pad_ms_per_launch": m_p, "pad_ms_windows": t_p,
             "pad_gbytes_per_s_read_plus_written": N * (read + written) / m_p / 1e6, "copy_rate_gbytes_per_s": rate, "copy_rate_calls": rates,
             "copy_ms_of_the_written_bytes": copy_ms, "pad_over_copy": m_p / copy_ms}
        res.append(r)
        print(json.dumps(r), flush=True)
    for b in d_src + d_dst:
        b.free()

# ---- context: streams in batch mode ----------------------------------------------------------------------------------------------
BT, NF, STEPS, SWARM = 32, 32, 6, 3


def stream(fmt, clip, fb, pitch, fb_out, out_pitch, **params):
    s = vs.stabilizer(vs.params(max_corners=400, **params))
    s.set_batch(BT)
    s.set_zero_copy(True)
    if fmt == capi.FMT_NV12 and params.get("border_size"):
        s.set_yuv_border_pad(True)
    out = capi.DevBuf(vs, fb_out * BT * 2)
    state = {"i": 0, "k": 0}

    def steps(n):
        for _ in range(n * BT):
            i, k = state["i"], state["k"]
            state["k"] = (k + s.push_dev(clip.ptr + (i % NF) * fb, W, H, pitch, fmt, out.ptr + (k % (2 * BT)) * fb_out, out_pitch)) % (2 * BT)
            state["i"] = i + 1
        s.sync()
    return s, out, steps


nv12 = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF, nv12=True)
bgr = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF)
fb_nv, fb_bgr = W * H * 3 // 2, W * H * 3
runs = {"nv12_border0": stream(capi.FMT_NV12, nv12, fb_nv, W, fb_nv, W),
        "nv12_pad_b30": stream(capi.FMT_NV12, nv12, fb_nv, W, PW * PH * 3 // 2, PW, border_size=B),
        "bgr8_pad_b30": stream(capi.FMT_BGR8, bgr, fb_bgr, 3 * W, 3 * PW * PH, 3 * PW, border_size=B)}
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
