"""The fade border on YUV surfaces at 3840 x 2160 with border_size 30 (DESIGN section 8 "Fade on YUV", profiles/r26_yuvfade_*).

1. The two k_yuvfade launches of ONE surface, as a stream queues them (vs_op_fade_blend_jobs / vs_op_fade_update_jobs: 2 jobs for
   NV12 / P010), sources in the stream's packed input layout, history and destination in its scratch layout (rows of whole 256-byte
   lines), results in the packed padded layout.  A launch rotates over POOL sets of surfaces, more than the last-level cache holds.
   The yardstick is vs_dev_copy_rate in the same process for the bytes the launch MOVES: the blend reads the source and the padded
   history and writes the padded surface, the update reads history and result and writes the history; a device copy of m bytes
   moves 2 m, so copy_ms = moved / rate.  Windows (ITERS launches between two device events on the null stream, after a warm-up) and
   yardstick calls alternate, REPS of each.
2. NV12 only: the route the library had before the fused kernel for the same padded, blended surface - vs_op_pad_jobs into a packed
   padded surface, then vs_op_fade_blend in place over its bytes: four plane passes where the fused launch makes three.
3. Context: the 4K NV12 stream per frame (batch 1, zero-copy, frames resident in HBM) with the fade border next to the same stream
   with the VS_BORDER_BLACK border pad, frames/s, alternated.
  python scratch/fade_measure.py OUT.json
One JSON line per case on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi, synth

W, H, B, POOL, ITERS, REPS, WARM = 3840, 2160, 30, 8, 40, 5, 3
PW, PH = W + 2 * B, H + 2 * B
FORMATS = ["NV12", "P010"]
PITCH_ALIGN = 256
ALPHA = 0.1

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("fade_measure: no device")
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
    for i in range(ITERS):
        fn(i)
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
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(POOL)]
    if fill:
        one = np.random.default_rng(nbytes % 9973).integers(0, 256, nbytes, np.uint8)
        for k, b in enumerate(bufs):
            b.upload(np.roll(one, 4099 * k))
    return bufs


def measure(what, fn, moved, extra):
    for i in range(WARM):
        fn(i)
    vs.sync()
    copy_rate(moved // 2)
    t, rates = [], []
    for _ in range(REPS):
        t.append(window(fn))
        rates.append(copy_rate(moved // 2))
    m, rate = statistics.median(t), statistics.median(rates)
    copy_ms = moved / rate / 1e6
    r = dict(what=what, w=W, h=H, border=B, launches_per_window=ITERS, bytes_moved_per_launch=moved, ms_per_launch=m, ms_windows=t,
             gbytes_per_s_moved=moved / m / 1e6, copy_rate_gbytes_per_s=rate, copy_rate_calls=rates, copy_ms_of_the_moved_bytes=copy_ms, over_copy=m / copy_ms, **extra)
    res.append(r)
    print(json.dumps(r), flush=True)
    return r


res = []
for name in FORMATS:
    f = capi.PIXFMT_BY_NAME[name]
    sb = f.sample_bytes
    lp = -(-(PW * sb) // PITCH_ALIGN) * PITCH_ALIGN
    planes = [(W, H, 1, B, B), (W // 2, H // 2, 2, B // 2, B // 2)]
    src_b, pad_b, out_b = W * sb * H * 3 // 2, lp * PH * 3 // 2, PW * sb * PH * 3 // 2
    d_src, d_hist, d_dst, d_res = pool(src_b, True), pool(pad_b, True), pool(pad_b, False), pool(out_b, True)
    fill = (16 << (8 * (sb - 1)), 128 << (8 * (sb - 1)))
    read = sum(pw * ph * cn * sb for pw, ph, cn, _, _ in planes)
    padded = sum((pw + 2 * bx) * (ph + 2 * by) * cn * sb for pw, ph, cn, bx, by in planes)
    blends, updates = [], []
    for a, hb, d, r in zip(d_src, d_hist, d_dst, d_res):
        bj, uj = (capi.VsFadeJob * 2)(), (capi.VsFadeUpdateJob * 2)()
        for k, (pw, ph, cn, bx, by) in enumerate(planes):
            so, po, ro = k * W * sb * H, k * lp * PH, k * PW * sb * PH
            j = bj[k]
            j.src, j.src_stride, j.sw, j.sh, j.hist, j.hist_stride, j.dst, j.dst_stride = a.ptr + so, W * sb, pw, ph, hb.ptr + po, lp, d.ptr + po, lp
            j.bx, j.by, j.cn = bx, by, cn
            j.fill[0], j.fill[1] = (fill[0], 0) if k == 0 else (fill[1], fill[1])
            u = uj[k]
            u.hist, u.hist_stride, u.res, u.res_stride, u.w, u.h, u.cn = hb.ptr + po, lp, r.ptr + ro, PW * sb, pw + 2 * bx, ph + 2 * by, cn
        blends.append(bj); updates.append(uj)

    def blend(i):
        vs.check(vs.lib.vs_op_fade_blend_jobs(blends[i % POOL], 2, sb, ALPHA, 1.0 - ALPHA, None))

    def update(i):
        vs.check(vs.lib.vs_op_fade_update_jobs(updates[i % POOL], 2, sb, None))
    fused = measure("yuvfade_blend_%s" % name.lower(), blend, read + 2 * padded, dict(jobs=2))
    measure("yuvfade_update_%s" % name.lower(), update, 3 * padded, dict(jobs=2))
    if name == "NV12":
        # the route without the fused kernel: pad into a packed padded surface, blend in place with a packed history
        packed = PW * PH * 3 // 2
        d_pk, d_ph = pool((packed + 3) & ~3, False), pool((packed + 3) & ~3, True)
        pads = []
        for a, d in zip(d_src, d_pk):
            pj = (capi.VsPadJob * 2)()
            for k, (pw, ph, cn, bx, by) in enumerate(planes):
                j = pj[k]
                j.src, j.src_stride, j.sw, j.sh, j.dst, j.dst_stride, j.bx, j.by, j.cn, j.border = a.ptr + k * W * H, W, pw, ph, d.ptr + k * PW * PH, PW, bx, by, cn, 0
                j.fill[0], j.fill[1] = (fill[0], 0) if k == 0 else (fill[1], fill[1])
            pads.append(pj)

        def two_launches(i):
            vs.check(vs.lib.vs_op_pad_jobs(pads[i % POOL], 2, 1, None))
            vs.check(vs.lib.vs_op_fade_blend(C.c_void_p(d_ph[i % POOL].ptr), C.c_void_p(d_pk[i % POOL].ptr), (packed + 3) & ~3, ALPHA, 1.0 - ALPHA, None))
        two = measure("pad_then_fade_blend_nv12", two_launches, read + 4 * padded, dict(launches=2))
        r = dict(what="fused_over_two_launches_nv12", fused_ms=fused["ms_per_launch"], two_launches_ms=two["ms_per_launch"], ratio=fused["ms_per_launch"] / two["ms_per_launch"])
        res.append(r)
        print(json.dumps(r), flush=True)
        for b in d_pk + d_ph:
            b.free()
    for b in d_src + d_hist + d_dst + d_res:
        b.free()

if os.environ.get("FADE_MEASURE_KERNELS_ONLY") == "1":          # (a lane-shape variant of the library: the launches alone)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    sys.exit(0)

# ---- context: streams per frame ----------------------------------------------------------------------------------------------------
NF, FRAMES, SWARM = 32, 192, 64


def stream(fade):
    s = vs.stabilizer(vs.params(max_corners=400, border_size=B, border_type=capi.BORDER_FADE if fade else capi.BORDER_BLACK))
    s.set_zero_copy(True)
    if fade:
        s.set_yuv_fade(True)
    else:
        s.set_yuv_border_pad(True)
    out = capi.DevBuf(vs, PW * PH * 3 // 2 * 4)
    state = {"i": 0, "k": 0}

    def frames(n):
        for _ in range(n):
            i, k = state["i"], state["k"]
            state["k"] = (k + s.push_dev(clip.ptr + (i % NF) * fb, W, H, W, capi.FMT_NV12, out.ptr + (k % 4) * (PW * PH * 3 // 2), PW)) % 4
            state["i"] = i + 1
        s.sync()
    return s, out, frames


clip = synth.make_clip_dev(vs, synth.SEED_CONFIG3, W, H, NF, nv12=True)
fb = W * H * 3 // 2
runs = {"nv12_pad_black_b30": stream(False), "nv12_fade_b30": stream(True)}
times = {k: [] for k in runs}
for k, (_, _, frames) in runs.items():
    frames(SWARM)
for _ in range(REPS):
    for k, (_, _, frames) in runs.items():
        t0 = time.perf_counter()
        frames(FRAMES)
        times[k].append(time.perf_counter() - t0)
r = {"what": "streams_per_frame", "w": W, "h": H, "border": B, "frames_per_window": FRAMES,
     "frames_per_s": {k: FRAMES / statistics.median(v) for k, v in times.items()},
     "frames_per_s_windows": {k: [FRAMES / t for t in v] for k, v in times.items()}}
res.append(r)
print(json.dumps(r), flush=True)
for s, out, _ in runs.values():
    s.close(); out.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
