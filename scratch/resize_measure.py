"""The resize to an output size at 3840 x 2160 class sizes (DESIGN section 8 "Resize to an output size", profiles/r33_resize_*).

32 surfaces per call, NV12 and P010, through vs_op_resample_jobs (the jobs vs_op_resize_yuv builds: luma cn 1, the UV plane cn 2):
  a  3900 x 2220 -> 3840 x 2160, LINEAR and LANCZOS4 (the reference's case behind border pad / fade)
  b  3840 x 2160 -> 1920 x 1080, LINEAR (the 2 x 2 mean) and LANCZOS4
  c  3780 x 2100 -> 3840 x 2160, LINEAR, beside vs_op_resize_jobs on the same jobs
  d  path 0 against path 1 for the LANCZOS4 cases of a and b (NV12)
The candidates of a case alternate in one process, REPS windows of ITERS launches each between device events on the null stream
after a warm-up; every time stands against a plain device copy of the bytes the call reads plus writes (vs_dev_copy_rate, same
process).  One JSON line per case on stdout; OUT.json holds the list.  Fails without a device.
  python scratch/resize_measure.py OUT.json"""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

N, ITERS, REPS, WARM = 32, 10, 5, 2
LINEAR, LANCZOS4 = capi.INTERP_LINEAR, capi.INTERP_LANCZOS4

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("resize_measure: no device")
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


def window(fn, iters):
    hip_ok(hip.hipEventRecord(ev0, None))
    for _ in range(iters):
        fn()
    hip_ok(hip.hipEventRecord(ev1, None))
    hip_ok(hip.hipEventSynchronize(ev1))
    ms = C.c_float()
    hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
    return ms.value / iters


def copy_ms(moved):
    """ms of a plain device copy that reads plus writes `moved` bytes."""
    g = C.c_double()
    vs.check(vs.lib.vs_dev_copy_rate(moved // 2, 10, C.byref(g)))
    return moved / g.value / 1e6, g.value


def surfaces(name, w, h, fill):
    """N surfaces of a format at a 256-byte pitch -> buffers, the pitch, the UV offset."""
    sb = capi.PIXFMT_BY_NAME[name].sample_bytes
    pitch = -(-(w * sb) // 256) * 256
    nbytes = pitch * h * 3 // 2
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(N)]
    if fill:
        one = np.random.default_rng(w).integers(0, 256, nbytes, np.uint8)
        for k, b in enumerate(bufs):
            b.upload(np.roll(one, 4099 * k))
    return bufs, pitch, pitch * h


def case(name, sw, sh, dw, dh, candidates, what, iters=ITERS):
    """candidates: {label: fn(arr, njobs, sb)}; alternated."""
    sb = capi.PIXFMT_BY_NAME[name].sample_bytes
    src, sp, suv = surfaces(name, sw, sh, True)
    dst, dp, duv = surfaces(name, dw, dh, False)
    jobs = []
    for a, b in zip(src, dst):
        jobs.append((a.ptr, sp, sw, sh, b.ptr, dp, dw, dh, 1))
        jobs.append((a.ptr + suv, sp, sw // 2, sh // 2, b.ptr + duv, dp, dw // 2, dh // 2, 2))
    arr = vs._scale_job_array(jobs)
    moved = N * (sw * sh + dw * dh) * 3 // 2 * sb
    fns = {k: (lambda f=f: f(arr, len(jobs), sb)) for k, f in candidates.items()}
    for f in fns.values():
        for _ in range(WARM):
            f()
    vs.sync()
    times = {k: [] for k in fns}
    copies = []
    for _ in range(REPS):
        for k, f in fns.items():
            times[k].append(window(f, iters))
        copies.append(copy_ms(moved))
    c_ms = statistics.median(c[0] for c in copies)
    r = {"what": what, "format": name, "src": [sw, sh], "dst": [dw, dh], "surfaces": N, "jobs": len(jobs), "launches_per_window": iters,
         "bytes_read_plus_written_per_call": moved, "copy_ms_same_bytes": c_ms, "copy_ms_windows": [c[0] for c in copies],
         "copy_gbytes_per_s": statistics.median(c[1] for c in copies)}
    for k, t in times.items():
        m = statistics.median(t)
        r[k] = {"ms_per_call": m, "ms_windows": t, "gbytes_per_s": moved / m / 1e6, "over_copy": m / c_ms}
    print(json.dumps(r), flush=True)
    for b in src + dst:
        b.free()
    return r


def resample(interp, path=0):
    return lambda arr, n, sb: vs.check(vs.lib.vs_op_resample_jobs(arr, n, sb, interp, 0, path, None))


def zoom(arr, n, sb):
    vs.check(vs.lib.vs_op_resize_jobs(arr, n, sb, None))


res = []
for name in ("NV12", "P010"):
    res.append(case(name, 3900, 2220, 3840, 2160, {"linear": resample(LINEAR), "lanczos4": resample(LANCZOS4)}, "a_pad_back_to_frame"))
    res.append(case(name, 3840, 2160, 1920, 1080, {"linear_mean": resample(LINEAR), "lanczos4": resample(LANCZOS4)}, "b_4k_to_1080p"))
    res.append(case(name, 3780, 2100, 3840, 2160, {"resample_linear": resample(LINEAR), "resize_jobs": zoom}, "c_zoom_in_beside_resize_jobs"))
res.append(case("NV12", 3900, 2220, 3840, 2160, {"path0_staged": resample(LANCZOS4, 0), "path1_direct": resample(LANCZOS4, 1)}, "d_paths_pad_back", iters=4))
res.append(case("NV12", 3840, 2160, 1920, 1080, {"path0_staged": resample(LANCZOS4, 0), "path1_direct": resample(LANCZOS4, 1)}, "d_paths_4k_to_1080p", iters=4))
res.append(case("NV12", 3900, 2220, 3840, 2160, {"path0_staged": resample(LINEAR, 0), "path1_direct": resample(LINEAR, 1)}, "d_paths_pad_back_linear", iters=4))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
