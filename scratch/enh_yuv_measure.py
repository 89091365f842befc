"""The enhancer on 32 YUV surfaces of 3840 x 2160 (NV12 and P010, distinct content): 32 calls of vs_enh_apply_yuv_dev - three launches
per surface through a BGR8 scratch frame - against ONE call of vs_enh_apply_yuv_batch_dev (the fused launch), in one process, the two
alternating repetition by repetition, and vs_dev_copy_rate for the bytes the fused launch moves (profiles/r17_enh_yuv_*).
3 warm-up and 20 timed repetitions each; the host clock is taken around every repetition and its sync.
  python scratch/enh_yuv_measure.py OUT.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/enh_yuv_measure.py OUT.json
  python scratch/enh_yuv_measure.py --reduce DIR OUT.csv      per-kernel medians of that run's kernel trace"""
import ctypes as C, glob, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np


def pct(d, q):
    d = sorted(d)
    return d[min(len(d) - 1, int(len(d) * q))]


if len(sys.argv) > 1 and sys.argv[1] == "--reduce":
    import csv
    by = {}
    for path in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            by.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(sys.argv[3], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "calls", "median_ns", "min_ns", "p10_ns", "p90_ns", "max_ns", "total_ns"])
        for name, d in sorted(by.items()):
            w.writerow([name, len(d), statistics.median(d), min(d), pct(d, 0.1), pct(d, 0.9), max(d), sum(d)])
    sys.exit(0)

from vsamd import capi

vs = capi.load()
enh = capi.Enhancer(vs)
W, H, N, WARM, ITERS = 3840, 2160, 32, 3, 20
TABLES = dict(brightness=1.5, contrast=1.1, gamma=1.2)
SETTINGS = {
    "points": TABLES,
    "shipped": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0),     # R = 3
    "wide": dict(TABLES, enable_unsharp=1, sharpness=2.0, blur_sigma=5.4),        # R = 16: every chroma sample converted once per staged row
}
FORMATS = {"NV12": (capi.FMT_NV12, np.uint8, W), "P010": (capi.PIXFMT_BY_NAME["P010"].fmt, np.uint16, 2 * W)}
rng = np.random.default_rng(1)
L = vs.lib
pa = capi._ptr_array


def many(nbytes, dtype):
    one = rng.integers(0, 256 if dtype == np.uint8 else 65536, nbytes // np.dtype(dtype).itemsize, dtype)
    bufs = []
    for k in range(N):
        b = capi.DevBuf(vs, nbytes)
        b.upload(np.roll(one, 4099 * k))
        bufs.append(b)
    return bufs


res = []
for fname, (fmt, dtype, pitch) in FORMATS.items():
    nbytes = pitch * H * 3 // 2
    src, out_a, out_b = many(nbytes, dtype), [capi.DevBuf(vs, nbytes) for _ in range(N)], [capi.DevBuf(vs, nbytes) for _ in range(N)]
    lay = capi.I420LayoutC(pitch, 0, 0, 0)
    for sname, kw in SETTINGS.items():
        p = capi.Enhancer.default_params(vs, **kw)
        assert vs.enh_yuv_plan(p, fmt) == 1

        def three_calls():
            for k in range(N):
                enh._check(L.vs_enh_apply_yuv_dev(enh.h, C.byref(p), fmt, src[k].ptr, C.byref(lay), out_a[k].ptr, C.byref(lay), W, H))
            enh.sync()

        def fused():
            enh._check(L.vs_enh_apply_yuv_batch_dev(enh.h, C.byref(p), fmt, pa(src), C.byref(lay), pa(out_b), C.byref(lay), N, W, H))
            enh.sync()

        t = {"three_calls": [], "fused": []}
        for it in range(WARM + ITERS):
            for label, fn in (("three_calls", three_calls), ("fused", fused)):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if it >= WARM:
                    t[label].append(dt * 1e3)
        assert enh.last_fused() == N
        # faster and different is not faster: the same bytes at this size, first and last surface
        same = all(np.array_equal(out_a[k].download((nbytes,), np.uint8), out_b[k].download((nbytes,), np.uint8)) for k in (0, N - 1))
        moved = 2 * N * nbytes
        g = C.c_double()
        vs.check(L.vs_dev_copy_rate(moved // 2, ITERS, C.byref(g)))
        r = {"format": fname, "setting": sname, "surfaces": N, "w": W, "h": H, "outputs_equal": bool(same), "bytes_moved_by_fused_launch": moved,
             "copy_rate_same_bytes_gbytes_per_s": g.value, "copy_ms_same_bytes": moved / g.value / 1e6}
        for label, d in t.items():
            r[label + "_ms"] = {"median": statistics.median(d), "p10": pct(d, 0.1), "p90": pct(d, 0.9), "min": min(d), "max": max(d), "all": [round(x, 3) for x in d]}
        r["fused_gbytes_per_s_host_clock"] = moved / r["fused_ms"]["median"] / 1e6
        res.append(r)
        print(fname, sname, "three calls %.2f ms (%.2f - %.2f)   fused %.2f ms (%.2f - %.2f)   copy %.2f ms   equal %s" % (
            r["three_calls_ms"]["median"], r["three_calls_ms"]["p10"], r["three_calls_ms"]["p90"], r["fused_ms"]["median"], r["fused_ms"]["p10"],
            r["fused_ms"]["p90"], r["copy_ms_same_bytes"], same), flush=True)
    for b in src + out_a + out_b:
        b.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
