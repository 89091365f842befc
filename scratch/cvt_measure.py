"""The colour conversion at 3840 x 2160, 32 surfaces per launch: NV12 -> BGR8, BGR8 -> NV12, P010 -> BGR8, 3 + 20 launches each, and
vs_dev_copy_rate for the same number of bytes in the same process (profiles/r16_cvt_*).
  python scratch/cvt_measure.py OUT.json                 host clock around the 20 launches and a sync
  rocprofv3 --kernel-trace --stats -d DIR -o cvt -- python scratch/cvt_measure.py OUT.json
  python scratch/cvt_measure.py --reduce DIR/cvt_results.db OUT.csv      per-kernel medians of that run's database"""
import ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

if len(sys.argv) > 1 and sys.argv[1] == "--reduce":
    import csv, sqlite3, statistics
    rows = sqlite3.connect(sys.argv[2]).execute("select name, end - start from kernels order by start").fetchall()
    by = {}
    for name, ns in rows:
        by.setdefault(name, []).append(ns)
    with open(sys.argv[3], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "calls", "median_ns", "min_ns", "p10_ns", "p90_ns", "max_ns", "total_ns"])
        for name, d in by.items():
            d.sort()
            w.writerow([name, len(d), statistics.median(d), d[0], d[len(d) // 10], d[len(d) * 9 // 10], d[-1], sum(d)])
    sys.exit(0)

vs = capi.load()
W, H, N, ITERS = 3840, 2160, 32, 20
nv12_b, p010_b, bgr_b = W * H * 3 // 2, W * H * 3, W * H * 3
rng = np.random.default_rng(1)

def many(nbytes, dtype):
    one = rng.integers(0, 256 if dtype == np.uint8 else 65536, nbytes // np.dtype(dtype).itemsize, dtype)
    bufs = []
    for k in range(N):
        b = capi.DevBuf(vs, nbytes)
        b.upload(np.roll(one, 4099 * k))
        bufs.append(b)
    return bufs

nv12, p010, bgr, bgr2, nv12o = many(nv12_b, np.uint8), many(p010_b, np.uint16), many(bgr_b, np.uint8), many(bgr_b, np.uint8), many(nv12_b, np.uint8)
pa = capi._ptr_array
lay8, lay16 = capi.I420LayoutC(W, 0, 0, 0), capi.I420LayoutC(2 * W, 0, 0, 0)
L = vs.lib

def run(label, fn, moved):
    for _ in range(3):
        vs.check(fn())
    vs.sync()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        vs.check(fn())
    vs.sync()
    dt = (time.perf_counter() - t0) / ITERS
    return {"what": label, "bytes_moved_per_launch": moved, "host_timed_ms_per_launch": dt * 1e3, "host_timed_gbytes_per_s": moved / dt / 1e9}

res = []
res.append(run("nv12_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb(capi.FMT_NV12, pa(nv12), C.byref(lay8), capi.FMT_BGR8, pa(bgr), W * 3, N, W, H, None), N * (nv12_b + bgr_b)))
res.append(run("bgr8_to_nv12", lambda: L.vs_op_cvt_rgb_to_yuv(capi.FMT_BGR8, pa(bgr2), W * 3, capi.FMT_NV12, pa(nv12o), C.byref(lay8), N, W, H, None), N * (nv12_b + bgr_b)))
res.append(run("p010_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb(capi.FMT_P010, pa(p010), C.byref(lay16), capi.FMT_BGR8, pa(bgr), W * 3, N, W, H, None), N * (p010_b + bgr_b)))
for r in list(res):
    g = C.c_double()
    vs.check(L.vs_dev_copy_rate(r["bytes_moved_per_launch"] // 2, ITERS, C.byref(g)))
    r["copy_rate_same_bytes_gbytes_per_s"] = g.value
    r["copy_ms_same_bytes"] = r["bytes_moved_per_launch"] / g.value / 1e6
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res, indent=1))
