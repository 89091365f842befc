"""The colour conversion and the fused enhancer batch at 3840 x 2160, 32 surfaces per launch, under colorimetry descriptors - several
builds of the library in ONE process, alternating slot by slot (DESIGN section 8 "Colorimetry", profiles/r18_cs_*).
  python scratch/cvt_cs_measure.py OUT.json parent=PATH/libvideo-stab.so [label=PATH ...]
      the library of this tree is always measured, as "this"; the first build named on the command line is measured in two slots of
      every round ("<label>" and "<label>_again"): the difference between the two is the spread that repeating a build gives.
      A slot is 5 launches and a sync under the host clock; 3 warm-up and 20 timed rounds.  The order of the launches goes to
      OUT.json as "sequence" (one label per kernel launch).
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/cvt_cs_measure.py OUT.json parent=...
  python scratch/cvt_cs_measure.py --reduce DIR OUT.json OUT.csv
      per-slot kernel medians of that run: the builds share their kernel names, so the kernels of the trace - in start order - take
      their labels from the sequence."""
import ctypes as C, glob, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np

KERNELS = re.compile(r"cvt_yuv_to_rgb_kernel|cvt_rgb_to_yuv_kernel|enh_point_kernel|enh_unsharp_kernel")


def pct(d, q):
    d = sorted(d)
    return d[min(len(d) - 1, int(len(d) * q))]


def summary(d):
    return {"median": statistics.median(d), "p10": pct(d, 0.1), "p90": pct(d, 0.9), "min": min(d), "max": max(d)}


if len(sys.argv) > 1 and sys.argv[1] == "--reduce":
    import csv
    rows = []
    for path in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if KERNELS.search(r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    seq = json.load(open(sys.argv[3]))["sequence"]
    assert len(rows) == len(seq), (len(rows), len(seq))
    by = {}
    for (_, ns), (label, timed) in zip(rows, seq):
        if timed:
            by.setdefault(label, []).append(ns)
    with open(sys.argv[4], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["slot", "kernels", "median_ns", "min_ns", "p10_ns", "p90_ns", "max_ns"])
        for label, d in by.items():
            w.writerow([label, len(d), statistics.median(d), min(d), pct(d, 0.1), pct(d, 0.9), max(d)])
    sys.exit(0)

from vsamd import capi

W, H, N, WARM, ROUNDS, PER_SLOT = 3840, 2160, 32, 3, 20, 5
BT709_TOPLEFT, BT709_MEAN = capi.CvtColorimetry(1, 0, 0, 0), capi.CvtColorimetry(1, 0, 1, 0)
libs = [(a.split("=", 1)[0], capi.VsLib(C.CDLL(a.split("=", 1)[1]))) for a in sys.argv[2:]]
this = capi.load()
vs = this
rng = np.random.default_rng(1)
pa = capi._ptr_array


def many(nbytes, dtype, fill=True):
    one = rng.integers(0, 256 if dtype == np.uint8 else 65536, nbytes // np.dtype(dtype).itemsize, dtype)
    bufs = []
    for k in range(N):
        b = capi.DevBuf(vs, nbytes)
        if fill:
            b.upload(np.roll(one, 4099 * k))
        bufs.append(b)
    return bufs


nv12_b, p010_b, bgr_b = W * H * 3 // 2, W * H * 3, W * H * 3
nv12, p010, bgr_src = many(nv12_b, np.uint8), many(p010_b, np.uint16), many(bgr_b, np.uint8)
bgr_out, nv12_out = many(bgr_b, np.uint8, False), many(nv12_b, np.uint8, False)
lay8, lay16 = capi.I420LayoutC(W, 0, 0, 0), capi.I420LayoutC(2 * W, 0, 0, 0)
P010 = capi.PIXFMT_BY_NAME["P010"].fmt


def cvt_slots(label, lib, cs):
    """The three conversions of one build under one descriptor (None: the entry points without one)."""
    L = lib.lib
    if cs is None:
        return [(label + ":nv12_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb(capi.FMT_NV12, pa(nv12), C.byref(lay8), capi.FMT_BGR8, pa(bgr_out), W * 3, N, W, H, None), lib.sync),
                (label + ":bgr8_to_nv12", lambda: L.vs_op_cvt_rgb_to_yuv(capi.FMT_BGR8, pa(bgr_src), W * 3, capi.FMT_NV12, pa(nv12_out), C.byref(lay8), N, W, H, None), lib.sync),
                (label + ":p010_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb(P010, pa(p010), C.byref(lay16), capi.FMT_BGR8, pa(bgr_out), W * 3, N, W, H, None), lib.sync)]
    r = C.byref(cs)
    return [(label + ":nv12_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb_cs(capi.FMT_NV12, pa(nv12), C.byref(lay8), capi.FMT_BGR8, pa(bgr_out), W * 3, N, W, H, r, None), lib.sync),
            (label + ":bgr8_to_nv12", lambda: L.vs_op_cvt_rgb_to_yuv_cs(capi.FMT_BGR8, pa(bgr_src), W * 3, capi.FMT_NV12, pa(nv12_out), C.byref(lay8), N, W, H, r, None), lib.sync),
            (label + ":p010_to_bgr8", lambda: L.vs_op_cvt_yuv_to_rgb_cs(P010, pa(p010), C.byref(lay16), capi.FMT_BGR8, pa(bgr_out), W * 3, N, W, H, r, None), lib.sync)]


ENH = {"points": dict(brightness=1.5, contrast=1.1, gamma=1.2),
       "shipped": dict(brightness=1.5, contrast=1.1, gamma=1.2, enable_unsharp=1, sharpness=2.0, blur_sigma=1.0)}
keep = []


def enh_slots(label, lib, cs):
    """The fused batch of one build: 32 NV12 surfaces, tables only and the shipped settings (unsharp, R = 3)."""
    enh = capi.Enhancer(lib)
    keep.append(enh)
    if cs is not None:
        enh.set_yuv_colorimetry(cs)
    out = []
    for sname, kw in ENH.items():
        p = capi.Enhancer.default_params(lib, **kw)
        keep.append(p)

        def fn(enh=enh, p=p):
            return lib.lib.vs_enh_apply_yuv_batch_dev(enh.h, C.byref(p), capi.FMT_NV12, pa(nv12), C.byref(lay8), pa(nv12_out), C.byref(lay8), N, W, H)
        out.append((label + ":enh_" + sname, fn, enh.sync))
    return out


slots = []
first = True
for label, lib in libs:
    slots += cvt_slots(label, lib, None) + enh_slots(label, lib, None)
    if first:
        slots += cvt_slots(label + "_again", lib, None) + enh_slots(label + "_again", lib, None)
    first = False
slots += cvt_slots("this", this, None) + enh_slots("this", this, None)
slots += cvt_slots("this_709_topleft", this, BT709_TOPLEFT) + enh_slots("this_709_topleft", this, BT709_TOPLEFT)
slots += cvt_slots("this_709_mean", this, BT709_MEAN) + enh_slots("this_709_mean", this, BT709_MEAN)

times = {s[0]: [] for s in slots}
sequence = []
for rnd in range(WARM + ROUNDS):
    order = slots if rnd % 2 == 0 else slots[::-1]           # no build always runs behind the same neighbour
    for label, fn, sync in order:
        t0 = time.perf_counter()
        for _ in range(PER_SLOT):
            rc = fn()
            assert rc == 0, (label, rc)
        sync()
        dt = (time.perf_counter() - t0) / PER_SLOT
        sequence += [(label, rnd >= WARM)] * PER_SLOT       # one kernel per launch
        if rnd >= WARM:
            times[label].append(dt * 1e3)

res = {"w": W, "h": H, "surfaces": N, "rounds": ROUNDS, "launches_per_slot": PER_SLOT,
       "host_clock_ms_per_launch": {k: dict(summary(v), all=[round(x, 4) for x in v]) for k, v in times.items()},
       "sequence": sequence}
for k, v in times.items():
    print("%-36s %.3f ms (%.3f - %.3f)" % (k, statistics.median(v), pct(v, 0.1), pct(v, 0.9)), flush=True)
json.dump(res, open(sys.argv[1], "w"))
