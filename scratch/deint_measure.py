"""The deinterlacer and the weave at 3840 x 2160 (DESIGN section 8 "Deinterlace", profiles/r37_deint_*).

16 frames per call, NV12 and P010, chained as a batch (prev[i] = cur[i - 1], next[i] = cur[i + 1], the ends frames of their own):
  yadif   one double-rate VS_DEINT_YADIF call of vs_op_deint_yuv: 64 jobs, 32 progressive frames out
  linear  the same with VS_DEINT_LINEAR
  weave   vs_op_interlace_yuv of 32 pairs of progressive frames
Every time stands against a plain device copy, in the same process, of exactly the bytes the call must move: its distinct source
rows plus its destination rows (yadif: 18 + 32 surfaces, linear: 16 + 32, weave: 32 + 32 - half the rows of each of 64 sources).
The candidates of a format alternate, REPS windows of ITERS launches each between device events on the null stream after a
warm-up.  One JSON line per case on stdout; OUT.json holds the list.  Fails without a device.
  python scratch/deint_measure.py OUT.json
  python scratch/deint_measure.py --once      # four launches of every case and nothing else: for a counter pass under rocprofv3"""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

W, H, N, ITERS, REPS, WARM = 3840, 2160, 16, 10, 5, 2
ONCE = "--once" in sys.argv

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("deint_measure: no device")
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


def fmt_case(name):
    f = capi.PIXFMT_BY_NAME[name]
    pitch = W * f.sample_bytes
    surface = pitch * H * 3 // 2
    one = np.random.default_rng(W).integers(0, 256, surface, np.uint8)
    src = [capi.DevBuf(vs, surface) for _ in range(N + 2)]                 # the frame before the batch, the batch, the frame behind it
    for k, b in enumerate(src):
        b.upload(np.roll(one, 4099 * k))
    prog = [capi.DevBuf(vs, surface) for _ in range(2 * N)]                # first fields, then second fields
    woven = [capi.DevBuf(vs, surface) for _ in range(2 * N)]
    s = [b.ptr for b in src]
    p = [b.ptr for b in prog]
    lay = (pitch, 0, 0, 0)

    def deint(mode):
        return lambda: vs.deint_yuv(f.fmt, s[:N], s[1:N + 1], s[2:], lay, W, H, p[:N], p[N:], lay, 1, mode)

    def weave():
        vs.interlace_yuv(f.fmt, p, p[1:] + p[:1], lay, W, H, [b.ptr for b in woven], lay, 1)
    cands = {"yadif": (deint(capi.DEINT_YADIF), (N + 2 + 2 * N) * surface), "linear": (deint(capi.DEINT_LINEAR), (N + 2 * N) * surface),
             "weave": (weave, (2 * N + 2 * N) * surface)}
    for fn, _ in cands.values():
        for _ in range(4 if ONCE else WARM):
            fn()
    vs.sync()
    out = []
    if not ONCE:
        times, copies = {k: [] for k in cands}, {k: [] for k in cands}
        for _ in range(REPS):
            for k, (fn, moved) in cands.items():
                times[k].append(window(fn, ITERS))
                copies[k].append(copy_ms(moved))
        for k, (fn, moved) in cands.items():
            m, c = statistics.median(times[k]), statistics.median(x[0] for x in copies[k])
            ratios = [t / x[0] for t, x in zip(times[k], copies[k])]
            r = {"case": k, "format": name, "size": [W, H], "frames": N, "launches_per_window": ITERS, "bytes_the_call_must_move": moved, "ms_per_call": m,
                 "ms_windows": times[k], "copy_ms_same_bytes": c, "copy_ms_windows": [x[0] for x in copies[k]], "copy_gbytes_per_s": statistics.median(x[1] for x in copies[k]),
                 "gbytes_per_s": moved / m / 1e6, "over_copy": m / c, "over_copy_windows": [min(ratios), max(ratios)]}
            print(json.dumps(r), flush=True)
            out.append(r)
    for b in src + prog + woven:
        b.free()
    return out


res = []
for name in ("NV12", "P010"):
    res += fmt_case(name)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    json.dump(res, open(args[0], "w"), indent=1)
