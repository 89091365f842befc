"""vs_op_cvt_packed_to_yuv / vs_op_cvt_yuv_to_packed at 3840 x 2160, 32 surfaces per launch: UYVY -> NV12, NV12 -> UYVY, YUY2 -> I422,
v210 -> P010, P010 -> v210 and Y210 -> P010, each next to (a) hipMemcpyAsync device-to-device copies that read plus write the same
number of bytes and (b) the sibling vs_op_cvt_yuv_to_yuv call - I422 -> NV12 for the 8-bit cases, I210 -> P010 for the 16-bit ones -
in the same process (DESIGN section 8 "Packed capture formats", profiles/packed_*).  The three alternate, REPS windows of ITERS
launches each, timed with device events on the null stream after a warm-up; every window moves more than the Infinity Cache holds.
The whole list runs twice, the second time in reversed order.  The yardstick is bytes per second, not surfaces: v210 holds 6 pixels
in 16 bytes where I210 holds them in 24.
  python scratch/packed_measure.py OUT.json
One JSON line per case and pass on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

W, H, N, ITERS, REPS, WARM = 3840, 2160, 32, 40, 5, 3
# (packed, surface, to_packed, sibling source, sibling destination)
CASES = [("UYVY", "NV12", False, "I422", "NV12"), ("UYVY", "NV12", True, "I422", "NV12"), ("YUY2", "I422", False, "I422", "NV12"),
         ("v210", "P010", False, "I210", "P010"), ("v210", "P010", True, "I210", "P010"), ("Y210", "P010", False, "I210", "P010")]

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("packed_measure: no device")
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


NOISE = np.random.default_rng(1).integers(0, 256, 40 << 20, np.uint8)


def pool(nbytes, fill=False):
    """N device buffers of nbytes; filled: with distinct windows of seeded bytes."""
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(N)]
    if fill:
        for k, b in enumerate(bufs):
            b.upload(NOISE[4099 * k:4099 * k + nbytes])
    return bufs


def one(packed, surf, to_packed, sib_src, sib_dst, order):
    pf, f = capi.PACKED_BY_NAME[packed], capi.PIXFMT_BY_NAME[surf]
    fs, fd = capi.PIXFMT_BY_NAME[sib_src], capi.PIXFMT_BY_NAME[sib_dst]
    _, ppitch, pbytes = vs.packed_layout(pf, W, H)
    _, ybytes = vs.yuv_surface_layout(f.fmt, W, H)
    (_, sbytes), (_, dbytes) = vs.yuv_surface_layout(fs.fmt, W, H), vs.yuv_surface_layout(fd.fmt, W, H)
    d_packed, d_surf = pool(pbytes, not to_packed), pool(ybytes, to_packed)
    s_src, s_dst = pool(sbytes, True), pool(dbytes)
    half = (pbytes + ybytes) // 2                         # a copy of `half` bytes reads and writes pbytes + ybytes
    c_src, c_dst = pool(half, True), pool(half)
    pp, py, ps, pd = (capi._ptr_array(x) for x in (d_packed, d_surf, s_src, s_dst))
    lay, lin, lout = (capi.I420LayoutC(x.sample_bytes * W, 0, 0, 0) for x in (f, fs, fd))

    def convert():
        if to_packed:
            vs.check(vs.lib.vs_op_cvt_yuv_to_packed(f.fmt, py, C.byref(lay), pf, pp, ppitch, N, W, H, None, None))
        else:
            vs.check(vs.lib.vs_op_cvt_packed_to_yuv(pf, pp, ppitch, f.fmt, py, C.byref(lay), N, W, H, None, None))

    def sibling():
        vs.check(vs.lib.vs_op_cvt_yuv_to_yuv(fs.fmt, ps, C.byref(lin), fd.fmt, pd, C.byref(lout), N, W, H, None, None))

    def copy():
        for a, b in zip(c_src, c_dst):
            hip_ok(hip.hipMemcpyAsync(b.ptr, a.ptr, half, D2D, None))
    for _ in range(WARM):
        convert()
        sibling()
        copy()
    vs.sync()
    t = {"convert": [], "sibling": [], "copy": []}
    for _ in range(REPS):
        t["convert"].append(window(convert))
        t["sibling"].append(window(sibling))
        t["copy"].append(window(copy))
    moved, sib_moved = N * (pbytes + ybytes), N * (sbytes + dbytes)
    m = {k: statistics.median(v) for k, v in t.items()}
    r = {"what": ("%s_to_%s" % ((surf, packed) if to_packed else (packed, surf))).lower(), "pass": order, "w": W, "h": H, "surfaces": N,
         "launches_per_window": ITERS, "bytes_read_plus_written_per_launch": moved,
         "convert_ms_per_launch": m["convert"], "convert_ms_windows": t["convert"], "convert_gbytes_per_s": moved / m["convert"] / 1e6,
         "convert_gbytes_per_s_windows": [moved / x / 1e6 for x in t["convert"]],
         "copy_ms_same_bytes": m["copy"], "copy_ms_windows": t["copy"], "copy_gbytes_per_s": moved / m["copy"] / 1e6,
         "convert_over_copy": m["convert"] / m["copy"],
         "sibling": "%s_to_%s" % (sib_src.lower(), sib_dst.lower()), "sibling_bytes_read_plus_written_per_launch": sib_moved,
         "sibling_ms_per_launch": m["sibling"], "sibling_ms_windows": t["sibling"], "sibling_gbytes_per_s": sib_moved / m["sibling"] / 1e6,
         "sibling_gbytes_per_s_windows": [sib_moved / x / 1e6 for x in t["sibling"]]}
    for b in d_packed + d_surf + s_src + s_dst + c_src + c_dst:
        b.free()
    return r


res = []
for order, cases in (("forward", CASES), ("reversed", CASES[::-1])):
    for case in cases:
        res.append(one(*case, order))
        print(json.dumps(res[-1]), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
