"""vs_op_cvt_yuv_to_yuv at 3840 x 2160, 32 surfaces per launch: I420 -> NV12, I010 -> P010, I210 -> P010 (MEAN), I422 -> NV12 and
P010 -> NV12, each next to hipMemcpyAsync device-to-device copies that read plus write the same number of bytes, in the same process
(DESIGN section 8 "Surface format conversion", profiles/yuvcvt_*).  Conversion and copy alternate, REPS windows of ITERS launches
each, timed with device events on the null stream after a warm-up; every window moves more than the Infinity Cache holds.
  python scratch/yuvcvt_measure.py OUT.json
One JSON line per case on stdout; OUT.json holds the list.  Fails without a device: there is nothing to measure on a CPU."""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
import numpy as np
from vsamd import capi

W, H, N, ITERS, REPS, WARM = 3840, 2160, 32, 50, 5, 3
CASES = [("I420", "NV12", (0, 0)), ("I010", "P010", (0, 0)), ("I210", "P010", (0, 1)), ("I422", "NV12", (0, 0)), ("P010", "NV12", (0, 0))]

vs = capi.load()
if vs.lib.vs_device_count() <= 0:
    sys.exit("yuvcvt_measure: no device")
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


def pool(nbytes, dtype=None, seed=0):
    """N device buffers of nbytes; with a dtype, filled with distinct seeded samples."""
    bufs = [capi.DevBuf(vs, nbytes) for _ in range(N)]
    if dtype is not None:
        one = np.random.default_rng(seed).integers(0, 256 if dtype == np.uint8 else 65536, nbytes // np.dtype(dtype).itemsize, dtype)
        for k, b in enumerate(bufs):
            b.upload(np.roll(one, 4099 * k))
    return bufs


res = []
for src, dst, desc in CASES:
    fs, fd = capi.PIXFMT_BY_NAME[src], capi.PIXFMT_BY_NAME[dst]
    (_, sbytes), (_, dbytes) = vs.yuv_surface_layout(fs.fmt, W, H), vs.yuv_surface_layout(fd.fmt, W, H)
    d_src, d_dst = pool(sbytes, capi.fmt_dtype(fs.fmt), 1), pool(dbytes)
    half = (sbytes + dbytes) // 2                         # a copy of `half` bytes reads and writes sbytes + dbytes
    c_src, c_dst = pool(half, np.uint8, 2), pool(half)
    ps, pd = capi._ptr_array(d_src), capi._ptr_array(d_dst)
    lin, lout = capi.I420LayoutC(fs.sample_bytes * W, 0, 0, 0), capi.I420LayoutC(fd.sample_bytes * W, 0, 0, 0)
    dsc = capi.VsYuvCvtDesc(*desc)

    def convert():
        vs.check(vs.lib.vs_op_cvt_yuv_to_yuv(fs.fmt, ps, C.byref(lin), fd.fmt, pd, C.byref(lout), N, W, H, C.byref(dsc), None))

    def copy():
        for a, b in zip(c_src, c_dst):
            hip_ok(hip.hipMemcpyAsync(b.ptr, a.ptr, half, D2D, None))
    for _ in range(WARM):
        convert()
        copy()
    vs.sync()
    t_cvt, t_copy = [], []
    for _ in range(REPS):
        t_cvt.append(window(convert))
        t_copy.append(window(copy))
    moved = N * (sbytes + dbytes)
    m_cvt, m_copy = statistics.median(t_cvt), statistics.median(t_copy)
    r = {"what": "%s_to_%s" % (src.lower(), dst.lower()), "desc": {"depth_down": desc[0], "chroma_down": desc[1]}, "w": W, "h": H, "surfaces": N,
         "launches_per_window": ITERS, "bytes_read_plus_written_per_launch": moved,
         "convert_ms_per_launch": m_cvt, "convert_ms_windows": t_cvt, "convert_gbytes_per_s": moved / m_cvt / 1e6,
         "copy_ms_same_bytes": m_copy, "copy_ms_windows": t_copy, "copy_gbytes_per_s": moved / m_copy / 1e6,
         "convert_over_copy": m_cvt / m_copy}
    res.append(r)
    print(json.dumps(r), flush=True)
    for b in d_src + d_dst + c_src + c_dst:
        b.free()
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
