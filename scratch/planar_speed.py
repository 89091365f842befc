"""Speed of the stabilizer on planar streams at 3840 x 2160 - I420, I422, I444, I010, I210 and I410 streams of ONE clip in ONE
process ("I422 / I444"; profiles/r13_planar_speed_4k.json).

Every stream: batch mode 64, zero-copy, 64 input surfaces in a cycle (a picture of the clip generator under a steady pan, converted to
the format: real chroma, live low bits in the 10-bit forms), results into buffers of their own.  One warm-up step of 64 pushes fills
the smoothing queue; then `steps` timed steps of 64 pushes and a sync each, a host clock around them, and the warp stage's own
time from the library's stage events (vs_stab_set_profiling(s, 1)).  The six formats are run one after the other, `rounds` times
over, so every format's own runs give the spread its figures are read against.

Per format: frames/s (median step), warp time per surface, bytes moved per surface by the warp (read + write = 2 x the frame's
bytes) and the fraction of the 8 TB/s HBM peak that is; and against its 4:2:0 sibling (I422, I444 : I420; I210, I410 : I010) the
ratio of bytes/s in the warp - a 4:2:2 surface moves 4/3 of the sibling's bytes, a 4:4:4 surface twice.

Usage: python scratch/planar_speed.py out.json [steps] [rounds] [distinct pictures] [formats, comma-separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))

from vsamd import capi, synth         # noqa: E402

W, H = 3840, 2160
NSRC = 64
HBM_PEAK = 8.0e12
# name -> (format, sx, sy, bits, 4:2:0 sibling)
FORMATS = {
    "I420": (capi.FMT_I420, 1, 1, 8, None), "I422": (capi.FMT_I422, 1, 0, 8, "I420"), "I444": (capi.FMT_I444, 0, 0, 8, "I420"),
    "I010": (capi.FMT_I010, 1, 1, 10, None), "I210": (capi.FMT_I210, 1, 0, 10, "I010"), "I410": (capi.FMT_I410, 0, 0, 10, "I010"),
}


def upload(vs, bgr, name, distinct):
    """NSRC surfaces of the format on the device - `distinct` pictures in a cycle: the rendered picture moved by (4 i, 2 i) pixels, a
    camera panning over it - and a surface's size in bytes.  (Rendering one 4K picture takes the host ten seconds; its planes are
    rolled, every chroma plane by its share of the shift.)"""
    _, sx, sy, bits, _ = FORMATS[name]
    planes = synth.bgr_to_yuv_planes(bgr, sx, sy)
    if bits != 8:
        planes = synth.yuv_to_depth(planes, bits, 1)
    host = []
    for i in range(distinct):
        y, u, v = (np.roll(p, (2 * i >> (sy if k else 0), 4 * i >> (sx if k else 0)), axis=(0, 1)) for k, p in enumerate(planes))
        host.append(synth.yuv_pack(y, u, v, sx, sy))
    sb = host[0].nbytes
    d = capi.DevBuf(vs, sb * NSRC)
    for i in range(NSRC):
        d.upload(np.ascontiguousarray(host[i % len(host)]), i * sb)
    return d, sb


def run(vs, name, d_in, d_out, sb, steps):
    fmt, _, _, bits, _ = FORMATS[name]
    pitch = W * (1 if bits == 8 else 2)
    s = vs.stabilizer(vs.params(smoothing_radius=30))
    s.set_batch(64)
    s.set_zero_copy(True)
    ins = [d_in.ptr + i * sb for i in range(NSRC)]
    outs = [d_out.ptr + i * sb for i in range(NSRC)]
    s.push_dev_n(ins, W, H, pitch, fmt, outs, pitch)            # warm-up: fills the queue (radius 30 < 64), code objects, work areas
    s.sync()
    s.set_profiling(1)
    s.stage_times()
    ts, produced = [], 0
    for _ in range(steps):
        t0 = time.perf_counter()
        k = s.push_dev_n(ins, W, H, pitch, fmt, outs, pitch)
        s.sync()
        ts.append(time.perf_counter() - t0)
        assert k == NSRC, k
        produced += k
    ms, _ = s.stage_times()
    s.close()
    return NSRC / float(np.median(ts)), ms[capi.STAGE_WARP] * 1e3 / produced


def main():
    out = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    distinct = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    vs = capi.load()
    if vs.lib.vs_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured here")
    only = sys.argv[5].split(",") if len(sys.argv) > 5 else list(FORMATS)         # (a build without the 4:2:2 / 4:4:4 formats: I420,I010)
    for name in list(FORMATS):
        if name not in only:
            del FORMATS[name]
    bgr = synth.make_clip(synth.SEED_CONFIG3, W, H, 1)[0]
    res = {"size": [W, H], "batch": 64, "timed_steps": steps, "rounds": rounds, "distinct_pictures": distinct, "build": vs.lib.vs_build_tag().decode(),
           "hbm_peak_bytes_per_s": HBM_PEAK, "formats": {}}
    bufs = {}
    for name in FORMATS:
        d_in, sb = upload(vs, bgr, name, distinct)
        bufs[name] = (d_in, capi.DevBuf(vs, sb * NSRC), sb)
        res["formats"][name] = {"bytes_per_surface_moved_by_the_warp": 2 * sb, "frames_per_s": [], "warp_us_per_surface": []}
    for _ in range(rounds):
        for name in FORMATS:
            d_in, d_out, sb = bufs[name]
            fps, us = run(vs, name, d_in, d_out, sb, steps)
            res["formats"][name]["frames_per_s"].append(fps)
            res["formats"][name]["warp_us_per_surface"].append(us)
            print("%s %.0f frames/s, warp %.2f us per surface, %.3f of the HBM peak" % (name, fps, us, 2 * sb / (us * 1e-6) / HBM_PEAK), flush=True)
    for name, (fmt, sx, sy, bits, sibling) in FORMATS.items():
        r = res["formats"][name]
        us = float(np.median(r["warp_us_per_surface"]))
        r["warp_bytes_per_s"] = r["bytes_per_surface_moved_by_the_warp"] / (us * 1e-6)
        r["hbm_fraction"] = r["warp_bytes_per_s"] / HBM_PEAK
        r["warp_spread"] = (max(r["warp_us_per_surface"]) - min(r["warp_us_per_surface"])) / us
        r["frames_per_s_spread"] = (max(r["frames_per_s"]) - min(r["frames_per_s"])) / float(np.median(r["frames_per_s"]))
    for name, (fmt, sx, sy, bits, sibling) in FORMATS.items():
        if sibling in FORMATS:
            r, q = res["formats"][name], res["formats"][sibling]
            r["sibling"] = sibling
            r["bytes_over_sibling"] = r["bytes_per_surface_moved_by_the_warp"] / q["bytes_per_surface_moved_by_the_warp"]
            r["warp_bytes_per_s_over_sibling"] = r["warp_bytes_per_s"] / q["warp_bytes_per_s"]
            r["frames_per_s_over_sibling"] = float(np.median(r["frames_per_s"])) / float(np.median(q["frames_per_s"]))
    for d_in, d_out, _ in bufs.values():
        d_in.free()
        d_out.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
