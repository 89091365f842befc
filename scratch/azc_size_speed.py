"""Speed of auto zoom/crop at a chosen output size, 3840 x 2160, ONE process ("Zoom at the surface's own size";
profiles/r15_azc_size_*).

  stages    the zoom stage alone on NV12, P010, I420 and I010 surfaces at the default size (640 x 360) and at (0, 0) - the surface's
            own size -, in surfaces per second: N surfaces per timed step (64 distinct inputs in a cycle, results into buffers of
            their own), a host clock around the calls and the stage's sync; the two sizes alternated ROUNDS times, so the default's
            own runs give the spread
  kernels   the crop-and-scale of ONE batch of eight surfaces at the surface's own size, as the stage builds it (rectangles from the
            stage's own info8): vs_op_scale_jobs with path 1 (the direct kernels) against path 0 (the plan: the staged kernel),
            alternated.  Run under `rocprofv3 --kernel-trace --stats` for the kernels' own times (one kind per run: the kernel names
            are the same for every kind); the host clock around REPS back-to-back calls and a sync is written as well, with the bytes
            of a batch - the crops read once plus the outputs written - and vs_dev_copy_rate of the same device

Usage: python scratch/azc_size_speed.py out.json stages [n_per_step] [steps] [rounds]
       python scratch/azc_size_speed.py out.json kernels KIND [pairs] [reps] [out_w out_h]          KIND: nv12 | p010 | i420 | i010"""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-stab_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle_lib                     # noqa: E402
from vsamd import capi, synth         # noqa: E402

W, H = 3840, 2160
NSRC = 64
NPIC = 8
I420, I010 = capi.FMT_I420, capi.FMT_I010
KINDS = ("nv12", "p010", "i420", "i010")
DEGS = [4.0, -2.5, 1.0, 7.5, -6.0, 0.5, 3.0, -1.0]

_pictures = []


def pictures():
    """NPIC distinct 4K NV12 pictures: textured content rotated about the centre, black corners (what roll correction hands over)."""
    if not _pictures:
        oracle = oracle_lib.load()
        for i, deg in enumerate(DEGS):
            rng = np.random.default_rng(i)
            y = rng.integers(40, 236, (H, W), dtype=np.uint8)
            a = math.radians(deg)
            al, be = math.cos(a), math.sin(a)
            M = [al, be, (1 - al) * W / 2 - be * H / 2, -be, al, be * W / 2 + (1 - al) * H / 2]
            s = np.empty((H * 3 // 2, W), np.uint8)
            s[:H] = oracle.warp_affine_d(y, M, border=0)
            s[H:] = rng.integers(16, 241, (H // 2, W), dtype=np.uint8)
            _pictures.append(s)
    return _pictures


def host_surface(kind, i):
    s = pictures()[i % NPIC]
    if kind == "nv12":
        return s
    if kind == "i420":
        return synth.nv12_to_i420(s)
    p = synth.nv12_to_p010(s, seed=i % NPIC)
    p[:H][s[:H] == 0] = 0               # black is sample 0
    return p if kind == "p010" else synth.p010_to_i010(p, W, H, 10)


def surfaces(vs, kind, n=NSRC):
    host = [np.ascontiguousarray(host_surface(kind, i)) for i in range(NPIC)]
    sb = host[0].nbytes
    d = capi.DevBuf(vs, sb * n)
    for i in range(n):
        d.upload(host[i % NPIC], i * sb)
    return d, sb


def hand_over(o, kind, ins, outs):
    sample = 2 if kind in ("p010", "i010") else 1
    pitch = W * sample
    lay = capi.i420_layout(pitch)
    if kind == "nv12":
        return o.apply_nv12_dev_n(ins, W, H, pitch, outs, pitch, pitch * H)
    if kind == "p010":
        return o.apply_p010_dev_n(ins, W, H, pitch, outs, pitch, pitch * H)
    return o.apply_i420_dev_n(I420 if kind == "i420" else I010, ins, W, H, lay, outs, lay)


def measure_stages(vs, n, steps, rounds):
    res = {}
    for kind in KINDS:
        d_in, sb = surfaces(vs, kind)
        d_out = capi.DevBuf(vs, sb * NSRC)
        ins = [d_in.ptr + (i % NSRC) * sb for i in range(n)]
        outs = [d_out.ptr + (i % NSRC) * sb for i in range(n)]
        runs = {"640x360": [], "own_size": []}
        cropped = None
        for _ in range(rounds):
            for name, size in (("640x360", (640, 360)), ("own_size", (0, 0))):
                o = vs.auto_zoom_crop()
                o.set_output_size(*size)
                tickets = hand_over(o, kind, ins, outs)      # warm-up: code objects, work areas, worker threads
                o.sync()
                cropped = sum(int(o.result(t)[2][7]) for t in tickets[:NPIC])
                ts = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    hand_over(o, kind, ins, outs)
                    o.sync()
                    ts.append(time.perf_counter() - t0)
                o.close()
                runs[name].append(n / float(np.median(ts)))
        d_in.free()
        d_out.free()
        a, b = float(np.median(runs["640x360"])), float(np.median(runs["own_size"]))
        res["zoom_" + kind] = {"surfaces_per_s": runs, "ratio_own_size_over_640x360": b / a, "spread_640x360": (max(runs["640x360"]) - min(runs["640x360"])) / a,
                               "cropped_of_the_%d_pictures" % NPIC: cropped}
        print(kind, {k: ["%.0f" % v for v in r] for k, r in runs.items()}, "ratio %.3f" % (b / a), "cropped", cropped, flush=True)
    return res


def batch_jobs(vs, kind, d_in, d_out, sb, OW=W, OH=H):
    """The jobs of one batch of eight surfaces at OW x OH (the surface's own size unless told), as azc_worker builds them, from the
    stage's own info8."""
    sample = 2 if kind in ("p010", "i010") else 1
    pitch = W * sample
    o = vs.auto_zoom_crop()
    tickets = hand_over(o, kind, [d_in.ptr + i * sb for i in range(8)], [d_out.ptr + i * sb for i in range(8)])
    o.sync()
    infos = [o.result(t)[2] for t in tickets]
    o.close()
    jobs, nbytes = [], 0
    for i, info in enumerate(infos):
        if not info[7]:
            continue
        cx, cy, cw, ch = (int(v) for v in info[2:6])
        ux, uy, uw, uh = cx // 2, cy // 2, max(1, cw // 2), max(1, ch // 2)
        src, dst = d_in.ptr + i * sb, d_out.ptr + i * sb
        jobs.append((src + cy * pitch + cx * sample, pitch, cw, ch, dst, pitch, OW, OH, 1))
        nbytes += (cw * ch + OW * OH) * sample
        if kind in ("nv12", "p010"):
            jobs.append((src + H * pitch + uy * pitch + ux * 2 * sample, pitch, uw, uh, dst + H * pitch, pitch, OW // 2, OH // 2, 2))
        else:
            cp = pitch // 2
            for plane in range(2):
                off = H * pitch + plane * (H // 2) * cp
                jobs.append((src + off + uy * cp + ux * sample, cp, uw, uh, dst + off, cp, OW // 2, OH // 2, 1))
        nbytes += 2 * (uw * uh + OW * OH // 4) * sample
    return jobs, nbytes, sample


def measure_kernels(vs, kind, pairs, reps, osize):
    d_in, sb = surfaces(vs, kind, 8)
    d_out = capi.DevBuf(vs, sb * 8)
    jobs, nbytes, sample = batch_jobs(vs, kind, d_in, d_out, sb, *osize)
    plan = vs.scale_jobs_plan(jobs, sample).tolist()
    rate = C.c_double()
    vs.check(vs.lib.vs_dev_copy_rate(256 << 20, 10, C.byref(rate)))
    times = {0: [], 1: []}
    for path in (1, 0):                  # warm-up
        vs.scale_jobs(jobs, sample, path)
    vs.sync()
    for _ in range(pairs):
        for path in (1, 0):
            t0 = time.perf_counter()
            for _ in range(reps):
                vs.scale_jobs(jobs, sample, path)
            vs.sync()
            times[path].append((time.perf_counter() - t0) / reps)
    d_in.free()
    d_out.free()
    direct, staged = float(np.median(times[1])), float(np.median(times[0]))
    res = {"kind": kind, "output_size": list(osize), "crops": [[j[2], j[3]] for j in jobs], "jobs": len(jobs), "staged_by_the_plan": plan, "bytes_of_a_batch": nbytes, "copy_rate_gb_per_s": rate.value,
           "host_clock_us_per_batch": {"direct_path_1": [t * 1e6 for t in times[1]], "plan_path_0": [t * 1e6 for t in times[0]]},
           "median_us": {"direct": direct * 1e6, "plan": staged * 1e6}, "direct_spread": (max(times[1]) - min(times[1])) / direct,
           "plan_gb_per_s_by_the_host_clock": nbytes / staged / 1e9, "share_of_the_copy_rate_by_the_host_clock": nbytes / staged / 1e9 / rate.value}
    print(kind, "jobs", len(jobs), "staged", sum(plan), "direct %.1f us  plan %.1f us  per batch (host clock, %d calls back to back)" % (direct * 1e6, staged * 1e6, reps),
          "bytes %.1f MB  copy rate %.0f GB/s" % (nbytes / 1e6, rate.value), flush=True)
    return res


def main():
    out, mode = sys.argv[1], sys.argv[2]
    vs = capi.load()
    if vs.lib.vs_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured here")
    res = {"size": [W, H], "build": vs.lib.vs_build_tag().decode(), "mode": mode}
    if mode == "stages":
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 128
        steps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
        rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 3
        res.update({"surfaces_per_step": n, "timed_steps": steps, "rounds": rounds})
        res.update(measure_stages(vs, n, steps, rounds))
    else:
        kind = sys.argv[3]
        pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 15
        reps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
        osize = (int(sys.argv[6]), int(sys.argv[7])) if len(sys.argv) > 7 else (W, H)
        res.update(measure_kernels(vs, kind, pairs, reps, osize))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
