"""Speed of roll correction, auto zoom/crop and the chain on planar 4:2:0 surfaces at 3840 x 2160, beside the two-plane format that
holds the same samples, in ONE process ("I420 chain"; profiles/r12_i420_chain_speed_4k.json).

  stages   roll alone and zoom alone: NV12 against I420, P010 against I010 - N surfaces per timed step (64 distinct inputs in a
           cycle, results into buffers of their own), a host clock around the calls and the stage's sync; the two formats alternated
           ROUNDS times, so the first format's own runs give the spread the ratio is read against
  chain    roll -> stabilize (batch mode, zero-copy) -> zoom, one stage at a time per chunk of 64: I420 surfaces as they are, against
           the NV12 chain with the two passes a caller of the two-plane entry points has to add - U, V -> UV in front, UV -> U, V
           behind -, each stood in for by a plain device copy of the bytes it moves (a lower bound of its cost)

Usage: python scratch/i420_chain_speed.py out.json [n_per_step] [steps] [rounds] [all | stages | chain]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-stab_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import roll_scene                     # noqa: E402
from vsamd import capi, synth         # noqa: E402

W, H = 3840, 2160
NSRC = 64
I420, I010 = capi.FMT_I420, capi.FMT_I010


_pictures = []


def pictures():
    """The seven distinct 4K NV12 pictures of the chain tests, rendered once (half a minute of host time)."""
    if not _pictures:
        _pictures.extend(roll_scene.chain_surfaces(W, H, 7))
    return _pictures


def surfaces(vs, kind):
    """NSRC input surfaces of `kind` on the device (seven distinct pictures in a cycle), and their size in bytes."""
    nv = pictures()
    if kind == "nv12":
        host = nv
    elif kind == "i420":
        host = [synth.nv12_to_i420(s) for s in nv]
    else:
        p = [synth.nv12_to_p010(s, seed=i) for i, s in enumerate(nv)]
        host = p if kind == "p010" else [synth.p010_to_i010(s, W, H, 10) for s in p]
    sb = host[0].nbytes
    d = capi.DevBuf(vs, sb * NSRC)
    for i in range(NSRC):
        d.upload(np.ascontiguousarray(host[i % 7]), i * sb)
    return d, sb


def stage_step(vs, stage, kind, d_in, d_out, sb, n):
    """One object, one timed step function: n surfaces through the stage, then its sync."""
    sample = 2 if kind in ("p010", "i010") else 1
    pitch = W * sample
    ins = [d_in.ptr + (i % NSRC) * sb for i in range(n)]
    outs = [d_out.ptr + (i % NSRC) * sb for i in range(n)]
    lay = capi.i420_layout(pitch)
    fmt = I420 if kind == "i420" else I010
    if stage == "roll":
        o = vs.roll_correction()
        if kind == "nv12":
            f = lambda: o.correct_nv12_dev_n(ins, W, H, pitch, outs, pitch)
        elif kind == "p010":
            f = lambda: o.correct_p010_dev_n(ins, W, H, pitch, outs, pitch)
        else:
            f = lambda: o.correct_i420_dev_n(fmt, ins, W, H, lay, outs, lay)
    else:
        o = vs.auto_zoom_crop()
        if kind == "nv12":
            f = lambda: o.apply_nv12_dev_n(ins, W, H, pitch, outs, pitch, pitch * H)
        elif kind == "p010":
            f = lambda: o.apply_p010_dev_n(ins, W, H, pitch, outs, pitch, pitch * H)
        else:
            f = lambda: o.apply_i420_dev_n(fmt, ins, W, H, lay, outs, lay)

    def step():
        f()
        o.sync()
    return o, step


def time_steps(step, steps):
    step()                               # warm-up: code objects, work areas, worker threads
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        out.append(time.perf_counter() - t0)
    return out


def measure_stages(vs, n, steps, rounds):
    res = {}
    for stage in ("roll", "zoom"):
        for a, b in (("nv12", "i420"), ("p010", "i010")):
            bufs = {}
            for k in (a, b):
                d_in, sb = surfaces(vs, k)
                bufs[k] = (d_in, capi.DevBuf(vs, sb * NSRC), sb)
            runs = {a: [], b: []}
            for _ in range(rounds):
                for k in (a, b):
                    d_in, d_out, sb = bufs[k]
                    o, step = stage_step(vs, stage, k, d_in, d_out, sb, n)
                    ts = time_steps(step, steps)
                    o.close()
                    runs[k].append(n / float(np.median(ts)))
            for k in (a, b):
                bufs[k][0].free()
                bufs[k][1].free()
            fa, fb = float(np.median(runs[a])), float(np.median(runs[b]))
            res["%s_%s_vs_%s" % (stage, b, a)] = {a + "_surfaces_per_s": runs[a], b + "_surfaces_per_s": runs[b], "ratio_%s_over_%s" % (b, a): fb / fa,
                                                  a + "_spread": (max(runs[a]) - min(runs[a])) / fa}
            print(stage, a, ["%.0f" % v for v in runs[a]], b, ["%.0f" % v for v in runs[b]], "ratio %.3f" % (fb / fa), flush=True)
    return res


def measure_chain(vs, steps, rounds):
    """n = NSRC surfaces per step.  The two repacking passes of the NV12 side are plain device copies of the bytes they would move
    (1.5 w h in front, 1.5 x 640 x 360 per result behind): no interleaving kernel can be faster than the copy of its bytes, so the
    figure is a LOWER bound of what the planar entry points save."""
    from test_gpu_chain import chain_params
    n = NSRC
    sb = W * H * 3 // 2
    src, _ = surfaces(vs, "i420")
    bufs = [capi.DevBuf(vs, sb * n) for _ in range(5)]
    t_nv, t_roll, t_stab, t_zoom, t_out = bufs
    ptrs = lambda d: [d.ptr + i * sb for i in range(n)]
    lay = capi.i420_layout(W)
    small = 640 * 360 * 3 // 2

    def make(planar):
        rc, az, st = vs.roll_correction(), vs.auto_zoom_crop(), vs.stabilizer(chain_params(vs))
        st.set_batch(64)
        st.set_zero_copy(True)

        def step():
            if planar:
                rc.correct_i420_dev_n(I420, ptrs(src), W, H, lay, ptrs(t_roll), lay)
                rc.sync()
                k = st.push_dev_n(ptrs(t_roll), W, H, W, I420, ptrs(t_stab), W)
                st.sync()
                if k:
                    az.apply_i420_dev_n(I420, ptrs(t_stab)[:k], W, H, lay, ptrs(t_zoom)[:k], lay)
                    az.sync()
            else:
                vs.check(vs.lib.vs_dev_memcpy_d2d(t_nv.ptr, src.ptr, sb * n))                 # stands for U, V -> UV in front
                rc.correct_nv12_dev_n(ptrs(t_nv), W, H, W, ptrs(t_roll), W)
                rc.sync()
                k = st.push_dev_n(ptrs(t_roll), W, H, W, capi.FMT_NV12, ptrs(t_stab), W)
                st.sync()
                if k:
                    az.apply_nv12_dev_n(ptrs(t_stab)[:k], W, H, W, ptrs(t_zoom)[:k], W, W * H)
                    az.sync()
                    vs.check(vs.lib.vs_dev_memcpy_d2d(t_out.ptr, t_zoom.ptr, small * k))      # stands for UV -> U, V behind
            return k
        return (rc, az, st), step

    runs = {"i420_direct": [], "nv12_with_copies_for_the_repacking": []}
    for _ in range(rounds):
        for name, planar in (("nv12_with_copies_for_the_repacking", False), ("i420_direct", True)):
            objs, step = make(planar)
            step()                       # fills the smoothing queue (radius 30 < n) and warms up
            ts = []
            for _ in range(steps):
                t0 = time.perf_counter()
                k = step()
                ts.append(time.perf_counter() - t0)
                assert k == n, k
            for o in objs:
                o.close()
            runs[name].append(n / float(np.median(ts)))
    for d in bufs + [src]:
        d.free()
    a, b = float(np.median(runs["nv12_with_copies_for_the_repacking"])), float(np.median(runs["i420_direct"]))
    print("chain", {k: ["%.0f" % v for v in r] for k, r in runs.items()}, "ratio %.3f" % (b / a), flush=True)
    return {"chain_serial_surfaces_per_s": runs, "ratio_i420_direct_over_nv12_with_copies": b / a,
            "nv12_with_copies_spread": (max(runs["nv12_with_copies_for_the_repacking"]) - min(runs["nv12_with_copies_for_the_repacking"])) / a}


def main():
    out = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    only = sys.argv[5] if len(sys.argv) > 5 else "all"          # all | stages | chain
    vs = capi.load()
    if vs.lib.vs_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured here")
    res = {"size": [W, H], "surfaces_per_step": n, "timed_steps": steps, "rounds": rounds, "build": vs.lib.vs_build_tag().decode()}
    if only in ("all", "stages"):
        res.update(measure_stages(vs, n, steps, rounds))
    if only in ("all", "chain"):
        res.update(measure_chain(vs, steps, rounds))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
