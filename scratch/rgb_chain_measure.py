"""Measurement for DESIGN section 8 "Interleaved chain": 1920 x 1080, 64 frames resident.  mode `new`: everything; mode `parent`:
the synchronous BGR8 loops only (run with VS_LAB=1 VS_LIB_PATH=<parent library>)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stab_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle_lib
import roll_scene
from test_azc import rotated_frame
from vsamd import capi, synth

mode = sys.argv[1]
W, H, N = 1920, 1080, 64
vs = capi.load()
oracle = oracle_lib.load()
oracle.lib.vso_set_threads(8)
out = {"mode": mode, "lib": os.environ.get("VS_LIB_PATH", "tree")}


def timed(f, frames, warm=2, rounds=7):
    for _ in range(warm):
        f()
    r = []
    for _ in range(rounds):
        t = time.perf_counter()
        f()
        r.append(frames / (time.perf_counter() - t))
    return {"median_fps": round(statistics.median(r)), "min_fps": round(min(r)), "max_fps": round(max(r))}


roll_bgr = [roll_scene.horizon_frame(W, H, 45 + i, seed=i, offset=i - 3) for i in range(8)]
zoom_bgr = [rotated_frame(oracle, W, H, d, seed=i) for i, d in enumerate([4.0, -2.5, 1.0, 7.5, -6.0, 0.5, 3.0, -1.0])]


def resident(frames8, fmt):
    """64 frames (the eight, repeated) of format fmt in one allocation -> (buffer, pointers, frame bytes, stride)."""
    if fmt == capi.FMT_NV12:
        fr = [synth.bgr_to_nv12(f) for f in frames8]
        stride = W
    else:
        a = np.random.default_rng(1).integers(0, 256, (H, W), np.uint8)
        fr = [f if fmt == capi.FMT_BGR8 else np.ascontiguousarray(np.dstack([f, a])) for f in frames8]
        stride = W * fr[0].shape[2]
    fb = fr[0].nbytes
    buf = capi.DevBuf(vs, fb * N)
    for i in range(N):
        buf.upload(fr[i % 8], i * fb)
    return buf, [buf.ptr + i * fb for i in range(N)], fb, stride


SYNC_REP = 24
REP = 300    # passes over the 64 frames per timed window (0.2 s and more)

# ---- roll
for name, fmt in (("bgr8", capi.FMT_BGR8), ("bgra8", capi.FMT_BGRA8), ("nv12", capi.FMT_NV12)):
    if mode == "parent" and name != "bgr8":
        continue
    src, ins, fb, stride = resident(roll_bgr, fmt)
    dst = capi.DevBuf(vs, fb * N)
    outs = [dst.ptr + i * fb for i in range(N)]
    rg = vs.roll_correction()
    if mode == "new":
        def run():
            for _ in range(REP):
                if fmt == capi.FMT_NV12:
                    rg.correct_nv12_dev_n(ins, W, H, stride, outs, stride)
                else:
                    rg.correct_rgb_dev_n(fmt, ins, W, H, stride, outs, stride)
            rg.sync()
        out["roll_async_" + name] = timed(run, N * REP)
    if name == "bgr8":
        def run_sync():
            for i in range(N * SYNC_REP):
                rg.correct_dev(ins[i % N], W, H, stride, outs[i % N], stride)
            rg.sync()
        out["roll_sync_loop_bgr8"] = timed(run_sync, N * SYNC_REP, rounds=5)
    rg.close(); src.free(); dst.free()

# ---- zoom
for name, fmt in (("bgr8", capi.FMT_BGR8), ("bgra8", capi.FMT_BGRA8), ("nv12", capi.FMT_NV12)):
    if mode == "parent" and name != "bgr8":
        continue
    src, ins, fb, stride = resident(zoom_bgr, fmt)
    dst = capi.DevBuf(vs, fb * N)
    outs = [dst.ptr + i * fb for i in range(N)]
    az = vs.auto_zoom_crop()
    if mode == "new":
        def run():
            for _ in range(REP):
                if fmt == capi.FMT_NV12:
                    az.apply_nv12_dev_n(ins, W, H, stride, outs, stride, stride * H)
                else:
                    az.apply_rgb_dev_n(fmt, ins, W, H, stride, outs, stride)
            az.sync()
        out["zoom_async_" + name] = timed(run, N * REP)
    if name == "bgr8":
        def run_sync():
            for i in range(N * SYNC_REP):
                az.apply_dev(ins[i % N], W, H, stride, 3, outs[i % N], stride)
            az.sync()
        out["zoom_sync_loop_bgr8"] = timed(run_sync, N * SYNC_REP, rounds=5)
    az.close(); src.free(); dst.free()

# ---- the staged scale launch beside a plain copy of the same bytes (eight jobs: crops of 1728 x 972 zoomed to 1920 x 1080)
if mode == "new":
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for cn in (3, 4):
        fb = W * H * cn
        src, dst = capi.DevBuf(vs, fb * 8), capi.DevBuf(vs, fb * 8)
        src.upload(np.random.default_rng(cn).integers(0, 256, fb * 8, np.uint8))
        jobs = [(src.ptr + i * fb + (54 * W + 96) * cn, W * cn, 1728, 972, dst.ptr + i * fb, W * cn, W, H, cn) for i in range(8)]
        assert vs.scale_jobs_rgb_plan(jobs).tolist() == [1] * 8
        K = 2000

        def launch():
            for _ in range(K):
                vs.scale_jobs_rgb(jobs)
            vs.sync()

        def copy():
            for _ in range(K):
                assert hip.hipMemcpy(dst.ptr, src.ptr, fb * 8, 3) == 0
            vs.sync()

        def us(f):
            f(); f()
            r = []
            for _ in range(7):
                t = time.perf_counter(); f(); r.append((time.perf_counter() - t) / K * 1e6)
            return {"median_us": round(statistics.median(r), 1), "min_us": round(min(r), 1), "max_us": round(max(r), 1)}
        out["scale_staged_cn%d_8x1080p" % cn] = us(launch)
        out["copy_same_bytes_cn%d" % cn] = us(copy)
        out["bytes_written_cn%d" % cn] = fb * 8
        src.free(); dst.free()

print(json.dumps(out))
os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
with open(os.path.join(ROOT, "build", "rgb_measure_%s_%s.json" % (mode, sys.argv[2] if len(sys.argv) > 2 else "0")), "w") as f:
    json.dump(out, f, indent=1)
