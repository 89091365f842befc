"""1920x1080 stabilisation in batches of 64 (bench configs[1] settings, zero-copy device frames): BGR8 and BGRA8 frames/s,
measured alternately in one process.  argv[1]: rounds (default 3), argv[2]: steps of 64 frames per measurement (default 20)."""
import json
import sys
import time

import numpy as np

sys.path[:0] = ["video-stab_amd"]
from vsamd import capi, synth  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
W, H, N, B = 1920, 1080, 64, 64
KW = dict(max_corners=200, lk_win_size=21, lk_max_level=2, lk_max_iters=20, lk_epsilon=0.03, smoothing_radius=30)
vs = capi.load()
d = synth.make_clip_dev(vs, synth.SEED_CONFIG2, W, H, N)
bgr = d.download((N, H, W, 3), np.uint8)
alpha = np.random.default_rng(3).integers(0, 256, (N, H, W, 1), np.uint8)
clips = {capi.FMT_BGR8: d, capi.FMT_BGRA8: capi.DevBuf.from_array(vs, np.ascontiguousarray(np.concatenate([bgr, alpha], 3)))}


def run(fmt):
    cn = capi.FMT_CHANNELS[fmt]
    fb = W * H * cn
    s = vs.stabilizer(vs.params(**KW))
    s.set_batch(B)
    s.set_zero_copy(True)
    out = capi.DevBuf(vs, fb * 2 * B)
    src = clips[fmt]
    k = 0

    def push(i):
        nonlocal k
        k += s.push_dev(src.ptr + (i % N) * fb, W, H, W * cn, fmt, out.ptr + (k % (2 * B)) * fb, W * cn)
    for i in range(4 * B):            # warm-up
        push(i)
    s.sync()
    t = time.perf_counter()
    for i in range(steps * B):
        push(i)
    s.sync()
    dt = time.perf_counter() - t
    s.close(); out.free()
    return steps * B / dt


res = []
for r in range(rounds):
    for fmt, name in ((capi.FMT_BGR8, "bgr8"), (capi.FMT_BGRA8, "bgra8")):
        fps = run(fmt)
        res.append({"round": r, "fmt": name, "frames_per_s": round(fps, 1)})
        print(json.dumps(res[-1]), flush=True)
print(json.dumps({"median_bgr8": float(np.median([x["frames_per_s"] for x in res if x["fmt"] == "bgr8"])),
                  "median_bgra8": float(np.median([x["frames_per_s"] for x in res if x["fmt"] == "bgra8"]))}))
