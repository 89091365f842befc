"""BASELINE configs[2] as bench.py drives it: RollCorrection -> stabilize (batch mode, zero-copy) -> AutoZoomCrop on 3840x2160
NV12 surfaces, chunk by chunk, ONE free-running host thread per stage over ring buffers that are written again while the other
stages still run.  The overlapped chain must produce exactly what the same chain produces with one stage at a time (and the
oracle's chain on the same surfaces): every result, every output byte, the roll stage's state and the stabilizer's counters."""
import threading

import numpy as np
import pytest

from vsamd import capi, synth

pytestmark = pytest.mark.gpu

W4K, H4K = 3840, 2160


def chain_params(vs, **over):
    """bench.py's make_params(vs, max_corners=400): configs[2]'s corners with configs[1]'s 3-level LK 21x21, radius 30."""
    kw = dict(max_corners=400, lk_win_size=21, lk_max_level=2, lk_max_iters=20, lk_epsilon=0.03, smoothing_radius=30)
    kw.update(over)
    return vs.params(**kw)


def run_chain(vs, W, H, CH, batch, params, rings, lags, n_chunks, src, overlap=True):
    """The schedule of bench.py's config2_chain (bench.py:497-612; keep the two in step) on n_chunks chunks of CH surfaces:
    roll(c) writes ring slot c % R of the roll results, stab(c) pushes them (batch `batch`, zero-copy) and writes its outputs to
    slot c % S, zoom(c) crops those into slot c % Z.  overlap=True: one thread per stage, roll(c) after stab(c - lags[0]),
    stab(c) after zoom(c - lags[1]), a failed stage releases the others.  overlap=False: the serial reference, roll -> sync ->
    stabilize -> sync -> zoom -> sync per chunk on this thread.  One chunk more than the bench runs: the stabilizer's flush
    (every surface comes out).  src(i): the device pointer of input surface i.  The zoom stage downloads every result right
    after its sync, before slot c % Z is written again.  Returns the results [(ow, oh, info, NV12 rows of the output)], the roll
    stage's state and the stabilizer's frames_out."""
    R, S, Z = rings
    lag_r, lag_s = lags
    sb = W * H * 3 // 2
    bufs = [capi.DevBuf(vs, sb * CH) for _ in range(R + S + Z)]     # (a zoom slot holds the fall-back: the unchanged surface)
    d_roll, d_stab, d_zoom = bufs[:R], bufs[R:R + S], bufs[R + S:]
    rc, az, st = vs.roll_correction(), vs.auto_zoom_crop(), vs.stabilizer(params)
    st.set_batch(batch)
    st.set_zero_copy(True)
    produced = {}                      # chunk -> stabilized surfaces it yielded
    results = []
    total = n_chunks + 1               # (the last chunk: the flush)

    def roll_stage(c):
        if c == n_chunks:
            return
        # ring invariant: the surfaces of chunk c - R, which slot c % R holds, are released - their results produced (and
        # synced) by stab(c - lag_r) at the latest
        assert sum(produced[j] for j in range(c - lag_r + 1)) >= (c - R + 1) * CH, ("R ring reused too early", c)
        rc.correct_nv12_dev_n([src(c * CH + i) for i in range(CH)], W, H, W, [d_roll[c % R].ptr + i * sb for i in range(CH)], W)
        rc.sync()

    def stab_stage(c):
        # ring invariant: the outputs of chunk c - S, which slot c % S holds, have been cropped by zoom(c - lag_s) at the latest
        assert sum(produced[j] for j in range(c - lag_s + 1)) >= sum(produced[j] for j in range(c - S + 1)), ("S ring reused too early", c)
        out = d_stab[c % S].ptr
        if c < n_chunks:
            produced[c] = st.push_dev_n([d_roll[c % R].ptr + i * sb for i in range(CH)], W, H, W, capi.FMT_NV12,
                                        [out + j * sb for j in range(CH)], W)
        else:
            k = 0
            while True:
                assert k < CH, "the flush holds more than a chunk"
                if not st.flush_dev(out + k * sb, W):
                    break
                k += 1
            produced[c] = k
        st.sync()

    def zoom_stage(c):
        k = produced[c]
        if not k:
            return
        slot = d_zoom[c % Z]
        tickets = az.apply_nv12_dev_n([d_stab[c % S].ptr + j * sb for j in range(k)], W, H, W, [slot.ptr + j * sb for j in range(k)], W, W * H)
        az.sync()
        for j, t in enumerate(tickets):
            ow, oh, info = az.result(t)
            y = slot.download((oh, W), np.uint8, j * sb)[:, :ow]
            uv = slot.download((oh // 2, W), np.uint8, j * sb + W * H)[:, :ow]
            results.append((ow, oh, info.tolist(), np.concatenate([y, uv])))

    try:
        if not overlap:
            for c in range(total):
                roll_stage(c)
                stab_stage(c)
                zoom_stage(c)
        else:
            done = {"roll": -1, "stab": -1, "zoom": -1}
            cond = threading.Condition()
            failed = []

            def wait_for(stage, c):
                with cond:
                    cond.wait_for(lambda: done[stage] >= c or failed)
                return not failed

            def stage_loop(name, f, before, after, lag):
                try:
                    for c in range(total):
                        if before and not wait_for(before, c):
                            return
                        if after and not wait_for(after, c - lag):
                            return
                        f(c)
                        with cond:
                            done[name] = c
                            cond.notify_all()
                except BaseException as e:          # (a failed stage must not leave the others waiting)
                    with cond:
                        failed.append(e)
                        cond.notify_all()

            ths = [threading.Thread(target=stage_loop, args=a) for a in (("roll", roll_stage, None, "stab", lag_r),
                                                                         ("stab", stab_stage, "roll", "zoom", lag_s),
                                                                         ("zoom", zoom_stage, "stab", None, 0))]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            if failed:
                raise failed[0]
        return results, rc.state(), st.counters().frames_out
    finally:
        for o in (st, rc, az):
            o.close()
        for b in bufs:
            b.free()


def test_overlapped_chain_at_the_bench_schedule_equals_the_serial_chain(gpu):
    """bench.py's chain as it is timed: the bench's device-built clip of 64 surfaces, chunks of 128, batch 64, rings 4 / 3 / 2,
    lags 3 / 3; six chunks, so every ring slot is written again while the other stages run.  Equal to the serial chain."""
    W, H, CH, NF, n_chunks = W4K, H4K, 128, 64, 6
    sb = W * H * 3 // 2
    clip = synth.make_clip_dev(gpu, synth.SEED_CONFIG3, W, H, NF, nv12=True)
    try:
        runs = [run_chain(gpu, W, H, CH, 64, chain_params(gpu), (4, 3, 2), (3, 3), n_chunks, lambda i: clip.ptr + (i % NF) * sb, overlap=o)
                for o in (False, True)]
    finally:
        clip.free()
    (ref, ref_state, ref_out), (got, state, out) = runs
    assert len(got) == len(ref) == n_chunks * CH
    for j, (a, b) in enumerate(zip(got, ref)):
        assert a[:3] == b[:3], j
        assert a[3].shape == b[3].shape and np.array_equal(a[3], b[3]), j
    assert state == ref_state
    assert out == ref_out == n_chunks * CH
    n_crop = sum(int(r[2][7]) for r in ref)
    assert n_crop >= len(ref) * 9 // 10, n_crop
    assert all((r[0], r[1]) == ((640, 360) if r[2][7] else (W, H)) for r in ref)


def test_overlapped_chain_against_the_oracle(gpu, oracle):
    """The overlapped chain with small chunks (16 surfaces, batch 8, radius 5): ring slots are reused in every stage from the
    fifth chunk on.  Six chunks of the existing 4K chain test's surfaces (the SEED_CONFIG3 clip with a tilted-horizon band)
    against the oracle's chain on the same 96 surfaces: every result, its bytes and the stages' states."""
    import roll_scene
    W, H, CH, n_chunks = W4K, H4K, 16, 6
    N = CH * n_chunks
    surfs = roll_scene.chain_surfaces(W, H, N)
    distinct = roll_scene.chain_surfaces(W, H, 7)
    assert all(surfs[i] is distinct[i % 7] for i in range(N))
    sb = W * H * 3 // 2
    params = dict(smoothing_radius=5, max_corners=400)
    # ---- oracle chain (tests/test_gpu_pipeline.py, the 4K chain test)
    oracle.lib.vso_set_threads(16)
    try:
        ro, so = oracle.roll_correction(), oracle.stabilizer(oracle.params(**params))
        ref = []
        for s in surfs:
            r = ro.correct_nv12(s, W, H)
            o = so.push(r, capi.FMT_NV12)
            if o is not None:
                ref.append(oracle.auto_zoom_crop_nv12(o, W, H))
        while True:
            o = so.flush(surfs[0], capi.FMT_NV12)
            if o is None:
                break
            ref.append(oracle.auto_zoom_crop_nv12(o, W, H))
        so.close()
    finally:
        oracle.lib.vso_set_threads(1)
    # ---- overlapped device chain
    d_in = capi.DevBuf(gpu, sb * len(distinct))
    try:
        for i, s in enumerate(distinct):
            d_in.upload(s, i * sb)
        got, state, out = run_chain(gpu, W, H, CH, 8, gpu.params(**params), (4, 3, 2), (3, 3), n_chunks, lambda i: d_in.ptr + (i % 7) * sb)
    finally:
        d_in.free()
    assert len(got) == len(ref) == N and out == N
    assert state == ro.state()
    n_crop = 0
    for j, ((ow, oh, info, px), (want, winfo)) in enumerate(zip(got, ref)):
        assert info == winfo.tolist(), j
        assert (ow, oh) == ((640, 360) if winfo[7] else (W, H)), j
        assert px.shape == want.shape and np.array_equal(px, want), j
        n_crop += int(winfo[7])
    assert n_crop >= N - 1
