"""The batch schedule issues a step's warps two steps after the step that analysed the frames (WARP_LAG, stab_internal.h): up to two
steps' warps are pending while a third step is built.  Nothing about the results may change: every run here is compared byte for
byte with the per-frame pipeline (set_batch never called, frames copied into the instance's queue) on the same clip, whole output
allocations, as test_zero_copy_input_matches_queued_copy does."""
import functools

import numpy as np
import pytest

from vsamd import capi, synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
CLIP_FRAMES = 96


class Clip:
    """A stream's input: frame i of a run is frame pos(i) of a short rendered clip played forwards and backwards (no jump where it
    turns), so that runs of several hundred pushes need no longer rendering.  `shift`: another picture of the same layout."""

    def __init__(self, kind, shift=0, border=0):
        self.kind, self.shift, self.border = kind, shift, border
        bgr = _rendered()
        if kind == "BGR8":
            self.fmt, self.pitch = capi.FMT_BGR8, W * 3
            frames = bgr
        else:
            self.fmt, self.pitch = capi.FMT_NV12, W
            frames = _rendered_nv12()
        if shift:
            frames = [np.roll(x, shift, axis=1) for x in frames]         # (an even number of samples: NV12 chroma pairs stay pairs)
        self.frames = np.stack(frames).reshape(len(frames), -1)
        self.fb = self.frames.shape[1]
        ow, oh = W + 2 * border, H + 2 * border
        self.out_pitch = ow * 3 if kind == "BGR8" else ow
        self.out_fb = self.out_pitch * (oh if kind == "BGR8" else oh * 3 // 2)

    @staticmethod
    def pos(i):
        i %= 2 * CLIP_FRAMES - 2
        return i if i < CLIP_FRAMES else 2 * CLIP_FRAMES - 2 - i

    def take(self, n):
        return self.frames[[self.pos(i) for i in range(n)]]


@functools.lru_cache(maxsize=None)
def _rendered():
    return synth.make_clip(synth.SEED_CONFIG1 + 57, W, H, CLIP_FRAMES)


@functools.lru_cache(maxsize=None)
def _rendered_nv12():
    return [synth.bgr_to_nv12(x) for x in _rendered()]


@functools.lru_cache(maxsize=None)
def clip(kind, shift=0, border=0):
    return Clip(kind, shift, border)


def drive(gpu, c, n, batch, zero_copy, params, setup=None, sync_at=(), at_sync=None, instance=None):
    """n pushes of clip c through the device entry points, then flush_dev to the end and a sync; the whole output allocation (zeroed
    first) comes back as (n, out_fb) bytes.  batch None: the per-frame pipeline.  at_sync(i, k, d_in, d_out): called behind the
    sync() that follows push i, with the number of results produced so far.  instance: a stabilizer to use (and keep) instead of a
    new one."""
    d_in = capi.DevBuf.from_array(gpu, c.take(n))
    d_out = capi.DevBuf(gpu, n * c.out_fb)
    d_out.zero()
    s = instance or gpu.stabilizer(gpu.params(**params))
    try:
        if instance is None:
            if batch is not None:
                s.set_batch(batch)
            s.set_zero_copy(zero_copy)
            if setup:
                setup(s)
        k = 0
        for i in range(n):
            k += s.push_dev(d_in.ptr + i * c.fb, W, H, c.pitch, c.fmt, d_out.ptr + k * c.out_fb, c.out_pitch)
            if i in sync_at:
                s.sync()
                if at_sync:
                    at_sync(i, k, d_in, d_out)
        while s.flush_dev(d_out.ptr + k * c.out_fb, c.out_pitch):
            k += 1
        s.sync()
        assert k == n
        return d_out.download((n, c.out_fb), np.uint8)
    finally:
        if instance is None:
            s.close()
        d_in.free(); d_out.free()


_refs = {}


def reference(gpu, c, n, params, setup=None):
    """The per-frame pipeline on the first n frames of c, computed once per (clip, n, params) and never modified."""
    key = (c.kind, c.shift, c.border, n, tuple(sorted(params.items())))
    if key not in _refs:
        ref = drive(gpu, c, n, None, False, params, setup)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def frames_for(batch, steps=5):
    """The first push only starts the stream; `steps` full steps, then a partial one of about half a step."""
    return 1 + steps * batch + batch // 2 + 1


@pytest.mark.parametrize("mode", ["BGR8-zero-copy", "BGR8-copy-in", "NV12-zero-copy"])
@pytest.mark.parametrize("batch", [2, 5, 33, 64])
def test_batch_sizes_equal_the_per_frame_pipeline(gpu, batch, mode):
    """Five full steps, a partial one and flush_dev to the end, with no sync in between: two steps' warps are pending from the
    second step on, and the last full step, the partial one and the one before them are all issued by the drain of the first flush."""
    kind, zc = mode.split("-", 1)
    c, params = clip(kind), dict(smoothing_radius=6)
    n = frames_for(batch)
    got = drive(gpu, c, n, batch, zc == "zero-copy", params)
    assert np.array_equal(got, reference(gpu, c, n, params))


def test_sync_meets_zero_one_and_two_pending_steps(gpu):
    """Batches of 8, radius 5; the first push only starts the stream, so the first step closes behind push 8, and every step has due
    outputs.  The sync behind push 8 meets one pending step; behind push 9 none, and one queued frame, which it analyses as a step
    of its own; behind push 10 the same.  The next steps close behind pushes 18 and 26: the sync behind push 26 meets two pending
    steps.  Then 34: the sync behind push 37 meets one pending step and three queued frames.  Then 45 and 53: two pending steps
    again.  Every result produced so far is complete when sync returns: it is downloaded and compared there."""
    c, params, batch = clip("BGR8"), dict(smoothing_radius=5), 8
    SYNCS = (8, 9, 10, 26, 37, 53)
    n = frames_for(batch, 6)
    assert n == 54
    ref = reference(gpu, c, n, params)
    seen = []

    def at_sync(i, k, d_in, d_out):
        seen.append((i, k))
        if k:
            assert np.array_equal(d_out.download((k, c.out_fb), np.uint8), ref[:k]), (i, k)

    got = drive(gpu, c, n, batch, True, params, sync_at=SYNCS, at_sync=at_sync)
    assert np.array_equal(got, ref)
    # a push produces the result of the frame pushed radius - 1 pushes earlier (warm-up: clamp(radius, 5, 35) queued frames)
    assert seen == [(i, i - 3) for i in SYNCS]


def test_zero_copy_inputs_may_be_overwritten_after_sync(gpu):
    """vs_stab_set_zero_copy: an input frame whose result has been produced is the caller's again once vs_stab_sync has returned.
    Batches of 5: the syncs behind pushes 5, 15, 16, 31 and 34 meet one pending step, two, none (and a queued frame), two, and none
    (and three queued frames).  Every such frame is overwritten behind each sync; the outputs equal the run with untouched inputs."""
    c, params, batch = clip("BGR8"), dict(smoothing_radius=6), 5
    n = frames_for(batch, 7)
    ref = reference(gpu, c, n, params)
    done = [0]
    junk = np.full(c.fb, 0xA5, np.uint8)

    def at_sync(i, k, d_in, d_out):
        for j in range(done[0], k):          # (result j is frame j's)
            d_in.upload(junk, j * c.fb)
        done[0] = k

    got = drive(gpu, c, n, batch, True, params, sync_at=(5, 15, 16, 31, 34), at_sync=at_sync)
    assert done[0] > 0
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("batch", [64, 32])
def test_copy_in_ring_holds_two_steps_of_pending_warps(gpu, batch):
    """Copy-in mode, radius 35, six steps and the start of a seventh without a sync: 35 queued frames, the batch being collected and two
    steps whose warps are still to come hold ring slots at once (35 + 3 x batch: more than the ring held when warps lagged one
    step).  No VS_ERR_CAPACITY ("frame ring exhausted" raises VsError), and the same outputs."""
    c, params = clip("BGR8"), dict(smoothing_radius=35)
    n = 1 + 6 * batch + batch - 1
    got = drive(gpu, c, n, batch, False, params)
    assert np.array_equal(got, reference(gpu, c, n, params))


def test_group_of_three_with_a_late_and_an_early_stream(gpu):
    """A vs_batch of three streams, steps of 4 frames per stream: stream 1 gets its first frame two steps late, stream 2 stops while
    its last two steps' warps are pending (they go out with the steps the others still run).  Each stream equals the per-frame
    pipeline on its own frames."""
    S, B, n, params = 3, 4, 1 + 7 * 4 + 2, dict(smoothing_radius=5)
    cl = [clip("BGR8", 12 * j) for j in range(S)]
    first, last = [0, 2 * B + 1, 0], [n, n, 1 + 4 * B]            # stream j takes part in the pushes first[j] <= i < last[j]
    cnt = [last[j] - first[j] for j in range(S)]
    d_in = [capi.DevBuf.from_array(gpu, cl[j].take(cnt[j])) for j in range(S)]
    d_out = [capi.DevBuf(gpu, cnt[j] * cl[j].out_fb) for j in range(S)]
    for b in d_out:
        b.zero()
    fb, pitch = cl[0].fb, cl[0].pitch
    g = gpu.batch(gpu.params(**params), S, B)
    try:
        g.set_zero_copy(True)
        k = [0] * S
        for i in range(n):
            on = [first[j] <= i < last[j] for j in range(S)]
            prod = g.push_dev([d_in[j].ptr + (i - first[j]) * fb if on[j] else None for j in range(S)], W, H, pitch, capi.FMT_BGR8,
                              [d_out[j].ptr + k[j] * fb if on[j] else None for j in range(S)], pitch)
            k = [k[j] + prod[j] for j in range(S)]
        while True:
            prod = g.flush_dev([d_out[j].ptr + min(k[j], cnt[j] - 1) * fb for j in range(S)], pitch)
            k = [k[j] + prod[j] for j in range(S)]
            if not any(prod):
                break
        g.sync()
        assert k == cnt
        got = [d_out[j].download((cnt[j], fb), np.uint8) for j in range(S)]
    finally:
        g.close()
        for b in d_in + d_out:
            b.free()
    for j in range(S):
        assert np.array_equal(got[j], reference(gpu, cl[j], cnt[j], params)), j


def test_kalman_stream_builds_its_tables_behind_the_tail(gpu):
    """A Kalman stream's maps come out of the tail workgroup and its coordinate tables are a launch behind it, in the step that
    analysed the frames - two steps before the warps that read them."""
    c, params, batch = clip("BGR8"), dict(smoothing_radius=6, smoothing_method=capi.SMOOTH_KALMAN), 8
    n = frames_for(batch)
    assert np.array_equal(drive(gpu, c, n, batch, True, params), reference(gpu, c, n, params))


def test_nv12_border_pad_scratch_surfaces_over_four_steps(gpu):
    """Border pad on NV12 pads the frames of a warp launch into the stream's scratch surfaces right in front of it; both pending steps
    name the same scratch surfaces, and only the order of their launches keeps them apart."""
    b, batch = 6, 8
    c, params = clip("NV12", 0, b), dict(smoothing_radius=6, border_size=b, border_type=capi.BORDER_BLACK)
    n = frames_for(batch)

    def setup(s):
        s.set_yuv_border_pad(True)

    got = drive(gpu, c, n, batch, True, params, setup)
    assert np.array_equal(got, reference(gpu, c, n, params, setup))


def test_clean_and_destroy_with_two_steps_pending(gpu):
    """vs_stab_clean drains two pending steps and the instance starts again like a fresh one; vs_stab_destroy with two steps pending
    leaves the device usable."""
    c, params, batch = clip("BGR8"), dict(smoothing_radius=6), 8
    n = frames_for(batch)
    ref = reference(gpu, c, n, params)
    d_in = capi.DevBuf.from_array(gpu, c.take(1 + 3 * batch))
    d_out = capi.DevBuf(gpu, (1 + 3 * batch) * c.out_fb)
    s = gpu.stabilizer(gpu.params(**params))
    try:
        s.set_batch(batch)
        s.set_zero_copy(True)

        def three_steps():
            k = 0
            for i in range(1 + 3 * batch):          # behind the third step the warps of the second and the third are pending
                k += s.push_dev(d_in.ptr + i * c.fb, W, H, c.pitch, c.fmt, d_out.ptr + k * c.out_fb, c.out_pitch)
            return k

        assert three_steps() == 3 * batch - 4
        s.clean()
        assert np.array_equal(drive(gpu, c, n, batch, True, params, instance=s), ref)
        s.clean()
        assert three_steps() == 3 * batch - 4
    finally:
        s.close()
        d_in.free(); d_out.free()
    assert np.array_equal(drive(gpu, c, n, batch, True, params), ref)
