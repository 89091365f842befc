"""tests/roi.py against fake numpy "operators" that misbehave by one byte: the proof that tests/test_gpu_roi.py can fail.

The operator is a horizontal [1 2 1] / 4 filter with a replicated border on a one-channel picture, written the way a kernel sees
memory: flat bytes, a start address and a pitch on either side.  One version is correct; each of the others does one thing wrong
that the packed wrappers of vsamd/capi.py cannot see.  Every faulty one must be reported in every layout of the table - by the
guard check or by the comparison with the reference of the picture alone - and the correct one must pass in every layout."""
import numpy as np
import pytest

import roi

SIZES = [(131, 19), (128, 16), (1, 1)]


def reference(pic):
    p = pic.astype(np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    return ((left + 2 * p + right + 2) >> 2).astype(np.uint8)


def fake_op(fault, src, sa, sp, dst, da, dp, w, h):
    """src / dst: the flat bytes of the two allocations; sa / da: address of the first pixel; sp / dp: pitches."""
    for y in range(h):
        row = src[sa + y * sp: sa + y * sp + w].astype(np.int32)
        lo = int(src[sa + y * sp - 1]) if fault == "reads_x_minus_1" else row[0]       # the parent's byte left of the ROI
        left = np.concatenate([[lo], row[:-1]])
        right = np.concatenate([row[1:], row[-1:]])
        dst[da + y * dp: da + y * dp + w] = (left + 2 * row + right + 2) >> 2
    if fault == "past_row_end":
        y = h // 2
        dst[da + y * dp + w] ^= 0x40
    elif fault == "before_first_row":
        dst[da - 1] ^= 0x40
    elif fault == "behind_last_row":
        dst[da + (h - 1) * dp + w] ^= 0x40
    return 0


def run(fault, layout, w, h):
    rng = np.random.default_rng(roi.case_seed("pic", w, h))
    pic = rng.integers(0, 256, (h, w), dtype=np.uint8)
    s, d = roi.pair(layout, roi.case_seed(fault, layout, w, h), (w, h), (w, h))
    s.put(pic).bind(None)
    d.bind(None)
    fake_op(fault, s.mem.data, s.ptr, s.pitch, d.mem.data, d.ptr, d.pitch, w, h)
    got, clean = d.result()
    return np.array_equal(got, reference(pic)), clean, s.untouched(), d


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", roi.LAYOUT_NAMES)
def test_correct_operator_passes(layout, w, h):
    equal, clean, src_kept, d = run(None, layout, w, h)
    assert equal and clean and src_kept, d.stray()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", roi.LAYOUT_NAMES)
@pytest.mark.parametrize("fault", ["past_row_end", "before_first_row", "behind_last_row"])
def test_stray_write_is_reported(fault, layout, w, h):
    equal, clean, _, d = run(fault, layout, w, h)
    if layout == "packed" and fault == "past_row_end" and h > 1:
        # today's blind spot, kept visible: in a packed picture the byte lands in the next row - the guards cannot see it, only
        # the comparison can (and on a GPU only if that row's own stores came first)
        assert clean and not equal
    else:
        assert equal and not clean
        assert "1 stray bytes" in d.stray()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", roi.LAYOUT_NAMES)
def test_read_of_the_parent_is_reported(layout, w, h):
    equal, clean, _, _ = run("reads_x_minus_1", layout, w, h)
    assert clean
    if layout == "packed" and h == 1:
        return                      # only the front guard lies left of a packed 1 x 1 picture: the read is foreign there too
    assert not equal


def test_packed_1x1_read_of_the_guard_is_reported():
    equal, clean, _, _ = run("reads_x_minus_1", "packed", 1, 1)
    assert clean and not equal


@pytest.mark.parametrize("px,frames", [(1, 1), (2, 1), (3, 1), (4, 1), (1, 5), (3, 5)])
@pytest.mark.parametrize("side", sorted(roi.SIDES))
def test_layout_table_numbers(side, px, frames):
    """The table's promises as numbers: guards, pitch, base alignment, foreign pixels around the ROI, frame distance."""
    w, rows = 131, 19
    s = roi.Surface(side, w, rows, px, frames, seed=1)
    rb = w * px
    spec = roi.SIDES[side]
    first, last = s.offset, s.offset + (frames - 1) * s.frame_bytes + (rows - 1) * s.pitch + rb
    assert first - s.oy * s.pitch - s.left >= roi.GUARD                       # front guard in front of the parent
    assert s.nbytes - last >= roi.GUARD                                        # back guard behind the last ROI byte
    assert s.roi_mask.sum() == frames * rows * rb
    if side == "packed":
        assert s.pitch == rb and first % 256 == 0 and s.frame_bytes == rows * rb
    if side == "padded16":
        assert s.pitch % 64 == 0 and s.pitch >= rb + 64 and s.left == 0 and first % 16 == 0
    if side.startswith("roi_off"):
        assert s.pitch % 64 == 0 and first % 4 == int(side[-1]) and s.left >= 3 * px and s.oy >= 3
        assert s.frame_bytes % 4 != 0
    if side == "odd_pitch":
        assert s.pitch == rb + 5 and first % 2 == 1 and s.oy >= 3 and s.left >= px and s.left + rb < s.pitch
        assert s.frame_bytes % 4 != 0
    if side == "tight_end":
        assert s.left + rb == s.pitch and spec.below == 0
        assert s.nbytes - last == roi.GUARD                                    # only the guard lies behind the ROI
    if frames > 1:
        assert s.frame_bytes >= (s.oy + rows + spec.below) * s.pitch


def test_table_has_the_named_layouts():
    assert set(roi.LAYOUTS) == {"packed", "padded16", "roi_off1", "roi_off2", "roi_off3", "odd_pitch", "mixed", "mixed_rev", "tight_end"}
    assert roi.LAYOUTS["mixed"] == ("padded16", "odd_pitch") and roi.LAYOUTS["mixed_rev"] == ("odd_pitch", "padded16")


def test_blob_guards():
    b = roi.blob(40, seed=3).bind(None)
    b.mem.data[b.ptr + 40] ^= 1
    _, clean = b.result()
    assert not clean and "guard" in b.stray()
    b = roi.blob(40, seed=3).bind(None)
    b.mem.data[b.ptr + 39] ^= 1
    _, clean = b.result()
    assert clean and not b.untouched()
