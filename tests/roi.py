"""Pictures as regions of interest (ROI) inside larger parent surfaces, with guards that are checked byte for byte.

The packed wrappers of vsamd/capi.py hand every operator a source with stride == w * cn at the start of a fresh allocation and a
destination of exactly w * h * cn bytes, so the alignment of a call is a function of w alone, a store past a row end lands in
the next row (or in slack nobody reads) and a tap at x = -1 reads the same picture.  Here a picture lies

    allocation = [ GUARD random bytes | lead | parent surface(s) | GUARD random bytes ]
    parent     = rows of `pitch` bytes; the ROI starts at column ox, row oy

and everything that is not ROI is random, from a seed fixed per case.  After the call the WHOLE allocation is read back:
`result()` returns the ROI and one boolean, "every byte outside the ROI equals the prefill" - guards, the parent rows above and
below, the bytes left and right of every ROI row, the gaps between the frames of a batch.

The module uses no GPU itself.  `bind(vs)` puts a surface into device memory through capi.DevBuf; `bind(None)` puts it into a
numpy array that stands for device memory, which is how tests/test_roi_cpu.py proves with faulty numpy "operators" that a stray
byte on either side, one row early or late, and a read of the parent's column -1 are all reported.
"""
import collections
import zlib

import numpy as np

GUARD = 256                      # random bytes in front of the parent and behind it (at least; `lead` adds to the front)

# One side of a call.  pitch: "packed" = the row's bytes, "pad64" = rounded up to 64 plus 64, "plus5" = row bytes + 5.
# ox: pixels left of the ROI (None: as many as fit, at most 3; "end": the ROI ends in the parent's last column).
# base: what (ox * px + lead) is modulo 4 - the alignment of the ROI's first byte, GUARD and pad64 pitches being multiples of 64;
#       "odd": an odd address.  below: parent rows under the ROI.  frame_gap: True = frames of a batch lie a distance apart that is
#       no multiple of 4.
Side = collections.namedtuple("Side", "pitch ox oy base below frame_gap")

SIDES = {
    "packed": Side("packed", 0, 0, 0, 0, False),
    "padded16": Side("pad64", 0, 3, 0, 3, False),
    "roi_off1": Side("pad64", 3, 3, 1, 3, True),
    "roi_off2": Side("pad64", 3, 3, 2, 3, True),
    "roi_off3": Side("pad64", 3, 3, 3, 3, True),
    "odd_pitch": Side("plus5", None, 3, "odd", 3, True),
    "tight_end": Side("pad64", "end", 3, None, 0, False),
}

# The named table: layout -> (source side, destination side).
LAYOUTS = collections.OrderedDict([
    ("packed", ("packed", "packed")),
    ("padded16", ("padded16", "padded16")),
    ("roi_off1", ("roi_off1", "roi_off1")),
    ("roi_off2", ("roi_off2", "roi_off2")),
    ("roi_off3", ("roi_off3", "roi_off3")),
    ("odd_pitch", ("odd_pitch", "odd_pitch")),
    ("mixed", ("padded16", "odd_pitch")),
    ("mixed_rev", ("odd_pitch", "padded16")),
    ("tight_end", ("tight_end", "tight_end")),
])
LAYOUT_NAMES = list(LAYOUTS)


def case_seed(*key):
    """A seed fixed per case: the same bytes on every run and on every machine."""
    return zlib.crc32(repr(key).encode())


class HostMem:
    """Stands for a device allocation where no device is used: address 0 is the first byte of `data`."""

    def __init__(self, data):
        self.data = data.copy()
        self.ptr = 0

    def download(self):
        return self.data.copy()

    def free(self):
        pass


class DevMem:
    """A device allocation (capi.DevBuf) that holds a copy of `data`."""

    def __init__(self, vs, data):
        from vsamd.capi import DevBuf
        self.buf = DevBuf.from_array(vs, data)
        self.ptr = self.buf.ptr
        self.n = data.size

    def download(self):
        return self.buf.download((self.n,), np.uint8)

    def free(self):
        self.buf.free()


class Surface:
    """`frames` pictures of `rows` rows of `w` pixels of `px` bytes, each an ROI of a parent of its own, in one allocation.

    side: a name of SIDES.  The numbers a call needs: `pitch`, `frame_bytes` (distance of two frames' ROIs), `ptr` (address of
    the first ROI's first byte, after bind()); `offset` is that address relative to the allocation."""

    def __init__(self, side, w, rows, px=1, frames=1, seed=0):
        s = SIDES[side]
        self.side, self.w, self.rows, self.px, self.frames = side, w, rows, px, frames
        rb = self.row_bytes = w * px
        if s.pitch == "packed":
            pitch = rb
        elif s.pitch == "pad64":
            pitch = (rb + 63) // 64 * 64 + 64
        else:
            pitch = rb + 5
        if s.ox == "end":
            left = pitch - rb                                     # bytes, not pixels: the ROI's last byte is the row's last
        elif s.ox is None:
            left = min(3, (pitch - rb - 1) // px) * px            # one byte at least stays to the right
        else:
            left = s.ox * px
        self.pitch, self.left, self.oy = pitch, left, s.oy
        parent_rows = s.oy + rows + s.below
        fb = parent_rows * pitch
        if s.frame_gap:
            fb += 1 if fb % 4 != 3 else 2
        self.frame_bytes = fb
        start = GUARD + s.oy * pitch + left                       # the ROI's first byte with lead = 0
        if s.base == "odd":
            lead = (start + 1) % 2
        elif s.base is None:
            lead = 0
        else:
            lead = (s.base - start) % 4
        self.lead = lead
        self.offset = start + lead
        # the last frame needs no gap behind it: the back guard begins right behind the last parent row
        self.nbytes = GUARD + lead + (frames - 1) * fb + parent_rows * pitch + GUARD
        if s.pitch == "packed":
            assert self.offset == GUARD and self.nbytes == 2 * GUARD + frames * rows * rb
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 256, self.nbytes, dtype=np.uint8)
        self.roi_mask = np.zeros(self.nbytes, bool)
        self._view(self.roi_mask)[...] = True
        self.mem = None

    # ---- geometry ---------------------------------------------------------------------------------------------------------
    def _view(self, flat):
        """(frames, rows, row_bytes) view of the ROIs inside a flat array of the allocation's size."""
        return np.lib.stride_tricks.as_strided(flat[self.offset:], (self.frames, self.rows, self.row_bytes),
                                               (self.frame_bytes * flat.itemsize, self.pitch * flat.itemsize, flat.itemsize))

    def put(self, pictures):
        """Write the pictures (any shape of frames * rows * row_bytes bytes) into the ROIs of the prefill."""
        p = np.ascontiguousarray(pictures)
        self._view(self.host)[...] = p.view(np.uint8).reshape(self.frames, self.rows, self.row_bytes)
        return self

    # ---- memory -----------------------------------------------------------------------------------------------------------
    def bind(self, vs=None):
        self.mem = HostMem(self.host) if vs is None else DevMem(vs, self.host)
        return self

    @property
    def ptr(self):
        return self.mem.ptr + self.offset

    def frame_ptr(self, f):
        return self.ptr + f * self.frame_bytes

    def free(self):
        if self.mem is not None:
            self.mem.free()
            self.mem = None

    # ---- after the call ---------------------------------------------------------------------------------------------------
    def result(self, shape=None, dtype=np.uint8):
        """Download the whole allocation -> (the ROIs, every byte outside them equals the prefill).  shape: of the returned
        array (default (frames, rows, row_bytes), frames dropped for one frame)."""
        after = self.mem.download()
        self.after = after
        roi = np.ascontiguousarray(self._view(after))
        if shape is None:
            shape = (self.rows, self.row_bytes) if self.frames == 1 else (self.frames, self.rows, self.row_bytes)
        clean = bool(np.array_equal(after[~self.roi_mask], self.host[~self.roi_mask]))
        return roi.view(dtype).reshape(shape), clean

    def untouched(self):
        """The whole allocation equals the prefill, ROI included (inputs, and outputs of refused calls)."""
        self.after = self.mem.download()
        return bool(np.array_equal(self.after, self.host))

    def stray(self, limit=6):
        """For a failure message: where the last download differs from the prefill outside the ROI, as
        (frame, row relative to the ROI, byte relative to the ROI's first column) or ('guard', offset)."""
        bad = np.flatnonzero((self.after != self.host) & ~self.roi_mask)
        out = []
        for b in bad[:limit]:
            rel = int(b) - self.offset
            parent_first = -self.oy * self.pitch - self.left
            last = (self.frames - 1) * self.frame_bytes + (self.rows + SIDES[self.side].below) * self.pitch - self.left
            if rel < parent_first or rel >= last:
                out.append(("guard", int(b)))
                continue
            f = max(0, min(self.frames - 1, (rel - parent_first) // self.frame_bytes))
            r = rel - f * self.frame_bytes + self.left
            out.append((int(f), int(r // self.pitch), int(r % self.pitch) - self.left))
        return "%s: %d stray bytes, first %r" % (self.side, bad.size, out)


def blob(nbytes, seed=0):
    """An output that is no picture - a derivative image, a point list, a count, a map, a model: `nbytes` bytes with the same
    front and back guards around them, the first byte 256-byte aligned as a fresh allocation's."""
    return Surface("packed", int(nbytes), 1, 1, 1, seed)


def pair(layout, seed, src_args, dst_args):
    """The source and the destination surface of a layout of the table, each with random bytes of its own."""
    s, d = LAYOUTS[layout]
    return Surface(s, *src_args, seed=seed), Surface(d, *dst_args, seed=seed + 1)
