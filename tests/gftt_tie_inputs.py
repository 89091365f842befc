"""Pictures on which local maxima of the min-eigenvalue map TIE: what the corner detector (k_gftt.hip) does with equal
values is run by no rendered clip and no noise picture.  tests/test_gfttref_oracle.py asserts, from the oracle's map alone,
that each picture holds what it is here for (conditions()); tests/test_gpu_gftt_ties.py runs the kernels on them.

Why the plateaus exist: a picture that repeats a p x p tile has derivatives of period p, and a box sum over blockSize = p
covers exactly one period wherever it is taken.  The map is then one constant wherever the box and the Sobel taps stay inside
the picture, every pixel there equals its 3 x 3 maximum, and every one of them is a candidate: (w - 4) * (h - 4) at block
size 3, against the w * h / 4 that strict maxima allow."""
import numpy as np

# (maxCorners, qualityLevel, minDistance), each for a path of select_corners
PARAMS = [(4096, 1e-4, 0.0),      # no distance test: the output is the head of the sort order itself
          (4096, 1e-4, 1.0),      # cell 1
          (4096, 0.01, 2.5),      # lrint half-to-even: cell 2, more cells than the grid holds at 160 x 120: brute force
          (4096, 1e-4, 3.5),      # cell 4: the grid
          (200, 0.02, 15.0),      # the product's setting
          (1, 0.01, 3.0)]         # one corner

SORT_CAP = 8192                   # keys one sort of select_corners holds
FIRST_CHUNK = 1400                # keys its first chunk asks for; later ones ask for SORT_CAP / 2


def old_cap(w, h):
    """what the candidate list held before it was sized by the interior"""
    return w * h // 4 + 64


def tiled(p, seed, w, h):
    t = np.random.default_rng(seed).integers(0, 256, (p, p), dtype=np.uint8)
    return np.ascontiguousarray(np.tile(t, (h // p + 1, w // p + 1))[:h, :w])


def checker(cell, w, h):
    y, x = np.mgrid[:h, :w]
    return ((((x // cell) + (y // cell)) & 1) * 255).astype(np.uint8)


def mirrored(seed, w, h):
    n = np.random.default_rng(seed).integers(0, 256, (h, w // 2), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([n, n[:, ::-1]], axis=1))


# name -> (picture, block sizes)
_MAKERS = {
    "plateau3": (lambda: tiled(3, 0, 160, 120), (3,)),
    "plateau3_two": (lambda: tiled(3, 1, 160, 120), (3,)),
    "plateau5": (lambda: tiled(5, 0, 160, 120), (5,)),
    "checker8": (lambda: checker(8, 160, 120), (3, 5)),
    "mirror": (lambda: mirrored(7, 160, 120), (3, 5)),
    "tile16": (lambda: tiled(16, 2, 322, 242), (3, 5)),
    "tile16_vga": (lambda: tiled(16, 2, 640, 480), (3, 5)),
}
NAMES = list(_MAKERS)
CASES = [(name, bs) for name in NAMES for bs in _MAKERS[name][1]]
_cache = {}


def picture(name):
    if name not in _cache:
        g = _MAKERS[name][0]()
        g.setflags(write=False)
        _cache[name] = g
    return _cache[name]


CLIP_SIZE = (960, 540)            # the stream's analysis size (Stabilizer.cpp:410): frames of this size are analysed as they are
CLIP_FRAMES = 12                  # the first frame and one batch of 8, and three frames that a flush drains


def plateau_clip():
    """BGR frames whose analysis gray is a plateau picture: windows of one canvas of period 3 that move a pixel a frame.
    Equal channels, so BGR2GRAY returns the channel; the frame's size is the analysis size, so the resize is the identity."""
    if "clip" not in _cache:
        w, h = CLIP_SIZE
        canvas = tiled(3, 0, w + CLIP_FRAMES, h + CLIP_FRAMES)
        clip = []
        for k in range(CLIP_FRAMES):
            ox, oy = k, k // 2
            f = np.ascontiguousarray(np.repeat(canvas[oy:oy + h, ox:ox + w, None], 3, axis=2))
            f.setflags(write=False)
            clip.append(f)
        _cache["clip"] = clip
    return _cache["clip"]


def groups(eig, quality):
    """The candidates of a map by value: (values descending, counts), and the number of adjacent (4-neighbour) tied pairs."""
    import gfttref
    h, w = eig.shape
    idx, val = gfttref.candidates(eig, quality)
    v, n = np.unique(val, return_counts=True)
    m = np.zeros(h * w, np.float32)
    m[idx] = val
    m = m.reshape(h, w)
    pairs = int(((m[:, 1:] == m[:, :-1]) & (m[:, 1:] != 0)).sum() + ((m[1:] == m[:-1]) & (m[1:] != 0)).sum())
    return v[::-1], n[::-1], pairs


def conditions(name, bs, eig):
    """Asserts what the picture is for, from the min-eigenvalue map `eig` of block size bs."""
    h, w = eig.shape
    v, n, pairs = groups(eig, 1e-4)
    total = int(n.sum())
    ends = np.cumsum(n)                                    # positions in the sort order at which a group of one value ends

    def inside(pos):
        """the group that holds position pos of the order, when pos is not its last"""
        k = int(np.searchsorted(ends, pos))
        return int(n[k]) if ends[k] != pos else 0

    if name == "plateau3":
        # one value from the second pixel off the frame on (the reflected border changes the ring next to the frame): more than
        # the old list held, more than one sort holds
        assert total == (w - 4) * (h - 4) > old_cap(w, h) and len(v) == 1 and n[0] > SORT_CAP, (total, n)
    elif name == "plateau3_two":
        assert total > old_cap(w, h) and len(v) == 2 and n[0] < FIRST_CHUNK and n[1] > SORT_CAP, (total, n)
    elif name == "plateau5":
        # (the reflected border reaches three pixels into the map at block size 5: a few small groups beside the plateau)
        assert total > old_cap(w, h) and n.max() > SORT_CAP, (total, n)
    elif name == "checker8":
        # every candidate has a tied 4-neighbour; no plateau: the list is shorter than the old cap
        assert len(v) == 1 and 1000 <= total < old_cap(w, h) and pairs >= total, (total, pairs)
    elif name == "mirror":
        # a value occurs at x and at w - 1 - x and nowhere else; the pairs next to the axis are adjacent
        assert total > 1000 and n.max() == 2 and pairs >= 10, (total, len(v), pairs)
    elif name == "tile16":
        # (the ragged edges add groups of 1 - 20, one candidate per tile along an edge: "every group >= 100" holds for no seed)
        assert total > 2100 and n[n >= 100].sum() >= 0.9 * total and inside(FIRST_CHUNK) >= 100, (total, n)
    elif name == "tile16_vga":
        assert total > SORT_CAP and len(v) <= 32 and n.max() <= 1200, (total, len(v), n)
        assert inside(FIRST_CHUNK) >= 100 and inside(FIRST_CHUNK + SORT_CAP // 2) >= 100, n
    else:
        raise KeyError(name)
    return total, len(v), pairs
