"""Deterministic synthetic clips (SURVEY.md 8d "Synthetic clip generator").

Integer-only arithmetic (numpy int64 + a Python-int xorshift64*), so the same
seed gives the same bytes on every machine: a world texture (square-wave
gratings + filled rectangles + hash noise) sampled through a per-frame
translation / small rotation with 8-bit fixed-point bilinear weights.
"""
import numpy as np

_MASK = (1 << 64) - 1

SEED_CONFIG1 = 0x5EED0001   # 640x480x300, smoothingRadius 25 (BASELINE.json configs[0])
SEED_CONFIG2 = 0x5EED0002   # 1920x1080 BGR8 (configs[1])
SEED_CONFIG3 = 0x5EED0003   # 3840x2160 NV12 (configs[2])


class XorShift64Star:
    def __init__(self, seed):
        self.s = (seed & _MASK) or 0x9E3779B97F4A7C15

    def next(self):
        x = self.s
        x ^= x >> 12
        x ^= (x << 25) & _MASK
        x ^= x >> 27
        self.s = x
        return (x * 0x2545F4914F6CDD1D) & _MASK

    def randint(self, lo, hi):
        return lo + (self.next() >> 11) % (hi - lo + 1)


def make_world(seed, width, height):
    """World texture (height+512, width+512, 3) uint8, BGR."""
    rng = XorShift64Star(seed)
    wt, ht = width + 512, height + 512
    yy, xx = np.mgrid[0:ht, 0:wt].astype(np.int64)
    img = np.full((ht, wt, 3), 96, dtype=np.int64)
    for _ in range(24):
        ux, uy = rng.randint(-8, 8), rng.randint(-8, 8)
        if ux == 0 and uy == 0:
            ux = 1
        period = rng.randint(96, 768)
        amp = [rng.randint(-22, 22) for _ in range(3)]
        wave = ((ux * xx + uy * yy) // period) & 1
        for c in range(3):
            img[:, :, c] += amp[c] * wave
    noise = (((xx * 73856093) ^ (yy * 19349663)) >> 7) & 7
    img += (noise - 3)[:, :, None]
    for _ in range(400):
        x0, y0 = rng.randint(0, wt - 9), rng.randint(0, ht - 9)
        rw, rh = rng.randint(8, 72), rng.randint(8, 72)
        col = [rng.randint(0, 255) for _ in range(3)]
        img[y0:y0 + rh, x0:x0 + rw, :] = col
    return np.clip(img, 0, 255).astype(np.uint8)


def motion_script(seed, n_frames, pan_q8=512, jitter_q8=384, rot_1e5=200, segments=None):
    """Per-frame (ox_q8, oy_q8, sin_q16) camera pose.

    pan_q8: pan in 1/256 px per frame (default 2 px/frame); jitter_q8: jitter
    std in 1/256 px (default 1.5 px); rot_1e5: rotation std in 1e-5 rad
    (default 0.002 rad).  `segments` = list of (first_frame, pan_x_q8,
    pan_y_q8, jitter_q8, rot_1e5) overrides, for clips that exercise all four
    motion-intent gains (SURVEY.md 8 "Clip design note").
    """
    rng = XorShift64Star(seed ^ 0xA5A5A5A5)
    poses = []
    px, py = 256 * 256, 256 * 256
    seg = (0, pan_q8, 0, jitter_q8, rot_1e5)
    segs = sorted(segments or [])
    for k in range(n_frames):
        while segs and segs[0][0] <= k:
            seg = segs.pop(0)
        _, panx, pany, jit, rot = seg
        if k > 0:
            px += panx
            py += pany

        def gauss(std):
            # Irwin-Hall(4) scaled: integer-only approximately normal sample
            s = sum(rng.randint(-1000, 1000) for _ in range(4))
            return (s * std) // 1155   # std of the sum is 1155
        jx, jy, ja = gauss(jit), gauss(jit), gauss(rot)
        sin_q16 = (ja * 65536) // 100000
        poses.append((px + jx, py + jy, sin_q16))
    return poses


def render_frame(world, width, height, pose):
    """Sample the world at `pose` -> (height, width, 3) uint8 BGR."""
    ox, oy, s16 = pose
    c16 = 65536 - ((s16 * s16) >> 17)
    ht, wt = world.shape[:2]
    cx, cy = width // 2, height // 2
    y, x = np.mgrid[0:height, 0:width].astype(np.int64)
    rx, ry = x - cx, y - cy
    sx = ox + cx * 256 + ((c16 * rx - s16 * ry) >> 8)
    sy = oy + cy * 256 + ((s16 * rx + c16 * ry) >> 8)
    ix, iy = sx >> 8, sy >> 8
    fx, fy = (sx & 255)[:, :, None], (sy & 255)[:, :, None]
    x0, x1 = ix % wt, (ix + 1) % wt
    y0, y1 = iy % ht, (iy + 1) % ht
    w = world.astype(np.int64)
    acc = ((256 - fx) * (256 - fy)) * w[y0, x0]
    acc += (fx * (256 - fy)) * w[y0, x1]
    acc += ((256 - fx) * fy) * w[y1, x0]
    acc += (fx * fy) * w[y1, x1]
    return ((acc + 32768) >> 16).astype(np.uint8)


def make_clip(seed, width, height, n_frames, **kw):
    world = make_world(seed, width, height)
    poses = motion_script(seed, n_frames, **kw)
    return [render_frame(world, width, height, p) for p in poses]


def bgr_to_nv12(frame):
    """BT.601 limited-range integer BGR -> NV12 (h*3/2, w) uint8; w,h even."""
    b = frame[:, :, 0].astype(np.int64)
    g = frame[:, :, 1].astype(np.int64)
    r = frame[:, :, 2].astype(np.int64)
    yp = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    h, w = yp.shape

    def sub(p):
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    uv = np.empty((h // 2, w), dtype=np.int64)
    uv[:, 0::2] = sub(u)
    uv[:, 1::2] = sub(v)
    return np.clip(np.vstack([yp, uv]), 0, 255).astype(np.uint8)


def nv12_to_p010(nv12, seed=0):
    """The P010 surface (uint16, same shape) whose samples' high bytes are the NV12 surface's bytes and whose ten-bit values carry
    two live low bits: (nv12 << 8) | (r << 6) with r a seeded random 0..3.  Works on one surface or a stack of them."""
    nv12 = np.asarray(nv12, np.uint8)
    r = np.random.default_rng(seed).integers(0, 4, nv12.shape, np.uint16)
    return (nv12.astype(np.uint16) << 8) | (r << 6)


def i420_layout(w, h, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """(pitch, c_pitch, u_off, v_off) of an I420 surface with the library's defaults filled in (vs_stab_set_i420_layout): chroma pitch
    = pitch / 2, U behind the h luma rows, V behind U.  YV12: give the two offsets swapped."""
    pitch = pitch or w
    c_pitch = c_pitch or pitch // 2
    u_off = u_off or h * pitch
    v_off = v_off or u_off + (h // 2) * c_pitch
    return pitch, c_pitch, u_off, v_off


def nv12_to_i420(nv12, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None, fill=0):
    """The I420 surface that holds the samples of one NV12 surface (h * 3 / 2, w).  Packed (no layout given): a (h * 3 / 2, w)
    array - h rows of Y, then the U plane, then the V plane, h / 2 rows of w / 2 bytes each.  With a layout: a flat buffer of
    `size` bytes (default: up to the end of the last plane), `fill` wherever no sample lies."""
    nv12 = np.asarray(nv12, np.uint8)
    w, h = nv12.shape[1], nv12.shape[0] * 2 // 3
    packed = not (pitch or c_pitch or u_off or v_off or size)
    pitch, c_pitch, u_off, v_off = i420_layout(w, h, pitch, c_pitch, u_off, v_off)
    end = max(h * pitch, u_off + (h // 2) * c_pitch, v_off + (h // 2) * c_pitch)
    buf = np.full(size or end, fill, np.uint8)
    buf[:h * pitch].reshape(h, pitch)[:, :w] = nv12[:h]
    buf[u_off:u_off + (h // 2) * c_pitch].reshape(h // 2, c_pitch)[:, :w // 2] = nv12[h:, 0::2]
    buf[v_off:v_off + (h // 2) * c_pitch].reshape(h // 2, c_pitch)[:, :w // 2] = nv12[h:, 1::2]
    return buf.reshape(h * 3 // 2, w) if packed else buf


def i420_to_nv12(buf, w, h, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """The NV12 surface (h * 3 / 2, w) of an I420 surface's samples; buf: what nv12_to_i420 returns for the same layout."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    pitch, c_pitch, u_off, v_off = i420_layout(w, h, pitch, c_pitch, u_off, v_off)
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = buf[:h * pitch].reshape(h, pitch)[:, :w]
    out[h:, 0::2] = buf[u_off:u_off + (h // 2) * c_pitch].reshape(h // 2, c_pitch)[:, :w // 2]
    out[h:, 1::2] = buf[v_off:v_off + (h // 2) * c_pitch].reshape(h // 2, c_pitch)[:, :w // 2]
    return out


def p010_to_i010(surface, w, h, bits=10, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None, fill=0):
    """The I010 (bits = 10) / I012 (12) surface that holds the samples of one P010 / P012 surface (h * 3 / 2, w) uint16: every sample
    shifted down to the low bits (sample >> (16 - bits)), U and V de-interleaved.  Packed (no layout given): a (h * 3 / 2, w) uint16
    array - Y, then the U plane, then the V plane.  With a layout - pitch, c_pitch, u_off, v_off and size in BYTES, even, defaults as
    i420_layout's at pitch = 2 w -: a flat uint16 buffer of size / 2 words, `fill` wherever no sample lies."""
    s = np.asarray(surface, np.uint16) >> (16 - bits)
    packed = not (pitch or c_pitch or u_off or v_off or size)
    pitch, c_pitch, u_off, v_off = i420_layout(2 * w, h, pitch, c_pitch, u_off, v_off)
    end = max(h * pitch, u_off + (h // 2) * c_pitch, v_off + (h // 2) * c_pitch)
    assert not ((pitch | c_pitch | u_off | v_off | (size or 0)) & 1), "16-bit samples: the layout is in even bytes"
    buf = np.full((size or end) // 2, fill, np.uint16)
    buf[:h * pitch // 2].reshape(h, pitch // 2)[:, :w] = s[:h]
    buf[u_off // 2:(u_off + (h // 2) * c_pitch) // 2].reshape(h // 2, c_pitch // 2)[:, :w // 2] = s[h:, 0::2]
    buf[v_off // 2:(v_off + (h // 2) * c_pitch) // 2].reshape(h // 2, c_pitch // 2)[:, :w // 2] = s[h:, 1::2]
    return buf.reshape(h * 3 // 2, w) if packed else buf


def i010_to_p010(buf, w, h, bits=10, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """The P010 / P012 surface (h * 3 / 2, w) of an I010 / I012 surface's samples (sample << (16 - bits)); buf: what p010_to_i010
    returns for the same layout."""
    buf = np.asarray(buf, np.uint16).reshape(-1)
    pitch, c_pitch, u_off, v_off = i420_layout(2 * w, h, pitch, c_pitch, u_off, v_off)
    out = np.empty((h * 3 // 2, w), np.uint16)
    out[:h] = buf[:h * pitch // 2].reshape(h, pitch // 2)[:, :w]
    out[h:, 0::2] = buf[u_off // 2:(u_off + (h // 2) * c_pitch) // 2].reshape(h // 2, c_pitch // 2)[:, :w // 2]
    out[h:, 1::2] = buf[v_off // 2:(v_off + (h // 2) * c_pitch) // 2].reshape(h // 2, c_pitch // 2)[:, :w // 2]
    return out << (16 - bits)


def planar_planes(buf, w, h, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """(Y (h, w), U (h / 2, w / 2), V (h / 2, w / 2)) of a planar 4:2:0 surface, uint8 (I420) or uint16 (I010 / I012), as copies.  buf:
    what nv12_to_i420 / p010_to_i010 return; the layout in BYTES, defaults as i420_layout's at pitch = w samples."""
    buf = np.asarray(buf)
    sb = buf.dtype.itemsize
    flat = buf.reshape(-1)
    pitch, c_pitch, u_off, v_off = i420_layout(sb * w, h, pitch, c_pitch, u_off, v_off)

    def plane(off, p, pw, ph):
        return flat[off // sb:(off + ph * p) // sb].reshape(ph, p // sb)[:, :pw].copy()
    return plane(0, pitch, w, h), plane(u_off, c_pitch, w // 2, h // 2), plane(v_off, c_pitch, w // 2, h // 2)


def planar_from_planes(y, u, v, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None, fill=0):
    """The inverse: a flat buffer (the packed (h * 3 / 2, w) array when no layout is given) that holds the three planes, `fill` elsewhere."""
    y = np.asarray(y)
    h, w = y.shape
    sb = y.dtype.itemsize
    packed = not (pitch or c_pitch or u_off or v_off or size)
    pitch, c_pitch, u_off, v_off = i420_layout(sb * w, h, pitch, c_pitch, u_off, v_off)
    end = max(h * pitch, u_off + (h // 2) * c_pitch, v_off + (h // 2) * c_pitch)
    buf = np.full((size or end) // sb, fill, y.dtype)
    buf[:h * pitch // sb].reshape(h, pitch // sb)[:, :w] = y
    buf[u_off // sb:(u_off + (h // 2) * c_pitch) // sb].reshape(h // 2, c_pitch // sb)[:, :w // 2] = u
    buf[v_off // sb:(v_off + (h // 2) * c_pitch) // sb].reshape(h // 2, c_pitch // sb)[:, :w // 2] = v
    return buf.reshape(h * 3 // 2, w) if packed else buf


# ---- planar 4:2:2 / 4:4:4 (I422, I444 and their 10- / 12-bit forms): chroma planes of (w >> sx) x (h >> sy) samples -----------------
def yuv_layout(w, h, sx, sy, sb=1, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """(pitch, c_pitch, u_off, v_off) in BYTES of a three-plane surface of w x h luma samples of sb bytes whose chroma planes have
    (w >> sx) x (h >> sy) samples, the library's defaults filled in: chroma pitch = pitch >> sx, U behind the h luma rows, V behind U.
    (sx, sy) = (1, 1): i420_layout; (1, 0): 4:2:2; (0, 0): 4:4:4."""
    pitch = pitch or sb * w
    c_pitch = c_pitch or pitch >> sx
    u_off = u_off or h * pitch
    v_off = v_off or u_off + (h >> sy) * c_pitch
    return pitch, c_pitch, u_off, v_off


def yuv_frame_rows(h, sx, sy):
    """Rows of w samples of a packed frame: h of luma and two chroma planes of (h >> sy) rows of w >> sx samples."""
    return h + ((2 * (h >> sy)) >> sx)


def bgr_to_yuv_planes(frame, sx, sy):
    """BT.601 limited-range integer BGR -> (Y (h, w), U, V ((h >> sy), (w >> sx))) uint8: bgr_to_nv12's luma and its chroma before the
    subsampling, averaged (rounded) over blocks of 2^sx x 2^sy samples.  w a multiple of 2^sx, h of 2^sy."""
    b = frame[:, :, 0].astype(np.int64)
    g = frame[:, :, 1].astype(np.int64)
    r = frame[:, :, 2].astype(np.int64)
    yp = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128

    def sub(p):
        h, w = p.shape
        bx, by = 1 << sx, 1 << sy
        t = p.reshape(h // by, by, w // bx, bx).sum(axis=(1, 3))
        return (t + ((bx * by) >> 1)) >> (sx + sy)
    return tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (yp, sub(u), sub(v)))


def yuv_to_depth(planes, bits, seed=0):
    """The 10- / 12-bit form of 8-bit planes: uint16 samples (byte << (bits - 8)) | r with r seeded random low bits, the value in the
    low bits of the word - so min(sample >> (bits - 8), 255) is the byte again and every low bit is live."""
    rng = np.random.default_rng(seed)
    return tuple((np.asarray(p, np.uint16) << (bits - 8)) | rng.integers(0, 1 << (bits - 8), np.shape(p), np.uint16) for p in planes)


def yuv_pack(y, u, v, sx, sy, pitch=None, c_pitch=None, u_off=None, v_off=None, size=None, fill=0):
    """A surface that holds the three planes (uint8 or uint16).  Packed (no layout given): the (yuv_frame_rows, w) array - Y, then the
    U plane, then the V plane.  With a layout (bytes; see yuv_layout): a flat buffer of `size` bytes, `fill` wherever no sample lies."""
    y = np.asarray(y)
    h, w = y.shape
    sb = y.dtype.itemsize
    cw, ch = w >> sx, h >> sy
    packed = not (pitch or c_pitch or u_off or v_off or size)
    pitch, c_pitch, u_off, v_off = yuv_layout(w, h, sx, sy, sb, pitch, c_pitch, u_off, v_off)
    end = max(h * pitch, u_off + ch * c_pitch, v_off + ch * c_pitch)
    assert sb == 1 or not ((pitch | c_pitch | u_off | v_off | (size or 0)) & 1), "16-bit samples: the layout is in even bytes"
    buf = np.full((size or end) // sb, fill, y.dtype)
    buf[:h * pitch // sb].reshape(h, pitch // sb)[:, :w] = y
    buf[u_off // sb:(u_off + ch * c_pitch) // sb].reshape(ch, c_pitch // sb)[:, :cw] = u
    buf[v_off // sb:(v_off + ch * c_pitch) // sb].reshape(ch, c_pitch // sb)[:, :cw] = v
    return buf.reshape(yuv_frame_rows(h, sx, sy), w) if packed else buf


def yuv_unpack(buf, w, h, sx, sy, pitch=None, c_pitch=None, u_off=None, v_off=None):
    """(Y, U, V) of a surface yuv_pack made, as copies; the layout as given there."""
    buf = np.asarray(buf)
    sb = buf.dtype.itemsize
    flat = buf.reshape(-1)
    pitch, c_pitch, u_off, v_off = yuv_layout(w, h, sx, sy, sb, pitch, c_pitch, u_off, v_off)

    def plane(off, p, pw, ph):
        return flat[off // sb:(off + ph * p) // sb].reshape(ph, p // sb)[:, :pw].copy()
    return plane(0, pitch, w, h), plane(u_off, c_pitch, w >> sx, h >> sy), plane(v_off, c_pitch, w >> sx, h >> sy)


def bgr_to_planar(frame, sx, sy, bits=8, seed=0):
    """One frame of the clip generator as a packed planar frame: I422 (sx, sy = 1, 0) / I444 (0, 0) at bits = 8, I210 / I410 at 10,
    I212 / I412 at 12.  The luma bytes - for the deeper forms min(sample >> (bits - 8), 255) - are those of bgr_to_nv12(frame)."""
    planes = bgr_to_yuv_planes(frame, sx, sy)
    if bits != 8:
        planes = yuv_to_depth(planes, bits, seed)
    return yuv_pack(*planes, sx, sy)


# ---- long clips rendered on the device (bench.py: more distinct input than the 256 MB Infinity Cache holds) -----------
def loop_script(seed, n_frames, pan_q8=512, jitter_q8=384, rot_1e5=200):
    """Per-frame camera pose of a CLOSED pan path: n/4 frames right, down, left, up at pan_q8 per frame (the same jitter
    and rotation model as motion_script), so that the clip can be played in a cycle without a cut - frame 0 follows frame
    n-1 by one camera step - and no frame is read again before all the others have been."""
    assert n_frames % 4 == 0 and n_frames >= 8
    rng = XorShift64Star(seed ^ 0xA5A5A5A5)
    q = n_frames // 4
    px, py = 256 * 256, 256 * 256
    poses = []
    for k in range(n_frames):
        if k > 0:
            side = (k - 1) // q
            px += (pan_q8, 0, -pan_q8, 0)[side]
            py += (0, pan_q8, 0, -pan_q8)[side]

        def gauss(std):
            s = sum(rng.randint(-1000, 1000) for _ in range(4))
            return (s * std) // 1155
        jx, jy, ja = gauss(jitter_q8), gauss(jitter_q8), gauss(rot_1e5)
        poses.append((px + jx, py + jy, (ja * 65536) // 100000))
    return poses


def _pose_forward_matrix(pose, width, height, scale=1.0):
    """Forward 2x3 matrix (cv::warpAffine's M) whose inverse samples the world at `pose`: frame(x, y) =
    world(R (x - cx, y - cy) + (cx + ox, cy + oy)).  scale 0.5: the same pose in the coordinates of a half-size plane."""
    ox, oy, s16 = pose
    s = s16 / 65536.0
    c = (1.0 - s * s) ** 0.5
    cx, cy = width * 0.5 * scale, height * 0.5 * scale
    tx, ty = cx + ox / 256.0 * scale, cy + oy / 256.0 * scale
    inv = np.array([[c, -s, tx - c * cx + s * cy], [s, c, ty - s * cx - c * cy], [0, 0, 1]], np.float64)
    return np.ascontiguousarray(np.linalg.inv(inv)[:2].reshape(6))


def make_clip_dev(vs, seed, width, height, n_frames, nv12=False, **kw):
    """A closed-loop clip of n_frames frames rendered ON THE DEVICE from the world texture (one upload) with the library's
    own warp operator (vs_op_warp_affine_ex); returns one DevBuf holding the packed frames (BGR8, or NV12: Y plane then
    the interleaved UV plane).  Synthetic input only - nothing is compared against these frames' provenance."""
    import ctypes as C
    from . import capi
    world = make_world(seed, width, height)
    hw, ww = world.shape[:2]
    poses = loop_script(seed, n_frames, **kw)
    f64p = C.POINTER(C.c_double)
    if not nv12:
        fb = width * height * 3
        d_world = capi.DevBuf.from_array(vs, world)
        clip = capi.DevBuf(vs, fb * n_frames)
        for i, p in enumerate(poses):
            M = _pose_forward_matrix(p, width, height)
            vs.check(vs.lib.vs_op_warp_affine_ex(d_world.ptr, ww * 3, ww, hw, clip.ptr + i * fb, width * 3, width, height, 3,
                                                 M.ctypes.data_as(f64p), capi.BORDER_BLACK, None))
        vs.sync()
        d_world.free()
        return clip
    wnv = bgr_to_nv12(world)
    d_y = capi.DevBuf.from_array(vs, wnv[:hw])
    d_uv = capi.DevBuf.from_array(vs, wnv[hw:])
    fb = width * height * 3 // 2
    clip = capi.DevBuf(vs, fb * n_frames)
    for i, p in enumerate(poses):
        M = _pose_forward_matrix(p, width, height)
        Mh = _pose_forward_matrix(p, width, height, 0.5)
        vs.check(vs.lib.vs_op_warp_affine_ex(d_y.ptr, ww, ww, hw, clip.ptr + i * fb, width, width, height, 1,
                                             M.ctypes.data_as(f64p), capi.BORDER_BLACK, None))
        vs.check(vs.lib.vs_op_warp_affine_ex(d_uv.ptr, ww, ww // 2, hw // 2, clip.ptr + i * fb + width * height, width,
                                             width // 2, height // 2, 2, Mh.ctypes.data_as(f64p), capi.BORDER_BLACK, None))
    vs.sync()
    d_y.free()
    d_uv.free()
    return clip
