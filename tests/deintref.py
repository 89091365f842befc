"""The deinterlacer and the weave of include/vs_stab.h, stated twice: a per-pixel loop written straight from the definition
(deint_loop, which also counts the branches it takes) and a vectorised numpy form (deint) that the GPU tests use.

The reference project has no deinterlacer: this is a DEFINITION of this library, modelled on the widely used yadif filter and
pinned to no other implementation.

A plane has h rows of w pixels of cn channels, 8- or 16-bit samples, here an array (h, w * cn).  Every channel is treated on its
own: x +- j means the same channel of the pixel j pixels away.  Plane row y belongs to field y & 1.  Inputs are three frames P
(previous), C (current) and N (next) and two job fields: rows with (y & 1) == keep are copied from C; second = 0 means this output
is the first field in time of frame C and the temporal pair is (A, B) = (P, C), second = 1 the second field and (A, B) = (C, N).
P or N None stands for C.  For a missing row y: up = y - 1 if y > 0 else y + 1, dn = y + 1 if y + 1 < h else y - 1 (h >= 2).

LINEAR uses C only and ignores `second`: out = (C[up][x] + C[dn][x] + 1) >> 1.

YADIF, in plain integers:

    c = C[up][x];  e = C[dn][x];  d = (A[y][x] + B[y][x]) >> 1
    td0 = |A[y][x] - B[y][x]|
    td1 = (|P[up][x] - c| + |P[dn][x] - e|) >> 1
    td2 = (|N[up][x] - c| + |N[dn][x] - e|) >> 1
    diff = max(td0 >> 1, td1, td2)
    sp = (c + e) >> 1
    if 3 <= x < w - 3:                      # edge-directed search
        best = |C[up][x-1] - C[dn][x-1]| + |c - e| + |C[up][x+1] - C[dn][x+1]| - 1
        score(j) = |C[up][x-1+j] - C[dn][x-1-j]| + |C[up][x+j] - C[dn][x-j]| + |C[up][x+1+j] - C[dn][x+1-j]|
        for g in (-1, +1), in this order:
            if score(g) < best:  best = score(g); sp = (C[up][x+g] + C[dn][x-g]) >> 1
                if score(2g) < best:  best = score(2g); sp = (C[up][x+2g] + C[dn][x-2g]) >> 1     # only after g itself won
    if not (y == 1 or y + 2 == h):          # spatial interlacing check: upp / dnn lie inside the plane exactly then
        upp = y + 2 (up - y);  dnn = y + 2 (dn - y)
        b = (A[upp][x] + B[upp][x]) >> 1;  f = (A[dnn][x] + B[dnn][x]) >> 1
        mx = max(d - e, d - c, min(b - c, f - e));  mn = min(d - e, d - c, max(b - c, f - e))
        diff = max(diff, mn, -mx)
    out = d + diff if sp > d + diff else d - diff if sp < d - diff else sp

The result lies between sp and d.  Weave: destination row y is F's where (y & 1) == (0 if tff else 1), else S's."""
import numpy as np

LINEAR, YADIF = 0, 1

# what deint_loop counts: the five search picks, the three clamp outcomes, the widened diff
BRANCHES = ("pick_0", "pick_m1", "pick_m2", "pick_p1", "pick_p2", "clamp_hi", "clamp_lo", "clamp_none", "diff_widened")


def _rows(y, h):
    return (y - 1 if y > 0 else y + 1), (y + 1 if y + 1 < h else y - 1)


def deint_loop(P, C, N, cn, keep, second, mode, counts=None, trace=None):
    """The definition, pixel by pixel.  counts: a dict that receives how often each of BRANCHES was taken (YADIF); trace: a list
    that receives (y, i, sp, d, out) of every missing sample (YADIF)."""
    P = C if P is None else P
    N = C if N is None else N
    h, wc = C.shape
    w = wc // cn
    assert h >= 2 and wc == w * cn
    Pi, Ci, Ni = (np.asarray(a).astype(np.int64).tolist() for a in (P, C, N))
    A, B = (Ci, Ni) if second else (Pi, Ci)
    out = np.array(C, copy=True)
    if counts is not None:
        for k in BRANCHES:
            counts.setdefault(k, 0)
    for y in range(h):
        if (y & 1) == keep:
            continue
        up, dn = _rows(y, h)
        U, D = Ci[up], Ci[dn]
        for i in range(wc):
            x = i // cn
            c, e = U[i], D[i]
            if mode == LINEAR:
                out[y, i] = (c + e + 1) >> 1
                continue
            d = (A[y][i] + B[y][i]) >> 1
            td0 = abs(A[y][i] - B[y][i])
            td1 = (abs(Pi[up][i] - c) + abs(Pi[dn][i] - e)) >> 1
            td2 = (abs(Ni[up][i] - c) + abs(Ni[dn][i] - e)) >> 1
            diff = max(td0 >> 1, td1, td2)
            sp = (c + e) >> 1
            pick = "pick_0"
            if 3 <= x < w - 3:
                def score(j):
                    return sum(abs(U[i + (k + j) * cn] - D[i + (k - j) * cn]) for k in (-1, 0, 1))
                best = score(0) - 1
                for g in (-1, 1):
                    if score(g) < best:
                        best = score(g)
                        sp = (U[i + g * cn] + D[i - g * cn]) >> 1
                        pick = "pick_m1" if g < 0 else "pick_p1"
                        if score(2 * g) < best:
                            best = score(2 * g)
                            sp = (U[i + 2 * g * cn] + D[i - 2 * g * cn]) >> 1
                            pick = "pick_m2" if g < 0 else "pick_p2"
            if not (y == 1 or y + 2 == h):
                upp, dnn = y + 2 * (up - y), y + 2 * (dn - y)
                b = (A[upp][i] + B[upp][i]) >> 1
                f = (A[dnn][i] + B[dnn][i]) >> 1
                mx = max(d - e, d - c, min(b - c, f - e))
                mn = min(d - e, d - c, max(b - c, f - e))
                wide = max(diff, mn, -mx)
                if counts is not None and wide > diff:
                    counts["diff_widened"] += 1
                diff = wide
            if sp > d + diff:
                o, cl = d + diff, "clamp_hi"
            elif sp < d - diff:
                o, cl = d - diff, "clamp_lo"
            else:
                o, cl = sp, "clamp_none"
            if counts is not None:
                counts[pick] += 1
                counts[cl] += 1
            if trace is not None:
                trace.append((y, i, sp, d, o))
            out[y, i] = o
    return out


def _shift(a, j, cn):
    """a[:, i + j * cn] where that lies inside the row (elsewhere any value of the row: the caller masks)."""
    return np.roll(a, -j * cn, axis=1)


def deint(P, C, N, cn, keep, second, mode, counts=None):
    """The same, vectorised over the missing rows; counts as in deint_loop."""
    P = C if P is None else P
    N = C if N is None else N
    h, wc = C.shape
    w = wc // cn
    assert h >= 2 and wc == w * cn
    out = np.array(C, copy=True)
    ys = np.arange(1 - keep, h, 2)
    if ys.size == 0:
        return out
    up = np.where(ys > 0, ys - 1, ys + 1)
    dn = np.where(ys + 1 < h, ys + 1, ys - 1)
    Pi, Ci, Ni = (np.asarray(a).astype(np.int64) for a in (P, C, N))
    U, D = Ci[up], Ci[dn]
    if mode == LINEAR:
        out[ys] = ((U + D + 1) >> 1).astype(C.dtype)
        return out
    A, B = (Ci, Ni) if second else (Pi, Ci)
    d = (A[ys] + B[ys]) >> 1
    td0 = np.abs(A[ys] - B[ys])
    td1 = (np.abs(Pi[up] - U) + np.abs(Pi[dn] - D)) >> 1
    td2 = (np.abs(Ni[up] - U) + np.abs(Ni[dn] - D)) >> 1
    diff = np.maximum(np.maximum(td0 >> 1, td1), td2)
    sp = (U + D) >> 1
    pick = np.zeros(sp.shape, np.int64)                # an index into BRANCHES[:5]
    if w >= 7:
        x = np.arange(wc) // cn
        inner = ((x >= 3) & (x < w - 3))[None, :]

        def score(j):
            return sum(np.abs(_shift(U, k + j, cn) - _shift(D, k - j, cn)) for k in (-1, 0, 1))

        def pred(j):
            return (_shift(U, j, cn) + _shift(D, -j, cn)) >> 1
        best = score(0) - 1
        for g in (-1, 1):
            s1, s2 = score(g), score(2 * g)
            m1 = inner & (s1 < best)
            best = np.where(m1, s1, best)
            sp = np.where(m1, pred(g), sp)
            m2 = m1 & (s2 < best)
            best = np.where(m2, s2, best)
            sp = np.where(m2, pred(2 * g), sp)
            pick = np.where(m2, 2 if g < 0 else 4, np.where(m1, 1 if g < 0 else 3, pick))
    chk = ~((ys == 1) | (ys + 2 == h))
    upp = np.clip(ys + 2 * (up - ys), 0, h - 1)
    dnn = np.clip(ys + 2 * (dn - ys), 0, h - 1)
    b = (A[upp] + B[upp]) >> 1
    f = (A[dnn] + B[dnn]) >> 1
    mx = np.maximum(np.maximum(d - D, d - U), np.minimum(b - U, f - D))
    mn = np.minimum(np.minimum(d - D, d - U), np.maximum(b - U, f - D))
    wide = np.where(chk[:, None], np.maximum(np.maximum(diff, mn), -mx), diff)
    if counts is not None:
        for k in BRANCHES:
            counts.setdefault(k, 0)
        for k in range(5):
            counts[BRANCHES[k]] += int(np.count_nonzero(pick == k))
        counts["clamp_hi"] += int(np.count_nonzero(sp > d + wide))
        counts["clamp_lo"] += int(np.count_nonzero((sp <= d + wide) & (sp < d - wide)))
        counts["clamp_none"] += int(np.count_nonzero((sp <= d + wide) & (sp >= d - wide)))
        counts["diff_widened"] += int(np.count_nonzero(wide > diff))
    diff = wide
    o = np.where(sp > d + diff, d + diff, np.where(sp < d - diff, d - diff, sp))
    out[ys] = o.astype(C.dtype)
    return out


def weave(F, S, tff):
    """Rows of field (0 if tff else 1) from F, the others from S."""
    out = np.array(S, copy=True)
    k = 0 if tff else 1
    out[k::2] = F[k::2]
    return out


# the known answer of the definition: 5 x 9, cn 1, 8-bit
KA_P = np.array([[34, 32, 204, 127, 151, 153, 182, 7, 124], [37, 102, 237, 140, 18, 138, 33, 193, 242], [250, 159, 222, 94, 37, 130, 113, 169, 254],
                 [70, 219, 35, 89, 201, 63, 171, 117, 131], [240, 209, 214, 140, 251, 251, 34, 52, 78]], np.uint8)
KA_C = np.array([[141, 210, 123, 251, 90, 237, 151, 184, 60], [151, 205, 226, 222, 247, 32, 199, 119, 175], [70, 3, 21, 249, 229, 77, 110, 61, 37],
                 [219, 172, 19, 51, 144, 230, 254, 55, 156], [8, 44, 51, 113, 88, 186, 120, 86, 231]], np.uint8)
KA_N = np.array([[160, 178, 190, 86, 228, 4, 78, 40, 1], [255, 22, 117, 209, 176, 219, 13, 127, 8], [49, 216, 18, 150, 5, 79, 238, 81, 79],
                 [22, 198, 44, 127, 6, 5, 214, 2, 119], [109, 32, 165, 189, 252, 50, 236, 15, 36]], np.uint8)
KA_YADIF_K0_S0 = {1: [105, 106, 90, 250, 243, 190, 130, 122, 68], 3: [39, 35, 36, 54, 80, 174, 115, 73, 134]}
KA_YADIF_K1_S1 = {0: [151, 205, 226, 222, 247, 32, 199, 119, 175], 2: [185, 188, 86, 217, 226, 250, 226, 87, 160], 4: [219, 101, 51, 51, 144, 230, 254, 55, 156]}
KA_LINEAR_K0 = {1: [106, 107, 72, 250, 160, 157, 131, 123, 49], 3: [39, 24, 36, 181, 159, 132, 115, 74, 134]}
