"""Plain Python / numpy restatement of the COCO mask codec (pycocotools' rleFrPoly, rleMerge with intersect = 0, rleToString /
rleFrString, rleDecode), written from the rule in DESIGN.md 9.10 and not from csrc/seg_codec.hip: ``fr_poly`` keeps rleFrPoly's own
ending (sort the boundary positions, take differences, merge zero-length runs), where the kernels toggle bits and take a running
XOR.  Python floats are IEEE doubles and every operation below is rounded on its own."""
import math

import numpy as np

SCALE = 5.0


def _scaled(c):
    return int(SCALE * float(c) + .5)                        # int() truncates toward zero, as C's (int)


def dense_points(ring):
    """(u, v) of the concatenated dense points of one ring [x0, y0, x1, y1, ...]; the v of a zero-length edge's one point is None:
    the rule never reads it, and a None would make any read fail loudly"""
    k = len(ring) // 2
    X = [_scaled(ring[2 * j]) for j in range(k)]
    Y = [_scaled(ring[2 * j + 1]) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx if dx else None
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5) if dx else None)
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def boundary_positions(ring, H, W):
    """the column-major positions rleFrPoly collects for one ring, unsorted, H * W included where the rule gives it"""
    u, v = dense_points(ring)
    pos = []
    for i in range(1, len(u)):
        if u[i] == u[i - 1]:
            continue
        xd = float(u[i] if u[i] < u[i - 1] else u[i] - 1)
        xd = (xd + .5) / SCALE - .5
        if math.floor(xd) != xd or xd < 0 or xd > W - 1:
            continue
        yd = float(min(v[i], v[i - 1]))
        yd = (yd + .5) / SCALE - .5
        if yd < 0:
            yd = 0.0
        elif yd > H:
            yd = float(H)
        yd = math.ceil(yd)
        pos.append(int(xd) * H + int(yd))
    return pos


def fr_poly(ring, H, W):
    """rleFrPoly: one ring -> the run lengths (a list starting with the run of zeros), in the sort / difference / merge form"""
    a = sorted(boundary_positions(ring, H, W) + [H * W])
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def decode(counts, H, W):
    """run lengths -> dense bool [H, W] (the runs fill the mask column-major, starting with zeros)"""
    flat = np.zeros(H * W, dtype=bool)
    p, on = 0, False
    for c in counts:
        if on:
            flat[p:p + c] = True
        p += c
        on = not on
    assert p == H * W, (p, H * W)
    return flat.reshape(W, H).T.copy()


def encode(dense):
    """dense [H, W] -> the canonical run lengths (column-major, starting with the possibly empty run of zeros)"""
    flat = np.asarray(dense).astype(bool).T.reshape(-1)
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate([[0], edges, [flat.size]])
    counts = np.diff(bounds).tolist()
    return ([0] if flat.size and flat[0] else []) + counts


def poly_mask(rings, H, W):
    """one object: the union of its rings (rleMerge, intersect = 0) -> dense bool [H, W]; no ring: empty"""
    m = np.zeros((H, W), dtype=bool)
    for ring in rings:
        m |= decode(fr_poly(ring, H, W), H, W)
    return m


def to_string(cnts):
    out = []
    for i in range(len(cnts)):
        x = int(cnts[i]) - (int(cnts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def from_string(s):
    cnts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[len(cnts) - 2]
        cnts.append(x)
    return cnts


def segm_mask(segm, H, W):
    """any of the forms of a COCO "segmentation" (polygons, RLE with a list or a string) or None -> dense bool [H, W]"""
    if segm is None:
        return np.zeros((H, W), dtype=bool)
    if isinstance(segm, dict):
        c = segm["counts"]
        if isinstance(c, bytes):
            c = c.decode("ascii")
        return decode(from_string(c) if isinstance(c, str) else c, H, W)
    return poly_mask(segm, H, W)
