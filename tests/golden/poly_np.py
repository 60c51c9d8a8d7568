"""NumPy / pure-Python restatement of COCO's polygon fill: rleFrPoly (maskApi.c) followed by merge as a union - the oracle of
tests/test_poly_cpu.py and tests/test_gpu_poly.py ("Polygon ground truth").  pycocotools itself is not
available to this project, so no golden was captured by running it; the cases of test_poly_cpu.py pin this file.

One polygon xy[0 .. 2k) on an h x w image, all arithmetic in fp64, int() truncating toward zero:
  1. vertices scaled by 5 and rounded, the first one repeated at the end;
  2. dense points along every edge (one per step of the longer axis), the edges concatenated;
  3. one crossing per change of u between neighbouring dense points, kept when it falls on a pixel-centre column;
  4. pixel p (column-major, p = x h + y) is set iff an odd number of crossings lie at positions <= p.
`dense_points_loop` and `published_counts` are the published statements as literal loops; `dense_points`, `crossings` and
`fill` are the same rules over arrays (the loops would take seconds per 480 x 640 image), tested equal to them.
"""
import math

import numpy as np

SCALE = 5.0
MAX_HW = 1 << 22                          # CIM_SEGM_MAX_HW of include/cim_hip.h
MAX_POINTS = 1 << 26                      # CIM_POLY_MAX_POINTS: dense points in one call
MAX_COORD = float(1 << 20)


# ---- step 1 --------------------------------------------------------------------------------------------------------------------
def vertices(xy):
    """-> (X, Y) int64 [k + 1], the first vertex repeated at the end."""
    xy = np.asarray(xy, dtype=np.float64).ravel()
    r = (SCALE * xy + .5).astype(np.int64)                               # (int)(5 x + .5): two roundings, then truncation
    X, Y = r[0::2], r[1::2]
    return np.concatenate([X, X[:1]]), np.concatenate([Y, Y[:1]])


def n_points(xy):
    """Dense points of one polygon: sum over the edges of max(dx, dy) + 1."""
    X, Y = vertices(xy)
    return int(np.sum(np.maximum(np.abs(np.diff(X)), np.abs(np.diff(Y))) + 1))


def check(polygons_per_annotation, h, w):
    """The refusals: ValueError for what the device path refuses before any launch."""
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w > MAX_HW:
        raise ValueError("poly: need h, w >= 1 and h * w <= %d (h=%d, w=%d)" % (MAX_HW, h, w))
    total = 0
    for i, polys in enumerate(polygons_per_annotation):
        for xy in polys:
            n = len(xy)
            if n % 2:
                raise ValueError("poly: annotation %d: a polygon of odd length %d" % (i, n))
            if n < 6:
                raise ValueError("poly: annotation %d: a polygon of %d numbers (need >= 6; a 4-number box is not read as one)"
                                 % (i, n))
            a = np.asarray(xy, dtype=np.float64)
            if not np.isfinite(a).all():
                raise ValueError("poly: annotation %d: a non-finite coordinate" % i)
            if (np.abs(a) > MAX_COORD).any():
                raise ValueError("poly: annotation %d: a coordinate outside [-2^20, 2^20]" % i)
            total += n_points(a)
    if total > MAX_POINTS:
        raise ValueError("poly: %d dense points in one call, the limit is %d" % (total, MAX_POINTS))
    return total


# ---- step 2 --------------------------------------------------------------------------------------------------------------------
def dense_points_loop(xy):
    """rleFrPoly's first loop nest, statement by statement -> (u, v) lists."""
    X, Y = (a.tolist() for a in vertices(xy))
    k = len(X) - 1
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx == 0 and dy == 0:                                          # s = 0 / 0 there; v is defined as ys
            u.append(xs)
            v.append(ys)
        elif dx >= dy:
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def dense_points(xy):
    """The same points, the loop over d as one array expression per edge -> (u, v) int64 arrays."""
    X, Y = (a.tolist() for a in vertices(xy))
    us, vs = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        n = max(dx, dy)
        t = np.arange(n, -1, -1, dtype=np.int64) if flip else np.arange(n + 1, dtype=np.int64)
        if n == 0:
            us.append(np.array([xs], np.int64))
            vs.append(np.array([ys], np.int64))
        elif dx >= dy:
            s = float(ye - ys) / dx
            us.append(t + xs)
            vs.append(((ys + s * t) + .5).astype(np.int64))
        else:
            s = float(xe - xs) / dy
            vs.append(t + ys)
            us.append(((xs + s * t) + .5).astype(np.int64))
    return np.concatenate(us), np.concatenate(vs)


# ---- step 3 --------------------------------------------------------------------------------------------------------------------
def crossings_loop(u, v, h, w):
    """rleFrPoly's second loop, statement by statement -> list of positions a = xd h + yd (unsorted)."""
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / SCALE - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / SCALE - .5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            a.append(int(xd) * h + int(yd))
    return a


def crossings(u, v, h, w):
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    u1, u0, v1, v0 = u[1:], u[:-1], v[1:], v[:-1]
    xd = np.where(u1 < u0, u1, u1 - 1).astype(np.float64)
    xd = (xd + .5) / SCALE - .5
    keep = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.minimum(v1, v0).astype(np.float64)
    yd = (yd + .5) / SCALE - .5
    yd = np.ceil(np.where(yd < 0, 0.0, np.where(yd > h, float(h), yd)))
    return (xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64))


# ---- step 4 --------------------------------------------------------------------------------------------------------------------
def fill(a, h, w):
    """Parity form: flat column-major uint8 [h w], pixel p set iff the number of positions <= p is odd."""
    a = np.asarray(a, np.int64)
    hit = np.bincount(a[a < h * w], minlength=h * w)
    return (np.cumsum(hit) & 1).astype(np.uint8)


def published_counts(a, h, w):
    """rleFrPoly's ending, statement by statement: sort the positions plus h w, take differences, merge zero-length runs."""
    a = sorted([int(x) for x in a] + [h * w])
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


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def polygon_mask(xy, h, w):
    """One polygon -> [h, w] uint8."""
    u, v = dense_points(xy)
    return fill(crossings(u, v, h, w), h, w).reshape(w, h).T.copy()


def annotation_masks(polygons_per_annotation, h, w):
    """[[polygon, ...], ...] -> [n, h, w] uint8: the union of each annotation's polygon fills (frPyObjects + merge)."""
    check(polygons_per_annotation, h, w)
    out = np.zeros((len(polygons_per_annotation), h, w), np.uint8)
    for i, polys in enumerate(polygons_per_annotation):
        for xy in polys:
            out[i] |= polygon_mask(xy, h, w)
    return out
