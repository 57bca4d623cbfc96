"""Host restatement of cocoapi's polygon rasteriser (maskApi.c rleFrPoly, then rleMerge with intersect = 0 for a mask of several
polygons) in cocoapi's OWN form: upsample by 5, walk every edge, collect the column crossings, SORT the flat positions, append H W,
difference them into runs and fuse the zero-length runs.  csrc/plane_eval.hip computes the same masks from a toggle bitmap and a prefix
parity and never sorts, so the two share nothing but the per-point arithmetic the algorithm prescribes.  Plain Python integers and
floats (IEEE double, one operation at a time); `int()` truncates toward zero like the C cast.

pycocotools is not available to the tests, so this file has the standing of oracle/rle_oracle.py: the published algorithm restated,
pinned by hand-worked cases (tests/test_poly_cpu.py)."""
import math

import numpy as np

SCALE = 5.0


def _upsampled(xy):
    k = len(xy) // 2
    X = [int(SCALE * float(xy[2 * j]) + 0.5) for j in range(k)]
    Y = [int(SCALE * float(xy[2 * j + 1]) + 0.5) for j in range(k)]
    return X + X[:1], Y + Y[:1], k


def boundary_points(xy):
    """(u, v): the dense points along the closed boundary, every edge in its own direction, edges concatenated."""
    X, Y, k = _upsampled(xy)
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        if dx == 0 and dy == 0:                  # cocoapi divides 0 by 0 here; the one point is the vertex itself
            u.append(xs); v.append(ys)
            continue
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs); v.append(int(ys + s * t + 0.5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys); u.append(int(xs + s * t + 0.5))
    return u, v


def crossings(xy, h, w):
    """Flat positions x h + y of the column crossings, in boundary order (unsorted, repeats kept)."""
    u, v = boundary_points(xy)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + 0.5) / SCALE - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / SCALE - 0.5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        yd = math.ceil(yd)
        out.append(int(xd) * h + int(yd))
    return out


def poly_runs(xy, h, w):
    """Run lengths of ONE polygon (flat [x0, y0, x1, y1, ...]) on an h x w image: cocoapi's sort / difference / fuse."""
    a = sorted(crossings(xy, h, w)) + [h * w]
    p = 0
    for j in range(len(a)):
        a[j], p = a[j] - p, a[j]
    b, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j]); j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]; j += 1
    return b


def _dense_flat(runs):
    return np.repeat((np.arange(len(runs)) & 1).astype(bool), runs)


def mask_runs(polys, h, w):
    """Run lengths of a mask made of several polygons: the union (rleMerge, intersect = 0) of their masks."""
    flat = np.zeros(h * w, bool)
    for xy in polys:
        flat |= _dense_flat(poly_runs(xy, h, w))
    edges = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)) != 0)
    return np.diff(np.concatenate([[0], edges, [h * w]])).tolist()


def mask_rle(polys, h, w):
    """The mask as an uncompressed COCO RLE dict."""
    return {"size": [int(h), int(w)], "counts": [int(c) for c in mask_runs(polys, h, w)]}


def mask_dense(polys, h, w):
    """bool [h, w]."""
    return _dense_flat(mask_runs(polys, h, w)).reshape((h, w), order="F")


def packed(dense):
    """uint32 words of a dense mask: bit p & 31 of word p >> 5, p = x H + y."""
    b = np.packbits(np.asarray(dense, bool).reshape(-1, order="F"), bitorder="little")
    return np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view(np.uint32)
