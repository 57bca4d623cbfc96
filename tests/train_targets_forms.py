"""Cases and references of the training-target tests (tests/test_train_targets_cpu.py, tests/test_train_targets_gpu.py): a numpy
restatement of every step of the reference's prepare_targets / get_coordinate_map / mapper depth conversion that shares nothing with
csrc/train_targets.hip - np.unique for the ids, ids[:, None, None] == map for the masks, float64 centroid sums, astype(float32) / 1000.
for the depth, the f32 x / y and a float64 K^-1 . xy1 for the coordinate map.  tests/golden/train_targets/*.npz (written by
scripts/gen_train_targets_golden.py from the reference's own functions) pins the restatement to the reference."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_targets")
LIMIT = 50                                              # the reference's cap on planes per view
SIZES = [(1, 1), (3, 5), (16, 16), (17, 33), (30, 40), (63, 257)]
DEFAULT_K = np.array([[517.97, 0, 320], [0, 517.97, 240], [0, 0, 1]], np.float64)
SCANNET_KS = [np.array([[577.870605, 0, 319.5], [0, 577.870605, 239.5], [0, 0, 1]], np.float64),
              np.array([[1170.187988, 0.37, 647.75], [0, 1170.187988, 483.75], [0, 0, 1]], np.float64)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def unique_ids(m: np.ndarray) -> np.ndarray:
    ids = np.unique(m)                                  # ascending, signed
    return ids[1:] if ids.size and ids[0] == 0 else ids


def label_ids(labels: np.ndarray, cap: int, limit: int = LIMIT):
    """-> ids int32 [B, cap] (0 past n_all), n_all, n, bad int32 [B]; an image with more than `cap` distinct values is refused."""
    B = labels.shape[0]
    ids, n_all, bad = np.zeros((B, cap), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        if np.unique(labels[b]).size > cap:
            bad[b] = 1
            continue
        u = unique_ids(labels[b])
        ids[b, :u.size], n_all[b] = u, u.size
    return ids, n_all, np.minimum(n_all, limit).astype(np.int32), bad


def centers64(masks: np.ndarray, n) -> np.ndarray:
    """masks [B, nmax, H, W], n [B] -> the centroids of (x / W, y / H) in float64 [B, nmax, 2] (0 past n): sum / W / count"""
    B, nmax, H, W = masks.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((B, nmax, 2), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            for j in range(int(n[b])):
                on = masks[b, j] != 0
                cnt = np.float64(on.sum())
                out[b, j] = xs[on].sum() / np.float64(W) / cnt, ys[on].sum() / np.float64(H) / cnt
    return out


def centers_of(masks: np.ndarray, n) -> tuple:
    """masks [B, nmax, H, W], n [B] -> plane_centers f32 [B, nmax, 2] (float64 sums, sum / W / count, rounded once) and pixel_centers f32
    [B, 2, H, W] (the f32 sum over planes, in plane order, of centre * mask)."""
    B, nmax, H, W = masks.shape
    centers, pixel = centers64(masks, n).astype(np.float32), np.zeros((B, 2, H, W), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            for j in range(int(n[b])):
                on = masks[b, j] != 0
                f = on.astype(np.float32)
                pixel[b, 0] += np.where(on, centers[b, j, 0] * f, np.float32(0))
                pixel[b, 1] += np.where(on, centers[b, j, 1] * f, np.float32(0))
    return centers, pixel


def label_targets(labels: np.ndarray, ids: np.ndarray, n, nmax: int):
    B, H, W = labels.shape
    masks = np.zeros((B, nmax, H, W), np.uint8)
    for b in range(B):
        k = int(n[b])
        masks[b, :k] = ids[b, :k, None, None] == labels[b][None]
    return (masks,) + centers_of(masks, n)


def depth_metres(u16: np.ndarray) -> np.ndarray:
    return u16.astype(np.float32) / 1000.


def coordinate_map(K: np.ndarray, H: int, W: int):
    """-> (float64 [3, H, W] from the float64 inverse of K as f32 and the reference's f32 x / y, the bound's magnitude
    |a x| + |b y| + |c| [3, H, W])."""
    kinv = np.linalg.inv(np.asarray(K, np.float64).astype(np.float32).astype(np.float64))
    x = (np.arange(W, dtype=np.float32) / np.float32(W) * np.float32(640)).astype(np.float64)
    y = (np.arange(H, dtype=np.float32) / np.float32(H) * np.float32(480)).astype(np.float64)
    xx, yy = np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W))
    out = kinv[:, 0, None, None] * xx + kinv[:, 1, None, None] * yy + kinv[:, 2, None, None]
    mag = np.abs(kinv[:, 0, None, None] * xx) + np.abs(kinv[:, 1, None, None] * yy) + np.abs(kinv[:, 2, None, None])
    return out, mag


def unpack_bits(bits: np.ndarray, H: int, W: int) -> np.ndarray:
    """int32 [n, ceil(H W / 32)], bit p = x H + y -> uint8 [n, H, W]"""
    flat = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :H * W]
    return np.ascontiguousarray(flat.reshape(-1, W, H).transpose(0, 2, 1))


def to_rle(mask: np.ndarray) -> dict:
    """uncompressed COCO RLE of an [H, W] mask (column-major runs, the first of zeros)"""
    flat = np.asarray(mask, np.uint8).reshape(-1, order="F")
    edges = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return {"size": list(mask.shape), "counts": ([0] if flat.size and flat[0] else []) + runs}


# ---- seeded cases ---------------------------------------------------------------------------------------------------------------------
def partition(H: int, W: int, values, seed: int, band: bool = True) -> np.ndarray:
    """A label map: a nearest-seed partition of the image into len(values) regions carrying `values`, with a band of zeros at the left
    when `band` (and room).  Every value owns at least one pixel when H W >= len(values) (+ the band)."""
    rng = np.random.default_rng(seed)
    values = np.asarray(values, np.int64)
    k = values.size
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if k <= 64:
        sy, sx = rng.integers(0, H, k), rng.integers(0, W, k)
        own = ((ys[None] - sy[:, None, None]) ** 2 + (xs[None] - sx[:, None, None]) ** 2).argmin(0)
    else:
        own = rng.integers(0, k, (H, W))
    m = values[own]
    if band and W >= 8:
        m[:, :W // 8] = 0
    free = np.flatnonzero((m != 0).reshape(-1) if band and W >= 8 else np.ones(H * W, bool))
    missing = [v for v in values if not (m == v).any()]
    assert len(missing) <= free.size, (H, W, k)
    # give every missing value one pixel of a value that owns more than one
    flat = m.reshape(-1)
    for v in missing:
        vals, counts = np.unique(flat[free], return_counts=True)
        donor = vals[counts.argmax()]
        assert counts.max() > 1, (H, W, k)
        flat[free[np.flatnonzero(flat[free] == donor)[0]]] = v
    return m.reshape(H, W).astype(np.int32)


def label_cases(cap: int, slots: int) -> dict:
    """name -> labels int32 [B, H, W]: the value sets of the issue at the smallest sizes that hold them"""
    c = {"zeros": np.zeros((1, 16, 16), np.int32),
         "one_id": partition(16, 16, [7], 1)[None],
         "ids50": partition(30, 40, np.arange(1, 51), 2)[None],
         "ids51": partition(30, 40, np.arange(1, 52), 3)[None],
         "ids1000": partition(63, 257, np.arange(1, 1001) * 3, 4)[None],
         "collide": partition(30, 40, np.arange(1, 41) * slots, 5)[None],                  # every value lands in slot 0
         "collide_neg": partition(17, 33, (np.arange(-6, 7) * slots).tolist() + [5, 5 + slots], 6, band=False)[None],
         "negative": partition(17, 33, [-5, -1, 0, 3, 9], 7, band=False)[None],            # 0 stays a plane
         "int_max": partition(16, 16, [2**31 - 1, -2**31, 1], 8)[None],
         "too_many": (np.arange(63 * 257, dtype=np.int64) % (cap + 1) + 1).astype(np.int32).reshape(1, 63, 257),
         "exactly_cap": (np.arange(63 * 257, dtype=np.int64) % cap + 1).astype(np.int32).reshape(1, 63, 257),
         "cap_with_zero": (np.arange(63 * 257, dtype=np.int64) % (cap + 1)).astype(np.int32).reshape(1, 63, 257)}
    last = partition(30, 40, [4, 9], 9)
    last[-1, -1] = 77                                                                       # one pixel, at the last address
    c["last_pixel"] = last[None]
    c["ragged"] = np.stack([partition(30, 40, np.arange(1, 4), 10), partition(30, 40, np.arange(5, 65), 11), partition(30, 40, [2], 12)])
    for H, W in SIZES:
        k = min(6, H * W)
        c["size_%dx%d" % (H, W)] = np.stack([partition(H, W, np.arange(1, k + 1) * 11, 20 + H, band=H * W > 64),
                                             partition(H, W, np.arange(1, max(k - 2, 1) + 1), 40 + H, band=H * W > 64)])
    return c


def big_case() -> np.ndarray:
    """B = 2 at 480 x 640: 20 and 50 planes"""
    return np.stack([partition(480, 640, np.arange(1, 21) * 5, 100), partition(480, 640, np.arange(1, 51), 101)])


GOLDEN_CASES = {"g_a": (30, 40, [3, 8, 9, 12, 40], 61, DEFAULT_K), "g_b": (17, 33, [-4, 0, 2, 5], 62, SCANNET_KS[0]),
                "g_c": (63, 257, list(range(1, 52)), 63, SCANNET_KS[1])}


def golden_case(name: str):
    H, W, values, seed, K = GOLDEN_CASES[name]
    return partition(H, W, values, seed, band=min(values) > 0), K


def polygon_views(H: int, W: int):
    """three views of COCO polygon segmentations: overlapping polygons, a view with none, a view with more masks than `nmax` = 3"""
    sq = lambda x0, y0, x1, y1: [[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]]
    a = [sq(1, 1, W * 0.6, H * 0.6), sq(W * 0.3, H * 0.3, W - 1, H - 1), [[1.0, H - 2.0, W / 2.0, 2.0, W - 2.0, H - 2.0]]]
    c = [sq(0, 0, W / 2.0, H / 2.0), sq(W / 2.0, 0, W, H / 2.0), sq(0, H / 2.0, W / 2.0, H), sq(W / 2.0, H / 2.0, W, H), sq(2, 2, W - 2, H - 2)]
    return [a, [], c]


def mask_views(H: int, W: int, seed: int):
    """the same shape of case as byte masks (for the RLE route): per view a list of [H, W] masks, overlapping"""
    rng = np.random.default_rng(seed)
    views = []
    for k in (3, 0, 5):
        ms = []
        for _ in range(k):
            m = np.zeros((H, W), np.uint8)
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            m[y0:y0 + 1 + rng.integers(0, H), x0:x0 + 1 + rng.integers(0, W)] = 1
            m ^= (rng.random((H, W)) < 0.1).astype(np.uint8)
            ms.append(m)
        views.append(ms)
    return views
