"""Seeded inputs of the plane detection evaluator (mp3d_evaluation.py:467-743), shared by scripts/gen_plane_eval_golden.py (which
runs the reference function on them and stores only its results, tests/golden/J_plane_eval_<seed>.npz) and the tests.  Modelled on
tests/golden_inputs.py::matching_eval_case: the GT of an image is a partition of a small image into blobs; the predictions are
shifted / eroded copies of GT blobs, a second prediction for one blob and a spurious stripe pattern, with distinct scores and plane
parameters = GT plane + noise on either side of the 30 degree / 0.3 m thresholds.

No thresholded outcome may sit on a rounding edge (the reference computes the errors in float32): a case whose chosen normal error
lies within 1e-3 degrees of 10 or 30, whose offset error lies within 1e-4 of 0.3 or 0.5, or that has an IoU within 1e-9 of 0.5 is
rejected and drawn again."""
import numpy as np

from tests import plane_eval_ref as REF

SEEDS = (11, 12, 13)
NORMAL_EDGES, OFFSET_EDGES = (10.0, 30.0), (0.3, 0.5)
NORMAL_MARGIN, OFFSET_MARGIN, IOU_MARGIN = 1e-3, 1e-4, 1e-9


def _rotate(n, angle_deg, rng):
    """Unit vector `n` turned by angle_deg about a random axis perpendicular to it."""
    a = rng.normal(size=3)
    a -= n * (a @ n)
    a /= np.linalg.norm(a)
    t = np.deg2rad(angle_deg)
    return n * np.cos(t) + a * np.sin(t)


def _image(rng, h, w, with_preds=True):
    n_gt = int(rng.integers(4, 7))
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = rng.uniform(0, w, n_gt), rng.uniform(0, h, n_gt)
    lab = np.argmin((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2, 0)
    gt = np.stack([lab == k for k in range(n_gt)])
    normals = rng.normal(size=(n_gt, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    gt_plane = (normals * rng.uniform(1.0, 4.0, (n_gt, 1))).astype(np.float32)
    img = {"gt": gt, "gt_label": np.ones(n_gt, np.int64), "gt_plane": gt_plane}
    img.update(_predictions(rng, img, h, w) if with_preds else
               {"pred": np.zeros((0, h, w), bool), "score": np.zeros(0, np.float32), "label": np.zeros(0, np.int64),
                "pred_plane": np.zeros((0, 3), np.float32)})
    return img


def _predictions(rng, img, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    gt, gt_plane = img["gt"], img["gt_plane"]
    preds, src = [], []
    for k in range(len(gt)):
        if rng.uniform() < 0.8:
            m = np.roll(gt[k], int(rng.integers(-1, 2)), axis=int(rng.integers(0, 2)))
            if rng.uniform() < 0.3:                              # a poor detection: IoU with its blob drops below 0.5
                m = m & (xx % 3 == 0)
            preds.append(m); src.append(k)
    twice = int(rng.integers(0, len(gt)))                        # two predictions for the same GT blob
    for shift in (1, -2):
        preds.append(np.roll(gt[twice], shift, axis=1)); src.append(twice)
    preds.append((xx + yy) % 7 == 0); src.append(-1)             # spurious stripes
    n = len(preds)
    score = (np.linspace(0.95, 0.30, n) + rng.uniform(-0.01, 0.01, n))[rng.permutation(n)].astype(np.float32)
    assert len(np.unique(score)) == n
    planes = []
    for k in src:
        if k < 0:
            planes.append(rng.normal(size=3) * 2.0)
            continue
        off = float(np.linalg.norm(gt_plane[k]))
        nrm = gt_plane[k].astype(np.float64) / off
        lo, hi = ((0.0, 8.0), (12.0, 28.0), (32.0, 60.0))[int(rng.integers(0, 3))]
        dlo, dhi = ((0.0, 0.2), (0.35, 0.45), (0.55, 0.9))[int(rng.integers(0, 3))]
        planes.append(_rotate(nrm, rng.uniform(lo, hi), rng) * (off + rng.choice([-1.0, 1.0]) * rng.uniform(dlo, dhi)))
    return {"pred": np.stack(preds), "score": score, "label": np.zeros(n, np.int64), "pred_plane": np.asarray(planes, np.float32)}


def margins(view):
    """(smallest distance of a chosen normal error to 10 / 30, of a chosen offset error to 0.3 / 0.5, of any IoU to 0.5) of a view."""
    if len(view["score"]) == 0 or len(view["gt"]) == 0:
        return np.inf, np.inf, np.inf
    iou = REF.mask_iou(view["pred"], view["gt"])
    g = iou.argmax(1)
    nerr, oerr = REF.plane_errors(view["pred_plane"], view["gt_plane"])
    i = np.arange(len(g))
    return (min(np.abs(nerr[i, g] - e).min() for e in NORMAL_EDGES), min(np.abs(oerr[i, g] - e).min() for e in OFFSET_EDGES),
            np.abs(iou - 0.5).min())


def margins_ok(view) -> bool:
    n, o, i = margins(view)
    return n > NORMAL_MARGIN and o > OFFSET_MARGIN and i > IOU_MARGIN


def plane_eval_case(seed: int, h: int = 48, w: int = 64):
    """Three pairs: [{"ids": (id0, id1), "views": (view0, view1)}]; view = {"pred" bool [n,H,W], "score" f32 [n], "label" [n]
    (contiguous, all 0), "pred_plane" f32 [n,3], "gt" bool [m,H,W], "gt_label" [m] (all 1), "gt_plane" f32 [m,3]}.  Image "B" is view 1
    of pair 0 and view 0 of pair 1 - the same GT, but the second occurrence carries other predictions, which a correct
    de-duplication never looks at; image "E" has GT and no prediction (it only counts in npos)."""
    for attempt in range(100):
        rng = np.random.default_rng(1000 * seed + attempt)
        A, B, C, D = (_image(rng, h, w) for _ in range(4))
        E = _image(rng, h, w, with_preds=False)
        B2 = {**B, **_predictions(rng, B, h, w)}
        t = f"s{seed}"
        pairs = [{"ids": (t + "A", t + "B"), "views": (A, B)}, {"ids": (t + "B", t + "C"), "views": (B2, C)},
                 {"ids": (t + "D", t + "E"), "views": (D, E)}]
        if all(margins_ok(v) for p in pairs for v in p["views"]):
            return pairs
    raise RuntimeError("no case with the margins found")


def unique_views(pairs):
    """[(image id, view)] with every image once, first occurrence wins - the reference's _siamese_to_single / _siamese_to_coco."""
    seen, out = set(), []
    for p in pairs:
        for image_id, view in zip(p["ids"], p["views"]):
            if image_id not in seen:
                seen.add(image_id)
                out.append((image_id, view))
    return out


def npos_of(pairs):
    return {1: float(sum(len(v["gt"]) for _, v in unique_views(pairs)))}


def reference_order_rows(pairs):
    """tests/plane_eval_ref.py on the case, rows in the REFERENCE's order: unique views with predictions one after the other, each
    view's predictions by descending score."""
    out = []
    for _, v in unique_views(pairs):
        if len(v["score"]):
            rows = REF.evaluate([v])
            out.append(rows[np.argsort(-rows[:, 0], kind="stable")])
    return np.concatenate(out)


def product_inputs(pairs, compressed_gt=lambda image_id: sum(map(ord, image_id)) % 2 == 0):
    """The case in the product's input format -> (predictions, dataset_dict) of evaluation.evaluate_for_planes: predicted masks as
    compressed COCO strings, GT masks as compressed strings or uncompressed run lists, by image."""
    from oracle import rle_oracle as R
    preds, dataset = [], {}
    for p in pairs:
        pred, entry = {}, {}
        for v, image_id, view in zip("01", p["ids"], p["views"]):
            pred[v] = {"image_id": image_id, "pred_plane": view["pred_plane"],
                       "instances": [{"segmentation": R.encode(m), "score": float(s), "category_id": int(c)}
                                     for m, s, c in zip(view["pred"], view["score"], view["label"])]}
            enc = R.encode if compressed_gt(image_id) else (lambda m: {"size": list(m.shape), "counts": R.run_lengths(m)})
            entry[v] = {"image_id": image_id, "annotations": [{"segmentation": enc(m), "plane": [float(x) for x in pl], "category_id": int(c)}
                                                              for m, pl, c in zip(view["gt"], view["gt_plane"], view["gt_label"])]}
        dataset[p["ids"][0] + "__" + p["ids"][1]] = entry
        preds.append(pred)
    return preds, dataset
