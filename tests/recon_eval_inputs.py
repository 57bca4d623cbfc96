"""Seeded inputs of the two-view reconstruction AP (the reference's offline eval.py --evaluate AP), shared by
scripts/gen_recon_eval_golden.py (which runs the reference functions on them and stores only their results,
tests/golden/K_recon_eval_<seed>.npz) and the tests.  Modelled on tests/plane_eval_inputs.py: 48 x 64 masks, a view's GT is a
partition of the image into blobs, predictions are shifted / thinned copies of GT blobs plus a spurious stripe pattern.

The geometry is consistent: a pair's GT planes are drawn in the common frame (view 1's, after the y / z flip); view 1's local
plane is the flipped global one, view 0's is derived through the GT camera, so the two views of a matched GT plane agree (the
reference asserts 1e-3).  Predicted planes are GT planes turned and shifted to either side of the 30 degree / 1 m thresholds, the
predicted camera is the GT camera with a small error.

Every case keeps its decisive quantities away from their thresholds: a draw with a merged IoU within IOU_MARGIN of 0.5, a normal
error within NORMAL_MARGIN of 30, an offset error within OFFSET_MARGIN of 1 or a matched pair of predictions with |n0 . n1| within
DOT_MARGIN of 0 (the merged normal is then ill-defined) is rejected and drawn again with the next sub-seed.  Scores are distinct
over the whole case and above 0.1 (the reference is only defined there: its create_instances drops lower ones from the planes but
not from the IoU rows)."""
import numpy as np

from tests import recon_eval_ref as REF
from tests.plane_eval_inputs import IOU_MARGIN, NORMAL_MARGIN, OFFSET_MARGIN, _rotate
from tests.plane_eval_ref import mask_iou

SEEDS = (21, 22, 23)
DOT_MARGIN = 1e-3
FLIP = np.array([1.0, -1.0, -1.0])

# What the pairs of a seed are; between them the seeds cover every situation the evaluator distinguishes.
#   match: "none" no predicted correspondence | "some" | "all0" every prediction of view 0 is matched
#   preds: which views have predictions;  gt0: view 0 has GT;  shared: GT planes seen in both views (0: empty gt_corrs)
#   trap: two predictions of one GT plane next to a parallel GT plane (the walk must not move on to the free one)
#   negdot: a predicted correspondence between planes whose global normals point apart
#   qscale: (predicted, GT) camera quaternion scale;  turn180: GT rotation within 2 degrees of 180
PLAN = {
    21: [dict(match="some", trap=True), dict(match="none"), dict(match="some", preds=(True, False)), dict(match="none", preds=(False, False))],
    22: [dict(match="all0", negdot=True), dict(match="none", gt0=False), dict(match="some", shared=0), dict(match="some", qscale=(1.7, 0.6))],
    23: [dict(match="some", turn180=True, negdot=True), dict(match="some", trap=True, qscale=(0.5, 1.0)), dict(match="all0")],
}


def _unit(v):
    return v / np.linalg.norm(v)


def _camera(rng, turn180=False):
    axis = _unit(rng.normal(size=3))
    angle = np.deg2rad(rng.uniform(178.0, 179.5) if turn180 else rng.uniform(10.0, 70.0))
    return {"position": rng.uniform(-1.0, 1.0, 3), "rotation": np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])}


def _local_in_view0(g, cam):
    """The plane with global parameters g (normal * offset) in view 0's frame: b = lambda n with lambda = d - t . n, turned back."""
    d = np.linalg.norm(g)
    n = g / d
    lam = d - cam["position"] @ n
    return (REF.rotation_matrix(cam["rotation"]).T @ (lam * n)) * FLIP, lam


def _blobs(rng, h, w, n):
    if n == 0:
        return np.zeros((0, h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    lab = np.argmin((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2, 0)
    return np.stack([lab == k for k in range(n)])


def _perturbed(rng, plane, small=False):
    off = float(np.linalg.norm(plane))
    lo, hi = (0.0, 8.0) if small else ((0.0, 8.0), (12.0, 26.0), (34.0, 60.0))[int(rng.integers(0, 3))]
    dlo, dhi = (0.0, 0.15) if small else ((0.0, 0.3), (0.4, 0.7), (1.4, 2.0))[int(rng.integers(0, 3))]
    delta = rng.uniform(dlo, dhi) * rng.choice([-1.0, 1.0])
    if off + delta < 0.3:
        delta = abs(delta)
    return _rotate(plane / off, rng.uniform(lo, hi), rng) * (off + delta)


def _pair(rng, h, w, tag, match="some", preds=(True, True), gt0=True, shared=None, trap=False, negdot=False, qscale=(1.0, 1.0), turn180=False):
    yy, xx = np.mgrid[0:h, 0:w]
    gt_cam = _camera(rng, turn180)
    n_shared = int(rng.integers(2, 4)) if shared is None else shared
    if not gt0:
        n_shared = 0
    n_own = [int(rng.integers(1, 3)) if gt0 else 0, int(rng.integers(1, 3))]
    # global planes: the shared ones, view 0's own, view 1's own (+ the trap's parallel pair, + the plane that faces shared plane 0)
    def draw():
        return _unit(rng.normal(size=3)) * rng.uniform(1.5, 4.0)
    glob = [[draw() for _ in range(n_shared + n_own[0])], None]
    glob[1] = glob[0][:n_shared] + [draw() for _ in range(n_own[1])]
    trap_ids = None
    if trap:
        g = draw()
        trap_ids = (len(glob[1]), len(glob[1]) + 1)
        glob[1] += [g, g * (1.0 + 0.4 / np.linalg.norm(g))]
    facing = None
    if negdot:                                           # view 1's own plane whose normal is shared plane 0's, turned by 155 degrees
        facing = len(glob[1])
        glob[1].append(_rotate(_unit(glob[0][0]), 155.0, rng) * rng.uniform(1.5, 4.0))
    local = [[], []]
    for g in glob[0]:
        p, lam = _local_in_view0(g, gt_cam)
        if abs(lam) < 0.3:
            return None
        local[0].append(p)
    local[1] = [g * FLIP for g in glob[1]]
    gt_corrs = [[k, k] for k in range(n_shared)]
    if n_shared > 1:                                     # not the identity: view 1 lists the shared planes in another order
        perm = np.roll(np.arange(n_shared), 1)
        head = [local[1][perm[k]] for k in range(n_shared)]
        local[1][:n_shared] = head
        gt_corrs = [[int(perm[k]), k] for k in range(n_shared)]
        gt_corrs.sort()
    views, srcs = [], []
    for v in range(2):
        m = len(local[v])
        gt = _blobs(rng, h, w, m)
        masks, src, planes = [], [], []
        if preds[v]:
            for k in range(m):
                forced = negdot or (trap and v == 1 and k in trap_ids)
                if forced or rng.uniform() < 0.85:
                    msk = np.roll(gt[k], int(rng.integers(-1, 2)), axis=int(rng.integers(0, 2)))
                    if not forced and rng.uniform() < 0.25:
                        msk = msk & (xx % 3 == 0)           # a poor detection: IoU with its blob below 0.5
                    masks.append(msk); src.append(k)
                    planes.append(_perturbed(rng, local[v][k], small=trap and v == 1 and k == trap_ids[0]))
            if trap and v == 1:                           # a second prediction of the trap's first plane
                masks.append(np.roll(gt[trap_ids[0]], -2, axis=1)); src.append(trap_ids[0])
                planes.append(_perturbed(rng, local[1][trap_ids[0]], small=True))
            masks.append((xx + yy) % 7 == v); src.append(-1)
            planes.append(rng.normal(size=3) * 2.0)
            order = rng.permutation(len(masks))
            masks, src, planes = [masks[i] for i in order], [src[i] for i in order], [planes[i] for i in order]
        views.append({"pred": np.stack(masks) if masks else np.zeros((0, h, w), bool), "pred_plane": np.asarray(planes, np.float32).reshape(-1, 3),
                      "gt": gt, "gt_plane": np.asarray(local[v], np.float32).reshape(-1, 3)})
        srcs.append(src)
    # predicted correspondences: predictions of the two views of a shared GT plane, a wrong one for `negdot`
    n0, n1 = len(srcs[0]), len(srcs[1])
    A = np.zeros((n0, n1), np.uint8)
    view1_of = {a: b for a, b in gt_corrs}
    if match != "none":
        for i, s in enumerate(srcs[0]):
            js = [j for j, t in enumerate(srcs[1]) if s >= 0 and t == view1_of.get(s, -2) and not A[:, j].any()]
            if js and (match == "all0" or rng.uniform() < 0.75):
                A[i, js[0]] = 1
        if negdot:
            i = [i for i, s in enumerate(srcs[0]) if s == gt_corrs[0][0]]
            j = [j for j, t in enumerate(srcs[1]) if t == facing]
            if not i or not j:
                return None
            A[i[0], :] = 0
            A[:, j[0]] = 0
            A[i[0], j[0]] = 1
        if match == "some" and not A.any() and n0 and n1:  # no shared GT plane with a prediction in both views: a wrong correspondence
            A[int(rng.integers(0, n0)), int(rng.integers(0, n1))] = 1
        if match == "all0":                               # whatever is left of view 0 takes any free plane of view 1
            for i in range(n0):
                free = [j for j in range(n1) if not A[:, j].any()]
                if not A[i].any():
                    if not free:
                        return None
                    A[i, free[int(rng.integers(0, len(free)))]] = 1
    err_axis = _unit(rng.normal(size=3))
    err_angle = np.deg2rad(rng.uniform(1.0, 6.0))
    dq = np.concatenate([[np.cos(err_angle / 2)], np.sin(err_angle / 2) * err_axis])
    w0, v0, w1, v1 = gt_cam["rotation"][0], gt_cam["rotation"][1:], dq[0], dq[1:]
    rot = np.concatenate([[w1 * w0 - v1 @ v0], w1 * v0 + w0 * v1 + np.cross(v1, v0)])
    pred_cam = {"position": gt_cam["position"] + rng.normal(size=3) * 0.1, "rotation": rot * qscale[0]}
    gt_cam = {"position": gt_cam["position"], "rotation": gt_cam["rotation"] * qscale[1]}
    return {"ids": (tag + "a", tag + "b"), "views": tuple(views), "pred_cam": pred_cam, "gt_cam": gt_cam, "assignment": A,
            "gt_corrs": gt_corrs, "src": srcs}


def pair_args(pair):
    """The pair as tests/recon_eval_ref.py's pair_errors takes it (IoU from the dense masks)."""
    v0, v1 = pair["views"]
    return (mask_iou(v0["pred"], v0["gt"]), mask_iou(v1["pred"], v1["gt"]), v0["score"], v1["score"], v0["pred_plane"], v1["pred_plane"],
            v0["gt_plane"], v1["gt_plane"], pair["pred_cam"], pair["gt_cam"], np.argwhere(pair["assignment"]), pair["gt_corrs"])


def margins(pair):
    """(smallest distance of a merged IoU to 0.5, of a normal error to 30, of an offset error to 1, of a matched |n0 . n1| to 0)."""
    e = REF.pair_errors(*pair_args(pair))
    dist = lambda x, t: float(np.abs(x - t).min()) if x.size else np.inf      # noqa: E731
    dots = [np.inf]
    if pair["assignment"].any():
        n0, n1 = REF.global_planes(pair["views"][0]["pred_plane"], pair["pred_cam"])[1], REF.global_planes(pair["views"][1]["pred_plane"], REF.IDENTITY)[1]
        dots += [abs(float(n0[a] @ n1[b])) for a, b in np.argwhere(pair["assignment"])]
    return dist(e["mask_iou"], 0.5), dist(e["err_normals"], 30.0), dist(e["err_offsets"], 1.0), min(dots)


def margins_ok(pair) -> bool:
    i, n, o, d = margins(pair)
    return i > IOU_MARGIN and n > NORMAL_MARGIN and o > OFFSET_MARGIN and d > DOT_MARGIN


def has_trap(pair) -> bool:
    """Some criterion has two entries with the same first flagged GT entry while a later entry the second one flags stays free."""
    rows, _, e = REF.pair_rows(*pair_args(pair))
    for k in range(5):
        flags = (e["mask_iou"] >= REF.MASK_T[k]) & (e["err_normals"] <= REF.NORMAL_T[k]) & (e["err_offsets"] <= REF.OFFSET_T[k])
        first = [int(np.argmax(f)) if f.any() else -1 for f in flags]
        claimed = {f for f in first if f >= 0}
        for r in range(len(first)):
            if first[r] >= 0 and first[r] in first[:r] and any(c > first[r] and c not in claimed for c in np.flatnonzero(flags[r])):
                return True
    return False


def has_negative_dot(pair) -> bool:
    n0, n1 = REF.global_planes(pair["views"][0]["pred_plane"], pair["pred_cam"])[1], REF.global_planes(pair["views"][1]["pred_plane"], REF.IDENTITY)[1]
    return any(float(n0[a] @ n1[b]) < 0 for a, b in np.argwhere(pair["assignment"]))


def gt_agrees(pair) -> bool:
    """The reference's assertion: both views of a matched GT plane name the same global plane within 1e-3."""
    o0, n0 = REF.global_planes(pair["views"][0]["gt_plane"], pair["gt_cam"])
    o1, n1 = REF.global_planes(pair["views"][1]["gt_plane"], REF.IDENTITY)
    return all(np.linalg.norm(n0[a] - n1[b]) < 1e-3 and abs(o0[a] - o1[b]) < 1e-3 for a, b in pair["gt_corrs"])


def recon_eval_case(seed: int, h: int = 48, w: int = 64):
    """The pairs of PLAN[seed]: [{"ids", "views": (view0, view1), "pred_cam", "gt_cam": {"position", "rotation" wxyz}, "assignment"
    uint8 [n0, n1], "gt_corrs": [[a, b], ...]}]; view = {"pred" bool [n, H, W], "score" f32 [n], "pred_plane" f32 [n, 3], "gt" bool
    [m, H, W], "gt_plane" f32 [m, 3]}."""
    for attempt in range(400):
        rng = np.random.default_rng(1000 * seed + attempt)
        pairs = [_pair(rng, h, w, f"r{seed}p{i}", **kw) for i, kw in enumerate(PLAN[seed])]
        if any(p is None for p in pairs):
            continue
        total = sum(len(v["pred"]) for p in pairs for v in p["views"])
        score = (np.linspace(0.95, 0.2, total) + rng.uniform(-0.002, 0.002, total))[rng.permutation(total)].astype(np.float32)
        assert len(np.unique(score)) == total and score.min() > 0.1
        at = 0
        for p in pairs:
            for v in p["views"]:
                v["score"] = score[at:at + len(v["pred"])]
                at += len(v["pred"])
        ok = all(margins_ok(p) and gt_agrees(p) for p in pairs)
        ok = ok and all(has_trap(p) for p, kw in zip(pairs, PLAN[seed]) if kw.get("trap"))
        ok = ok and all(has_negative_dot(p) for p, kw in zip(pairs, PLAN[seed]) if kw.get("negdot"))
        ok = ok and all(p["assignment"].any() for p, kw in zip(pairs, PLAN[seed]) if kw["match"] != "none" and all(kw.get("preds", (True, True))))
        if ok:
            return pairs
    raise RuntimeError("no case with the margins found")


def reference_rows(pairs):
    """tests/recon_eval_ref.py on the case -> (rows [entries, 8], pair after pair; GT entry count per pair; the errors dict per pair)."""
    out = [REF.pair_rows(*pair_args(p)) for p in pairs]
    return np.concatenate([o[0] for o in out]), [o[1] for o in out], [o[2] for o in out]


def product_inputs(pairs, compressed_gt=lambda pair_no: pair_no % 2 == 0):
    """The case in the product's formats -> (predictions, dataset_dict) of evaluation.evaluate_for_reconstruction - records as
    PoseEvaluator.prediction_record keeps them - with predicted masks as compressed COCO strings and GT masks as compressed strings or
    uncompressed run lists, by pair."""
    import torch
    from oracle import rle_oracle as R
    preds, dataset = [], {}
    for no, p in enumerate(pairs):
        enc = R.encode if compressed_gt(no) else (lambda m: {"size": list(m.shape), "counts": R.run_lengths(m)})
        pred = {"camera": {"pred": {"tran": np.asarray(p["pred_cam"]["position"]), "rot": np.asarray(p["pred_cam"]["rotation"])},
                           "gts": {"tran": list(p["gt_cam"]["position"]), "rot": list(p["gt_cam"]["rotation"])}},
                "pred_assignment": torch.from_numpy(p["assignment"].copy())}
        entry = {"gt_corrs": [list(c) for c in p["gt_corrs"]],
                 "rel_pose": {"position": list(p["gt_cam"]["position"]), "rotation": list(p["gt_cam"]["rotation"])}}
        for v, image_id, view in zip("01", p["ids"], p["views"]):
            pred[v] = {"image_id": image_id, "pred_plane": torch.from_numpy(view["pred_plane"].copy()),
                       "instances": [{"segmentation": R.encode(m), "score": float(s), "category_id": 0} for m, s in zip(view["pred"], view["score"])]}
            entry[v] = {"image_id": image_id, "height": view["gt"].shape[1], "width": view["gt"].shape[2],
                        "annotations": [{"segmentation": enc(m), "plane": [float(x) for x in pl], "category_id": 1}
                                        for m, pl in zip(view["gt"], view["gt_plane"])]}
        dataset[p["ids"][0] + "__" + p["ids"][1]] = entry
        preds.append(pred)
    return preds, dataset


def evaluator_batches(pairs):
    """The case as ReconEvaluator.process takes it: (inputs, outputs)."""
    preds, dataset = product_inputs(pairs)
    inputs = [dataset[key] for key in dataset]
    outputs = [{"0": {k: p["0"][k] for k in ("instances", "pred_plane")}, "1": {k: p["1"][k] for k in ("instances", "pred_plane")},
                "camera": p["camera"]["pred"], "pred_assignment": p["pred_assignment"]} for p in preds]
    return inputs, outputs
