"""Host restatement (numpy, float64, plain loops) of the plane detection evaluator, written from its description - the reference's
evaluate_for_planes (evaluation/mp3d_evaluation.py:467-743), compare_planes (utils/metrics.py:6-24) and VOCap.compute_ap.  The CPU
tests hold it against what the reference function itself produced on the fixture seeds (tests/golden/J_plane_eval_*.npz); the GPU
tests compare the kernels against it at shapes the fixture does not cover.  Nothing here is shared with nopesac_amd.evaluation."""
import math

import numpy as np

COLS = ("score", "label", "tp_mask", "tp_plane", "tp_normal", "tp_offset", "normal_err_deg", "offset_err", "best_iou", "gt_id")


def plane_errors(pred_planes, gt_planes):
    """(normal error in degrees [n_pred, n_gt], offset error [n_pred, n_gt]) in float64 from float32 plane parameters:
    offset = |p| + 1e-5, normal = p / offset, d = clamp(|n_pred - n_gt|, 0, 2), normal error = 2 asin(d / 2) 180 / pi."""
    p = np.asarray(pred_planes, np.float32).reshape(-1, 3).astype(np.float64)
    g = np.asarray(gt_planes, np.float32).reshape(-1, 3).astype(np.float64)
    po, go = np.sqrt((p * p).sum(1)) + 1e-5, np.sqrt((g * g).sum(1)) + 1e-5
    pn, gn = p / po[:, None], g / go[:, None]
    d = np.clip(np.sqrt(((pn[:, None, :] - gn[None, :, :]) ** 2).sum(-1)), 0.0, 2.0)
    return 2.0 * np.arcsin(d / 2.0) / math.pi * 180.0, np.abs(po[:, None] - go[None, :])


def mask_iou(dt, gt):
    """[n_dt, n_gt] float64 IoU of dense boolean masks, integer counts."""
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)), np.float64)
    dt, gt = np.asarray(dt, bool).reshape(len(dt), -1), np.asarray(gt, bool).reshape(len(gt), -1)
    out = np.zeros((len(dt), len(gt)), np.float64)
    for i, d in enumerate(dt):
        for j, g in enumerate(gt):
            inter, union = int((d & g).sum()), int((d | g).sum())
            out[i, j] = inter / union if union > 0 else 0.0
    return out


def assign(iou, score, pred_label, pred_plane, gt_label, gt_plane, iou_thresh=0.5, normal_thresh=30.0, offset_thresh=0.3):
    """One view: rows [n_pred, 10] (COLS) in the predictions' own order.  Predictions are visited in descending score order (ties:
    lower index first); gt_id = first maximum of the IoU row; four independent lists of GT ids already taken."""
    iou = np.asarray(iou, np.float64)
    score = np.asarray(score, np.float32)
    n_pred, n_gt = len(score), len(gt_label)
    rows = np.zeros((n_pred, len(COLS)), np.float64)
    rows[:, 0], rows[:, 1] = score.astype(np.float64), np.asarray(pred_label, np.float64)
    if n_gt == 0:
        rows[:, 6:8], rows[:, 9] = np.nan, -1.0
        return rows
    nerr, oerr = plane_errors(pred_plane, gt_plane)
    order = sorted(range(n_pred), key=lambda i: (-float(score[i]), i))
    covered = [[], [], [], []]
    for i in order:
        g = 0
        for j in range(1, n_gt):
            if iou[i, j] > iou[i, g]:
                g = j
        normal, offset = nerr[i, g], oerr[i, g]
        base = int(pred_label[i]) == int(gt_label[g]) and iou[i, g] > iou_thresh
        conds = (base, base and normal < normal_thresh and offset < offset_thresh, base and normal < normal_thresh,
                 base and offset < offset_thresh)
        for c in range(4):
            if conds[c] and g not in covered[c]:
                rows[i, 2 + c] = 1.0
                covered[c].append(g)
        rows[i, 6], rows[i, 7], rows[i, 8], rows[i, 9] = normal, offset, iou[i, g], g
    return rows


def compute_ap(scores, tp, npos):
    """VOCap.compute_ap / xVOCap in float64, with its loops."""
    scores, tp = np.asarray(scores, np.float64), np.asarray(tp, np.float64)
    if len(scores) == 0:
        return 0.0
    order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))
    ctp = cfp = 0.0
    rec, prec = [], []
    for i in order:
        ctp += 1.0 if tp[i] == 1 else 0.0
        cfp += 1.0 if tp[i] == 0 else 0.0
        rec.append(ctp / npos)
        prec.append(ctp / (cfp + ctp))
    mrec, mpre = [0.0] + rec + [1.0], [0.0] + prec + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap


def table(rows, npos_by_cat, iou_thresh=0.5, normal_thresh=30, offset_thresh=0.3, names=None):
    """The reference's final table, its keys (the last class mean formats the NORMAL threshold into its `offset` key)."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(COLS))
    names = names or {1: "plane"}
    ok = ~np.isnan(rows[:, 6])
    nerr, oerr = rows[ok, 6], rows[ok, 7]
    out = {"%normal<10": (nerr < 10).sum() / len(nerr) * 100, "%normal<30": (nerr < 30).sum() / len(nerr) * 100,
           "%offset<0.5": (oerr < 0.5).sum() / len(oerr) * 100, "%offset<0.3": (oerr < 0.3).sum() / len(oerr) * 100,
           "mean_normal": nerr.mean(), "median_normal": np.median(nerr), "mean_offset": oerr.mean(), "median_offset": np.median(oerr)}
    heads = ["mask_ap@%.1f" % iou_thresh, "plane_ap@iou%.1fnormal%.1foffset%.1f" % (iou_thresh, normal_thresh, offset_thresh),
             "plane_ap@iou%.1fnormal%.1f" % (iou_thresh, normal_thresh), "plane_ap@iou%.1foffset%.1f" % (iou_thresh, offset_thresh)]
    sums, valid = [0.0] * 4, 0
    for cat in sorted(npos_by_cat):
        if npos_by_cat[cat] == 0:
            continue
        valid += 1
        mine = rows[rows[:, 1] == cat]
        for c in range(4):
            ap = compute_ap(mine[:, 0], mine[:, 2 + c], npos_by_cat[cat])
            sums[c] += ap
            out[heads[c] + " - " + names[cat]] = ap
    heads[3] = "plane_ap@iou%.1foffset%.1f" % (iou_thresh, normal_thresh)
    for c in range(4):
        out[heads[c]] = sums[c] / valid
    return {k: float(v) for k, v in out.items()}


def evaluate(views, iou_thresh=0.5, normal_thresh=30.0, offset_thresh=0.3, id_map=None):
    """views: [{"pred": bool [n, H, W], "score", "label" (contiguous), "pred_plane", "gt": bool [m, H, W], "gt_label", "gt_plane"}],
    each image once -> rows [sum n, 10], view after view."""
    id_map = id_map or {0: 1}
    out = []
    for v in views:
        if len(v["score"]) == 0:
            continue
        labels = [id_map[int(x)] for x in v["label"]]
        out.append(assign(mask_iou(v["pred"], v["gt"]), v["score"], labels, v["pred_plane"], v["gt_label"], v["gt_plane"],
                          iou_thresh, normal_thresh, offset_thresh))
    return np.concatenate(out) if out else np.zeros((0, len(COLS)), np.float64)
