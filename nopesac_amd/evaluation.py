"""Camera-pose evaluator counterpart of `MP3DEvaluator` (evaluation/mp3d_evaluation.py), restricted to the part
that consumes the hot path's outputs: per-pair pose errors and their summary table.

  * process(inputs, outputs)  ~ mp3d_evaluation.py:184-257: collects every output key containing "camera"
    together with the ground truth `input["rel_pose"]{"position","rotation"}`;
  * evaluate()                ~ :315-366 + `_eval_camera_reg` :382-425: gathers across ranks (ONE all_gather of
    fixed-width fp32 rows over RCCL instead of pickled predictions over Gloo), then
    T err = ||t - t_gt||2, R err = 2 acos|<q, q_gt>| 180/pi, medians / means / accuracy at 1.0|0.5|0.2 m, 30|15|10 deg.
  * dump(output_dir)          ~ :330-341 (`eval_full_scene`): `NopeSAC_instances_predictions.pth` (torch.save of the
    per-pair prediction dicts, schema of :193-257) and `continuous.pkl` (`get_optimized_dict` :259-313 + `save_dict`
    :852-860) - the two files the reference's offline eval.py / vis tools read.
  * evaluate_for_matchings()  ~ :746-849: plane-matching precision / recall / F-score from the predictions' RLE instances, the
    GT annotations' RLE masks and `gt_corrs` (mask IoU from nopesac_amd/rle.py instead of pycocotools.mask.iou).
  * evaluate_for_planes() / PlaneEvaluator / plane_table()  ~ :467-743: the plane detection table - mask AP, the three plane APs
    and the normal / offset error statistics, key for key.  RLE decoding, pairwise mask IoU and the score-ordered true-positive
    assignment run on the device (csrc/plane_eval.hip) for all views of a batch at once; the final reduction (AP over a few thousand
    rows, once per run) is plain numpy.
  * evaluate_for_reconstruction() / ReconEvaluator / recon_table()  ~ the offline eval.py --evaluate AP (:343-619, :657-779,
    :830-1007): the AP of the planes of both views merged through the predicted camera and assignment, under five criteria.  The
    per-pair work (global planes, merged entries, error matrices, the walk) runs on the device (csrc/recon_eval.hip), the
    accumulation over all pairs is plain numpy.
GT masks are RLE dicts; with gt_polygons=True the matching, plane and reconstruction evaluators also take the polygon lists the
datasets are distributed with (the reference's mask_util.frPyObjects + merge, :544-554), rasterised on the device by
csrc/plane_eval.hip (rle.polygon_bits).  Out of scope: the depth metrics (:438-460).
"""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional

import numpy as np
import torch

from . import runner


def to_numpy(x) -> np.ndarray:
    """A tensor (any device) or anything numpy takes, as a numpy array."""
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)


def _world() -> int:
    dist = torch.distributed
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _nccl() -> bool:
    return _world() > 1 and torch.distributed.get_backend() == "nccl"


def gather_rows(local: np.ndarray, device) -> List[np.ndarray]:
    """Per-rank blocks of a [n, w] table, in rank order, in the table's dtype.  Ranks may hold different row counts (ceil sharding):
    pad to the max (at least one row), one all_gather of the padded blocks on `device`, drop the padding."""
    if _world() == 1:
        return [local]
    n = torch.tensor([local.shape[0]], device=device)
    counts = [torch.zeros_like(n) for _ in range(_world())]
    torch.distributed.all_gather(counts, n)
    nmax = max(int(max(c.item() for c in counts)), 1)
    rows = torch.from_numpy(local)
    padded = torch.zeros(nmax, local.shape[1], device=device, dtype=rows.dtype)
    padded[: local.shape[0]] = rows.to(device)
    allrows = runner.gather_metrics(padded).cpu().numpy()
    return [allrows[r * nmax: r * nmax + int(c.item())] for r, c in enumerate(counts)]


def camera_metrics(pred_tran: np.ndarray, pred_rot: np.ndarray, gt_tran: np.ndarray, gt_rot: np.ndarray) -> Dict[str, float]:
    """The reference's camera table (mp3d_evaluation.py:382-418), same keys."""
    t_err = runner.translation_error(pred_tran, gt_tran)
    r_err = runner.rotation_error_deg(pred_rot, gt_rot)
    n = max(len(t_err), 1)
    return {
        "T median err": float(np.median(t_err)), "T mean err": float(np.mean(t_err)),
        "T err < 1.0": 100.0 * float((t_err < 1.0).sum()) / n, "T err < 0.5": 100.0 * float((t_err < 0.5).sum()) / n,
        "T err < 0.2": 100.0 * float((t_err < 0.2).sum()) / n,
        "R median err": float(np.median(r_err)), "R mean err": float(np.mean(r_err)),
        "R err < 30": 100.0 * float((r_err < 30).sum()) / n, "R err < 15": 100.0 * float((r_err < 15).sum()) / n,
        "R err < 10": 100.0 * float((r_err < 10).sum()) / n,
    }


class PoseEvaluator:
    """DatasetEvaluator-style: reset() / process(inputs, outputs) / evaluate()."""

    def __init__(self, camera_keys=("camera", "camera_init", "camera_initRec", "camera_avgRef0", "camera_softRef0"),
                 device: Optional[torch.device] = None, keep_predictions: bool = False):
        self.camera_keys = tuple(camera_keys)
        self.device = device
        self.keep_predictions = keep_predictions
        self.reset()

    def reset(self):
        self._rows: List[np.ndarray] = []
        self._predictions: List[dict] = []

    @staticmethod
    def prediction_record(inp: dict, out: dict) -> dict:
        """One entry of the reference's `self._predictions` (mp3d_evaluation.py:193-257), CPU-only objects."""
        gt = inp.get("rel_pose") or {}
        gt_cam = {"tran": gt.get("position"), "rot": gt.get("rotation"), "tran_cls": gt.get("tran_cls"), "rot_cls": gt.get("rot_cls")}
        pred = {"0": {}, "1": {}}
        for v in "01":
            pred[v]["image_id"] = inp[v].get("image_id")
            pred[v]["file_name"] = inp[v].get("file_name")
            if out[v] is not None and "instances" in out[v]:
                pred[v]["instances"] = out[v]["instances"]
            pred[v]["pred_plane"] = out[v]["pred_plane"].detach().cpu().clone()      # package() hands out views of one pinned buffer per batch
        for k, val in out.items():
            if "camera" in k and "cls" not in k:
                # own copies: package() hands out numpy views of the batch's pinned host buffer, which would stay alive with the record
                pred[k] = {"pred": {kk: (np.array(vv) if isinstance(vv, np.ndarray) else vv) for kk, vv in val.items()} if isinstance(val, dict) else val,
                           "gts": gt_cam}
            elif "assignment" in k:
                pred[k] = val.detach().cpu().clone()
        pred["corrs"] = {"0": {}, "1": {}}
        return pred

    def process(self, inputs: List[dict], outputs: List[dict]):
        for inp, out in zip(inputs, outputs):
            gt = inp.get("rel_pose")
            gt_t = np.asarray(gt["position"], dtype=np.float32) if gt else np.zeros(3, np.float32)
            gt_q = np.asarray(gt["rotation"], dtype=np.float32) if gt else np.array([1, 0, 0, 0], np.float32)
            row = [gt_t, gt_q, np.array([1.0 if gt else 0.0, len(out["0"]["pred_plane"]), len(out["1"]["pred_plane"]),
                                          float(out.get("matched_num", 0))], np.float32)]
            for k in self.camera_keys:
                cam = out.get(k)
                row.append(np.asarray(cam["tran"], np.float32).reshape(-1)[:3] if cam else np.zeros(3, np.float32))
                row.append(np.asarray(cam["rot"], np.float32).reshape(-1)[:4] if cam else np.array([1, 0, 0, 0], np.float32))
            self._rows.append(np.concatenate(row))
            if self.keep_predictions:
                self._predictions.append(self.prediction_record(inp, out))

    @property
    def row_width(self) -> int:
        return 3 + 4 + 4 + 7 * len(self.camera_keys)

    def evaluate(self) -> Dict[str, dict]:
        local = np.stack(self._rows) if self._rows else np.zeros((0, self.row_width), np.float32)
        dev = self.device or (torch.device("cuda", torch.cuda.current_device()) if _nccl() else torch.device("cpu"))
        r = np.concatenate(gather_rows(local, dev))
        res: Dict[str, dict] = {"pairs": {"count": int(r.shape[0]), "mean planes/view": float(r[:, 8:10].mean()) if len(r) else 0.0,
                                          "mean matches": float(r[:, 10].mean()) if len(r) else 0.0}}
        has_gt = r[:, 7] > 0 if len(r) else np.zeros(0, bool)
        for i, k in enumerate(self.camera_keys):
            o = 11 + 7 * i
            if has_gt.any():
                res[k] = camera_metrics(r[has_gt, o:o + 3], r[has_gt, o + 3:o + 7], r[has_gt, 0:3], r[has_gt, 3:7])
        return res


def evaluate_for_matchings(predictions: List[dict], dataset_dict: Dict[str, dict], iou_thresh: float = 0.5, device=None,
                           gt_polygons: bool = False) -> Dict[str, dict]:
    """Plane-matching precision / recall / F-score (mp3d_evaluation.py:746-849).  For every pair: each predicted plane of a view
    is assigned the GT plane with the highest mask IoU (instances[k]["segmentation"] vs the GT annotations' RLE masks); a
    predicted correspondence (i, j) counts as correct when both IoUs reach `iou_thresh` and [gt_i, gt_j] is one of the pair's
    `gt_corrs`.  precision = TP / #predicted, recall = TP / #GT, over all pairs, separately for every "*assignment*" key of the
    predictions.  Returns {assignment key: {"precision", "recall", "F-score", "TP", "Pred. Num.", "GT Num."}} - the reference logs
    one table per key and returns only the last one; it also ignores its iou_thresh argument (0.5 is hard-coded, :830) and divides by
    zero when nothing was matched (here: 0.0).  By default GT masks must be RLE dicts (compressed or not;
    TypeError for anything else).  device: a GPU - the IoU matrices of all views then come
    from rle.iou_device_views in one set of launches (the same float64 numbers, bit for bit); None: rle.iou on the host, per view.
    gt_polygons=True: a GT segmentation may also be a list of polygons (rasterised on the device like cocoapi's frPyObjects + merge, at
    the size of the view's predictions); that needs a device (ValueError with device=None: there is no host rasteriser)."""
    from . import rle
    if gt_polygons and device is None:
        raise ValueError("evaluate_for_matchings: gt_polygons=True needs a device (polygons are rasterised on the GPU only)")
    jobs = []
    for pred in predictions:
        pair = dataset_dict[pred["0"]["image_id"] + "__" + pred["1"]["image_id"]]
        for v in ("0", "1"):
            for ann in pair[v]["annotations"]:
                _rle_of(ann["segmentation"], "evaluate_for_matchings", gt_polygons)
            gt_rles = [ann["segmentation"] for ann in pair[v]["annotations"]]
            jobs.append(([ins["segmentation"] for ins in pred[v]["instances"]], gt_rles, [0] * len(gt_rles)))
    # device: every view of every pair in one set of launches; host: view by view
    ious = iter(rle.iou_device_views(jobs, device) if device is not None else (rle.iou(*j) for j in jobs))
    keys = [k for k in predictions[0] if "assignment" in k] if predictions else []
    stats = {k: {"tp": 0, "pred": 0} for k in keys}
    gt_total = 0
    for pred in predictions:
        pair = dataset_dict[pred["0"]["image_id"] + "__" + pred["1"]["image_id"]]
        gt_corr = {(int(a), int(b)) for a, b in pair["gt_corrs"]}
        gt_total += len(pair["gt_corrs"])
        best_iou, best_gt = [], []
        for v in ("0", "1"):
            m = next(ious)
            if m.shape[1] == 0:
                best_iou.append(np.zeros(m.shape[0])); best_gt.append(np.full(m.shape[0], -1))
            else:
                best_iou.append(m.max(-1)); best_gt.append(m.argmax(-1))       # first maximum, like torch.max
        for k in keys:
            A = pred[k]
            idx = np.argwhere(to_numpy(A) != 0)
            stats[k]["pred"] += int(idx.shape[0])
            for i, j in idx:
                if best_iou[0][i] >= iou_thresh and best_iou[1][j] >= iou_thresh and (int(best_gt[0][i]), int(best_gt[1][j])) in gt_corr:
                    stats[k]["tp"] += 1
    out = {}
    for k in keys:
        tp, npred = stats[k]["tp"], stats[k]["pred"]
        prec = tp / npred if npred else 0.0
        rec = tp / gt_total if gt_total else 0.0
        out[k] = {"precision": prec, "recall": rec, "F-score": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0,
                  "TP": tp, "Pred. Num.": npred, "GT Num.": gt_total}
    return out


# ---- plane detection table (mp3d_evaluation.py:467-743) -------------------------------------------------------------------------
from .ops import PLANE_AP_COLS as PLANE_ROW_COLS  # noqa: E402  (the row nopesac_plane_ap_assign writes, named once, in ops.py)


def average_precision(scores: np.ndarray, tp: np.ndarray, npos: float) -> float:
    """utils/VOCap.py compute_ap + xVOCap in float64 without a loop over elements: descending sort (stable: tied scores keep their
    row order), cumulative TP / FP, precision envelope (reversed cumulative maximum), sum over the recall steps.  No rows: 0."""
    scores, tp = np.asarray(scores, np.float64).reshape(-1), np.asarray(tp, np.float64).reshape(-1)
    if scores.size == 0:
        return 0.0
    order = np.argsort(-scores, kind="stable")
    ctp = np.cumsum(tp[order] == 1)
    cfp = np.cumsum(tp[order] == 0)
    mrec = np.concatenate([[0.0], ctp / float(npos), [1.0]])
    mpre = np.concatenate([[0.0], ctp / (cfp + ctp), [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.flatnonzero(mrec[1:] != mrec[:-1]) + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]))


def plane_table(rows: np.ndarray, npos_by_cat: Dict[int, float], iou_thresh: float = 0.5, normal_threshold: float = 30,
                offset_threshold: float = 0.3, cat_names: Optional[Dict[int, str]] = None) -> Dict[str, float]:
    """The reference's final reduction (mp3d_evaluation.py:651-743) with exactly its keys.  rows: float64 [n, >= 8], columns
    PLANE_ROW_COLS (one row per prediction, any order); npos_by_cat: {dataset category id: number of GT planes}.  First the eight
    error statistics over all predictions (rows with NaN errors - views without GT - are left out; no row at all: percentages 0,
    means / medians NaN), then per category with npos > 0 the four APs "<metric> - <category name>", then their means over those
    categories (0 when there is none).  The last mean keeps the reference's key: it formats the NORMAL threshold into
    "plane_ap@iou0.5offset30.0" (:713-716), while the per-category key carries the offset threshold."""
    rows = np.asarray(rows, np.float64)
    rows = rows if rows.ndim == 2 else rows.reshape(-1, len(PLANE_ROW_COLS))
    names = {1: "plane", **(cat_names or {})}
    nerr, oerr = rows[:, 6], rows[:, 7]
    nerr, oerr = nerr[~np.isnan(nerr)], oerr[~np.isnan(oerr)]
    out: Dict[str, float] = {}
    for key, e, t in (("%normal<10", nerr, 10), ("%normal<30", nerr, 30), ("%offset<0.5", oerr, 0.5), ("%offset<0.3", oerr, 0.3)):
        out[key] = float((e < t).sum()) / len(e) * 100 if len(e) else 0.0
    out["mean_normal"] = float(nerr.mean()) if len(nerr) else float("nan")
    out["median_normal"] = float(np.median(nerr)) if len(nerr) else float("nan")
    out["mean_offset"] = float(oerr.mean()) if len(oerr) else float("nan")
    out["median_offset"] = float(np.median(oerr)) if len(oerr) else float("nan")
    heads = ("mask_ap@%.1f" % iou_thresh,
             "plane_ap@iou%.1fnormal%.1foffset%.1f" % (iou_thresh, normal_threshold, offset_threshold),
             "plane_ap@iou%.1fnormal%.1f" % (iou_thresh, normal_threshold),
             "plane_ap@iou%.1foffset%.1f" % (iou_thresh, offset_threshold))
    sums, valid = [0.0] * 4, 0
    for cat in sorted(npos_by_cat):
        if npos_by_cat[cat] == 0:
            continue                                     # no plane of this category in the dataset
        valid += 1
        mine = rows[rows[:, 1] == cat]
        for c, head in enumerate(heads):
            ap = average_precision(mine[:, 0], mine[:, 2 + c], npos_by_cat[cat])
            sums[c] += ap
            out["%s - %s" % (head, names.get(cat, str(cat)))] = ap
    mean_heads = heads[:3] + ("plane_ap@iou%.1foffset%.1f" % (iou_thresh, normal_threshold),)      # the reference's quirk (:713-716)
    for c, head in enumerate(mean_heads):
        out[head] = sums[c] / valid if valid else 0.0
    return out


def _rle_of(seg, who: str, polygons: bool = False):
    """A GT segmentation as the evaluators take it: an RLE dict, or with polygons=True (the evaluators' gt_polygons) a polygon list."""
    if isinstance(seg, dict) or (polygons and isinstance(seg, (list, tuple))):
        return seg
    if polygons:
        raise TypeError(f"{who}: GT segmentation must be an RLE dict or a list of polygons")
    raise TypeError(f"{who}: GT segmentation must be an RLE dict (polygons need cocoapi frPyObjects)")


def plane_rows(views: List[dict], device, iou_thresh: float = 0.5, normal_threshold: float = 30, offset_threshold: float = 0.3,
               id_map: Optional[Dict[int, int]] = None, gt_polygons: bool = False) -> np.ndarray:
    """The per-prediction part of the reference's evaluator (mp3d_evaluation.py:512-649) for a list of views in ONE set of launches:
    every mask of every view is decoded into bit-packed form (rle.decode_bits), one launch takes all IoU blocks, one the assignment.
    views: [{"instances": [{"segmentation", "score", "category_id"}], "pred_plane": [n, 3], "annotations": [{"segmentation", "plane",
    "category_id"}]}]; id_map: contiguous prediction label -> dataset category id (default {0: 1}).  Returns float64
    [number of predictions, 10] (PLANE_ROW_COLS), view after view, each view's predictions in their own order.
    A view with predictions but no annotation gets gt_id = -1, best_iou = 0, no true positive and NaN errors (the reference raises
    there: argmax of an empty IoU row); plane_table leaves such rows out of the error statistics.
    gt_polygons=True: an annotation's segmentation may also be a list of polygons (rle.segmentation_bits; the image size is the one
    of the predictions' RLE dicts)."""
    from . import ops, rle
    id_map = {0: 1} if id_map is None else id_map
    device = torch.device(device)
    n_dt = [len(v["instances"]) for v in views]
    n_gt = [len(v["annotations"]) for v in views]
    total = int(sum(n_dt))
    if total == 0:
        return np.zeros((0, len(PLANE_ROW_COLS)), np.float64)
    dt_segs = [[ins["segmentation"] for ins in v["instances"]] for v in views]
    gt_segs = [[_rle_of(a["segmentation"], "plane_rows", gt_polygons) for a in v["annotations"]] for v in views]
    iou, d_off, _, _ = rle.iou_views(dt_segs, gt_segs, device, polygons=gt_polygons)
    planes = checked_planes(views, n_dt, lambda k, n, rows: f"plane_rows: {n} instances but {rows} pred_plane rows")
    f32 = np.concatenate([np.asarray([ins["score"] for v in views for ins in v["instances"]], np.float32),
                          np.concatenate(planes).reshape(-1),
                          np.asarray([a["plane"] for v in views for a in v["annotations"]], np.float32).reshape(-1)])
    i32 = np.asarray([id_map[int(ins["category_id"])] for v in views for ins in v["instances"]]
                     + [int(a["category_id"]) for v in views for a in v["annotations"]], np.int32)
    d_f32, d_i32 = torch.from_numpy(f32).to(device), torch.from_numpy(i32).to(device)
    n_g = int(sum(n_gt))
    score, pred_plane, gt_plane = d_f32[:total], d_f32[total:4 * total], d_f32[4 * total:]
    rows = ops.plane_ap_assign(iou, d_off[2], d_off[0], d_off[1], score, d_i32[:total], pred_plane, d_i32[total:total + n_g], gt_plane,
                               max(n_dt), max(n_gt), iou_thresh, normal_threshold, offset_threshold)
    return rows.cpu().numpy()


def _unique_views(records: List[dict], seen: set):
    """The reference's _siamese_to_single / _siamese_to_coco de-duplication: every image once, first occurrence wins."""
    for rec in records:
        for v in ("0", "1"):
            image_id = rec[v]["image_id"]
            if image_id not in seen:
                seen.add(image_id)
                yield image_id, rec[v]


def evaluate_for_planes(predictions: List[dict], dataset_dict: Dict[str, dict], device, iou_thresh: float = 0.5,
                        normal_threshold: float = 30, offset_threshold: float = 0.3, id_map: Optional[Dict[int, int]] = None,
                        categories: Optional[List[dict]] = None, gt_polygons: bool = False) -> Dict[str, float]:
    """Plane detection table (mp3d_evaluation.py:467-743) over kept prediction records, the offline form: predictions = per pair
    {"0" / "1": {"image_id", "instances", "pred_plane"}}, dataset_dict = {"<id0>__<id1>": {"0" / "1": {"image_id"?, "annotations"}}}
    (the shape evaluate_for_matchings takes).  Every image counts once (first occurrence wins, in the predictions and in the dataset);
    a view without instances is skipped; npos counts the annotations of every image of dataset_dict.  categories: the dataset json's
    `categories` ([{"id", "name"}]) for the key names; id 1 is "plane".  GT masks must be RLE dicts (TypeError otherwise), or with
    gt_polygons=True RLE dicts or polygon lists."""
    gt_of, npos = {}, {}
    for key, pair in dataset_dict.items():
        ids = key.split("__") if "__" in key else (None, None)
        for v, fallback in zip(("0", "1"), ids):
            image_id = pair[v].get("image_id", fallback)
            if image_id in gt_of:
                continue
            gt_of[image_id] = pair[v]["annotations"]
            for a in pair[v]["annotations"]:
                _rle_of(a["segmentation"], "evaluate_for_planes", gt_polygons)
                npos[int(a["category_id"])] = npos.get(int(a["category_id"]), 0.0) + 1.0
    views = [{"instances": view["instances"], "pred_plane": view["pred_plane"], "annotations": gt_of[image_id]}
             for image_id, view in _unique_views(predictions, set()) if len(view.get("instances") or []) and image_id in gt_of]
    rows = plane_rows(views, device, iou_thresh, normal_threshold, offset_threshold, id_map, gt_polygons)
    names = {int(c["id"]): c["name"] for c in (categories or [])}
    return plane_table(rows, npos or {1: 0.0}, iou_thresh, normal_threshold, offset_threshold, names)


class PlaneEvaluator:
    """DatasetEvaluator-style plane detection evaluator: reset() / process(inputs, outputs) / evaluate() -> plane_table's dict.
    process() takes each view of each pair once, by image_id (first occurrence wins; a view without instances is skipped but its
    annotations still count in npos), and runs decode, IoU and assignment for the whole batch in one set of launches (plane_rows).
    Ranks see disjoint pairs but may see the same image: every row carries its image's number (image_index[image_id] - the
    image's index in the dataset json - when given, else the id itself when it is an integer), evaluate() gathers rows and
    per-image GT counts from all ranks and keeps, per image, the lowest rank's copy, so the table does not depend on the world size.
    A single process may leave image_index out with any ids (images are numbered as they come); several ranks with string ids
    need it (ValueError).  gt_polygons=True: annotations may carry polygon lists instead of RLE dicts (plane_rows)."""

    def __init__(self, device, iou_thresh: float = 0.5, normal_threshold: float = 30, offset_threshold: float = 0.3,
                 id_map: Optional[Dict[int, int]] = None, image_index: Optional[Dict[str, int]] = None,
                 categories: Optional[List[dict]] = None, gt_polygons: bool = False):
        self.device = torch.device(device)
        self.gt_polygons = bool(gt_polygons)
        self.iou_thresh, self.normal_threshold, self.offset_threshold = iou_thresh, normal_threshold, offset_threshold
        self.id_map = {0: 1} if id_map is None else dict(id_map)
        self.image_index = image_index
        self.cat_names = {int(c["id"]): c["name"] for c in (categories or [])}
        self.reset()

    def reset(self):
        self._seen: set = set()
        self._numbers: Dict[object, float] = {}     # single process without image_index: images numbered as they come
        self._rows: List[np.ndarray] = []           # [n, 11]: PLANE_ROW_COLS + image number
        self._gt: List[np.ndarray] = []             # [m, 3]: image number, category id, count

    def _number(self, image_id) -> float:
        if self.image_index is not None:
            return float(self.image_index[image_id])
        if isinstance(image_id, (int, np.integer)):
            return float(image_id)
        if _world() > 1:
            raise ValueError(f"PlaneEvaluator: image id {image_id!r} is no integer; with several ranks pass image_index "
                             "(image id -> index in the dataset json), the same on every rank")
        return self._numbers.setdefault(image_id, float(len(self._numbers)))

    def _register(self, number: float, cats: Dict[int, int]):
        """An image this rank has seen, with its GT count per category: one row per category and always at least one (count 0 for
        an image without annotations) - evaluate() learns from these rows which rank owns an image."""
        self._gt += [np.array([[number, c, k]], np.float64) for c, k in (cats or {0: 0}).items()]

    def process(self, inputs: List[dict], outputs: List[dict]):
        views, numbers = [], []
        for inp, out in zip(inputs, outputs):
            for v in ("0", "1"):
                image_id = inp[v].get("image_id")
                if image_id in self._seen or "annotations" not in inp[v]:
                    continue
                self._seen.add(image_id)
                num, anns = self._number(image_id), inp[v]["annotations"]
                cats: Dict[int, int] = {}
                for a in anns:
                    _rle_of(a["segmentation"], "PlaneEvaluator", self.gt_polygons)
                    cats[int(a["category_id"])] = cats.get(int(a["category_id"]), 0) + 1
                self._register(num, cats)
                o = out[v] if out.get(v) is not None else {}
                if len(o.get("instances") or []):
                    views.append({"instances": o["instances"], "pred_plane": o["pred_plane"], "annotations": anns})
                    numbers.append(num)
        if views:
            rows = plane_rows(views, self.device, self.iou_thresh, self.normal_threshold, self.offset_threshold, self.id_map,
                              self.gt_polygons)
            num = np.repeat(np.asarray(numbers, np.float64), [len(v["instances"]) for v in views])
            self._rows.append(np.concatenate([rows, num[:, None]], 1))

    def evaluate(self) -> Dict[str, float]:
        rows = np.concatenate(self._rows) if self._rows else np.zeros((0, len(PLANE_ROW_COLS) + 1), np.float64)
        gts = np.concatenate(self._gt) if self._gt else np.zeros((0, 3), np.float64)
        owner: Dict[float, int] = {}                 # image number -> the lowest rank that saw it
        dev = self.device if _nccl() else torch.device("cpu")
        gt_parts = gather_rows(gts, dev)
        for r, part in enumerate(gt_parts):
            for num in part[:, 0]:
                owner.setdefault(float(num), r)
        npos: Dict[int, float] = {}
        for r, part in enumerate(gt_parts):
            for num, cat, k in part:
                if owner[float(num)] == r and k > 0:
                    npos[int(cat)] = npos.get(int(cat), 0.0) + float(k)
        kept = [part[[owner[float(num)] == r for num in part[:, -1]]] if len(part) else part
                for r, part in enumerate(gather_rows(rows, dev))]
        return plane_table(np.concatenate(kept)[:, :len(PLANE_ROW_COLS)], npos or {1: 0.0}, self.iou_thresh, self.normal_threshold,
                           self.offset_threshold, self.cat_names)


# ---- two-view reconstruction AP (the reference's offline eval.py --evaluate AP, :343-619, :657-779, :830-1007) -----------------------
from .ops import RECON_AP_COLS as RECON_ROW_COLS  # noqa: E402  (the row nopesac_recon_ap_assign writes, named once, in ops.py)

RECON_CRITERIA = ("all", "-offset", "-normal", "-mask", "-normal-offset")       # eval.py's EP_ap_str, columns 1..5 of a row


def recon_table(rows: np.ndarray, npos: float) -> Dict[str, float]:
    """The reference's accumulation over all pairs (eval.py inst_bench :975-990 + VOCap :993-1007): per criterion the VOC area under
    the monotone precision envelope, IN PERCENT as the reference prints it, plus "npos".  rows: float64 [n, >= 6] (RECON_ROW_COLS),
    ordered by (pair, entry); npos: the sum of the pairs' GT entry counts.  Scores are sorted descending with a stable sort, so equal
    scores keep the (pair, entry) order (the reference leaves them in whatever order np.argsort of the ascending scores yields).
    npos = 0 (no GT entry anywhere): every AP is 0 (the reference divides by zero and prints nan)."""
    rows = np.asarray(rows, np.float64)
    rows = rows if rows.ndim == 2 else rows.reshape(-1, len(RECON_ROW_COLS))
    out = {name: (100.0 * average_precision(rows[:, 0], rows[:, 1 + c], npos) if npos > 0 else 0.0)
           for c, name in enumerate(RECON_CRITERIA)}
    out["npos"] = float(npos)
    return out


def f32_planes(p) -> np.ndarray:
    return np.asarray(to_numpy(p), np.float32).reshape(-1, 3)


def checked_planes(views: List[dict], n_inst: List[int], message) -> List[np.ndarray]:
    """Every view's `pred_plane` as f32 [n, 3]; a view whose row count is not its instance count n_inst[k] is a
    ValueError(message(k, instances, rows)) - the caller's own words."""
    planes = [f32_planes(v["pred_plane"]) for v in views]
    for k, (p, n) in enumerate(zip(planes, n_inst)):
        if p.shape[0] != n:
            raise ValueError(message(k, n, p.shape[0]))
    return planes


def camera7(cam: dict, who: str) -> np.ndarray:
    """{"position" | "tran", "rotation" | "rot"} -> float64 [7]: position, quaternion wxyz."""
    t = cam["position"] if "position" in cam else cam["tran"]
    q = cam["rotation"] if "rotation" in cam else cam["rot"]
    t, q = (np.asarray(to_numpy(x), np.float64).reshape(-1) for x in (t, q))
    if t.size != 3 or q.size != 4:
        raise ValueError(f"{who}: a camera is a position [3] and a quaternion [4] (got {t.size}, {q.size})")
    return np.concatenate([t, q])


def corr_pairs(corrs) -> np.ndarray:
    return to_numpy(corrs).reshape(-1, 2).astype(np.int32)


def assignment_corrs(assignment) -> np.ndarray:
    """The correspondences of a 0 / 1 assignment matrix [n0, n1] in np.argwhere order (row-major), int32 [k, 2]."""
    a = to_numpy(assignment)
    return np.argwhere(a.reshape(a.shape[-2:]) if a.ndim > 2 else a).astype(np.int32).reshape(-1, 2)


def recon_rows(pairs: List[dict], device, with_errors: bool = False, gt_polygons: bool = False):
    """The per-pair part of the reconstruction AP (eval.py:343-619, :657-779, :830-913) for a list of pairs in ONE set of launches:
    every mask of every view is decoded once (rle.decode_bits), one launch takes all IoU blocks, one the merge, the error matrices and
    the walk (ops.recon_ap_assign).  pairs: [{"views": (view0, view1), "pred_camera", "gt_camera": {"position", "rotation" wxyz},
    "pred_corrs": int [k, 2] in row-major order of the assignment (assignment_corrs), "gt_corrs": [[a, b], ...]}] with
    view = {"instances": [{"segmentation", "score"}], "pred_plane": [n, 3], "annotations": [{"segmentation", "plane"}]}.
    Returns (rows float64 [entries, 8] (RECON_ROW_COLS), pair after pair, n_entries int64 [P], n_gt_entries int64 [P]); with_errors: a
    fourth result, per pair the float64 [3, entries, GT entries] offset / normal / IoU matrices.
    Every instance counts: the reference's create_instances drops predictions with score <= 0.1 from the planes but not from the IoU
    rows or the correspondence indices, so it is only defined when every score is above 0.1, and there both agree.
    A correspondence that names a plane a view does not have, or a plane named twice, is a ValueError.
    gt_polygons=True: an annotation's segmentation may also be a list of polygons (rle.segmentation_bits; the image size is the one
    of the predictions' RLE dicts, and a batch without any prediction, whose IoU blocks are all empty, rasterises nothing)."""
    from . import ops, rle
    device = torch.device(device)
    P = len(pairs)
    if P == 0:
        z = np.zeros(0, np.int64)
        return (np.zeros((0, len(RECON_ROW_COLS)), np.float64), z, z) + (([],) if with_errors else ())
    views = [v for p in pairs for v in p["views"]]
    n_dt = [len(v["instances"]) for v in views]
    n_gt = [len(v["annotations"]) for v in views]
    total, n_g = int(sum(n_dt)), int(sum(n_gt))
    planes = checked_planes(views, n_dt, lambda k, n, rows: f"recon_rows: {n} instances but {rows} pred_plane rows")
    dt_segs = [[ins["segmentation"] for ins in v["instances"]] for v in views]
    gt_segs = [[_rle_of(a["segmentation"], "recon_rows", gt_polygons) for a in v["annotations"]] for v in views]
    pc = [corr_pairs(p["pred_corrs"]) for p in pairs]
    gc = [corr_pairs(p["gt_corrs"]) for p in pairs]
    coffs = np.stack([rle.exclusive_offsets([len(c) for c in pc]), rle.exclusive_offsets([len(c) for c in gc])])
    n_entries = np.asarray([n_dt[2 * i] + n_dt[2 * i + 1] - len(pc[i]) for i in range(P)], np.int64)
    if (n_entries < 0).any():
        raise ValueError(f"recon_rows: pair {int(np.argmax(n_entries < 0))} has more correspondences than planes")
    n_rows = int(n_entries.sum())
    f32 = np.concatenate([np.asarray([ins["score"] for v in views for ins in v["instances"]], np.float32),
                          np.concatenate(planes).reshape(-1),
                          np.asarray([a["plane"] for v in views for a in v["annotations"]], np.float32).reshape(-1)])
    cams = np.stack([np.stack([camera7(p["pred_camera"], "recon_rows") for p in pairs]),
                     np.stack([camera7(p["gt_camera"], "recon_rows") for p in pairs])])
    i32 = np.concatenate(pc + gc).reshape(-1)
    d_coff = torch.from_numpy(coffs).to(device)
    d_f32, d_cam, d_i32 = torch.from_numpy(f32).to(device), torch.from_numpy(cams).to(device), torch.from_numpy(i32).to(device)
    # nothing to decode: no mask at all, or polygons only (no prediction names the image size) - then every IoU block is empty
    iou, d_off, _, _ = rle.iou_views(dt_segs, gt_segs, device, polygons=gt_polygons,
                                     decode=bool(total + n_g) and not (gt_polygons and total == 0))
    n_pc = 2 * int(coffs[0, -1])
    err_off = None
    if with_errors:
        n_ge = [n_gt[2 * i] + n_gt[2 * i + 1] - len(gc[i]) for i in range(P)]
        err_off = rle.exclusive_offsets([3 * int(a) * max(b, 0) for a, b in zip(n_entries, n_ge)])
    res = ops.recon_ap_assign(iou, d_off[2], d_off[0], d_off[1], d_f32[:total], d_f32[total:4 * total], d_f32[4 * total:], d_cam[0], d_cam[1],
                              d_i32[:n_pc], d_coff[0], d_i32[n_pc:], d_coff[1], n_rows, max(n_dt), max(n_gt),
                              err_off=torch.from_numpy(err_off).to(device) if with_errors else None,
                              err_total=int(err_off[-1]) if with_errors else 0)
    rows, n_gt_entries, bad = res[0].cpu().numpy(), res[1].cpu().numpy().astype(np.int64), res[2].cpu().numpy()
    if bad.any():
        raise ValueError(f"recon_rows: pair(s) {np.flatnonzero(bad).tolist()} of the batch have a correspondence that names a plane "
                         "their view does not have, or name a plane twice")
    if not with_errors:
        return rows, n_entries, n_gt_entries
    flat = res[3].cpu().numpy()
    errs = [flat[err_off[i]:err_off[i + 1]].reshape(3, int(n_entries[i]), int(n_gt_entries[i])) for i in range(P)]
    return rows, n_entries, n_gt_entries, errs


def _recon_pair(views_pred, annotations, pred_camera, gt_camera, assignment, gt_corrs, who: str, gt_polygons: bool = False) -> dict:
    for anns in annotations:
        for a in anns:
            _rle_of(a["segmentation"], who, gt_polygons)
    return {"views": tuple({"instances": vp.get("instances") or [], "pred_plane": vp["pred_plane"], "annotations": anns}
                           for vp, anns in zip(views_pred, annotations)),
            "pred_camera": pred_camera, "gt_camera": gt_camera, "pred_corrs": assignment_corrs(assignment), "gt_corrs": gt_corrs}


def _recon_gt(entry: Optional[dict]):
    """(annotations of both views, gt_corrs, GT camera or None) of a dataset pair, or None when it lacks one of the first two."""
    if entry is None or "gt_corrs" not in entry or any("annotations" not in entry.get(v, {}) for v in "01"):
        return None
    return [entry["0"]["annotations"], entry["1"]["annotations"]], entry["gt_corrs"], entry.get("rel_pose")


def evaluate_for_reconstruction(predictions: List[dict], dataset_dict: Dict[str, dict], device, camera_key: str = "camera",
                                assignment_key: str = "pred_assignment", pairs_per_launch: int = 64,
                                gt_polygons: bool = False) -> Dict[str, float]:
    """The reconstruction AP table of the reference's offline `eval.py --evaluate AP` over kept prediction records: predictions = per
    pair {"0" / "1": {"image_id", "instances", "pred_plane"}, camera_key: {"pred": {"tran", "rot"}, "gts": {"tran", "rot"}},
    assignment_key: 0 / 1 matrix} (PoseEvaluator.prediction_record; the camera and assignment optimized_dict writes to continuous.pkl),
    dataset_dict = {"<id0>__<id1>": {"0" / "1": {"annotations"}, "gt_corrs", "rel_pose"?}} (the shape evaluate_for_matchings takes).
    The GT camera is the record's "gts" when it has one, else the dataset pair's `rel_pose`.  A pair without dataset entry, `gt_corrs`,
    `annotations` or GT camera is skipped and counted.  pairs_per_launch bounds the bit masks resident on the device at once (a split
    of a thousand pairs at 480 x 640 would be gigabytes in one piece); the rows do not depend on it.  gt_polygons=True: annotations may
    carry polygon lists instead of RLE dicts (recon_rows).  Returns recon_table's dict plus "pairs" and "skipped"."""
    rows, npos, todo, skipped = [], 0, [], 0
    for pred in predictions:
        gt = _recon_gt(dataset_dict.get(pred["0"]["image_id"] + "__" + pred["1"]["image_id"]))
        cam = pred.get(camera_key)
        gts = (cam or {}).get("gts") or {}
        gt_cam = {"tran": gts["tran"], "rot": gts["rot"]} if gts.get("tran") is not None and gts.get("rot") is not None else (gt[2] if gt else None)
        if gt is None or cam is None or gt_cam is None or assignment_key not in pred:
            skipped += 1
            continue
        todo.append(_recon_pair((pred["0"], pred["1"]), gt[0], cam["pred"], gt_cam, pred[assignment_key], gt[1], "evaluate_for_reconstruction",
                                gt_polygons))
    for i in range(0, len(todo), max(1, pairs_per_launch)):
        r, _, n_ge = recon_rows(todo[i:i + pairs_per_launch], device, gt_polygons=gt_polygons)
        rows.append(r)
        npos += int(n_ge.sum())
    table = recon_table(np.concatenate(rows) if rows else np.zeros((0, len(RECON_ROW_COLS))), npos)
    table.update(pairs=len(todo), skipped=skipped)
    return table


class ReconEvaluator:
    """DatasetEvaluator-style reconstruction AP: reset() / process(inputs, outputs) / evaluate() -> recon_table's dict plus "pairs" and
    "skipped".  process() runs decode, IoU and the per-pair kernel for the whole batch in one set of launches (recon_rows); a pair
    without `rel_pose`, `gt_corrs` or `annotations` in both views is skipped and counted.  Ranks hold disjoint pairs, so nothing is
    de-duplicated: every row carries its pair's number (pair_index["<id0>__<id1>"] - the pair's index in the dataset - when given) and
    its entry index, evaluate() gathers rows and per-pair GT entry counts from all ranks and orders the rows by (pair, entry), so
    equal scores rank the same at every world size.  A single process may leave pair_index out (pairs are numbered as they come);
    several ranks need it (ValueError).  gt_polygons=True: annotations may carry polygon lists instead of RLE dicts (recon_rows)."""

    def __init__(self, device, camera_key: str = "camera", assignment_key: str = "pred_assignment",
                 pair_index: Optional[Dict[str, int]] = None, gt_polygons: bool = False):
        self.device = torch.device(device)
        self.gt_polygons = bool(gt_polygons)
        self.camera_key, self.assignment_key, self.pair_index = camera_key, assignment_key, pair_index
        self.reset()

    def reset(self):
        self._rows: List[np.ndarray] = []           # [n, 10]: RECON_ROW_COLS + pair number + entry index
        self._gt: List[np.ndarray] = []             # [m, 2]: pair number, GT entry count
        self._skipped = 0
        self._count = 0

    def _number(self, key: str) -> float:
        if self.pair_index is not None:
            return float(self.pair_index[key])
        if _world() > 1:
            raise ValueError("ReconEvaluator: with several ranks pass pair_index ('<id0>__<id1>' -> index in the dataset), the same on "
                             "every rank")
        self._count += 1
        return float(self._count - 1)

    def _add(self, numbers, rows: np.ndarray, n_entries, n_gt_entries):
        """Rows of a batch (recon_rows' results) under their pairs' numbers."""
        num = np.repeat(np.asarray(numbers, np.float64), n_entries)
        ent = np.concatenate([np.arange(k, dtype=np.float64) for k in n_entries]) if len(n_entries) else np.zeros(0)
        self._rows.append(np.concatenate([rows, num[:, None], ent[:, None]], 1))
        self._gt.append(np.stack([np.asarray(numbers, np.float64), np.asarray(n_gt_entries, np.float64)], 1))

    def process(self, inputs: List[dict], outputs: List[dict]):
        todo, numbers = [], []
        for inp, out in zip(inputs, outputs):
            gt = _recon_gt(inp)
            cam = out.get(self.camera_key)
            if gt is None or gt[2] is None or cam is None or self.assignment_key not in out:
                self._skipped += 1
                continue
            views = tuple(out[v] if out.get(v) is not None else {"instances": [], "pred_plane": np.zeros((0, 3), np.float32)} for v in "01")
            todo.append(_recon_pair(views, gt[0], cam, gt[2], out[self.assignment_key], gt[1], "ReconEvaluator", self.gt_polygons))
            numbers.append(self._number(str(inp["0"].get("image_id")) + "__" + str(inp["1"].get("image_id"))))
        if todo:
            self._add(numbers, *recon_rows(todo, self.device, gt_polygons=self.gt_polygons))

    def evaluate(self) -> Dict[str, float]:
        w = len(RECON_ROW_COLS) + 2
        rows = np.concatenate(self._rows) if self._rows else np.zeros((0, w), np.float64)
        gts = np.concatenate(self._gt) if self._gt else np.zeros((0, 2), np.float64)
        gts = np.concatenate([gts, [[-1.0, float(self._skipped)]]])              # (the rank's skipped pairs ride along under number -1)
        dev = self.device if _nccl() else torch.device("cpu")
        rows, gts = np.concatenate(gather_rows(rows, dev)), np.concatenate(gather_rows(gts, dev))
        rows = rows[np.lexsort((rows[:, w - 1], rows[:, w - 2]))]
        counted = gts[gts[:, 0] >= 0]
        table = recon_table(rows[:, :len(RECON_ROW_COLS)], float(counted[:, 1].sum()))
        table.update(pairs=int(len(counted)), skipped=int(gts[gts[:, 0] < 0, 1].sum()))
        return table


def optimized_dict(predictions: List[dict]) -> Dict[int, dict]:
    """`get_optimized_dict` (mp3d_evaluation.py:259-313): the `continuous.pkl` schema read by eval.py:1027-1038."""
    ret = {}
    for idx, p in enumerate(predictions):
        best = p["pred_assignment"].numpy()
        cam = p["camera"]
        ret[idx] = {
            "n_corr": best.sum(), "cost": 0.1,
            "best_camera": {"position": cam["pred"]["tran"], "rotation": cam["pred"]["rot"]},
            "gt_camera": {"position": cam["gts"]["tran"], "rotation": cam["gts"]["rot"]},
            "best_assignment": best,
            "plane_param_override": {"0": p["0"]["pred_plane"].cpu().numpy(), "1": p["1"]["pred_plane"].cpu().numpy()},
            "image_ids": {"0": p["0"]["image_id"], "1": p["1"]["image_id"]},
        }
    return ret


def dump_predictions(predictions: List[dict], output_dir: str) -> Dict[str, str]:
    """Rank-0 side of `eval_full_scene` (mp3d_evaluation.py:330-341).  With a process group the per-rank lists are
    concatenated in rank order first (comm.gather semantics, :317-319); non-zero ranks return {}."""
    if _world() > 1:
        parts = [None] * _world()
        torch.distributed.all_gather_object(parts, predictions)
        if torch.distributed.get_rank() != 0:
            return {}
        predictions = [p for part in parts for p in part]
    os.makedirs(output_dir, exist_ok=True)
    inst = os.path.join(output_dir, "NopeSAC_instances_predictions.pth")
    torch.save(predictions, inst)
    cont = os.path.join(output_dir, "continuous.pkl")
    with open(cont, "wb") as f:
        pickle.dump(optimized_dict(predictions), f)
    return {"instances_predictions": inst, "continuous": cont}


def create_small_table(d: Dict[str, float]) -> str:
    keys, vals = list(d), ["%.4f" % d[k] for k in d]
    w = [max(len(k), len(v)) for k, v in zip(keys, vals)]
    return "\n".join(["| " + " | ".join(k.ljust(x) for k, x in zip(keys, w)) + " |",
                      "|" + "|".join("-" * (x + 2) for x in w) + "|",
                      "| " + " | ".join(v.ljust(x) for v, x in zip(vals, w)) + " |"])
