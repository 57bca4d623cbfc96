"""Pin the plane detection evaluator to the reference: run the reference's evaluate_for_planes (evaluation/mp3d_evaluation.py) with
its compare_planes (utils/metrics.py) and VOCap.compute_ap / xVOCap (utils/VOCap.py) - each compiled from its file on its own with
oracle.ref_shim.load_reference_function, because the modules import COCO tooling and visualisers - on the seeded cases of
tests/plane_eval_inputs.py, and write tests/golden/J_plane_eval_<seed>.npz.  RESULTS ONLY (the inputs are regenerated from their seeds):
  keys / values      the reference's table;
  score, flags [n,4], normal, offset
                     the per-prediction lists in the reference's order (unique views one after the other, each view's predictions
                     by descending score): what it hands to compute_ap for the four criteria and averages for the error statistics;
  gap_normal, gap_offset, gap_values
                     the largest absolute gap between the reference's value (float32 norms / cdist / asin, float32 cumulative sums)
                     and the float64 restatement of the same formula in tests/plane_eval_ref.py, on these very inputs - the tests
                     derive their tolerances from them.
The reference function gets: the shim's run-merging mask IoU and encoder as `mask_util`, a small stand-in for the COCO API object,
metadata.thing_dataset_id_to_contiguous_id = {1: 0} and a silent logger.  Needs the reference tree (NOPESAC_REFERENCE_ROOT); the
fixtures it writes are committed, nothing of the reference's text is.  Not imported by any test, smoke() or bench.py."""
import logging
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import plane_eval_inputs as PI  # noqa: E402
from tests import plane_eval_ref as REF  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


class CocoStandIn:
    """The part of pycocotools.coco.COCO the function touches."""

    def __init__(self, views):
        self.images, self.anns, self.by_image = {}, {}, {}
        for image_id, view in views:
            h, w = view["gt"].shape[1:]
            self.images[image_id] = {"id": image_id, "height": h, "width": w}
            self.by_image[image_id] = []
            for m, plane, cat in zip(view["gt"], view["gt_plane"], view["gt_label"]):
                ann = {"id": len(self.anns) + 1, "image_id": image_id, "category_id": int(cat), "plane": [float(x) for x in plane],
                       "segmentation": ref_shim._mask_encode(np.asfortranarray(m.astype(np.uint8)))}
                self.anns[ann["id"]] = ann
                self.by_image[image_id].append(ann["id"])
        self.dataset = {"annotations": list(self.anns.values()), "images": list(self.images.values()),
                        "categories": [{"id": 1, "name": "plane"}]}

    def getCatIds(self):
        return [1]

    def loadCats(self, ids):
        return [c for c in self.dataset["categories"] if c["id"] in ids]

    def loadImgs(self, ids):
        return [self.images[i] for i in ids]

    def getAnnIds(self, imgIds):
        return [a for i in imgIds for a in self.by_image[i]]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


class Recording:
    """`np` as the function sees it: numpy, with the lists it turns into arrays kept (its last two are the error lists, :722-723)."""

    def __init__(self):
        self.arrays = []

    def __getattr__(self, name):
        return getattr(np, name)

    def array(self, obj, *a, **k):
        out = np.array(obj, *a, **k)
        self.arrays.append(out)
        return out


def reference_functions():
    from nopesac_amd.evaluation import create_small_table
    ap_ns = {"torch": torch}
    ref_shim.load_reference_function("NopeSAC_Net/utils/VOCap.py", "xVOCap", ap_ns)
    compute_ap = ref_shim.load_reference_function("NopeSAC_Net/utils/VOCap.py", "compute_ap", ap_ns)
    compare_planes = ref_shim.load_reference_function("NopeSAC_Net/utils/metrics.py", "compare_planes", {"torch": torch, "np": np})
    calls = []

    def recorded_ap(scores, labels, npos, device=None):
        calls.append((scores.detach().cpu().numpy().astype(np.float64), labels.detach().cpu().numpy().astype(np.float64)))
        return compute_ap(scores, labels, npos, device)
    rec = Recording()
    ns = {"np": rec, "torch": torch, "compare_planes": compare_planes, "create_small_table": create_small_table,
          "VOCap": types.SimpleNamespace(compute_ap=recorded_ap, xVOCap=ap_ns["xVOCap"]),
          "mask_util": types.SimpleNamespace(iou=ref_shim._mask_iou, encode=ref_shim._mask_encode, frPyObjects=None, merge=None)}
    fn = ref_shim.load_reference_function("NopeSAC_Net/evaluation/mp3d_evaluation.py", "evaluate_for_planes", ns)
    return fn, calls, rec


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not found at %s" % ref_shim.REFERENCE_ROOT)
    log = logging.getLogger("gen_plane_eval_golden.null")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    os.makedirs(GOLD, exist_ok=True)
    for seed in PI.SEEDS:
        pairs = PI.plane_eval_case(seed)
        views = PI.unique_views(pairs)
        fn, calls, rec = reference_functions()
        predictions = [{"image_id": image_id, "pred_plane": view["pred_plane"].tolist(),
                        "instances": [{"score": float(s), "category_id": int(c), "segmentation": ref_shim._mask_encode(np.asfortranarray(m.astype(np.uint8)))}
                                      for m, s, c in zip(view["pred"], view["score"], view["label"])]} for image_id, view in views]
        table = fn(predictions, CocoStandIn(views), types.SimpleNamespace(thing_dataset_id_to_contiguous_id={1: 0}), _logger=log)
        assert len(calls) == 4, len(calls)                     # one category, four criteria
        score = calls[0][0]
        assert all(np.array_equal(c[0], score) for c in calls)
        flags = np.stack([c[1] for c in calls], 1)
        normal, offset = rec.arrays[-2].astype(np.float64), rec.arrays[-1].astype(np.float64)
        assert normal.shape == offset.shape == score.shape
        # float64 restatement on the same inputs, same order
        mine = PI.reference_order_rows(pairs)
        assert np.array_equal(mine[:, 0], score), "order of the predictions"
        mine_table = REF.table(mine, PI.npos_of(pairs))
        assert list(mine_table) == list(table), (list(mine_table), list(table))
        keys = list(table)
        values = np.asarray([float(table[k]) for k in keys], np.float64)
        gaps = np.abs(values - np.asarray([mine_table[k] for k in keys]))
        out = {"keys": np.asarray(keys), "values": values, "score": score, "flags": flags, "normal": normal, "offset": offset,
               "gap_normal": np.abs(normal - mine[:, 6]).max(), "gap_offset": np.abs(offset - mine[:, 7]).max(), "gap_values": gaps}
        np.savez_compressed(os.path.join(GOLD, f"J_plane_eval_{seed}.npz"), **out)
        print(f"seed {seed}: {len(score)} predictions, flags equal to the restatement: {np.array_equal(flags, mine[:, 2:6])}, "
              f"gap normal {out['gap_normal']:.3g} offset {out['gap_offset']:.3g} table {gaps.max():.3g}")
        for k, v, g in zip(keys, values, gaps):
            print(f"   {k:48s} {v:.9g}   gap {g:.3g}")


if __name__ == "__main__":
    main()
