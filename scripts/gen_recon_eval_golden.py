"""Pin the two-view reconstruction AP to the reference: run the reference's offline evaluator (eval.py --evaluate AP) on the seeded
cases of tests/recon_eval_inputs.py and write tests/golden/K_recon_eval_<seed>.npz.  CPU only.  Compiled from the reference tree, each
on its own because eval.py imports detectron2, pycocotools and numpy-quaternion: the module-level functions evaluate_by_idx,
inst_bench_image, inst_bench, VOCap (eval.py) and get_plane_params_in_global (utils/mesh_utils.py) with
oracle.ref_shim.load_reference_function, and the Evaluator methods evaluate_ap_by_idx, get_maskiou, get_maskiou_merged and
get_single2merge with the small AST step below, bound to a stand-in object that carries rcnn_data, dataset_dict, optimized_dict and
score_threshold.  Their namespace gets: the shim's run-merging mask IoU as `mask_util`, numpy with the removed aliases np.bool /
np.float and np.quaternion, scipy.linalg.eigh, a create_instances stand-in that keeps every instance, a quaternion stand-in
(from_float_array, as_rotation_matrix = q v q^-1 by Hamilton products), and eval.py's five criteria (its module-level EP_* lists) as numbers.

RESULTS ONLY (the inputs are regenerated from their seeds):
  ap [5], npos          the reference's table (fractions, its order: all, -offset, -normal, -mask, -normal-offset) and GT entry total;
  score [n], flags [n, 5]
                        per predicted entry, pair after pair in entry order, what the reference hands to inst_bench;
  err_<pair> [3, entries, GT entries]
                        the reference's err_offsets, err_normals and mask_iou of every pair;
  gap_offset, gap_normal, gap_iou, gap_ap [5]
                        the largest absolute gap between the reference's value and tests/recon_eval_ref.py on the same inputs - the
                        tests derive their tolerances from them (4 x the gap, floored at 1e-12).
The flags must equal the restatement's exactly (asserted).  Three situations the reference cannot run are bridged here and nowhere
else: a pair with empty gt_corrs gets an empty [0, 2] array (np.array([]) has no second axis for its `[:, i]`), a view without GT
gets an empty [0, 3] plane array for the same reason (the `np` the functions see turns an empty list into one), and a pair without any
prediction skips evaluate_ap_by_idx (its empty merged arrays do not broadcast against the GT's) and feeds evaluate_by_idx the
[0, GT entries] matrix of get_maskiou_merged, whose ndt == 0 branch only counts the GT entries.
Needs the reference tree (NOPESAC_REFERENCE_ROOT); nothing of the reference's text is committed.  Not imported by any test."""
import ast
import os
import sys
import types

import numpy as np
import torch
from scipy.linalg import eigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import recon_eval_inputs as RI  # noqa: E402
from tests import recon_eval_ref as REF  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
METHODS = ("evaluate_ap_by_idx", "get_maskiou", "get_maskiou_merged", "get_single2merge")


class Quat:
    def __init__(self, w, x, y, z):
        self.c = (float(w), float(x), float(y), float(z))

    def __mul__(self, o):
        a, b, c, d = self.c
        e, f, g, h = o.c
        return Quat(a * e - b * f - c * g - d * h, a * f + b * e + c * h - d * g, a * g - b * h + c * e + d * f, a * h + b * g - c * f + d * e)


def as_rotation_matrix(q):
    """Columns q e_k q^-1: q^-1 = conj(q) / |q|^2."""
    w, x, y, z = q.c
    n = w * w + x * x + y * y + z * z
    inv = Quat(w / n, -x / n, -y / n, -z / n)
    return np.array([(q * Quat(0, *e) * inv).c[1:] for e in np.eye(3)], np.float64).T


class NumpyWithOldAliases:
    bool, float, quaternion = bool, float, Quat

    def __getattr__(self, name):
        return getattr(np, name)

    def array(self, obj, *a, **k):
        """np.array, except that an empty list becomes a [0, 3] array: the plane list of a view without GT (see the module text)."""
        return np.zeros((0, 3)) if isinstance(obj, list) and len(obj) == 0 else np.array(obj, *a, **k)


def create_instances(predictions, image_size, pred_planes=None, conf_threshold=0.1):
    assert all(p["score"] > conf_threshold for p in predictions), "the reference is only defined when every score passes its threshold"
    return types.SimpleNamespace(scores=np.asarray([p["score"] for p in predictions], np.float64), pred_planes=pred_planes)


def load_methods(rel_path, cls, names, namespace):
    """Compile the named methods of class `cls` of a reference file as plain functions in `namespace`."""
    path = os.path.join(ref_shim.REFERENCE_ROOT, rel_path)
    tree = ast.parse(open(path).read(), filename=path)
    (node,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls]
    body = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), namespace)
    return {n: namespace[n] for n in names}


class EvaluatorStandIn:
    score_threshold = 0.1

    def __init__(self, pairs, methods):
        enc = lambda m: ref_shim._mask_encode(np.asfortranarray(m.astype(np.uint8)))      # noqa: E731
        self.rcnn_data, self.dataset_dict, self.optimized_dict = [], {}, {}
        for idx, p in enumerate(pairs):
            rec, entry = {}, {"gt_corrs": np.asarray(p["gt_corrs"], np.int64).reshape(-1, 2)}
            for v, image_id, view in zip("01", p["ids"], p["views"]):
                rec[v] = {"image_id": image_id, "pred_plane": torch.from_numpy(view["pred_plane"].copy()),
                          "instances": [{"segmentation": enc(m), "score": float(s)} for m, s in zip(view["pred"], view["score"])]}
                entry[v] = {"height": view["gt"].shape[1], "width": view["gt"].shape[2],
                            "annotations": [{"segmentation": enc(m), "plane": [float(x) for x in pl]} for m, pl in zip(view["gt"], view["gt_plane"])]}
            self.rcnn_data.append(rec)
            self.dataset_dict[p["ids"][0] + "__" + p["ids"][1]] = entry
            self.optimized_dict[idx] = {"best_assignment": p["assignment"], "best_camera": dict(p["pred_cam"]), "gt_camera": dict(p["gt_cam"]),
                                        "plane_param_override": {v: view["pred_plane"].astype(np.float32) for v, view in zip("01", p["views"])}}
        for name, fn in methods.items():
            setattr(self, name, types.MethodType(fn, self))

    def rcnnidx2datasetkey(self, idx):
        return self.rcnn_data[idx]["0"]["image_id"] + "__" + self.rcnn_data[idx]["1"]["image_id"]

    def get_gt_affinity(self, idx, rtnformat="list", gtbox=True):
        assert rtnformat == "list" and gtbox
        return self.dataset_dict[self.rcnnidx2datasetkey(idx)]["gt_corrs"]


def reference_functions():
    npx = NumpyWithOldAliases()
    quaternion = types.SimpleNamespace(from_float_array=lambda a: Quat(*np.asarray(a, np.float64).reshape(4)), as_rotation_matrix=as_rotation_matrix)
    ns = {"np": npx, "quaternion": quaternion, "eigh": eigh, "create_instances": create_instances,
          "mask_util": types.SimpleNamespace(iou=ref_shim._mask_iou, frPyObjects=None, merge=None),
          "EP_mask_delta_thresh": [0.5, 0.5, 0.5, 0.0, 0.5], "EP_normal_delta_thresh": [30.0, 30.0, 1000.0, 30.0, 1000.0],
          "EP_offset_delta_thresh": [1.0, 1000.0, 1.0, 1.0, 1000.0], "EP_ap_str": list(REF.CRITERIA)}
    ref_shim.load_reference_function("NopeSAC_Net/utils/mesh_utils.py", "get_plane_params_in_global", ns)
    for name in ("evaluate_by_idx", "inst_bench_image", "inst_bench", "VOCap"):
        ref_shim.load_reference_function("eval.py", name, ns)
    return ns, load_methods("eval.py", "Evaluator", METHODS, ns)


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not found at %s" % ref_shim.REFERENCE_ROOT)
    os.makedirs(GOLD, exist_ok=True)
    for seed in RI.SEEDS:
        pairs = RI.recon_eval_case(seed)
        ns, methods = reference_functions()
        ev = EvaluatorStandIn(pairs, methods)
        stats, errs = [], []
        for idx, p in enumerate(pairs):
            if sum(len(v["pred"]) for v in p["views"]) == 0:
                corr = np.zeros((0, 2), np.int64)
                e = {"mask_iou": ev.get_maskiou_merged(idx, pred_corr=corr, gt_corr=ev.get_gt_affinity(idx))}
                e["err_offsets"] = e["err_normals"] = e["mask_iou"]
            else:
                e = ev.evaluate_ap_by_idx(idx)
            errs.append(np.stack([e["err_offsets"], e["err_normals"], e["mask_iou"]]).astype(np.float64))
            stats.append(ns["evaluate_by_idx"](e))
        per_crit = list(zip(*stats))
        ap, npos, flags, score = [], None, [], None
        for k in range(len(REF.CRITERIA)):
            tp, fp, sc, num_inst, _, _, _ = zip(*per_crit[k])
            a, _, _, n, _ = ns["inst_bench"](None, None, None, tp, fp, sc, num_inst)
            ap.append(float(np.asarray(a).reshape(-1)[0]))
            assert npos is None or npos == n
            npos = n
            flags.append(np.vstack(tp).astype(np.float64).reshape(-1))
            assert np.array_equal(np.vstack(tp) ^ np.vstack(fp), np.ones_like(np.vstack(tp)))      # every entry is one or the other
            score = np.vstack(sc).astype(np.float64).reshape(-1)
        flags = np.stack(flags, 1)
        mine_rows, mine_nge, mine_errs = RI.reference_rows(pairs)
        assert np.array_equal(mine_rows[:, 0], score), "scores / order of the entries"
        assert np.array_equal(mine_rows[:, 1:6], flags), "flags differ from the restatement: it, or the reading of the reference, is wrong"
        assert int(npos) == sum(mine_nge)
        mine_table = REF.table(mine_rows, sum(mine_nge))
        gaps = np.zeros(3)
        for e, m in zip(errs, mine_errs):
            mine = np.stack([m["err_offsets"], m["err_normals"], m["mask_iou"]])
            assert mine.shape == e.shape, (mine.shape, e.shape)
            if e.size:
                gaps = np.maximum(gaps, np.abs(e - mine).reshape(3, -1).max(1))
        gap_ap = np.abs(np.asarray(ap) - np.asarray([mine_table[c] / 100.0 for c in REF.CRITERIA]))
        out = {"ap": np.asarray(ap, np.float64), "npos": np.float64(npos), "score": score, "flags": flags, "gap_offset": gaps[0],
               "gap_normal": gaps[1], "gap_iou": gaps[2], "gap_ap": gap_ap, **{f"err_{i}": e for i, e in enumerate(errs)}}
        np.savez_compressed(os.path.join(GOLD, f"K_recon_eval_{seed}.npz"), **out)
        print(f"seed {seed}: {len(score)} entries, npos {int(npos)}, flags equal to the restatement; gap offset {gaps[0]:.3g} normal {gaps[1]:.3g} "
              f"iou {gaps[2]:.3g} ap {gap_ap.max():.3g}")
        for c, a in zip(REF.CRITERIA, ap):
            print("{:>20s}: {:5.3f}".format(c, a * 100.0))


if __name__ == "__main__":
    main()
