"""Byte-for-byte A/B of the two-view evaluators and the mesh export: the seeded cases of the test input modules through
evaluation.plane_rows, evaluation.recon_rows(with_errors=True), rle.iou_device_views, ops.recon_mesh_merge and mesh.pair_meshes at
strides 1 and 2, one sha256 per result array.  Run it in a fresh process per build and compare the listings line by line:
  python scripts/two_view_ab.py                                   this tree, its library
  python scripts/two_view_ab.py --root <other checkout>           another checkout's Python and library on the same inputs
  NOPESAC_AB_LIBRARY=<other .so> python scripts/two_view_ab.py    this tree's Python over another build of the library
"""
import argparse
import hashlib
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from nopesac_amd import evaluation, mesh, ops, rle
    from tests import plane_eval_inputs as PI
    from tests import recon_eval_inputs as RI
    from tests import recon_mesh_inputs as MI
    device = torch.device("cuda")

    def line(name, a):
        a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
        print(f"{name} {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}")

    def views_of(pred, entry):
        return tuple({"instances": pred[v]["instances"], "pred_plane": pred[v]["pred_plane"], "annotations": entry[v]["annotations"]} for v in "01")

    for seed in (11, 12, 13):
        preds, dataset = PI.product_inputs(PI.plane_eval_case(seed, 48, 64))
        views = [v for pred, entry in zip(preds, dataset.values()) for v in views_of(pred, entry) if len(v["instances"])]
        line(f"plane_rows/{seed}", evaluation.plane_rows(views, device))
    for seed in (21, 22, 23):
        case = RI.recon_eval_case(seed, 48, 64)
        preds, dataset = RI.product_inputs(case)
        pairs = [{"views": views_of(pred, entry), "pred_camera": p["pred_cam"], "gt_camera": p["gt_cam"],
                  "pred_corrs": evaluation.assignment_corrs(p["assignment"]), "gt_corrs": p["gt_corrs"]}
                 for p, pred, entry in zip(case, preds, dataset.values())]
        rows, n_entries, n_gt_entries, errs = evaluation.recon_rows(pairs, device, with_errors=True)
        line(f"recon_rows/{seed}/rows", rows); line(f"recon_rows/{seed}/n_entries", n_entries)
        line(f"recon_rows/{seed}/n_gt_entries", n_gt_entries)
        for i, e in enumerate(errs):
            line(f"recon_rows/{seed}/errs{i}", e)
        jobs = [([ins["segmentation"] for ins in v["instances"]], [a["segmentation"] for a in v["annotations"]],
                 [j % 2 for j in range(len(v["annotations"]))] if k % 2 else None) for k, v in enumerate(v for p in pairs for v in p["views"])]
        for k, m in enumerate(rle.iou_device_views(jobs, device)):
            line(f"iou_device_views/{seed}/view{k}", m)
    for seed in (31, 32, 33):
        case = MI.recon_mesh_case(seed, 24, 32)
        counts = [len(v["planes"]) for p in case for v in p["views"]]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
        merged, bad = ops.recon_mesh_merge(
            dev(np.concatenate([v["planes"] for p in case for v in p["views"]]).astype(np.float32)), dev(np.concatenate([[0], np.cumsum(counts)])),
            dev(np.stack([np.concatenate([p["camera"]["position"], p["camera"]["rotation"]]) for p in case])),
            dev(np.concatenate([np.asarray(p["corrs"], np.int32).reshape(-1) for p in case])),
            dev(np.concatenate([[0], np.cumsum([len(p["corrs"]) for p in case])])), max(counts))
        line(f"recon_mesh_merge/{seed}/merged", merged); line(f"recon_mesh_merge/{seed}/bad", bad)
        for stride in (1, 2):
            for i, m in enumerate(mesh.pair_meshes(MI.product_pairs(case), device, stride=stride)):
                for k in ("verts", "uvs", "faces", "vert_off", "face_off", "planes"):
                    line(f"pair_meshes/{seed}/stride{stride}/pair{i}/{k}", getattr(m, k))


if __name__ == "__main__":
    main()
