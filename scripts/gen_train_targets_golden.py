"""Pin the training-target restatement (tests/train_targets_forms.py) to the reference: run the reference's own prepare_targets (a method of
PlaneTR_NopeSAC, called on a stand-in `self` that carries the five attributes it reads) and get_coordinate_map
(modeling/meta_arch/siamese_planeTR.py, imported through oracle.ref_shim.install) on the seeded label maps of forms.GOLDEN_CASES, and write
tests/golden/train_targets/<case>.npz.  RESULTS ONLY (the inputs are regenerated from their seeds):
  n, masks (bit-packed), labels, plane_params, plane_centers, pixel_centers, k_inv_dot_xy1
                     what the reference returns for the view (at most 50 planes);
  gap_plane_centers, gap_pixel_centers, gap_k_inv_dot_xy1 [3]
                     the largest absolute gap between the reference's value (f32 sums over an f32 x / W map; an f32 matrix inverse and
                     matmul) and the float64 restatement on these very inputs - per channel for the coordinate map, whose third
                     channel is 1 and whose first two are not.  The tests derive their tolerances from them.
Needs the reference tree (NOPESAC_REFERENCE_ROOT); the fixtures it writes are committed, nothing of the reference's text is.  Not imported
by any test, smoke() or bench.py."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import train_targets_forms as F  # noqa: E402


class Instances:
    def __init__(self, classes, planes):
        self.gt_classes, self.gt_planes = torch.as_tensor(classes), torch.as_tensor(planes, dtype=torch.float32)

    def __len__(self):
        return len(self.gt_classes)


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not found at %s" % ref_shim.REFERENCE_ROOT)
    from oracle.d2_resnet import build_resnet50_backbone
    ref_shim.install(build_resnet50_backbone)
    import NopeSAC_Net.modeling  # noqa: F401
    from NopeSAC_Net.modeling.meta_arch import siamese_planeTR as M
    os.makedirs(F.GOLD, exist_ok=True)
    for name in F.GOLDEN_CASES:
        labels, K = F.golden_case(name)
        H, W = labels.shape
        ids = F.unique_ids(labels)
        rng = np.random.default_rng(len(ids))
        planes = rng.normal(size=(len(ids), 3)).astype(np.float32)
        me = types.SimpleNamespace(device=torch.device("cpu"),
                                   cfg=ref_shim.CfgNode(MODEL=ref_shim.CfgNode(SEM_SEG_HEAD=ref_shim.CfgNode(CENTER_ON=True, PARAM_ON=True))))
        M.PlaneTR_NopeSAC.precompute_xy_map(me, h=H, w=W)
        me.pre_defined_k_inv_dot_xy1 = M.get_coordinate_map(device=me.device, h=H, w=W)
        view = {"instances": Instances(np.zeros(len(ids), np.int64), planes), "semantic_map": torch.from_numpy(labels),
                "depth": torch.ones(H, W)}
        if K is not F.DEFAULT_K:
            view["camera_K"] = K.astype(np.float64)
        t = M.PlaneTR_NopeSAC.prepare_targets(me, [view], types.SimpleNamespace(tensor=torch.zeros(1, 3, H, W)))[0]
        n = int(t["masks"].shape[0])
        masks = t["masks"].numpy().astype(np.uint8)
        # the float64 restatement on the same input
        r_ids, r_n_all, r_n, bad = F.label_ids(labels[None], 1024)
        assert not bad[0] and int(r_n[0]) == n and int(r_n_all[0]) == len(ids)
        r_masks, r_centers, r_pixel = F.label_targets(labels[None], r_ids, r_n, n)
        assert np.array_equal(r_masks[0], masks), name
        c64 = F.centers64(r_masks, r_n)[0]
        p64 = (c64[:, :, None, None] * r_masks[0][:, None].astype(np.float64)).sum(0)
        k64, _ = F.coordinate_map(K, H, W)
        centers, pixel, kmap = t["plane_centers"].numpy(), t["pixel_centers"].numpy(), t["k_inv_dot_xy1"].numpy()
        out = {"n": np.int32(n), "masks": np.packbits(masks.reshape(n, -1), axis=1), "labels": t["labels"].numpy(),
               "plane_params": t["plane_params"].numpy(), "plane_centers": centers, "pixel_centers": pixel, "k_inv_dot_xy1": kmap,
               "gap_plane_centers": np.abs(centers.astype(np.float64) - c64).max(), "gap_pixel_centers": np.abs(pixel.astype(np.float64) - p64).max(),
               "gap_k_inv_dot_xy1": np.abs(kmap.astype(np.float64) - k64).reshape(3, -1).max(1)}
        assert np.array_equal(out["plane_params"], planes[:n])
        np.savez_compressed(os.path.join(F.GOLD, name + ".npz"), **out)
        print(f"{name}: {H}x{W}, n = {n} of {len(ids)}, gap centres {out['gap_plane_centers']:.3g}, centre map {out['gap_pixel_centers']:.3g}, "
              f"coordinate map {out['gap_k_inv_dot_xy1']}")


if __name__ == "__main__":
    main()
