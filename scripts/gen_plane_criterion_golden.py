"""Pin tests/plane_criterion_ref.py to the reference: run the reference's HungarianMatcher + SetCriterion (imported through
oracle.ref_shim.install, on the CPU, in float64, built with the default config's weights) on the seeded inputs of
tests/plane_criterion_inputs.py and write tests/golden/H_plane_criterion_<case>.npz: the Hungarian indices of every layer, the loss values
and the gradients of the summed weighted loss at the five outputs.  Outputs only - the inputs are regenerated from their seeds.  Needs the
reference tree (NOPESAC_REFERENCE_ROOT); the fixtures it writes are committed, nothing of the reference's text is."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import plane_criterion_inputs as PI  # noqa: E402
from tests import plane_criterion_ref as R  # noqa: E402

OUT_KEYS = ("pred_logits", "pred_mask_logits", "pred_centers", "pred_params", "pixel_centers")


def main():
    from oracle.d2_resnet import build_resnet50_backbone
    ref_shim.install(build_resnet50_backbone)
    from NopeSAC_Net.modeling.criterion import SetCriterion
    from NopeSAC_Net.modeling.matcher import HungarianMatcher
    from nopesac_amd.config import get_cfg
    from nopesac_amd.training import PlaneCriterion
    ours = PlaneCriterion.from_cfg(get_cfg())
    w, wd = ours.weights, ours.weight_dict
    for name in PI.GOLDEN_CASES:
        outputs, targets = PI.make(name)
        layers = [outputs] + list(outputs.get("aux_outputs", []))
        leaves = [(l, k, o[k].requires_grad_(True)) for l, o in enumerate(layers) for k in OUT_KEYS if k in o]
        centers, pixel = R.prepare_targets(targets["masks"], targets["n"], torch.float64)
        n = targets["n"]
        tg = [{"labels": torch.zeros(n[b], dtype=torch.int64), "masks": targets["masks"][b, : n[b]].bool(), "plane_centers": centers[b, : n[b]],
               "pixel_centers": pixel[b], "plane_params": targets["plane_params"][b, : n[b]], "depth": targets["depth"][b],
               "k_inv_dot_xy1": targets["k_inv_dot_xy1"][b]} for b in range(len(n))]
        matcher = HungarianMatcher(cost_class=w["cost_class"], cost_mask=w["cost_mask"], cost_dice=w["cost_dice"], cost_center=w["cost_center"],
                                   cost_param=w["cost_param"], cost_param_offset=w["cost_offset"], cost_param_normal_angle=w["cost_angle"],
                                   param_on=True)
        crit = SetCriterion(num_classes=1, matcher=matcher, weight_dict=wd, eos_coef=w["eos_coef"], losses=["labels", "masks", "centers", "params"],
                            losses_aux=["labels", "masks", "centers", "params"]).to(torch.float64)
        losses, _ = crit(outputs, tg)
        indices = [matcher(o, tg) for o in layers]
        total = sum(v * wd[k] for k, v in losses.items() if k in wd)
        grads = torch.autograd.grad(total, [v for _, _, v in leaves])
        rec = {"loss_names": np.array(sorted(losses)), "loss_values": np.array([float(losses[k].detach()) for k in sorted(losses)], dtype=np.float64)}
        for l, per in enumerate(indices):
            for b, (s, t) in enumerate(per):
                rec["src_%d_%d" % (l, b)], rec["tgt_%d_%d" % (l, b)] = s.numpy(), t.numpy()
        for (l, k, _), g in zip(leaves, grads):
            rec["grad_%d_%s" % (l, k)] = g.numpy()
        path = os.path.join(ROOT, "tests", "golden", "H_plane_criterion_%s.npz" % name)
        np.savez_compressed(path, **rec)
        print(name, len(losses), "losses ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
