"""The plane criterion at the production shape (csrc/plane_criterion.hip): L = 3 supervised layers, B = 32, nq = 50, 120x160 -> 480x640, forward
(targets, costs, assignment, losses) + backward of the weighted sum through PlaneCriterion, next to the f32 torch restatement of the tests
(tests/plane_criterion_ref.py, given the device's indices so that scipy stays out of its time) on the same GPU.  Warm-up, then the median
of `--reps` event-timed runs.  Prints both figures and one JSON line.  `--batch N` changes B."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd.config import get_cfg  # noqa: E402
from nopesac_amd.training import PlaneCriterion  # noqa: E402
from tests import plane_criterion_ref as R  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L, B, nq, h, w, s = 3, a.batch, 50, 120, 160, 4
    H, W = s * h, s * w
    g = torch.Generator().manual_seed(0)
    n = [int(v) for v in torch.randint(5, 31, (B,), generator=g)]
    nmax = max(n)
    own = torch.randint(0, nmax + 2, (B, H // 16, W // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    masks = torch.stack([torch.stack([(own[b] == j) & (j < n[b]) for j in range(nmax)]) for b in range(B)]).to(torch.uint8).to(dev)
    for b in range(B):
        masks[b, torch.arange(n[b]), 0, torch.arange(n[b])] = 1                       # no empty plane
    r = lambda *shape: torch.rand(*shape, generator=g).to(dev)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    targets = {"masks": masks, "n": torch.tensor(n, dtype=torch.int32), "plane_params": rn(B, nmax, 3) + 2.0, "depth": 1.0 + r(B, H, W),
               "k_inv_dot_xy1": torch.cat([r(B, 2, H, W) - 0.5, torch.ones(B, 1, H, W, device=dev)], 1)}

    def layer(pixel):
        o = {"pred_logits": rn(B, nq, 2), "pred_mask_logits": 2 * rn(B, nq, h, w), "pred_centers": r(B, nq, 2), "pred_params": rn(B, nq, 3) + 2.0}
        if pixel:
            o["pixel_centers"] = r(B, 2, h, w)
        return {k: v.requires_grad_(True) for k, v in o.items()}
    layers = [layer(True)] + [layer(False) for _ in range(L - 1)]
    leaves = [v for o in layers for v in o.values()]
    outputs = dict(layers[0], aux_outputs=layers[1:])
    crit = PlaneCriterion.from_cfg(get_cfg())
    state = {}

    def hip():
        losses, state["indices"] = crit(outputs, targets)
        torch.autograd.grad(sum(crit.weighted(losses).values()), leaves)
    t_hip = timed(hip, a.reps)
    idx = [crit.indices_as_reference(state["indices"], l) for l in range(L)]
    t_ref = dict(targets, n=n)
    ref_out = outputs

    class OnDevice:
        """the restatement creates its small constants on the CPU: run it under the device as default"""
        def __enter__(self):
            torch.set_default_device(dev)
        def __exit__(self, *a):
            torch.set_default_device("cpu")

    def torch32():
        with OnDevice():
            losses, _, _ = R.criterion(ref_out, t_ref, crit.weights, indices=[[(s_.to(dev), t_.to(dev)) for s_, t_ in per] for per in idx])
            torch.autograd.grad(sum(v * crit.weight_dict[k] for k, v in losses.items()), leaves)
    t_torch = timed(torch32, max(a.reps // 2, 1), warmup=1)
    print("plane criterion fwd+bwd, L=%d B=%d nq=%d %dx%d -> %dx%d: HIP %.2f ms, f32 torch restatement %.2f ms" % (L, B, nq, h, w, H, W, t_hip, t_torch))
    print(json.dumps({"L": L, "B": B, "nq": nq, "hip_ms": round(t_hip, 3), "torch_f32_ms": round(t_torch, 3), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
