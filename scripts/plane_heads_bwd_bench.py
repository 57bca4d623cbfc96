"""Backward of the plane head's instance heads at the workload's shape (csrc/plane_head_bwd.hip): B = 32 images, L = 3 supervised
layers, nq = 50, a 120 x 160 map of 256 channels.  Times one PlaneInstanceHeadsTrainer.losses call forward + backward (hs and p1 asking
for gradients), each of the two product launches alone (ops.mask_product_backward which="wgrad" / "dgrad", centre rows included), and the
float32 torch restatement of the same two products on the same GPU as the yardstick.  For each launch also its compulsory bytes (every
operand read once, every result written once) divided by its time.  Warm-up, then the median of `--reps` event-timed runs.  Prints one JSON
line and writes profiles/plane_heads_bwd_times.json.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from nopesac_amd.training import PlaneInstanceHeadsTrainer  # noqa: E402
from tests import plane_criterion_inputs as PI  # noqa: E402


def timed(fn, reps, warmup=2):
    """median of `reps` single runs (ms), each between two events, after `warmup` runs"""
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
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_heads_bwd_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, nq, h, w, C = a.batch, a.layers, 50, 120, 160, 256
    hw = h * w
    g = torch.Generator().manual_seed(5)
    hs = torch.randn(L, B, nq, C, generator=g).to(dev).requires_grad_(True)
    p1 = torch.relu(torch.randn(B, h, w, C, generator=g)).to(dev).requires_grad_(True)
    _, t = PI.cast(*PI.make("real"), torch.float32, dev)                 # one 480 x 640 image with 12 planes, repeated over the batch
    rep = lambda x: x.expand(B, *x.shape[1:]).contiguous()
    targets = {"masks": rep(t["masks"]), "n": torch.tensor(t["n"] * B, dtype=torch.int32), "plane_params": rep(t["plane_params"]),
               "depth": rep(t["depth"]), "k_inv_dot_xy1": rep(t["k_inv_dot_xy1"])}
    tr = PlaneInstanceHeadsTrainer.from_state_dict(synth_state_dict(nq), nq, dev)

    def fwd_bwd():
        tr.backward(tr.losses(hs, p1, targets)[0])

    def fwd():
        with torch.no_grad():
            tr.losses(hs, p1, targets)

    dM = torch.randn(L, B, nq, h, w, generator=g).to(dev)
    dZ = torch.randn(B, 2, h, w, generator=g).to(dev)
    F = torch.randn(L * B * nq, C, generator=g).to(dev)
    wc = torch.randn(2, C, generator=g).to(dev)
    x = p1.detach()
    S = ops.mask_product_splits(L, B, nq, hw, 2)
    ws_bytes = 4 * ops.mask_product_workspace_floats(L, B, nq, 2, S)
    wgrad = lambda: ops.mask_product_backward(dM, F, x, dZ, wc, which="wgrad")
    dgrad = lambda: ops.mask_product_backward(dM, F, x, dZ, wc, which="dgrad")
    dM4, x3, F4 = dM.view(L, B, nq, hw), x.view(B, hw, C), F.view(L, B, nq, C)

    def torch_wgrad():
        return (torch.einsum("lbqp,bpk->lbqk", dM4, x3), dM4.sum(-1), torch.einsum("bcp,bpk->ck", dZ.view(B, 2, hw), x3), dZ.sum((0, 2, 3)))

    def torch_dgrad():
        return torch.einsum("lbqp,lbqk->bpk", dM4, F4) + torch.einsum("bcp,ck->bpk", dZ.view(B, 2, hw), wc)

    operand = 4 * (dM.numel() + dZ.numel())
    nbytes = {"wgrad": operand + 4 * x.numel() + 4 * (F.numel() + L * B * nq + wc.numel() + 2), "dgrad": operand + 4 * (F.numel() + wc.numel()) + 4 * x.numel()}
    out = {"batch": B, "layers": L, "nq": nq, "h": h, "w": w, "device": torch.cuda.get_device_name(0), "wgrad_splits": S,
           "wgrad_workspace_bytes": ws_bytes, "gflop_per_product": 2e-9 * B * (L * nq + 2) * hw * C}
    for key, fn in (("losses_fwd_bwd_ms", fwd_bwd), ("losses_fwd_ms", fwd), ("wgrad_ms", wgrad), ("dgrad_ms", dgrad), ("torch_wgrad_ms", torch_wgrad),
                    ("torch_dgrad_ms", torch_dgrad)):
        med, lo, hi = timed(fn, a.reps)
        out[key] = med
        out[key + "_min_max"] = [lo, hi]
    for k in ("wgrad", "dgrad"):
        out[k + "_compulsory_bytes"] = nbytes[k]
        out[k + "_gb_per_s"] = nbytes[k] / (out[k + "_ms"] * 1e-3) / 1e9
        out[k + "_tflops"] = out["gflop_per_product"] / out[k + "_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
