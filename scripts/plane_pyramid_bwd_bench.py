"""Training step of the plane head's top-down pyramid at the workload's shape (csrc/pyramid_train.hip): B = 32 images, res5 at 15 x 20,
p1 at 120 x 160.  Times one PlanePyramidTrainer.forward + backward_from (feature gradients off: the backbone is frozen), the forward
alone, every new launch alone at the finest level's shape (n = B 120 160 rows of 256 channels: the c1 lateral in the plain form, up_conv1
in the upsampled form with t at 60 x 80) beside the HBM bytes it cannot avoid, and, as the yardstick on the same GPU, the float32 torch
restatement of the whole pyramid under autograd (tests/plane_pyramid_forms.pyramid_forward: the reference's operation order).  Warm-up,
then the median of `--reps` event-timed runs.  Prints one JSON line and writes profiles/plane_pyramid_bwd_times.json.  Nothing is gated
on these numbers."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from nopesac_amd.training import PlanePyramidTrainer  # noqa: E402
from tests import plane_pyramid_forms as P  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_pyramid_bwd_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, h, w, C = a.batch, 15, 20, 256
    g = torch.Generator().manual_seed(5)
    feats = {k: torch.relu(torch.randn(B, f * h, f * w, c, generator=g)).to(dev) for k, f, c in (("res5", 1, 2048), ("res4", 2, 1024), ("res3", 4, 512), ("res2", 8, 256))}
    memory = torch.randn(B * h * w, 256, generator=g).to(dev)
    tr = PlanePyramidTrainer.from_state_dict(synth_state_dict(7), dev)
    H1, W1 = 8 * h, 8 * w
    d_p1 = (torch.randn(B, H1, W1, C, generator=g) / 16).to(dev)

    def fwd_bwd():
        tr.forward(feats, memory, B)
        tr.backward_from(d_p1)

    def fwd():
        with torch.no_grad():
            tr.forward(feats, memory, B)

    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in tr.params.items()}
    bufs = {k: v.clone() for k, v in tr.buffers.items() if v.dtype == torch.float32}
    mem_leaf = memory.clone().requires_grad_(True)

    def torch_fwd_bwd():
        for t in list(leaves.values()) + [mem_leaf]:
            t.grad = None
        torch.autograd.backward(P.pyramid_forward(leaves, bufs, feats, mem_leaf, B), d_p1)

    # the finest level's launches alone
    c = torch.randn(B, H1, W1, C, generator=g).to(dev)                      # a lateral's conv output
    t = torch.randn(B, H1 // 2, W1 // 2, C, generator=g).to(dev)            # an up stage's conv output, at the low resolution
    gamma, beta = torch.rand(C, generator=g).to(dev) + 0.5, torch.randn(C, generator=g).to(dev)
    mc, _, rc = ops.bn_train_stats(c)
    mt, _, rt = ops.bn_train_stats(t, up=True)
    full, quarter = c.numel() * 4, t.numel() * 4                            # bytes of a high-resolution / low-resolution map
    launches = (
        ("stats_plain", lambda: ops.bn_train_stats(c), full),
        ("stats_up", lambda: ops.bn_train_stats(t, up=True), quarter),
        ("apply_plain", lambda: ops.bn_train_apply(c, gamma, beta, mc, rc), 2 * full),
        ("apply_up_lateral", lambda: ops.bn_train_apply(t, gamma, beta, mt, rt, ops.ACT_RELU, c, up=True), quarter + 2 * full),
        ("backward_plain", lambda: ops.bn_train_backward(d_p1, c, gamma, beta, mc, rc), 2 * (2 * full) + full),
        ("backward_up_fused", lambda: ops.bn_train_backward(d_p1, t, gamma, beta, mt, rt, up=True), 2 * (full + quarter) + quarter),
        ("bilinear_adjoint", lambda: ops.upsample2x_bilinear_backward(d_p1), full + quarter))
    out = {"batch": B, "res5": [h, w], "p1": [H1, W1], "device": torch.cuda.get_device_name(0), "rows_per_partial_block": ops._H.NPS_BN_TRAIN_RPS}
    for key, fn in (("pyramid_fwd_bwd_ms", fwd_bwd), ("pyramid_fwd_ms", fwd), ("torch_f32_fwd_bwd_ms", torch_fwd_bwd)):
        med, lo, hi = timed(fn, a.reps)
        out[key] = med
        out[key + "_min_max"] = [lo, hi]
    for key, fn, nbytes in launches:
        med, lo, hi = timed(fn, a.reps)
        out[key + "_ms"] = med
        out[key + "_min_max"] = [lo, hi]
        out[key + "_compulsory_MB"] = nbytes / 1e6
        out[key + "_TBps_of_compulsory"] = nbytes / (med * 1e-3) / 1e12
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
