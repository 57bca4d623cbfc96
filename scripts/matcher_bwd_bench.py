"""Backward of the matching head at 32 pairs (csrc/matcher_bwd.hip): for nq in {50, 64, 128} with full plane sets, one
MatchingHeadTrainer.matching_losses call forward + backward, and the Sinkhorn stage alone (forward = the inference launch + the loss;
backward = the replay that keeps the potentials + the gradient of the 200 unrolled iterations) next to the inference Sinkhorn launch.
Warm-up, then the median of `--reps` event-timed runs.  Prints a table and one JSON line, and writes profiles/matcher_bwd_times.json.  `--pairs N` changes the batch."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from nopesac_amd.training import MatchingHeadTrainer, _SinkhornEmbLoss  # noqa: E402


def timed(fn, reps, warmup=3):
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
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matcher_bwd_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.pairs
    out = {"pairs": B, "iterations": 200, "device": torch.cuda.get_device_name(0), "rows": []}
    print("%5s %14s %14s %14s %14s %14s" % ("nq", "fwd+bwd ms", "fwd ms", "sink fwd us", "sink bwd us", "inference us"))
    for nq in (50, 64, 128):
        g = torch.Generator().manual_seed(nq)
        tr = MatchingHeadTrainer.from_state_dict(synth_state_dict(nq), nq, dev)
        app = torch.randn(2 * B, nq, 256, generator=g).to(dev)
        n_all = torch.full((2 * B,), nq, dtype=torch.int32, device=dev)
        planes = lambda: (torch.nn.functional.normalize(torch.randn(B, nq, 3, generator=g), dim=-1) * (1 + torch.rand(B, nq, 1, generator=g))).to(dev)
        p1, p2 = planes(), planes()
        cam7 = torch.cat([0.3 * torch.randn(B, 3, generator=g), torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)], 1).to(dev)
        gt = torch.zeros(B, nq + 1, nq + 1, dtype=torch.uint8)
        idx = torch.arange(nq)
        gt[:, idx[: nq // 2], idx[: nq // 2]] = 1
        gt[:, idx[nq // 2:], nq] = 1
        gt[:, nq, idx[nq // 2:]] = 1
        gt = gt.to(dev)

        def fwd_bwd():
            tr.backward(tr.matching_losses(app, n_all, cam7, p1, p2, gt))

        def fwd():
            with torch.no_grad():
                tr.matching_losses(app, n_all, cam7, p1, p2, gt)

        fwd_bwd()
        dots = tr.last["desc_dot"].clone().requires_grad_(True)
        bs = tr.params["matching_head.bin_score"].detach().view(1).clone().requires_grad_(True)
        n1 = n_all[:B].contiguous()
        state = {}

        def sink_fwd():
            state["loss"] = _SinkhornEmbLoss.apply(dots, bs, p1, p2, cam7, n1, n1, gt, 4.0, 8.0, 200)[0]

        def sink_bwd():
            dots.grad = bs.grad = None
            state["loss"].backward(retain_graph=True)

        def inference():
            ops.matcher_sinkhorn(dots.detach(), p1, p2, cam7, n1, n1, bs.detach(), 4.0, 8.0, 200, 0.2)

        row = {"nq": nq}
        for key, fn, scale in (("train_fwd_bwd_ms", fwd_bwd, 1.0), ("train_fwd_ms", fwd, 1.0), ("sinkhorn_train_fwd_us", sink_fwd, 1e3),
                               ("sinkhorn_train_bwd_us", sink_bwd, 1e3), ("sinkhorn_inference_us", inference, 1e3)):
            med, lo, hi = timed(fn, a.reps)
            row[key] = med * scale
            row[key + "_min_max"] = [lo * scale, hi * scale]
        out["rows"].append(row)
        print("%5d %14.2f %14.2f %14.1f %14.1f %14.1f" % (nq, row["train_fwd_bwd_ms"], row["train_fwd_ms"], row["sinkhorn_train_fwd_us"],
                                                         row["sinkhorn_train_bwd_us"], row["sinkhorn_inference_us"]))
        del tr
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
