"""Training step of the plane head's decoder at the workload's shape (csrc/decoder_train.hip): B = 32 images, nq = 50 queries, a 15 x 20
encoder memory (Lm = 300), L = 3 supervised layers, dropout p = 0.1.  Times one PlaneDecoderTrainer.forward + backward_from, the forward
alone, the cross-attention launches alone (ops.attention_train and ops.attention_train_backward at Lq = 50, Lk = 300, 8 heads) and, as the
yardstick on the same GPU, the float32 torch restatement of the whole decoder (tests/plane_decoder_forms.decoder_forward under autograd
with the six sites' masks materialised by ops.dropout_keep_mask).  Warm-up, then the median of `--reps` event-timed runs.  Prints one JSON
line and writes profiles/plane_decoder_bwd_times.json.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from nopesac_amd.training import PlaneDecoderTrainer  # noqa: E402
from tests import plane_decoder_forms as D  # noqa: E402


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
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_decoder_bwd_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, nq, Lm, L, p, seed, step = a.batch, 50, 300, 3, a.p, 7, 11
    g = torch.Generator().manual_seed(5)
    memory = torch.randn(B * Lm, 256, generator=g).to(dev)
    pos = torch.randn(Lm, 256, generator=g).to(dev)
    d_hs = (torch.randn(L, B, nq, 256, generator=g) / 16).to(dev)
    sd = synth_state_dict(nq)
    tr = PlaneDecoderTrainer.from_state_dict(sd, nq, dev)

    def fwd_bwd():
        tr.forward(memory, pos, B, p, seed, step)
        tr.backward_from(d_hs)

    def fwd():
        with torch.no_grad():
            tr.forward(memory, pos, B, p, seed, step)

    # the float32 torch restatement, masks materialised once (they are inputs of the restatement, outside its time)
    shapes = {0: (B, 8, nq, nq), 1: (B * nq, 256), 2: (B, 8, nq, Lm), 3: (B * nq, 256), 4: (B * nq, D.FFN), 5: (B * nq, 256)}
    masks = {(i, s): ops.dropout_keep_mask(shapes[s], p, seed, ops.dropout_stream(step, i, s), device=dev) for i in range(6) for s in range(6)} if p else None
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in tr.params.items()}
    mem_leaf = memory.clone().requires_grad_(True)

    def torch_fwd_bwd():
        for t in list(leaves.values()) + [mem_leaf]:
            t.grad = None
        hs = D.decoder_forward(leaves, mem_leaf, pos, B, nq, masks, p)
        torch.autograd.backward(hs, d_hs)

    W, scale = 256, 32 ** -0.5
    q = torch.randn(B * nq, W, generator=g).to(dev)
    k, v = torch.randn(B * Lm, W, generator=g).to(dev), torch.randn(B * Lm, W, generator=g).to(dev)
    go = torch.randn(B * nq, W, generator=g).to(dev)
    stream = ops.dropout_stream(step, 0, 2)
    out = {"batch": B, "nq": nq, "Lm": Lm, "layers_out": L, "p": p, "device": torch.cuda.get_device_name(0),
           "tile": [ops.ATT_TRAIN_TQ, ops.ATT_TRAIN_TK]}
    for key, fn in (("decoder_fwd_bwd_ms", fwd_bwd), ("decoder_fwd_ms", fwd), ("torch_f32_fwd_bwd_ms", torch_fwd_bwd),
                    ("cross_attention_fwd_ms", lambda: ops.attention_train(q, k, v, B, nq, Lm, 8, scale, p=p, seed=seed, stream=stream)),
                    ("cross_attention_bwd_ms", lambda: ops.attention_train_backward(q, k, v, go, B, nq, Lm, 8, scale, p=p, seed=seed, stream=stream)),
                    ("cross_attention_small_fwd_ms", lambda: ops.attention(q, k, v, B, nq, Lm, 8, scale))):
        med, lo, hi = timed(fn, a.reps)
        out[key] = med
        out[key + "_min_max"] = [lo, hi]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
