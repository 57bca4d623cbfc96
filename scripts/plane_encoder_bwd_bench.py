"""Training step of the plane head's encoder at the workload's shape (csrc/linear_bwd.hip): B = 32 images, res5 at 15 x 20 (L = 300,
M = 9600 rows per Linear), dropout p = 0.1.  Times PlaneEncoderTrainer.forward + backward_from with LINEAR = _LinearInPlace (every
Linear's backward one ops.linear_backward call) and with LINEAR = _Linear (the composition the other trainers use: ReLU pass, three
transposes, two GEMMs, a column sum - the baseline), counts the submitting library calls of each leg, times ops.linear_backward against the body of
_Linear.backward alone at the five production (K, N) pairs with the gates of their sites, and, as the yardstick on the same GPU, the
float32 torch restatement of the whole encoder (tests/plane_encoder_forms.encoder_forward under autograd with the four sites' masks
materialised by ops.dropout_keep_mask).  Warm-up, then the median of `--reps` event-timed runs.  Prints one JSON line and writes
profiles/plane_encoder_bwd_times.json.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd import training as T  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from scripts.plane_decoder_bwd_bench import timed  # noqa: E402
from tests import plane_encoder_forms as E  # noqa: E402


SIZE_QUERIES = ("_workspace_floats", "_workspace_bytes")      # the endings of the entries that return a number and submit nothing


class _Counter:
    """ops._C behind a counter: every library call that submits work (one host submission; linear_backward is up to three kernel
    launches) is counted; the size queries are not."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name.endswith(SIZE_QUERIES):
            return fn

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def count_calls(fn):
    real = ops._C
    ops._C = counter = _Counter(real)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops._C = real
    return counter.calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_encoder_bwd_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, h, w, p, seed, step = a.batch, 15, 20, a.p, 7, 11
    L = h * w
    M = B * L
    g = torch.Generator().manual_seed(5)
    res5 = torch.randn(B, h, w, E.CIN, generator=g).clamp_min(0.0).to(dev)
    d_memory = (torch.randn(M, 256, generator=g) / 16).to(dev)
    sd = synth_state_dict(50)

    class Composed(T.PlaneEncoderTrainer):
        LINEAR = T._Linear
    legs = {"in_place": T.PlaneEncoderTrainer.from_state_dict(sd, dev, feature_grads=True), "composed": Composed.from_state_dict(sd, dev, feature_grads=True)}

    def fwd_bwd(tr):
        def run():
            tr.forward(res5, B, p, seed, step)
            tr.backward_from(d_memory)
        return run

    def fwd(tr):
        def run():
            with torch.no_grad():
                tr.forward(res5, B, p, seed, step)
        return run

    out = {"batch": B, "h": h, "w": w, "rows": M, "p": p, "device": torch.cuda.get_device_name(0), "tile": [ops.LINEAR_BWD_TILE, ops.LINEAR_BWD_STAGE]}
    for name, tr in legs.items():
        for key, fn in (("fwd_bwd", fwd_bwd(tr)), ("fwd", fwd(tr))):
            med, lo, hi = timed(fn, a.reps)
            out["encoder_%s_%s_ms" % (name, key)] = med
            out["encoder_%s_%s_ms_min_max" % (name, key)] = [lo, hi]
        calls = count_calls(fwd_bwd(tr))
        out["encoder_%s_library_calls" % name] = sum(calls.values())
        out["encoder_%s_library_calls_by_entry" % name] = dict(sorted(calls.items()))
    same = all(torch.equal(legs["in_place"].grads[k], legs["composed"].grads[k]) for k in legs["in_place"].grads)
    out["legs_agree_bit_for_bit"] = bool(same)               # (not expected: the two Linear backwards sum in different orders)

    # one Linear's backward alone: (K, N, ReLU gate, dropout gate) of the five production sites
    sites = {"in_proj_qk": (256, 512, False, False), "out_proj": (256, 256, False, True), "linear1": (256, 1024, True, True),
             "linear2": (1024, 256, False, True), "input_proj": (2048, 256, False, False)}
    stream = ops.encoder_dropout_stream(step, 0, 2)
    for name, (K, N, relu, drop) in sites.items():
        x, wt = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        gr = torch.randn(M, N, generator=g).to(dev)
        y = torch.randn(M, N, generator=g).clamp_min(0.0).to(dev) if relu else None
        pd = p if drop else 0.0

        def in_place():
            ops.linear_backward(x, wt, gr, y=y, p=pd, seed=seed, stream=stream)

        def composed():                                             # _Dropout.backward, then the body of _Linear.backward
            g2 = ops.dropout(gr, pd, seed, stream) if pd else gr
            if y is not None:
                g2 = ops.relu_backward(g2, y)
            ops.linear(g2, T.transpose(wt))
            ops.linear(T.transpose(g2), T.transpose(x))
            T.col_sum(g2)
        for key, fn in (("linear_backward", in_place), ("composed", composed)):
            med, lo, hi = timed(fn, a.reps)
            out["%s_K%d_N%d_%s_ms" % (name, K, N, key)] = med
            out["%s_K%d_N%d_%s_ms_min_max" % (name, K, N, key)] = [lo, hi]
        out["%s_K%d_N%d_splits" % (name, K, N)] = ops.linear_backward_splits(M, K, N)
        del x, wt, gr, y

    # the float32 torch restatement, masks materialised once (they are inputs of the restatement, outside its time)
    masks = None
    if p:
        shapes = {0: (B, E.NHEADS, L, L), 1: (M, 256), 2: (M, E.FFN), 3: (M, 256)}
        masks = {(i, s): ops.dropout_keep_mask(shapes[s], p, seed, ops.encoder_dropout_stream(step, i, s), device=dev) for i in range(E.LAYERS) for s in range(4)}
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in legs["in_place"].params.items()}
    res5_leaf = res5.clone().requires_grad_(True)
    pos = legs["in_place"].pos(h, w, dev)

    def torch_fwd_bwd():
        for t in list(leaves.values()) + [res5_leaf]:
            t.grad = None
        memory = E.encoder_forward(leaves, res5_leaf, pos, B, masks, p).reshape(M, 256)
        torch.autograd.backward(memory, d_memory)
    med, lo, hi = timed(torch_fwd_bwd, a.reps)
    out["torch_f32_fwd_bwd_ms"] = med
    out["torch_f32_fwd_bwd_ms_min_max"] = [lo, hi]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
