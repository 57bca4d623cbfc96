"""Pin the plane head's top-down pyramid in TRAINING mode to the reference: build the reference model (through oracle.ref_shim, on the
CPU) with the name-seeded synthetic checkpoint, run its plane head once in eval mode on tests/golden_inputs.feature_maps at the smallest
size (batch 2) to take the two inputs of top_down - the backbone maps and the encoder's memory -, then put top_down alone in TRAIN mode
(nn.BatchNorm2d on batch statistics, running buffers updated) and run it ONCE on those inputs as autograd leaves, and back from the
seeded cotangent the tests share (tests/plane_pyramid_forms.cotangent).  Writes tests/golden/L_plane_pyramid_<h>x<w>.npz: memory
[B Lm, 256], p1 subsampled [:, ::4, ::4] (NHWC), the 16 running statistics and the eight num_batches_tracked counters after that one
forward, the eight BatchNorm biases as settled and given to the reference, all 16 BatchNorm affine gradients, the conv weight gradients
at rows [::16], d memory in full and d res5 at channels [::32].
Results only; needs the reference tree (NOPESAC_REFERENCE_ROOT); nothing of its text is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import golden_inputs as GI  # noqa: E402
from tests import plane_pyramid_forms as P  # noqa: E402

CASES = ((23, 6, 8, 2, 7),)             # (feature seed, h5, w5, batch, nq)


def main():
    from nopesac_amd.synth import synth_state_dict
    for seed, h5, w5, B, nq in CASES:
        model = ref_shim.build_reference_model(synth_state_dict(nq), num_queries=nq)
        head = model.sem_seg_head
        head.eval()
        kept = {}
        hook = head.top_down.register_forward_pre_hook(lambda m, args: kept.__setitem__("in", args))
        feats = GI.feature_maps(seed, h5, w5, batch=B)
        with torch.no_grad():
            head(feats)
        hook.remove()
        maps, memory = kept["in"]                                         # (c1, c2, c3, c4) NCHW, memory [B, 256, h5, w5]
        assert all(torch.equal(m, feats[k]) for m, k in zip(maps, P.LEVELS)) and tuple(memory.shape) == (B, 256, h5, w5)
        maps = [m.detach().clone().requires_grad_(True) for m in maps]
        mem = memory.detach().clone().requires_grad_(True)
        # the ReLU decisions of the case keep their margins (tests/plane_pyramid_forms.py): the synthetic checkpoint's BatchNorm biases are
        # settled on these inputs, given to the reference and stored beside its results
        td = head.top_down
        full = {P.PREFIX + k: v.detach().clone() for k, v in td.state_dict().items()}
        sd = {k: full[k].float() for k in P.pyramid_parameter_names(full.keys())}
        bufs = {k: full[k].float() for k in P.pyramid_buffer_names(full.keys())}
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
        P.settle_biases(sd, bufs, {k: nhwc(m) for k, m in zip(P.LEVELS, maps)}, nhwc(memory).reshape(B * h5 * w5, 256), B)
        with torch.no_grad():
            for name, p in td.named_parameters():
                if name.endswith(".1.bias"):
                    p.copy_(sd[P.PREFIX + name])
        td.train()
        for p in td.parameters():
            p.requires_grad_(True)
            p.grad = None
        p1 = td(tuple(maps), mem)                                         # the one training-mode forward
        cot = P.cotangent(seed, B, h5, w5)                                # NHWC
        (p1 * cot.permute(0, 3, 1, 2)).sum().backward()
        rec = {"seed": np.int64(seed), "memory": nhwc(memory).reshape(B * h5 * w5, 256).numpy(), "p1_sub": nhwc(p1)[:, ::4, ::4].contiguous().numpy(),
               "d_memory": nhwc(mem.grad).reshape(B * h5 * w5, 256).numpy(), "d_res5_sub": nhwc(maps[3].grad)[..., ::32].contiguous().numpy()}
        for name, t in td.state_dict().items():
            if name.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                rec[P.PREFIX + name] = t.detach().numpy()
        for name, p in td.named_parameters():
            g = p.grad.detach()
            rec["d." + P.PREFIX + name] = (g[::16].contiguous() if g.dim() == 4 else g).numpy()
            if name.endswith(".1.bias"):
                rec["bias." + P.PREFIX + name] = p.detach().numpy().copy()
        assert sum(k.startswith("d." + P.PREFIX) for k in rec) == 24 and sum(k.startswith(P.PREFIX) for k in rec) == 24
        path = os.path.join(ROOT, "tests", "golden", "L_plane_pyramid_%dx%d.npz" % (h5, w5))
        np.savez_compressed(path, **rec)
        print({k: v.shape for k, v in rec.items()}, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
