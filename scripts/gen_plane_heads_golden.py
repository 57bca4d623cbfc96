"""Pin the plane head's deep-supervision forward to the reference: build the reference model (through oracle.ref_shim, on the CPU) with
the name-seeded synthetic checkpoint, put sem_seg_head in TRAINING mode - so that it emits aux_outputs - with context_SA,
context2plane_decoder and top_down in eval mode - so that dropout and BatchNorm's batch statistics stay off - and run it on
tests/golden_inputs.feature_maps at the smallest size.  Writes tests/golden/L_plane_heads_<h>x<w>_nq<nq>.npz: all three supervised layers'
pred_logits / pred_params / pred_centers, pixel_centers, the mask logits subsampled [::4, ::4] (as B_plane_head_6x8.npz stores them) and
the two tensors where the trunk ends - hs [3, B, nq, 256] and p1 at the same [::4, ::4] positions - so that the heads can be restated
from them without the trunk.  Results only; needs the reference tree (NOPESAC_REFERENCE_ROOT); nothing of its text is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import golden_inputs as GI  # noqa: E402

CASES = ((21, 6, 8, 7),)                # (feature seed, h5, w5, nq)


def main():
    from nopesac_amd.synth import synth_state_dict
    for seed, h5, w5, nq in CASES:
        model = ref_shim.build_reference_model(synth_state_dict(nq), num_queries=nq)
        head = model.sem_seg_head
        assert head.deep_supervision
        head.train()
        for trunk in (head.context_SA, head.context2plane_decoder, head.top_down):
            trunk.eval()
        kept = {}
        hooks = [head.context2plane_decoder.register_forward_hook(lambda m, i, o: kept.__setitem__("hs", o)),
                 head.top_down.register_forward_hook(lambda m, i, o: kept.__setitem__("p1", o))]
        feats = GI.feature_maps(seed, h5, w5)
        with torch.no_grad():
            out, _ = head(feats)
        for hk in hooks:
            hk.remove()
        layers = list(out["aux_outputs"]) + [out]                         # decoder layers 3, 4, 5
        assert len(layers) == 3
        hs = kept["hs"].transpose(1, 2)[-3:]                              # [3, B, nq, 256]
        rec = {"nq": np.int64(nq), "hs": hs.numpy(), "p1_sub": kept["p1"].permute(0, 2, 3, 1)[:, ::4, ::4].contiguous().numpy(),
               "pixel_centers": out["pixel_centers"].numpy(), "pixel_centers_sub": out["pixel_centers"][:, :, ::4, ::4].contiguous().numpy(),
               "mask_logits_sub": np.stack([l["pred_mask_logits"][:, :, ::4, ::4].numpy() for l in layers])}
        for k in ("pred_logits", "pred_params", "pred_centers"):
            rec[k] = np.stack([l[k].numpy() for l in layers])
        path = os.path.join(ROOT, "tests", "golden", "L_plane_heads_%dx%d_nq%d.npz" % (h5, w5, nq))
        np.savez_compressed(path, **rec)
        print({k: v.shape for k, v in rec.items()}, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
