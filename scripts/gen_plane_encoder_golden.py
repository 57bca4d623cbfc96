"""Pin the plane head's transformer encoder to the reference: build the reference model (through oracle.ref_shim, on the CPU), give its
input_proj and context_SA the 76 tensors of tests/plane_encoder_forms.encoder_inputs (the name-seeded synthetic checkpoint with the
settled linear1 biases), run input_proj, the reference's own PositionEmbeddingSine and context_SA on the case's res5 as an autograd leaf,
and back from the case's seeded cotangent at the memory.  Two runs at B = 2, 3 x 4: "eval" - the modules in eval mode (no dropout) - and
"train" - the modules in train mode with torch.nn.functional.dropout replaced by a function that applies, in call order, the materialised
keep masks of ops.encoder_dropout_stream (layer by layer: attention probabilities, indexed in [B x heads, L, L]; dropout1; the FFN's
inner dropout; dropout2 - the three indexed in (b, token) rows), which pins the site order and the index convention to the reference.
Writes tests/golden/L_plane_encoder_3x4.npz: per run the memory [B L, 256] in (b, token) rows, d res5 (NHWC) at channels [::64], the 76
gradients (matrices at rows [::64]) and the reference's position embedding.  Results only; needs the reference tree
(NOPESAC_REFERENCE_ROOT); nothing of its text is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import plane_encoder_forms as E  # noqa: E402


def routes_through_functional_dropout(head) -> bool:
    """True if this torch sends nn.MultiheadAttention's probability dropout and nn.Dropout through torch.nn.functional.dropout: one
    train-mode layer on a tiny input must call it four times."""
    import torch.nn.functional as F
    calls, real = [], F.dropout

    def spy(x, p=0.5, training=True, inplace=False):
        calls.append(tuple(x.shape))
        return real(x, p, training, inplace)
    layer = head.context_SA.layers[0]
    F.dropout = spy
    try:
        layer.train()
        with torch.no_grad():
            layer(torch.zeros(3, 2, 256), pos=torch.zeros(3, 2, 256))
    finally:
        F.dropout = real
        layer.eval()
    return calls == [(2 * E.NHEADS, 3, 3), (3, 2, 256), (3, 2, E.FFN), (3, 2, 256)]


def run(head, key, train: bool):
    import torch.nn.functional as F
    c = E.encoder_inputs(key)
    B, h, w, L = c["B"], c["h"], c["w"], c["L"]
    mods = torch.nn.ModuleDict({"input_proj": head.input_proj, "context_SA": head.context_SA})
    with torch.no_grad():
        for name, t in mods.named_parameters():
            t.copy_(c["sd"][E.PREFIX + name])
    for t in mods.parameters():
        t.requires_grad_(True)
        t.grad = None
    mods.train(train)
    c4 = c["res5"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    sites, real = [], F.dropout
    order = [(i, s) for i in range(E.LAYERS) for s in range(4)]

    def masked(x, p=0.5, training=True, inplace=False):              # (torch.nn.functional.dropout's signature)
        assert training and abs(p - 0.1) < 1e-12 and len(sites) < len(order)
        i, s = order[len(sites)]
        sites.append((i, s))
        m = c["masks"][(i, s)].to(x.dtype)
        m = m.view(B * E.NHEADS, L, L) if s == 0 else m.view(B, L, -1).transpose(0, 1)           # modules run on [L, B, D]
        assert tuple(m.shape) == tuple(x.shape), (i, s, m.shape, x.shape)
        return x * m / (1.0 - c["p"])
    if train:
        F.dropout = masked
    try:
        pos_map = head.position_embedding(c4)
        seq = head.input_proj(c4).flatten(2).permute(2, 0, 1)
        memory = head.context_SA(seq, pos=pos_map.flatten(2).permute(2, 0, 1))                      # [L, B, 256]
    finally:
        F.dropout = real
    assert sites == (order if train else [])
    memory = memory.transpose(0, 1).reshape(B * L, 256)
    (memory * c["d_memory"]).sum().backward()
    full = {E.PREFIX + name: t.grad.detach() for name, t in mods.named_parameters()}
    assert len(full) == 76
    full["memory"] = memory.detach()
    full["res5"] = c4.grad.detach().permute(0, 2, 3, 1).contiguous()
    out = {k: v.contiguous().numpy() for k, v in E.fixture_view(full).items()}
    out["pos"] = pos_map.detach()[0].flatten(1).t().contiguous().numpy()
    mods.eval()
    return out


def main():
    from nopesac_amd.synth import synth_state_dict
    model = ref_shim.build_reference_model(synth_state_dict(7), num_queries=7)
    head = model.sem_seg_head
    head.eval()
    routed = routes_through_functional_dropout(head)
    print("torch", torch.__version__, "routes the encoder's dropouts through torch.nn.functional.dropout:", routed)
    rec = {"train_mode": np.int64(routed)}
    for tag, key in E.GOLDEN_CASES.items():
        if tag == "train" and not routed:
            continue
        for k, v in run(head, key, tag == "train").items():
            rec[tag + "." + k] = v
    h, w = E.GOLDEN_CASES["eval"][1:3]
    path = os.path.join(ROOT, "tests", "golden", E.GOLDEN % (h, w))
    np.savez_compressed(path, **rec)
    print(len(rec), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
