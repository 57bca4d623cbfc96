"""Plain-torch restatement of the plane head's instance heads under deep supervision (reference PlaneTRHead.forward,
planeTR_head.py:146-192), dtype-generic and autograd-able, and the seeded route from (hs, p1) through tests/plane_criterion_ref.py that
tests/test_plane_heads_training_gpu.py holds PlaneInstanceHeadsTrainer to.  The pixel-embedding map is materialised here, as in the
reference - the trainer's folded form is what is under test.  Imports without a GPU."""
import torch

from tests import plane_criterion_inputs as PI
from tests import plane_criterion_ref as R

PREFIX = "sem_seg_head."
HEADS = ("plane_embedding", "pixel_embedding", "plane_prob", "plane_param", "plane_center", "pixel_plane_center")
CRITERION_CASES = ("border_s4", "ragged", "s1")              # the targets of tests/plane_criterion_inputs.py the trainer is run against


def parameter_names(sd):
    return sorted(k for k in sd if k.startswith(PREFIX) and k[len(PREFIX):].split(".")[0] in HEADS)


def _mlp(sd, name, x):
    i = 0
    while PREFIX + "%s.layers.%d.weight" % (name, i + 1) in sd:
        x = torch.relu(x @ sd[PREFIX + "%s.layers.%d.weight" % (name, i)].T + sd[PREFIX + "%s.layers.%d.bias" % (name, i)])
        i += 1
    return x @ sd[PREFIX + "%s.layers.%d.weight" % (name, i)].T + sd[PREFIX + "%s.layers.%d.bias" % (name, i)]


def heads(sd, hs, p1):
    """sd: the 24 tensors under their state-dict keys (in the dtype of hs); hs [L, B, nq, 256]; p1 [B, h, w, 256] channel-last
    -> pred_logits [L, B, nq, 2], pred_params [L, B, nq, 3], pred_centers [L, B, nq, 2], pred_mask_logits [L, B, nq, h, w],
    pixel_centers [B, 2, h, w]"""
    emb = _mlp(sd, "plane_embedding", hs)
    w_pe = sd[PREFIX + "pixel_embedding.weight"].reshape(256, 256)
    pix = p1 @ w_pe.T + sd[PREFIX + "pixel_embedding.bias"]
    w_pc = sd[PREFIX + "pixel_plane_center.weight"].reshape(2, 256)
    return {"pred_logits": hs @ sd[PREFIX + "plane_prob.weight"].T + sd[PREFIX + "plane_prob.bias"],
            "pred_params": _mlp(sd, "plane_param", hs),
            "pred_centers": torch.sigmoid(_mlp(sd, "plane_center", hs)),
            "pred_mask_logits": torch.einsum("lbqc,bhwc->lbqhw", emb, pix),
            "pixel_centers": torch.sigmoid(p1 @ w_pc.T + sd[PREFIX + "pixel_plane_center.bias"]).permute(0, 3, 1, 2)}


def training_dict(out):
    """heads() -> the reference's training dict: the last layer first, aux_outputs = the layers 0 .. L - 2"""
    L = out["pred_logits"].shape[0]
    layer = lambda l: {k: out[k][l] for k in ("pred_logits", "pred_mask_logits", "pred_centers", "pred_params")}
    d = layer(L - 1)
    d["pixel_centers"] = out["pixel_centers"]
    if L > 1:
        d["aux_outputs"] = [layer(l) for l in range(L - 1)]
    return d


def seeded_inputs(name):
    """hs ~ N(0, 1) [L, B, nq, 256], p1 = relu(N(0, 1)) [B, h, w, 256] in float32, from the seed 100 + the case's seed"""
    L, B, nq, h, w = PI.CASES[name][:5]
    g = torch.Generator().manual_seed(100 + PI.CASES[name][-1])
    return torch.randn(L, B, nq, 256, generator=g), torch.relu(torch.randn(B, h, w, 256, generator=g))


def weight_dict():
    from nopesac_amd.config import get_cfg
    from nopesac_amd.training import PlaneCriterion
    return PlaneCriterion.from_cfg(get_cfg()).weight_dict


def through_criterion(name, sd, dtype, indices=None, noise=None, grads=True):
    """(seeded hs, p1) -> heads -> the criterion's restatement on the targets of PI.make(name), in `dtype`: losses, the gradients of the
    weighted sum at the 24 tensors and at hs / p1, the indices of every layer (last layer first).  noise = (relative size, generator):
    hs and p1 are multiplied by 1 + size * N(0, 1)."""
    hs, p1 = (t.to(dtype) for t in seeded_inputs(name))
    if noise is not None:
        hs = hs * (1 + noise[0] * torch.randn(hs.shape, generator=noise[1]).to(dtype))
        p1 = p1 * (1 + noise[0] * torch.randn(p1.shape, generator=noise[1]).to(dtype))
    names = parameter_names(sd)
    assert len(names) == 24
    P = {k: sd[k].detach().to(dtype).requires_grad_(grads) for k in names}
    hs.requires_grad_(grads)
    p1.requires_grad_(grads)
    out = heads(P, hs, p1)
    _, targets = PI.cast(*PI.make(name), dtype)
    losses, idx, _ = R.criterion(training_dict(out), targets, indices=indices)
    res = {"losses": {k: v.detach() for k, v in losses.items()}, "idx": idx, "out": {k: v.detach() for k, v in out.items()}}
    if grads:
        wd = weight_dict()
        total = sum(v * wd[k] for k, v in losses.items() if k in wd)
        g = torch.autograd.grad(total, list(P.values()) + [hs, p1])
        res["grads"] = dict(zip(names, g[:24]))
        res["input_grads"] = {"hs": g[24], "p1": g[25]}
    return res
