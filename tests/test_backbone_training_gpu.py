"""BackboneTrainer against the inference backbone (forward, bit for bit), the float64 restatement of tests/backbone_forms.py (all 53
gradients), itself (two runs), the optimiser step with write_back, and the plane head's chain behind its maps."""
import os

import pytest
import torch

from tests import backbone_forms as BF
from tests.util import ROOT

pytestmark = pytest.mark.gpu
NQ = 7


def _trainer(device):
    from nopesac_amd.training import BackboneTrainer
    return BackboneTrainer.from_state_dict(BF.backbone_state_dict(), device)


def _backbone(device):
    from nopesac_amd.modeling.backbone import HipResNet50
    bb = HipResNet50().to(device)
    bb.load_state_dict({k[len(BF.PREFIX):]: v for k, v in BF.backbone_state_dict().items()})
    return bb


@pytest.mark.parametrize("case", BF.NET_CASES, ids=lambda c: "n%d_%dx%d" % c)
def test_the_forward_is_the_inference_backbones(device, case):
    x = BF.net_inputs(case)[0].to(device)
    tr = _trainer(device)
    assert len(tr.params) == 53 and all(p.is_leaf and p.requires_grad for p in tr.params.values())
    feats = tr.forward(x)
    with torch.no_grad():
        ref = _backbone(device).forward(x)
    assert list(feats) == list(BF.MAPS) and all(feats[k].requires_grad for k in feats)
    assert all(torch.equal(feats[k].detach(), ref[k]) for k in BF.MAPS)
    from_model = type(tr).from_backbone(_backbone(device))
    assert all(torch.equal(from_model.params[k], tr.params[k]) for k in tr.params)
    assert all(torch.equal(from_model.norms[k][i], tr.norms[k][i]) for k in tr.norms for i in (0, 1))


@pytest.mark.parametrize("which", BF.COTANGENTS)
@pytest.mark.parametrize("case", BF.NET_CASES, ids=lambda c: "n%d_%dx%d" % c)
def test_gradients_against_the_float64_backbone(device, case, which):
    x, cots = BF.net_inputs(case)
    maps64, ref = BF.backbone_reference(case, which)
    tr = _trainer(device)
    feats = tr.forward(x.to(device))
    assert all(BF.norm_err(feats[k].detach(), maps64[k]) <= BF.NORM_FLOOR for k in BF.MAPS)
    d = {k: cots[k].to(device) for k in (BF.MAPS if which == "all" else ("res5",))}
    grads = tr.backward_from(d)
    assert sorted(grads) == sorted(ref) and len(grads) == 53
    worst = {}
    for k in ref:
        assert grads[k].shape == ref[k].shape and bool(torch.isfinite(grads[k]).all()), k
        worst[k] = BF.norm_err(grads[k], ref[k])
    for fam in BF.F32_NORM_ERR[(case, which)]:
        print("%s: worst normalised error %.3g (bound %.3g)" % (fam, max(v for k, v in worst.items() if BF.family_of(k) == fam),
                                                                 BF.norm_bound(case, which, BF.PREFIX + fam)))
    bad = {k: v for k, v in worst.items() if not v <= BF.norm_bound(case, which, k)}
    assert not bad, bad
    # a second run of the same step: the same bits
    tr.forward(x.to(device))
    again = tr.backward_from(d)
    assert all(torch.equal(again[k], grads[k]) for k in grads)


def test_one_step_moves_every_tensor_and_write_back_reaches_the_inference_backbone(device):
    from nopesac_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "Base.yaml"))
    case = BF.NET_CASES[0]
    x, cots = BF.net_inputs(case)
    x = x.to(device)
    tr, bb = _trainer(device), _backbone(device)
    assert tr.lr_multiplier(cfg) == float(cfg.SOLVER.BACKBONE_MULTIPLIER) == 0.1
    before = {k: p.detach().clone() for k, p in tr.params.items()}
    tr.forward(x)
    tr.backward_from({k: cots[k].to(device) for k in BF.MAPS})
    tr.step_from_cfg(cfg)
    assert tr.steps == 1 and all(not torch.equal(before[k], p.detach()) for k, p in tr.params.items())
    tr.write_back(bb)
    with torch.no_grad():
        ref = bb.forward(x)
    feats = tr.forward(x)
    assert all(torch.equal(feats[k].detach(), ref[k]) for k in BF.MAPS)


def test_the_plane_heads_chain_runs_on_into_the_backbone(device):
    """the backbone's maps feed PlaneEncoderTrainer.losses as they are; joined_backward fills 235 + 53 gradients, and the backbone's are,
    bit for bit, a fresh forward + backward_from of what the chain reports at the maps"""
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlaneDecoderTrainer, PlaneEncoderTrainer, PlaneInstanceHeadsTrainer, PlanePyramidTrainer
    from tests.test_plane_heads_training_gpu import _head_targets
    N, H, W = BF.NET_CASES[0]
    sd = synth_state_dict(NQ)
    enc, dec = PlaneEncoderTrainer.from_state_dict(sd, device), PlaneDecoderTrainer.from_state_dict(sd, NQ, device)
    pyr, heads = PlanePyramidTrainer.from_state_dict(sd, device), PlaneInstanceHeadsTrainer.from_state_dict(sd, NQ, device)
    targets = _head_targets("border_s4", device, H // 4, W // 4)
    x = BF.net_inputs(BF.NET_CASES[0])[0].to(device)
    tr = _trainer(device)
    feats = tr.forward(x)
    losses, _ = enc.losses(heads, dec, pyr, feats, targets, p=0)
    grads = tr.joined_backward(enc, losses)
    assert len(grads) == 235 + 53 and all(grads[k] is tr.grads[k] for k in tr.params)
    assert all(float(tr.grads[k].abs().max()) > 0 and bool(torch.isfinite(tr.grads[k]).all()) for k in tr.params)
    assert set(pyr.input_grads) >= set(BF.MAPS) and torch.equal(pyr.input_grads["res5"], enc.input_grads["res5"])
    d = {k: pyr.input_grads[k].clone() for k in BF.MAPS}
    keep = {k: tr.grads[k].clone() for k in tr.params}
    tr.forward(x)
    fresh = tr.backward_from(d)
    assert all(torch.equal(fresh[k], keep[k]) for k in keep), [k for k in keep if not torch.equal(fresh[k], keep[k])]
