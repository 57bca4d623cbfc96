"""PlaneInstanceHeadsTrainer on the device (nopesac_amd/training.py; csrc/plane_head_bwd.hip) against the reference's deep-supervision
forward (tests/golden/L_plane_heads_*.npz), the inference head, and the float64 restatement tests/plane_heads_ref.py through
tests/plane_criterion_ref.py.  Error rule of the criterion tests: |kernel - f64| <= max(10 e32, 1e-6 max|f64|), e32 = the error of the same
restatement run in float32 (given the float64 indices).  nq = 7 at 6 x 8 unless stated."""
import functools

import pytest
import torch

from tests import golden_inputs as GI
from tests import plane_criterion_inputs as PI
from tests import plane_heads_ref as PR
from tests.util import gold, make_model, nhwc, rel_err

pytestmark = pytest.mark.gpu

NQ = 7
HEAD_KEYS = ("pred_logits", "pred_params", "pred_centers")


def _tol(r64, r32):
    return max(10 * float((r32.double() - r64).abs().max()), 1e-6 * float(r64.abs().max()))


def _gate(what, got, r64, r32, factor=1.0):
    ek = float((got.detach().double().cpu().reshape(r64.shape) - r64).abs().max())
    tol = factor * _tol(r64, r32)
    print("%-58s kernel %.3e  tol %.3e" % (what, ek, tol))
    assert ek <= tol, (what, ek, tol)


def _stacked(out):
    """the trainer's training dict -> per-layer tensors in decoder order [L, ...] (the order of hs)"""
    layers = list(out.get("aux_outputs", [])) + [out]
    d = {k: torch.stack([l[k] for l in layers]) for k in HEAD_KEYS + ("pred_mask_logits",)}
    d["pixel_centers"] = out["pixel_centers"]
    return d


def _private_model(device):
    """an instance no other test shares (write_back changes its tensors)"""
    return make_model(device, overrides=("SOLVER.SEM_SEG_HEAD_MULTIPLIER", 1.0), nq=NQ)


def _features(device, batch=1):
    return {k: nhwc(v).to(device) for k, v in GI.feature_maps(21, 6, 8, batch=batch).items()}


def _restated(sd, hs, p1):
    """PR.heads in float64 and float32 on the device's own hs / p1"""
    out = {}
    for dt in (torch.float64, torch.float32):
        P = {k: sd[k].detach().cpu().to(dt) for k in PR.parameter_names(sd)}
        with torch.no_grad():
            out[dt] = PR.heads(P, hs.detach().cpu().to(dt), p1.detach().cpu().to(dt))
    return out[torch.float64], out[torch.float32]


def test_forward_against_the_reference(device):
    from nopesac_amd.training import PlaneInstanceHeadsTrainer
    g = gold("L_plane_heads_6x8_nq%d" % NQ)
    head = make_model(device, nq=NQ).sem_seg_head
    hs, p1 = head.training_inputs(_features(device))
    assert hs.shape == (3, 1, NQ, 256) and p1.shape == (1, 48, 64, 256) and hs.dtype == p1.dtype == torch.float32
    assert rel_err(hs, g["hs"]) < 3e-4 and rel_err(p1[:, ::4, ::4], g["p1_sub"]) < 3e-4
    tr = PlaneInstanceHeadsTrainer.from_head(head)
    assert len(tr.params) == 24 and all(k.startswith("sem_seg_head.") for k in tr.params)
    with torch.no_grad():
        out = tr.forward(hs, p1)
    assert len(out["aux_outputs"]) == 2 and "pixel_centers" not in out["aux_outputs"][0]
    s = _stacked(out)
    for l in range(3):
        for k in HEAD_KEYS:
            assert rel_err(s[k][l], g[k][l]) < 3e-4, (l, k)
        assert rel_err(s["pred_mask_logits"][l][:, :, ::4, ::4], g["mask_logits_sub"][l]) < 3e-4, l
    assert rel_err(s["pixel_centers"], g["pixel_centers"]) < 3e-4


def _tie_in(head, tr, feats, hs, p1, sd):
    """the trainer's last layer against head.forward(want_logits=True) on the f32 route: each side within the rule's tolerance of
    float64, the difference within twice that - and zero, since the trainer makes the head's own launches"""
    with torch.no_grad():
        ho, _ = head(feats, want_logits=True)
        s = _stacked(tr.forward(hs, p1))
    r64, r32 = _restated(sd, hs, p1)
    pairs = [(k, s[k][-1], ho[k].float(), r64[k][-1], r32[k][-1]) for k in HEAD_KEYS]
    pairs.append(("pred_mask_logits", s["pred_mask_logits"][-1], ho["pred_mask_logits"].permute(0, 3, 1, 2), r64["pred_mask_logits"][-1],
                  r32["pred_mask_logits"][-1]))
    pairs.append(("pixel_centers", s["pixel_centers"], ho["pixel_centers"].permute(0, 3, 1, 2), r64["pixel_centers"], r32["pixel_centers"]))
    for k, mine, theirs, a64, a32 in pairs:
        _gate("trainer " + k, mine, a64, a32)
        _gate("head " + k, theirs, a64, a32)
        diff = float((mine.double() - theirs.double()).abs().max())
        print("%-58s |trainer - head| %.3e" % (k, diff))
        assert diff <= 2 * _tol(a64, a32), (k, diff)
        assert torch.equal(mine, theirs.contiguous().view_as(mine)), k
    return s


def test_last_layer_is_the_inference_heads(device):
    from nopesac_amd.training import PlaneInstanceHeadsTrainer
    head = make_model(device, nq=NQ).sem_seg_head
    feats = _features(device, batch=2)
    hs, p1 = head.training_inputs(feats)
    tr = PlaneInstanceHeadsTrainer.from_head(head)
    _tie_in(head, tr, feats, hs, p1, tr.params)


@functools.lru_cache(maxsize=None)
def reference(name):
    from nopesac_amd.synth import synth_state_dict
    sd = synth_state_dict(NQ)
    r64 = PR.through_criterion(name, sd, torch.float64)
    r32 = PR.through_criterion(name, sd, torch.float32, indices=r64["idx"])
    return r64, r32


def _device_targets(name, device):
    _, t = PI.cast(*PI.make(name), torch.float32, device)
    t["n"] = torch.tensor(t["n"], dtype=torch.int32)
    return t


@pytest.mark.parametrize("name", PR.CRITERION_CASES)
def test_through_the_criterion(device, name):
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlaneInstanceHeadsTrainer
    L, B, nq, h, w, s, n, _, _ = PI.CASES[name]
    assert nq == NQ
    r64, r32 = reference(name)
    tr = PlaneInstanceHeadsTrainer.from_state_dict(synth_state_dict(NQ), NQ, device)
    hs, p1 = (t.to(device).requires_grad_(True) for t in PR.seeded_inputs(name))
    losses, indices = tr.losses(hs, p1, _device_targets(name, device))
    mq = indices["match_q"].cpu()
    for l in range(L):                                            # the device's match = the float64 restatement's
        for b in range(B):
            src, tgt = r64["idx"][l][b]
            assert torch.equal(mq[l, b, : n[b]].long()[tgt], src), (l, b)
    assert set(losses) == set(r64["losses"]) and len(losses) == 6 * L + 2
    for k in sorted(losses):
        _gate(k, losses[k], r64["losses"][k], r32["losses"][k])
    grads = tr.backward(losses)
    assert sorted(grads) == sorted(r64["grads"]) and len(grads) == 24
    for k in sorted(grads):
        assert float(r64["grads"][k].abs().max()) > 0, k
        _gate("d " + k, grads[k], r64["grads"][k], r32["grads"][k])
    assert set(tr.input_grads) == {"hs", "p1"}
    for k in ("hs", "p1"):
        _gate("d " + k, tr.input_grads[k], r64["input_grads"][k], r32["input_grads"][k])
    # deterministic: a second pass gives the same bits
    hs2, p2 = (t.to(device).requires_grad_(True) for t in PR.seeded_inputs(name))
    again = tr.backward(tr.losses(hs2, p2, _device_targets(name, device))[0])
    assert all(torch.equal(grads[k], again[k]) for k in grads) and torch.equal(tr.input_grads["p1"], p2.grad)


def _head_targets(name, device, h, w, s=4):
    t = _device_targets(name, device)
    up = lambda x: torch.nn.functional.interpolate(x.float(), size=(s * h, s * w), mode="nearest")
    return {"masks": up(t["masks"]).to(torch.uint8), "n": t["n"], "plane_params": t["plane_params"], "depth": up(t["depth"][:, None])[:, 0],
            "k_inv_dot_xy1": up(t["k_inv_dot_xy1"])}


def test_step_and_write_back(device):
    """one optimiser step, write_back: the inference head at the new parameters gives the trainer's forward (a stale pe_fold would not);
    with SOLVER.SEM_SEG_HEAD_MULTIPLIER = 0 the parameters do not move"""
    from nopesac_amd.config import get_cfg
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlaneInstanceHeadsTrainer
    model = _private_model(device)
    head = model.sem_seg_head
    try:
        feats = _features(device, batch=2)
        hs, p1 = head.training_inputs(feats)
        tr = PlaneInstanceHeadsTrainer.from_head(head)
        before = {k: v.detach().clone() for k, v in tr.params.items()}
        with torch.no_grad():
            old, _ = head(feats, want_logits=True)
            old_logits = old["pred_mask_logits"].clone()
        targets = _head_targets("border_s4", device, p1.shape[1], p1.shape[2])
        losses, _ = tr.losses(hs, p1, targets)
        grads = tr.backward(losses)
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads.values())
        assert tr.input_grads == {}                                # hs / p1 did not ask for gradients
        frozen = get_cfg()
        frozen.SOLVER.SEM_SEG_HEAD_MULTIPLIER = 0.0
        tr.step_from_cfg(frozen)
        assert all(torch.equal(before[k], p.detach()) for k, p in tr.params.items())
        tr.state, tr.steps = {}, 0
        tr.step_from_cfg(get_cfg())
        assert all(not torch.equal(before[k], p.detach()) for k, p in tr.params.items())
        tr.write_back(head)
        s = _tie_in(head, tr, feats, hs, p1, tr.params)
        assert float((s["pred_mask_logits"][-1] - old_logits.permute(0, 3, 1, 2)).abs().max()) > 1e-3       # the step is visible
    finally:
        model.load_state_dict(synth_state_dict(NQ))


@pytest.mark.parametrize("name", ["square50", "q128"])
def test_wide_query_sets(device, name):
    """nq = 50 and nq = 128, one supervised layer: finite, non-zero gradients of every tensor and of both inputs"""
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlaneInstanceHeadsTrainer
    L, B, nq, h, w = PI.CASES[name][:5]
    assert L == 1
    tr = PlaneInstanceHeadsTrainer.from_state_dict(synth_state_dict(nq), nq, device)
    hs, p1 = (t.to(device).requires_grad_(True) for t in PR.seeded_inputs(name))
    losses, indices = tr.losses(hs, p1, _device_targets(name, device))
    assert "aux_outputs" not in tr.last and len(losses) == 8
    grads = tr.backward(losses)
    assert len(grads) == 24
    for k, g in list(grads.items()) + list(tr.input_grads.items()):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
