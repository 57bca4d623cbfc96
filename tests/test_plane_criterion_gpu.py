"""The plane head's set criterion on the device (csrc/plane_criterion.hip, nopesac_amd/training.py::PlaneCriterion) against the float64
restatement tests/plane_criterion_ref.py (pinned to the reference by tests/test_plane_criterion_cpu.py).  Error rule, as
tests/test_matcher_training_gpu.py: |kernel - f64| <= max(10 e32, 1e-6 max|f64|), e32 = the error of the same restatement run in float32."""
import functools

import numpy as np
import pytest
import torch

from tests import golden_inputs as GI
from tests import plane_criterion_inputs as PI
from tests import plane_criterion_ref as R
from tests.util import make_model, nhwc

pytestmark = pytest.mark.gpu

OUT_KEYS = ("pred_logits", "pred_mask_logits", "pred_centers", "pred_params", "pixel_centers")


def _criterion():
    from nopesac_amd.config import get_cfg
    from nopesac_amd.training import PlaneCriterion
    return PlaneCriterion.from_cfg(get_cfg())


def _leaves(outputs):
    layers = [outputs] + list(outputs.get("aux_outputs", []))
    return [(l, k, o[k]) for l, o in enumerate(layers) for k in OUT_KEYS if k in o]


def _restated(name, dtype, indices=None):
    """losses, per-leaf gradients of the weighted sum, indices, costs of the restatement in `dtype`"""
    crit = _criterion()
    o, t = PI.cast(*PI.make(name), dtype)
    for _, _, v in _leaves(o):
        v.requires_grad_(True)
    losses, idx, costs = R.criterion(o, t, indices=indices)
    total = sum(v * crit.weight_dict[k] for k, v in losses.items())
    grads = torch.autograd.grad(total, [v for _, _, v in _leaves(o)], allow_unused=True)
    return ({k: v.detach() for k, v in losses.items()}, {(l, k): g for (l, k, _), g in zip(_leaves(o), grads)}, idx,
            [[c.detach() for c in layer] for layer in costs])


@functools.lru_cache(maxsize=None)
def reference(name):
    l64, g64, idx, c64 = _restated(name, torch.float64)
    l32, g32, _, c32 = _restated(name, torch.float32, indices=idx)
    return dict(l64=l64, g64=g64, idx=idx, c64=c64, l32=l32, g32=g32, c32=c32)


def run_device(name, device, head_layout=False, only=None):
    crit = _criterion()
    o, t = PI.cast(*PI.make(name), torch.float32, device)
    if head_layout:
        o["pred_mask_logits"] = o["pred_mask_logits"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        o["pixel_centers"] = o["pixel_centers"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    for _, _, v in _leaves(o):
        v.requires_grad_(True)
    t["n"] = torch.tensor(t["n"], dtype=torch.int32)
    losses, indices = crit(o, t)
    total = losses[only] if only else sum(crit.weighted(losses).values())
    grads = torch.autograd.grad(total, [v for _, _, v in _leaves(o)], allow_unused=True)
    return ({k: v.detach().cpu() for k, v in losses.items()}, {(l, k): (None if g is None else g.cpu()) for (l, k, _), g in zip(_leaves(o), grads)},
            indices, crit.last["cost"].cpu(), crit)


def _gate(what, got, r64, r32):
    e32 = float((r32.double() - r64).abs().max())
    ek = float((got.double() - r64).abs().max())
    tol = max(10 * e32, 1e-6 * float(r64.abs().max()))
    print("%-34s kernel %.3e  f32 torch %.3e  tol %.3e" % (what, ek, e32, tol))
    assert ek <= tol, (what, ek, e32, tol)


@pytest.mark.parametrize("name", list(PI.CASES))
def test_costs_assignment_losses_and_gradients(device, name):
    from scipy.optimize import linear_sum_assignment
    L, B, nq, h, w, s, n, no_valid, _ = PI.CASES[name]
    ref = reference(name)
    losses, grads, indices, cost, crit = run_device(name, device)
    mq, mg = indices["match_q"].cpu(), indices["match_gt"].cpu()
    for l in range(L):
        for b in range(B):
            _gate("cost[%d,%d]" % (l, b), cost[l, b, :, : n[b]], ref["c64"][l][b], ref["c32"][l][b])
            src, tgt = ref["idx"][l][b]
            q_of = mq[l, b, : n[b]].long()
            assert torch.equal(q_of[tgt], src), (l, b, q_of, src, tgt)                      # scipy's match on the float64 costs
            assert bool((mq[l, b, n[b]:] == -1).all()) and len(set(q_of.tolist())) == n[b]  # every target once, no query twice
            back = mg[l, b].long()
            assert sorted(back[back >= 0].tolist()) == list(range(n[b])) and torch.equal(back[q_of], torch.arange(n[b]))
            own = cost[l, b, :, : n[b]].double().numpy()
            i, j = linear_sum_assignment(own)
            mine, best = float(own[q_of.numpy(), np.arange(n[b])].sum()), float(own[i, j].sum())
            assert abs(mine - best) <= 1e-5 * abs(best), (mine, best)
    ref_pairs = crit.indices_as_reference(indices)
    for b in range(B):
        assert torch.equal(ref_pairs[b][0], ref["idx"][0][b][0]) and torch.equal(ref_pairs[b][1], ref["idx"][0][b][1])
    assert set(losses) == set(ref["l64"]) and len(losses) == 6 * L + 2
    for k in sorted(losses):
        _gate(k, losses[k], ref["l64"][k], ref["l32"][k])
    for (l, k), g in grads.items():
        g64 = ref["g64"][(l, k)]
        _gate("d %s[%d]" % (k, l), g, g64, ref["g32"][(l, k)])
        assert float(g64.abs().max()) > 0
        if k in ("pred_mask_logits", "pred_centers", "pred_params"):
            for b in range(B):
                free = mg[l, b] < 0
                assert float(g64[b][free].abs().max() if free.any() else 0.0) == 0.0
                assert float(g[b][free].abs().max() if free.any() else 0.0) == 0.0, (l, k, b)          # exactly zero where the reference's is
        if k == "pred_mask_logits" and (h, w) == (6, 8):
            matched = g[mg[l] >= 0]
            border = torch.cat([matched[:, 0].flatten(), matched[:, -1].flatten(), matched[:, :, 0].flatten(), matched[:, :, -1].flatten()])
            assert bool((border != 0).all())
    again = run_device(name, device)
    assert all(torch.equal(losses[k], again[0][k]) for k in losses)                           # deterministic: bit-identical runs
    assert all(torch.equal(g, again[1][key]) for key, g in grads.items())


def test_q_loss_image_without_valid_pixels_contributes_nothing(device):
    L, B, nq, h, w, s, n, no_valid, _ = PI.CASES["border_s4"]
    assert no_valid == [1]
    losses, grads, indices, _, crit = run_device("border_s4", device, only="loss_q")
    g = grads[(0, "pred_params")]
    assert float(losses["loss_q"]) > 0 and float(g[0].abs().max()) > 0 and float(g[1].abs().max()) == 0.0
    ref = reference("border_s4")
    assert float(ref["l64"]["loss_q"]) > 0
    _gate("loss_q", losses["loss_q"], ref["l64"]["loss_q"], ref["l32"]["loss_q"])


def test_head_stride_order_gives_the_same_bits(device):
    a = run_device("square50", device)
    b = run_device("square50", device, head_layout=True)
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert torch.equal(a[2]["match_q"], b[2]["match_q"]) and torch.equal(a[3], b[3])
    for key, g in a[1].items():
        assert torch.equal(g, b[1][key].contiguous()), key
    assert b[1][(0, "pred_mask_logits")].stride() != a[1][(0, "pred_mask_logits")].stride()      # the gradient comes back in the head's order


def _corr_case(nq, device):
    """two views, three pairs: a gt plane index >= 50, a plane unmatched in one view (index >= n), one view with all planes matched"""
    g = torch.Generator().manual_seed(5)
    n1, n2 = [4, 6, 50], [5, 3, 50]
    nmax = 50

    def match(n):
        mq = torch.full((3, nmax), -1, dtype=torch.int32)
        for b, nb in enumerate(n):
            mq[b, :nb] = torch.randperm(nq, generator=g)[:nb].to(torch.int32)
        return mq
    m1, m2 = match(n1), match(n2)
    corrs = [[(0, 1), (2, 0), (3, 4)], [(1, 2), (5, 0), (4, 2), (0, 4)], [(j, (j * 7) % 50) for j in range(0, 50, 3)] + [(51, 2), (3, 60)]]
    K = max(len(c) for c in corrs)
    pad = torch.full((3, K, 2), -1, dtype=torch.int32)
    for b, c in enumerate(corrs):
        pad[b, : len(c)] = torch.tensor(c, dtype=torch.int32)
    as_ref = lambda mq, n: [(mq[b, :nb].long(), torch.arange(nb)) for b, nb in enumerate(n)]
    return corrs, pad, m1, m2, as_ref(m1, n1), as_ref(m2, n2)


def test_plane_corr_matrix_and_the_matching_trainer(device, sd50):
    from nopesac_amd.training import MatchingHeadTrainer, plane_corr_matrix
    nq = 50
    corrs, pad, m1, m2, idx1, idx2 = _corr_case(nq, device)
    want = R.plane_corr_matrix(corrs, idx1, idx2, nq)
    got = plane_corr_matrix(pad.to(device), m1.to(device), m2.to(device), nq)
    assert got.dtype == torch.uint8 and got.shape == (3, nq + 1, nq + 1) and torch.equal(got.cpu().bool(), want)
    assert bool(want[:, :nq, :nq].any()) and bool(want[0, :, nq].any()) and bool(want[0, nq, :].any())
    # device indices of the criterion -> gt_corr -> the matching head's loss
    _, _, indices, _, _ = run_device("square50", device)
    mq = indices["match_q"][0].expand(2, -1).contiguous()
    gt = plane_corr_matrix(torch.tensor([[[0, 1], [2, 2], [5, 9]], [[1, 1], [3, 0], [-1, -1]]], dtype=torch.int32, device=device), mq, mq, nq)
    g = torch.Generator().manual_seed(9)
    tr = MatchingHeadTrainer.from_state_dict(sd50, nq, device)
    app = torch.randn(4, nq, 256, generator=g).to(device).requires_grad_(True)
    n_all = torch.full((4,), nq, dtype=torch.int32, device=device)
    planes = lambda: (torch.nn.functional.normalize(torch.randn(2, nq, 3, generator=g), dim=-1) * (1 + torch.rand(2, nq, 1, generator=g))).to(device)
    cam7 = torch.cat([0.3 * torch.randn(2, 3, generator=g), torch.nn.functional.normalize(torch.randn(2, 4, generator=g), dim=-1)], 1).to(device)
    loss = tr.matching_losses(app, n_all, cam7, planes(), planes(), gt, suffix="t", iterations=20)["losses_emb_t"]
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0 and bool(torch.isfinite(app.grad).all()) and float(app.grad.abs().max()) > 0


def test_plane_head_outputs_through_the_criterion(device):
    """PlaneTRHead.forward(want_logits=True) on the synthetic checkpoint at the smallest feature size -> PlaneCriterion -> backward"""
    model = make_model(device)
    feats = GI.feature_maps(21, 6, 8, batch=2)
    with torch.no_grad():
        out, _ = model.sem_seg_head({k: nhwc(v).to(device) for k, v in feats.items()}, want_logits=True)
    B, h, w, nq = out["pred_mask_logits"].shape
    o = {"pred_logits": out["pred_logits"].float().clone(), "pred_centers": out["pred_centers"].float().clone(),
         "pred_params": out["pred_params"].float().clone(), "pred_mask_logits": out["pred_mask_logits"].permute(0, 3, 1, 2),
         "pixel_centers": out["pixel_centers"].permute(0, 3, 1, 2)}
    for v in o.values():
        v.requires_grad_(True)
    _, t = PI.cast(*PI.make("border_s4"), torch.float32, device)
    s = 4
    up = lambda x: torch.nn.functional.interpolate(x.float(), size=(s * h, s * w), mode="nearest")
    targets = {"masks": up(t["masks"]).to(torch.uint8), "n": t["n"], "plane_params": t["plane_params"], "depth": up(t["depth"][:, None])[:, 0],
               "k_inv_dot_xy1": up(t["k_inv_dot_xy1"])}
    crit = _criterion()
    losses, indices = crit(o, targets)
    assert len(losses) == 8 and all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(crit.weighted(losses).values()).backward()
    for k, v in o.items():
        assert v.grad is not None and v.grad.shape == v.shape and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, k
