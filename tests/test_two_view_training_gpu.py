"""The two-view half of the training forward on the device (nopesac_amd/training.py: RefineTrainer.losses / camera_head_losses with
plane_grads, TwoViewLosses, joint_backward): nq = 50, B = 2, the synthetic checkpoint, the feature maps of
tests/test_training_gpu.py::test_camera_head_training_gradients.  The plane gradients are held to the float64 restatement of
tests/two_view_forms.py in the trainer-level form of the project (error over the tensor's own scale), the bound being LIMIT_FACTOR x the
float32 restatement's own error on these inputs (TRAINER_F32_ERR, measured on the CPU)."""
import functools

import numpy as np
import pytest
import torch

from tests import golden_inputs as GI
from tests import train_targets_forms as F
from tests import two_view_forms as T
from tests.util import make_model, nhwc

pytestmark = pytest.mark.gpu
NQ, B = T.TRAIN_CASE["nq"], len(T.TRAIN_CASE["ms"])
H, W, h, w = 24, 32, 6, 8


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _camera_args(c, device, planes=None):
    d = lambda k: c[k].to(device)
    p1, p2 = planes if planes is not None else (d("planes1"), d("planes2"))
    return (d("gt_planes1"), d("gt_planes2"), d("n1"), d("n2"), d("gt_A"), d("gt_pose"), p1, p2, d("n1"), d("n2"), d("A"), d("rand_rot"), d("rand_trans"))


def _feats(c, device):
    return {k: torch.cat([nhwc(c["feats1"][k]), nhwc(c["feats2"][k])]).to(device) for k in ("res3", "res4", "res5")}


def test_plane_grads_switch_of_the_camera_head(device):
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import CameraHeadTrainer
    c, sd = T.train_case(), synth_state_dict(NQ)
    head = make_model(device).camera_head_list[0]
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True)
    assert len(tr.params) == 179
    feats = _feats(c, device)
    # off: the call as it was, and the keyword spelled out
    losses0 = tr.camera_head_losses(head, feats, B, *_camera_args(c, device))
    grads0 = {k: v.clone() for k, v in tr.backward(losses0).items()}
    losses1 = tr.camera_head_losses(head, feats, B, *_camera_args(c, device), plane_grads=False)
    grads1 = tr.backward(losses1)
    assert len(losses0) == 34 and set(losses0) == set(losses1) and all(_bits(losses0[k].detach(), losses1[k].detach()) for k in losses0)
    assert all(_bits(grads0[k], grads1[k]) for k in grads0) and "planes1" not in tr.input_grads
    # on: the losses and the 179 parameter gradients keep their bits, the planes get theirs
    planes = tuple(c[k].to(device).requires_grad_(True) for k in ("planes1", "planes2"))
    losses2 = tr.camera_head_losses(head, feats, B, *_camera_args(c, device, planes), plane_grads=True)
    grads2 = tr.backward(losses2)
    assert all(_bits(losses0[k].detach(), losses2[k].detach()) for k in losses0)
    assert all(_bits(grads0[k], grads2[k]) for k in grads0)
    assert {"planes1", "planes2"} <= set(tr.input_grads)
    _, r1, r2 = T.camera_aux_restated(sd, c, NQ, head.plane_cam_weight_predplane, torch.float64, conv_feats=[t.cpu() for t in tr.conv_feats])
    for k, ref in (("planes1", r1), ("planes2", r2)):
        got = tr.input_grads[k].cpu()
        err, bound = T.scale_error(got, ref), T.LIMIT_FACTOR * T.TRAINER_F32_ERR[k]
        print("%s: error over scale %.3e, bound %.3e, scale %.3e" % (k, err, bound, float(ref.abs().max())))
        live = ref.abs().sum(-1) > 0
        assert int(live.sum()) == sum(T.TRAIN_CASE["ms"]) and bool((got[~live] == 0).all())      # matched planes only, exact zeros elsewhere
        assert err <= bound, (k, err, bound)
    # the GT planes are data: asking for plane gradients without an _Aux pass watches nothing
    tr.camera_head_losses(head, feats, B, *_camera_args(c, device)[:6], plane_grads=True)
    assert "planes1" not in tr._inputs


# ---- TwoViewLosses behind the plane head's instance heads ------------------------------------------------------------------------------------
def _records(seed, counts):
    recs = []
    rng = np.random.default_rng(seed)
    for i, k in enumerate(counts):
        sem = F.partition(H, W, list(range(2, 2 + k)), seed + i)
        planes = rng.standard_normal((k, 3))
        planes = planes / np.linalg.norm(planes, axis=1, keepdims=True) * (1.0 + 2.0 * rng.random((k, 1)))
        recs.append({"image_id": "v%d_%d" % (seed, i), "semantic_map": sem, "depth": np.full((H, W), 2.0, np.float32) + rng.random((H, W)).astype(np.float32),
                     "annotations": [{"plane": planes[j].tolist(), "category_id": 0} for j in range(k)]})
    return recs


def _entries(no_match_pair=None):
    v1, v2 = _records(40, (5, 7)), _records(50, (6, 4))
    corrs = [[(0, 1), (2, 3), (4, 0), (1, 5)], [(0, 0), (3, 2), (6, 1)]]
    if no_match_pair is not None:
        corrs[no_match_pair] = []
    poses = [{"position": [0.3, -0.1, 0.2], "rotation": [0.9, 0.1, -0.3, 0.2]}, {"position": [-0.2, 0.4, 0.1], "rotation": [0.8, -0.2, 0.1, 0.5]}]
    return [{"0": v1[b], "1": v2[b], "gt_corrs": corrs[b], "rel_pose": poses[b]} for b in range(B)]


@functools.lru_cache(maxsize=None)
def _setup(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.targets import TargetMapper
    from nopesac_amd.training import CameraHeadTrainer, MatchingHeadTrainer, PlaneInstanceHeadsTrainer, TwoViewLosses
    model = make_model(device)
    head = model.camera_head_list[0]
    heads = PlaneInstanceHeadsTrainer.from_head(model.sem_seg_head)
    matcher = MatchingHeadTrainer.from_head(model.matching_head)
    camera = CameraHeadTrainer.from_head(head)
    g = torch.Generator().manual_seed(123)
    hs = torch.randn(1, 2 * B, NQ, 256, generator=g).to(device)
    p1 = torch.relu(torch.randn(2 * B, h, w, 256, generator=g)).to(device)
    mapper = TargetMapper.from_cfg(get_cfg(), device)
    return dict(model=model, head=head, heads=heads, matcher=matcher, camera=camera, two_view=TwoViewLosses(matcher, camera, head), hs=hs, p1=p1,
                mapper=mapper, feats=_feats(T.train_case(), device))


def _forward(s, pair, hs, p1, seed=0, step=0):
    plane_losses, idx = s["heads"].losses(hs, p1, pair["targets"])
    mq, n = idx["match_q"][0], pair["targets"]["n"]
    tv = s["two_view"].losses(hs[-1], s["heads"].last["pred_params"], mq[:B], mq[B:], n[:B], n[B:], pair, s["feats"], B, seed=seed, step=step)
    return plane_losses, tv


CAMERA_LOSSES = 32


def test_two_view_losses_on_one_graph(device):
    from nopesac_amd.optim import ModelOptimizer
    from nopesac_amd.training import joint_backward
    s = _setup(device)
    heads, matcher, camera = s["heads"], s["matcher"], s["camera"]
    pair = s["mapper"].pair_targets(_entries())
    hs, p1 = s["hs"].clone().requires_grad_(True), s["p1"].clone().requires_grad_(True)
    plane_losses, tv = _forward(s, pair, hs, p1)
    s["two_view"].check()
    names = set(tv)
    assert "losses_emb_0" in names and len(names) == 1 + CAMERA_LOSSES and not any("randCamRec" in k for k in names)
    for sfx in ("", "_Aux"):
        for stage in ("initCamRef", "initRecCamRef"):
            assert "loss_paramL2_dist_%s%s" % (stage, sfx) in names and "loss_tran_planeSoftReg_%s%s" % (stage, sfx) in names
    assert {"loss_tran_pixelReg", "loss_rot_pixelReg", "loss_rot_initCamRec", "loss_trans_initCamRec"} <= names
    assert all(bool(torch.isfinite(v)) for v in tv.values()) and float(tv["losses_emb_0"].detach()) > 0
    weighted = heads.criterion.weighted(plane_losses)
    grads = joint_backward([heads, matcher, camera], {**weighted, **tv})
    assert set(grads) == set(heads.params) | set(matcher.params) | set(camera.params)
    for t in (heads, matcher, camera):
        assert set(t.grads) == set(t.params) and all(bool(torch.isfinite(g).all()) for g in t.grads.values())
        assert sum(float(g.abs().max()) > 0 for g in t.grads.values()) > len(t.grads) // 2
    assert {"planes1", "planes2"} <= set(camera.input_grads) and "app" in matcher.input_grads
    joint_hs = heads.input_grads["hs"].clone()
    joint_param = {k: v.clone() for k, v in heads.grads.items() if ".plane_param." in k}
    assert joint_param
    # the three alone: the criterion, the matcher, the camera head - their gradients at hs add up to the joint one
    parts = []
    for pick in ("criterion", "matcher", "camera"):
        hs_i, p1_i = s["hs"].clone().requires_grad_(True), s["p1"].clone().requires_grad_(True)
        pl, tv_i = _forward(s, pair, hs_i, p1_i)
        sel = {"criterion": heads.criterion.weighted(pl), "matcher": {"losses_emb_0": tv_i["losses_emb_0"]},
               "camera": {k: v for k, v in tv_i.items() if k != "losses_emb_0"}}[pick]
        joint_backward([heads, matcher, camera], sel)
        parts.append(heads.input_grads["hs"].clone())
        if pick == "criterion":
            alone_param = {k: v.clone() for k, v in heads.grads.items() if ".plane_param." in k}
    assert all(float(p.abs().max()) > 0 for p in parts)
    total, mag = parts[0] + parts[1] + parts[2], parts[0].abs() + parts[1].abs() + parts[2].abs()
    # f32 rounding of the sum: the camera's share reaches hs through the three 256-wide Linears of plane_param, summed with the criterion's in
    # front of them in the joint pass and behind them here - 3 x 256 x 2^-24 = 4.6e-5 of the magnitudes, factor 2
    err = float((joint_hs - total).abs().max())
    print("joint hs gradient: |joint - sum of three| %.3e, bound %.3e" % (err, 1e-4 * float(mag.max())))
    assert err <= 1e-4 * float(mag.max())
    assert all(not torch.equal(joint_param[k], alone_param[k]) for k in joint_param)               # the camera losses train plane_param
    # one optimiser step over the three trainers moves plane_param
    try:
        before = {k: heads.params[k].detach().clone() for k in joint_param}
        plane_losses, tv = _forward(s, pair, hs, p1)
        joint_backward([heads, matcher, camera], {**heads.criterion.weighted(plane_losses), **tv})
        opt = ModelOptimizer([heads, matcher, camera], max_norm=1.0)
        coef = opt.step(lr=1e-4)
        assert bool(torch.isfinite(coef).all()) and opt.steps == 1
        assert all(not torch.equal(before[k], heads.params[k].detach()) for k in before)
    finally:
        _setup.cache_clear()                                    # the stepped trainers are not handed to another test


def test_random_pose_losses_follow_the_head_switch(device):
    s = _setup(device)
    pair = s["mapper"].pair_targets(_entries())
    head = s["head"]
    old = head.rand_cam_on
    try:
        head.rand_cam_on = True
        with torch.no_grad():
            _, tv = _forward(s, pair, s["hs"], s["p1"], seed=5, step=9)
            _, again = _forward(s, pair, s["hs"], s["p1"], seed=5, step=9)
            _, other = _forward(s, pair, s["hs"], s["p1"], seed=5, step=10)
    finally:
        head.rand_cam_on = old
    extra = {"loss_rot_randCamRecLBS_N1", "loss_trans_randCamRecLBS_N1"}
    assert extra <= set(tv) and len(tv) == 1 + CAMERA_LOSSES + 2
    assert all(_bits(tv[k], again[k]) for k in tv)
    assert all(not _bits(tv[k], other[k]) for k in extra) and all(_bits(tv[k], other[k]) for k in set(tv) - extra)


def test_a_pair_without_correspondences(device):
    """A pair whose gt_corrs match nothing: finite losses everywhere, and the camera head's gradients at that pair's planes are exact
    zeros (its sequences are empty: the refinement losses leave the pair out, the convention matching_losses has for a batch that selects
    nothing).  The matcher's share of that pair is NOT zero: plane_corr_matrix sends every plane of such a pair to the dustbin, and the
    embedding loss supervises those entries - finite, and checked as such."""
    from nopesac_amd.training import joint_backward
    s = _setup(device)
    heads, matcher, camera = s["heads"], s["matcher"], s["camera"]
    pair = s["mapper"].pair_targets(_entries(no_match_pair=1))
    hs, p1 = s["hs"].clone().requires_grad_(True), s["p1"].clone().requires_grad_(True)
    _, tv = _forward(s, pair, hs, p1)
    print({k: float(v.detach()) for k, v in tv.items()})
    assert all(bool(torch.isfinite(v)) for v in tv.values()), {k: float(v.detach()) for k, v in tv.items() if not bool(torch.isfinite(v))}
    grads = joint_backward([heads, matcher, camera], tv)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and bool(torch.isfinite(heads.input_grads["hs"]).all())
    for k in ("planes1", "planes2"):                            # the camera head's share: pair 0 is live, pair 1 gets exact zeros
        g = camera.input_grads[k]
        assert float(g[0].abs().max()) > 0 and float(g[1].abs().max()) == 0, k
    # the matcher's share of that pair is what plane_corr_matrix supervises without a correspondence: every plane against the dustbin
    joint_backward([heads, matcher, camera], {"losses_emb_0": _forward(s, pair, hs, p1)[1]["losses_emb_0"]})
    assert bool(torch.isfinite(heads.input_grads["hs"]).all())
