"""CameraHeadTrainer(conv_stacks=True): the whole training-mode camera head with the pixel pose net's conv stacks trainable (179
tensors; reference __forward_PixelCameraHead, camera_net/camera_head.py:642-683, trained in the step-2 / step-3 recipe) against float64
autograd on the oracle's pixel pose net, the solver's norm parameter groups against torch.optim.AdamW, and the inference head after
write_back."""
import pytest
import torch

from tests import golden_inputs as GI
from tests.test_training_gpu import _oracle_camera_head_train_like_the_reference
from tests.util import rel_err

pytestmark = pytest.mark.gpu
P = "camera_head_list.0."


def _setup(device, ms=(7, 2)):
    from nopesac_amd.synth import synth_state_dict
    from tests.util import make_model, nhwc
    nq = 50
    c = GI.camera_train_case(nq, ms, 80)
    sd = synth_state_dict(nq)
    model = make_model(device)
    head = model.camera_head_list[0]
    feats = {k: torch.cat([nhwc(c["feats1"][k]), nhwc(c["feats2"][k])]).to(device) for k in ("res3", "res4", "res5")}
    return nq, c, sd, model, head, feats


def _losses(tr, head, feats, c, device):
    d = lambda k: c[k].to(device)
    B = c["gt_pose"].shape[0]
    return tr.camera_head_losses(head, feats, B, d("gt_planes1"), d("gt_planes2"), d("n1"), d("n2"), d("gt_A"), d("gt_pose"), d("planes1"),
                                 d("planes2"), d("n1"), d("n2"), d("A"), d("rand_rot"), d("rand_trans"))


def _record_bn_layer_outputs(tr):
    """Wrap tr._cbl so that every conv / BN / LeakyReLU output of the next forward is kept (detached), by layer name."""
    rec, orig = {}, tr._cbl

    def cbl(x, name, stride=1):
        y = orig(x, name, stride)
        rec[name] = y.detach().permute(0, 3, 1, 2).double().cpu()
        return y

    tr._cbl = cbl
    return rec


class _KinkConsistentLeakyBN:
    """The oracle's conv + BN + LeakyReLU in float64, except that an activation within f32 rounding of the kink (|z| <= 1e-5 max |z|)
    takes the side the f32 forward took.  A pre-activation of 3e-7 can land on either side of zero in f32 (the case below has one in
    convs_rots.2), and the two sides differ by 0.99 in the derivative: that is the forward's rounding, not the backward's."""

    def __init__(self, rec, B):
        from oracle import nopesac_oracle as O
        self.O, self.rec, self.B, self.calls = O, rec, B, {}

    def __call__(self, x, sd, p, stride=1):
        import torch.nn.functional as F
        O = self.O
        z = O.eval_bn(F.conv2d(x, sd[p + ".0.weight"], None, stride, 1), sd, p + ".1", 1e-3)
        name = p[len(P):]
        ref = self.rec[name]
        if ref.shape[0] != z.shape[0]:                     # the siamese tower: view 1 images first, then view 2
            i = self.calls.get(name, 0)
            self.calls[name] = i + 1
            ref = ref[i * self.B:(i + 1) * self.B]
        near = z.detach().abs() <= 1e-5 * z.detach().abs().max()
        pos = torch.where(near, ref > 0, z.detach() > 0)
        return torch.where(pos, z, 0.01 * z)


def test_all_179_gradients_and_losses_match_the_oracle(device, monkeypatch):
    from nopesac_amd.training import CameraHeadTrainer
    from oracle import nopesac_oracle as O
    nq, c, sd, model, head, feats = _setup(device)
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True)
    names = list(tr.params)
    assert len(names) == 179
    rec = _record_bn_layer_outputs(tr)
    losses = _losses(tr, head, feats, c, device)
    grads = tr.backward(losses)
    monkeypatch.setattr(O, "_conv_bn_lrelu", _KinkConsistentLeakyBN(rec, c["gt_pose"].shape[0]))
    torch.set_default_dtype(torch.float64)
    try:
        o_loss, o_grads = _oracle_camera_head_train_like_the_reference(sd, c, nq, head, names)
    finally:
        torch.set_default_dtype(torch.float32)
    assert set(losses) == set(o_loss) and len(losses) == 34
    for k in o_loss:
        assert rel_err(losses[k].detach(), o_loss[k].float().detach()) < 1e-2, (k, float(losses[k]), float(o_loss[k]))
    gmax = max(float(o_grads[k].abs().max()) for k in names)
    report = []
    for k in names:
        ref = o_grads[k].float()
        assert torch.isfinite(grads[k]).all(), k
        assert grads[k].shape == ref.shape, k
        report.append((float((grads[k].cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax), k))
    report.sort(reverse=True)
    assert report[0][0] < 3e-3, report[:6]
    # the conv stacks really do receive gradients (the frozen default gives none of these keys)
    assert all(float(grads[k].abs().max()) > 0 for k in names if k.startswith(P + "convs_") or k.startswith(P + "pixel_decoder."))


def test_feature_gradients_match_the_oracle(device, monkeypatch):
    from nopesac_amd.training import CameraHeadTrainer
    from oracle import nopesac_oracle as O
    nq, c, sd, model, head, feats = _setup(device)
    B = 2
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True, feature_grads=True)
    rec = _record_bn_layer_outputs(tr)
    fm = {k: v.detach().float().clone().requires_grad_(True) for k, v in feats.items()}
    g = torch.Generator().manual_seed(1)
    r1, r2 = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
    yt, yr = tr.pixel_pose_convs(fm, B)
    _, _, tf, rf = tr.pixel_pose(yt.contiguous(), yr.contiguous())
    ((tf * r1.to(device)).sum() + (rf * r2.to(device)).sum()).backward()
    sdd = {k: v.double() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    f1 = {k: v.double().requires_grad_(True) for k, v in c["feats1"].items()}
    f2 = {k: v.double().requires_grad_(True) for k, v in c["feats2"].items()}
    torch.set_default_dtype(torch.float64)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(O, "_conv_bn_lrelu", _KinkConsistentLeakyBN(rec, B))
            _, _, otf, orf, _ = O.pixel_pose_net(sdd, f1, f2, P[:-1])
        ((otf * r1.double()).sum() + (orf * r2.double()).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    for k in ("res3", "res4", "res5"):
        ref = torch.cat([f1[k].grad, f2[k].grad]).permute(0, 2, 3, 1)
        assert rel_err(fm[k].grad, ref) < 3e-3, k
    # ... and through camera_head_losses: input_grads holds the three maps
    losses = _losses(tr, head, feats, c, device)
    tr.backward(losses)
    assert set(tr.input_grads) == {"res3", "res4", "res5"}
    assert all(tr.input_grads[k].shape == feats[k].shape and torch.isfinite(tr.input_grads[k]).all() for k in tr.input_grads)


def test_step_from_cfg_uses_the_norm_weight_decay(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.training import CameraHeadTrainer, is_norm_parameter
    nq, c, sd, model, head, feats = _setup(device)
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True)
    g = torch.Generator().manual_seed(2)
    ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in tr.params.items()}
    for k, p in tr.params.items():
        gr = torch.randn(p.shape, generator=g)
        p.grad = gr.to(device)
        ref[k].grad = gr.clone()
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.OPTIMIZER", "ADAMW", "SOLVER.BASE_LR", 0.01, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.WEIGHT_DECAY_NORM", 0.5,
                         "SOLVER.CLIP_GRADIENTS.ENABLED", False])
    groups = [{"params": [ref[k]], "weight_decay": 0.5 if is_norm_parameter(k) else 0.05} for k in ref]      # train_NopeSAC.py:116-131
    opt = torch.optim.AdamW(groups, lr=0.01)
    for _ in range(2):
        tr.step_from_cfg(cfg)
        opt.step()
    for k in ref:
        assert float((tr.params[k].detach().cpu() - ref[k].detach()).abs().max()) < 2e-6, k


def test_write_back_reaches_the_inference_pixel_pose_net_and_sgd_lowers_the_pixel_losses(device):
    from nopesac_amd.training import CameraHeadTrainer
    from oracle import nopesac_oracle as O
    nq, c, sd, model, head, feats = _setup(device)
    B = 2
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True)
    pix = ("loss_tran_pixelReg", "loss_rot_pixelReg")
    try:
        first = None
        for it in range(20):
            losses = _losses(tr, head, feats, c, device)
            cur = float(sum(losses[k].detach() for k in pix))
            first = cur if first is None else first
            tr.backward(losses, {k: (1.0 if k in pix else 0.0) for k in losses})
            tr.clip_grad_norm(1.0)
            tr.step(lr=5e-3, optimizer="SGD", weight_decay=0.0, momentum=0.0)
        last = float(sum(_losses(tr, head, feats, c, device)[k].detach() for k in pix))
        assert last < first, (first, last)
        tr.write_back(head)
        sd2 = {k: v.clone() for k, v in sd.items()}
        for k, p in tr.params.items():
            sd2[k] = p.detach().cpu().clone()
        with torch.no_grad():
            t0, _, tf, rf = head.pixel_pose_net(feats, B)
            ot, _, otf, orf, _ = O.pixel_pose_net(sd2, c["feats1"], c["feats2"], P[:-1])
        assert rel_err(tf, otf) < 1e-3 and rel_err(rf, orf) < 1e-3 and rel_err(t0, ot) < 1e-3
        assert not torch.equal(tr.params[P + "convs_backbone.0.0.weight"].detach().cpu(), sd[P + "convs_backbone.0.0.weight"])
    finally:                                                  # (tests/util.make_model caches the model: hand it back with its checkpoint)
        model.load_state_dict(sd)
