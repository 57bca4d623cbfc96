"""CameraHeadTrainer(conv_stacks=True, batch_stats=True): the training-mode camera head with the pixel pose net's 18 conv + BatchNorm +
LeakyReLU blocks on BATCH statistics (per view in the siamese tower), held to the oracle's own pixel pose net and training-mode head in
float64 with its _conv_bn_lrelu replaced by F.batch_norm(training=True, momentum 0.01, eps 1e-3) (tests/camera_bn_forms.py): all 179
gradients and 34 losses, the 36 running buffers and 18 counters after one and after three iterations, the stored-statistics path on the
trainer's own buffers, the inference head after write_back, descent, and the whole-model optimiser.  The case of
tests/test_pose_net_training_gpu.py: B = 2, res5 at 15 x 20, the synthetic checkpoint."""
import functools

import pytest
import torch

from tests import camera_bn_forms as F
from tests.test_pose_net_training_gpu import _losses, _record_bn_layer_outputs, _setup
from tests.util import rel_err

pytestmark = pytest.mark.gpu
P = F.CAM + "."
BN_LAYERS = F.TOWER + F.BRANCHES


def _same_bits(a, b):
    if not a.is_floating_point():
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _trainer(head, **kw):
    from nopesac_amd.training import CameraHeadTrainer
    return CameraHeadTrainer.from_head(head, conv_stacks=True, **kw)


def _snapshot(tr):
    return {k: v.detach().clone() for k, v in tr.buffers.items()}


@functools.lru_cache(maxsize=None)
def _one_iteration(device):
    """One training iteration of a fresh batch_stats trainer, shared by the tests that only read it: the trainer, the recorded block
    outputs, the losses and gradients, and the buffers before and after."""
    nq, c, sd, model, head, feats = _setup(device)
    tr = _trainer(head, batch_stats=True)
    before = _snapshot(tr)
    rec = _record_bn_layer_outputs(tr)
    losses = _losses(tr, head, feats, c, device)
    grads = {k: v.detach().clone() for k, v in tr.backward(losses).items()}
    del tr._cbl                                                # (the recorder; the class's method is back)
    return dict(nq=nq, c=c, sd=sd, model=model, head=head, feats=feats, tr=tr, rec=rec, before=before, after=_snapshot(tr),
                losses={k: v.detach().clone() for k, v in losses.items()}, grads=grads)


def test_all_179_gradients_and_losses_match_the_oracle_under_batch_statistics(device):
    """against float64 autograd; where float64 cannot decide - a LeakyReLU pre-activation, the two largest values of a max-pool window
    within float32 rounding - it takes the float32 forward's side.  Per tensor max(3e-3, LIMIT_FACTOR x the float32 torch
    restatement's own error)."""
    s = _one_iteration(device)
    names = list(s["tr"].params)
    assert len(names) == 179 and len(s["rec"]) == 18
    o_loss, o_grads, block = F.float64_like(s["sd"], s["c"], s["nq"], s["head"], names, s["rec"])
    assert set(s["losses"]) == set(o_loss) and len(o_loss) == 34
    for k in o_loss:
        assert rel_err(s["losses"][k], o_loss[k].float()) < 1e-2, (k, float(s["losses"][k]), float(o_loss[k]))
    assert all(torch.isfinite(s["grads"][k]).all() and s["grads"][k].shape == o_grads[k].shape for k in names)
    err = F.grad_errors(s["grads"], o_grads, names)
    report = sorted(((err[k] / F.grad_bound(k), err[k], k) for k in names), reverse=True)
    print("worst error / bound: %s" % [("%.3f" % q, "%.2e" % e, k[len(P):]) for q, e, k in report[:6]])
    print("worst conv-stack tensor: %s" % max((err[k], k) for k in names if "convs_" in k or "pixel_decoder" in k).__repr__())
    assert report[0][0] <= 1.0, report[:6]
    # the float64 run really ran on batch statistics per view: two calls per tower layer, one per branch layer
    assert all(len(block.stats[n]) == 2 for n in F.TOWER) and all(len(block.stats[n]) == 1 for n in F.BRANCHES)
    # ... and these are not the stored-statistics trainer's gradients: every tensor of the 18 blocks differs by far more than its bound
    old = _trainer(s["head"])
    g0 = old.backward(_losses(old, s["head"], s["feats"], s["c"], device))
    block_keys = [k for k in names if k[len(P):].rsplit(".", 2)[0] in BN_LAYERS]
    assert len(block_keys) == 54
    apart = {k: rel_err(g0[k], s["grads"][k]) for k in block_keys}
    print("stored against batch statistics, smallest relative difference: %.3f" % min(apart.values()))
    assert all(v > 10 * F.grad_bound(k) for k, v in apart.items()), min(apart.items(), key=lambda kv: kv[1])


def test_running_buffers_and_counters_after_one_and_three_iterations(device):
    """all 36 running buffers against the float64 progression within the "running" family's limit; the counters + 2 per iteration for a
    tower layer and + 1 for a branch layer; nothing else in `buffers`"""
    s = _one_iteration(device)
    nq, c, sd, head, feats = s["nq"], s["c"], s["sd"], s["head"], s["feats"]
    tr = _trainer(head, batch_stats=True)
    assert len(tr.buffers) == 54 and all(_same_bits(tr.buffers[k], s["before"][k]) for k in tr.buffers if tr.buffers[k].is_floating_point())
    ref, A = F.running_reference(sd, c, s["rec"], device)
    assert len(ref) == 72
    lim, worst = F.limit("running"), {}
    for k in (1, 2, 3):
        _losses(tr, head, feats, c, device)
        if k == 1:
            assert all(_same_bits(tr.buffers[q], s["after"][q]) for q in tr.buffers), "two trainers, one iteration each: different buffers"
        for name in BN_LAYERS:
            assert int(tr.buffers[P + name + ".1.num_batches_tracked"]) == (2 * k if name in F.TOWER else k), (name, k)
        if k in F.RUNNING_CALLS:
            for (q, n), r in ref.items():
                if n == k:
                    ratio = F.ratios(tr.buffers[q].cpu(), r, A[(q, n)])
                    worst[(q, n)] = float(torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("running buffers: worst error / (limit x A) %s" % [("%.3f" % (v / lim), q[len(P):], n) for (q, n), v in top])
    assert len(worst) == 72 and all(v <= lim for v in worst.values()), top
    moved = [q for q in tr.buffers if not q.endswith("num_batches_tracked") and not _same_bits(tr.buffers[q], s["before"][q])]
    assert len(moved) == 36
    # the head the trainer was built from still holds its own buffers
    assert all(_same_bits(head.raw(q[len(P):]).float(), s["before"][q]) for q in moved)


def test_stored_statistics_path_runs_on_the_trainers_buffers_and_leaves_them(device):
    """tr.batch_stats = False: bit for bit the losses and gradients of a batch_stats=False trainer built from the same parameters and
    buffers; buffers and counters untouched; back to True, the next iteration moves them again"""
    from nopesac_amd.training import CameraHeadTrainer
    s = _one_iteration(device)
    c, head, feats = s["c"], s["head"], s["feats"]
    tr = _trainer(head, batch_stats=True)
    _losses(tr, head, feats, c, device)
    held = _snapshot(tr)
    tr.batch_stats = False
    losses = _losses(tr, head, feats, c, device)
    grads = tr.backward(losses)
    assert all(_same_bits(tr.buffers[k], held[k]) for k in held)
    stats = {k: v.clone() for k, v in tr.buffers.items() if not k.endswith("num_batches_tracked")}
    twin = CameraHeadTrainer({k: v.detach().clone() for k, v in tr.params.items()}, s["nq"], head.warp_plane_in_cam_ref_on, stats, conv_stacks=True)
    assert not twin.batch_stats and len(twin.buffers) == 36
    l2 = _losses(twin, head, feats, c, device)
    g2 = twin.backward(l2)
    assert set(l2) == set(losses) and all(_same_bits(losses[k].detach(), l2[k].detach()) for k in losses)
    assert all(_same_bits(grads[k], g2[k]) for k in grads)
    assert not all(_same_bits(grads[k], s["grads"][k]) for k in grads)          # (and they are not the batch-statistics gradients)
    tr.batch_stats = True
    _losses(tr, head, feats, c, device)
    assert not any(_same_bits(tr.buffers[k], held[k]) for k in held)
    with pytest.raises(Exception):
        twin.batch_stats = True                                                  # a trainer built without the counters cannot switch
        _losses(twin, head, feats, c, device)


def test_write_back_reaches_the_inference_head_and_sgd_lowers_the_pixel_losses(device):
    """twenty SGD steps on the two pixel-regression losses under batch statistics lower them; after write_back the inference head's pixel
    pose net agrees with the oracle's eval-mode one on a state dict that carries the trainer's parameters AND buffers"""
    from oracle import nopesac_oracle as O
    s = _one_iteration(device)
    c, sd, model, head, feats = s["c"], s["sd"], s["model"], s["head"], s["feats"]
    B = 2
    tr = _trainer(head, batch_stats=True)
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
        after = _losses(tr, head, feats, c, device)
        last = float(sum(after[k].detach() for k in pix))
        print("pixel losses: %.4f -> %.4f" % (first, last))
        assert last < first, (first, last)
        counts = (int(tr.buffers[P + "convs_backbone.0.1.num_batches_tracked"]), int(tr.buffers[P + "convs_rots.5.1.num_batches_tracked"]))
        assert counts == (42, 21), counts                   # 21 forwards: + 2 per tower layer, + 1 per branch layer
        tr.write_back(head)
        sd2 = {k: v.clone() for k, v in sd.items()}
        for k, t in list(tr.params.items()) + list(tr.buffers.items()):
            sd2[k] = t.detach().cpu().clone()
        for k in tr.buffers:
            assert _same_bits(head.raw(k[len(P):]).to(tr.buffers[k].dtype), tr.buffers[k]), k
        with torch.no_grad():
            t0, _, tf, rf = head.pixel_pose_net(feats, B)
            ot, _, otf, orf, _ = O.pixel_pose_net(sd2, c["feats1"], c["feats2"], P[:-1])
        assert rel_err(tf, otf) < 1e-3 and rel_err(rf, orf) < 1e-3 and rel_err(t0, ot) < 1e-3
        sd_old = dict(sd2, **{k: sd[k] for k in tr.buffers})                     # the same parameters on the checkpoint's buffers: elsewhere
        with torch.no_grad():
            _, _, otf_old, _, _ = O.pixel_pose_net(sd_old, c["feats1"], c["feats2"], P[:-1])
        assert rel_err(tf, otf_old) > 1e-2
    finally:                                                  # (tests/util.make_model caches the model: hand it back with its checkpoint)
        model.load_state_dict(sd)


def test_the_model_optimiser_moves_the_179_parameters_and_no_buffer(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.optim import ModelOptimizer
    s = _one_iteration(device)
    c, head, feats = s["c"], s["head"], s["feats"]
    tr = _trainer(head, batch_stats=True)
    tr.backward(_losses(tr, head, feats, c, device))
    p0 = {k: v.detach().clone() for k, v in tr.params.items()}
    held = _snapshot(tr)
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.OPTIMIZER", "ADAMW", "SOLVER.BASE_LR", 0.01, "SOLVER.WARMUP_ITERS", 0])
    opt = ModelOptimizer.from_cfg([tr], cfg)
    assert len(opt.keys) == 179 and set(opt.keys) == set(tr.params) and not set(opt.keys) & set(tr.buffers)
    opt.step()
    torch.cuda.synchronize()
    assert all(not _same_bits(tr.params[k].detach(), p0[k]) for k in p0), [k for k in p0 if _same_bits(tr.params[k].detach(), p0[k])][:4]
    assert all(_same_bits(tr.buffers[k], held[k]) for k in held)
