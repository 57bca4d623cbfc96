"""PlaneDecoderTrainer on the device (nopesac_amd/training.py; csrc/decoder_train.hip): the p = 0 forward is the inference head's own
launches (torch.equal with PlaneTRHead.training_inputs), the gradients of all 111 tensors and of the memory stand within the
per-element allowance of the float64 restatement of the whole decoder (tests/plane_decoder_forms.py) at p = 0 and p = 0.1, the masks are
functions of (seed, step), and the chain decoder -> instance heads -> PlaneCriterion trains and writes back."""
import pytest
import torch

from tests import golden_inputs as GI
from tests import plane_decoder_forms as D
from tests.test_plane_heads_training_gpu import _head_targets
from tests.util import make_model, nhwc

pytestmark = pytest.mark.gpu


def _features(device, h5, w5, batch):
    return {k: nhwc(v).to(device) for k, v in GI.feature_maps(23, h5, w5, batch=batch).items()}


@pytest.mark.parametrize("B, nq, h5, w5", [(2, 7, 3, 4), (1, 50, 15, 20)])
def test_the_forward_without_dropout_is_the_inference_heads(device, B, nq, h5, w5):
    from nopesac_amd.training import PlaneDecoderTrainer
    head = make_model(device, nq=nq).sem_seg_head
    feats = _features(device, h5, w5, B)
    hs_head, p1_head = head.training_inputs(feats)
    memory, pos, p1 = head.decoder_training_inputs(feats)
    assert memory.shape == (B * h5 * w5, 256) and pos.shape == (h5 * w5, 256) and not memory.requires_grad
    assert torch.equal(p1, p1_head)
    tr = PlaneDecoderTrainer.from_head(head)
    assert len(tr.params) == 111 and tr.layers_out == 3
    hs = tr.forward(memory, pos, B)
    assert hs.shape == (3, B, nq, 256) and hs.requires_grad
    assert torch.equal(hs.detach(), hs_head)


@pytest.mark.parametrize("key", D.DEC_CASES, ids=lambda k: "B%d_nq%d_Lm%d_p%g" % k)
def test_gradients_against_the_float64_decoder(device, key):
    from nopesac_amd.training import PlaneDecoderTrainer
    c = D.decoder_inputs(key)
    B, nq, p = c["B"], c["nq"], c["p"]
    tr = PlaneDecoderTrainer.from_state_dict(c["sd"], nq, device)
    memory, pos, d_hs = (c[n].to(device) for n in ("memory", "pos", "d_hs"))
    hs = tr.forward(memory, pos, B, p, D.SEED, D.DEC_STEP)
    grads = tr.backward_from(d_hs)
    assert sorted(grads) == sorted(c["sd"]) and len(grads) == 111 and set(tr.input_grads) == {"memory"}
    got = {k: g.cpu() for k, g in grads.items()}
    got["memory"] = tr.input_grads["memory"].cpu()
    got["hs"] = hs.detach().cpu()
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    w = D.worst_ratio("decoder", key, got)
    lim = D.limit("decoder")
    top = sorted(w.items(), key=lambda kv: -kv[1][0])[:5]
    print("decoder %s: worst error / (limit x A): %s" % (key, [(k[len(D.PREFIX):], "%.3f" % (q / lim)) for k, (q, _) in top]))
    print("  memory %.3f  query_embed %.3f  hs %.3f" % tuple(w[k][0] / lim for k in ("memory", D.PREFIX + "query_embed.weight", "hs")))
    bad = {k: v for k, v in w.items() if not v[0] <= lim}
    assert not bad, (key, bad, lim)
    # deterministic: a second pass gives the same bits
    hs2 = tr.forward(memory, pos, B, p, D.SEED, D.DEC_STEP)
    again = tr.backward_from(d_hs)
    assert torch.equal(hs2, hs) and all(torch.equal(grads[k], again[k]) for k in grads) and torch.equal(tr.input_grads["memory"].cpu(), got["memory"])


def test_masks_follow_seed_and_step(device):
    from nopesac_amd.training import PlaneDecoderTrainer
    c = D.decoder_inputs((2, 7, 12, 0.1))
    tr = PlaneDecoderTrainer.from_state_dict(c["sd"], c["nq"], device)
    memory, pos = c["memory"].to(device), c["pos"].to(device)
    with torch.no_grad():
        a = tr.forward(memory, pos, 2, 0.1, seed=11, step=4)
        assert torch.equal(a, tr.forward(memory, pos, 2, 0.1, seed=11, step=4))
        assert not torch.equal(a, tr.forward(memory, pos, 2, 0.1, seed=11, step=5))
        assert not torch.equal(a, tr.forward(memory, pos, 2, 0.1, seed=12, step=4))
        plain = tr.forward(memory, pos, 2)
        assert not torch.equal(a, plain) and torch.equal(plain, tr.forward(memory, pos, 2, 0.0, seed=99, step=7))


def _chain(device):
    from nopesac_amd.training import PlaneDecoderTrainer, PlaneInstanceHeadsTrainer
    model = make_model(device, overrides=("SOLVER.SEM_SEG_HEAD_MULTIPLIER", 1.0, "SOLVER.WEIGHT_DECAY_EMBED", 0.0), nq=7)      # a private instance
    head = model.sem_seg_head
    feats = {k: nhwc(v).to(device) for k, v in GI.feature_maps(21, 6, 8, batch=2).items()}
    memory, pos, p1 = head.decoder_training_inputs(feats)
    targets = _head_targets("border_s4", device, p1.shape[1], p1.shape[2])
    return model, head, feats, memory, pos, p1, targets, PlaneDecoderTrainer.from_head(head), PlaneInstanceHeadsTrainer.from_head(head)


def test_backward_from_is_the_chains_backward(device):
    """dec.backward_from(heads.input_grads["hs"]) = the chained backward, bit for bit; dropout on"""
    model, head, feats, memory, pos, p1, targets, dec, heads = _chain(device)
    losses, _ = dec.losses(heads, memory, pos, p1, targets, p=0.1, seed=3, step=2)
    chained = dec.backward(losses)
    assert len(chained) == 111 + 24 and set(dec.input_grads) == {"memory"}
    mem_grad = dec.input_grads["memory"].clone()
    hs = dec.forward(memory, pos, 2, 0.1, 3, 2)
    leaf = hs.detach().clone().requires_grad_(True)
    heads.backward(heads.losses(leaf, p1, targets)[0])
    split = dec.backward_from(heads.input_grads["hs"])
    assert all(torch.equal(split[k], chained[k]) for k in split) and torch.equal(dec.input_grads["memory"], mem_grad)
    # (layer 0's norm1 normalises tgt = 0: xhat = 0 and its weight's gradient is identically zero)
    assert [k for k, g in split.items() if float(g.abs().max()) == 0] == [D.DEC + ".layers.0.norm1.weight"]


def test_forty_steps_lower_the_loss_and_write_back(device):
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, memory, pos, p1, targets, dec, heads = _chain(device)
    try:
        weighted = lambda losses: float(sum(v.detach() for v in heads.criterion.weighted(losses).values()))
        history = []
        for it in range(40):
            losses, _ = dec.losses(heads, memory, pos, p1, targets, p=0.0, seed=1, step=it)
            history.append(weighted(losses))
            dec.backward(losses)
            dec.step(lr=1e-4)
            heads.step(lr=1e-4)
        with torch.no_grad():
            out = heads.forward(dec.forward(memory, pos, 2), p1)
            final = weighted(heads.criterion(out, targets)[0])
        print("weighted loss: %.5f -> %.5f" % (history[0], final))
        assert final < history[0]
        dec.write_back(head)
        heads.write_back(head)
        with torch.no_grad():
            ho, _ = head(feats, want_logits=True)
        for k in ("pred_logits", "pred_params", "pred_centers"):
            assert torch.equal(out[k], ho[k].float().view_as(out[k])), k
        assert torch.equal(out["pred_mask_logits"], ho["pred_mask_logits"].permute(0, 3, 1, 2).contiguous().view_as(out["pred_mask_logits"]))
        assert torch.equal(dec.forward(memory, pos, 2).detach(), head.training_inputs(feats)[0])
    finally:
        model.load_state_dict(synth_state_dict(7))
