"""PlaneEncoderTrainer on the device (nopesac_amd/training.py; csrc/linear_bwd.hip): the p = 0 forward is the inference head's own
launches (torch.equal with PlaneTRHead.decoder_training_inputs' memory), the gradients of all 76 tensors, of res5 and the memory stand
within the per-element allowance of the float64 restatement of the whole encoder (tests/plane_encoder_forms.py, itself held to the
reference by tests/golden/L_plane_encoder_3x4.npz on the CPU) at p = 0 and p = 0.1 and of that fixture itself, the masks are functions of (seed, step), the
four-trainer chain equals backward_from of the three upstream trainers bit for bit, a shared res5 leaf sums both paths, and twenty
steps of the whole head lower the loss and write back."""
import pytest
import torch

from tests import golden_inputs as GI
from tests import plane_encoder_forms as E
from tests.test_plane_heads_training_gpu import _head_targets
from tests.util import make_model, nhwc

pytestmark = pytest.mark.gpu
NQ = 7


def _features(device, h5, w5, batch, seed=23):
    return {k: nhwc(v).to(device) for k, v in GI.feature_maps(seed, h5, w5, batch=batch).items()}


@pytest.mark.parametrize("B, h5, w5", [(2, 3, 4), (1, 15, 20)])
def test_the_forward_without_dropout_is_the_inference_heads(device, B, h5, w5):
    from nopesac_amd.training import PlaneEncoderTrainer, _Linear
    head = make_model(device, nq=NQ).sem_seg_head
    feats = _features(device, h5, w5, B)
    memory = head.decoder_training_inputs(feats)[0]
    f32_feats, pos = head.encoder_training_inputs(feats)
    assert sorted(f32_feats) == ["res2", "res3", "res4", "res5"] and pos.shape == (h5 * w5, 256) and not f32_feats["res5"].requires_grad
    assert all(torch.equal(f32_feats[k], head.pyramid_training_inputs(feats)[1][k]) for k in f32_feats)
    tr = PlaneEncoderTrainer.from_head(head)
    assert len(tr.params) == 76
    got = tr.forward(f32_feats["res5"], B)
    assert got.shape == (B * h5 * w5, 256) and got.requires_grad
    assert torch.equal(got.detach(), memory)
    assert torch.equal(tr.forward(f32_feats["res5"], B, pos=pos).detach(), memory)
    sd = {"sem_seg_head." + k: v for k, v in head.state_dict().items()}
    assert torch.equal(PlaneEncoderTrainer.from_state_dict(sd, device).forward(f32_feats["res5"], B).detach(), memory)

    class Composed(PlaneEncoderTrainer):                                      # the existing composition: the same forward bits
        LINEAR = _Linear
    assert torch.equal(Composed.from_head(head).forward(f32_feats["res5"], B).detach(), memory)


def _run(c, device, cls=None):
    from nopesac_amd.training import PlaneEncoderTrainer
    tr = (cls or PlaneEncoderTrainer).from_state_dict(c["sd"], device, feature_grads=True)
    res5, pos, d_memory = (c[n].to(device) for n in ("res5", "pos", "d_memory"))
    memory = tr.forward(res5, c["B"], c["p"], E.SEED, E.ENC_STEP, pos=pos)
    grads = tr.backward_from(d_memory)
    assert sorted(grads) == sorted(c["sd"]) and len(grads) == 76 and set(tr.input_grads) == {"res5"}
    got = {k: g.cpu() for k, g in grads.items()}
    got["res5"] = tr.input_grads["res5"].cpu()
    got["memory"] = memory.detach().cpu()
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    return got


@pytest.mark.parametrize("key", E.ENC_CASES, ids=lambda k: "B%d_%dx%d_p%g" % k)
def test_gradients_against_the_float64_encoder(device, key):
    c = E.encoder_inputs(key)
    got = _run(c, device)
    w = E.worst_ratio("encoder", key, got)
    assert len(w) == 78
    lim = E.limit("encoder")
    top = sorted(w.items(), key=lambda kv: -kv[1][0])[:5]
    print("encoder %s: worst error / (limit x A): %s" % (key, [(k.replace(E.PREFIX, ""), "%.3f" % (q / lim)) for k, (q, _) in top]))
    print("  res5 %.3f  memory %.3f" % tuple(w[k][0] / lim for k in ("res5", "memory")))
    bad = {k: v for k, v in w.items() if not v[0] <= lim}
    assert not bad, (key, bad, lim)
    again = _run(c, device)                                                   # deterministic: a second trainer gives the same bits
    assert all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("tag", sorted(E.GOLDEN_CASES))
def test_memory_and_gradients_are_the_references(device, tag):
    """against the fixture (the reference's input_proj + context_SA in eval mode / in train mode under the materialised masks):
    |trainer - reference| <= limit x A on every stored element, A from the float64 restatement"""
    key = E.GOLDEN_CASES[tag]
    gold = E.golden(key[1], key[2])
    got = _run(E.encoder_inputs(key), device)
    _, A = E.reference("encoder", key)
    view, av = E.fixture_view(got), E.fixture_view(A)
    assert len(view) == 78
    w = {}
    for k in view:
        ref = torch.from_numpy(gold[tag + "." + k]).double()
        assert tuple(view[k].shape) == tuple(ref.shape), k
        w[k] = float(E.ratios(view[k], ref, av[k]).max())
    lim = E.limit("encoder")
    top = sorted(w.items(), key=lambda kv: -kv[1])[:4]
    print("fixture %s: worst error / (limit x A): %s" % (tag, [(k.replace(E.PREFIX, ""), "%.3f" % (q / lim)) for k, q in top]))
    assert all(q <= lim for q in w.values()), {k: q for k, q in w.items() if not q <= lim}


def test_the_composition_gives_the_same_forward_and_stands_within_the_rule(device):
    """LINEAR = _Linear (the baseline of the timing script): the same forward bits at p = 0.1, gradients within the same allowance"""
    from nopesac_amd.training import PlaneEncoderTrainer, _Linear

    class Composed(PlaneEncoderTrainer):
        LINEAR = _Linear
    key = (2, 3, 4, 0.1)
    c = E.encoder_inputs(key)
    a, b = _run(c, device), _run(c, device, Composed)
    assert torch.equal(a["memory"], b["memory"])
    w = E.worst_ratio("encoder", key, b)
    assert all(q <= E.limit("encoder") for q, _ in w.values())


def test_masks_follow_seed_and_step(device):
    from nopesac_amd.training import PlaneEncoderTrainer
    c = E.encoder_inputs((2, 3, 4, 0.1))
    tr = PlaneEncoderTrainer.from_state_dict(c["sd"], device)
    res5 = c["res5"].to(device)
    with torch.no_grad():
        a = tr.forward(res5, 2, 0.1, seed=11, step=4)
        assert torch.equal(a, tr.forward(res5, 2, 0.1, seed=11, step=4))
        assert not torch.equal(a, tr.forward(res5, 2, 0.1, seed=11, step=5))
        assert not torch.equal(a, tr.forward(res5, 2, 0.1, seed=12, step=4))
        plain = tr.forward(res5, 2)
        assert not torch.equal(a, plain) and torch.equal(plain, tr.forward(res5, 2, 0.0, seed=99, step=7))


def _chain(device):
    from nopesac_amd.training import PlaneDecoderTrainer, PlaneEncoderTrainer, PlaneInstanceHeadsTrainer, PlanePyramidTrainer
    model = make_model(device, overrides=("SOLVER.SEM_SEG_HEAD_MULTIPLIER", 1.0, "SOLVER.WEIGHT_DECAY_EMBED", 0.0), nq=NQ)      # a private instance
    head = model.sem_seg_head
    feats = _features(device, 3, 4, 2, seed=21)
    f32_feats, pos = head.encoder_training_inputs(feats)
    targets = _head_targets("border_s4", device, 24, 32)
    return (model, head, feats, f32_feats, pos, targets, PlaneEncoderTrainer.from_head(head, feature_grads=True), PlaneDecoderTrainer.from_head(head),
            PlanePyramidTrainer.from_head(head, feature_grads=True), PlaneInstanceHeadsTrainer.from_head(head))


def test_backward_from_of_the_upstream_trainers_is_the_chains_backward(device):
    """the four-trainer chain's backward = heads.backward, then backward_from of the decoder and the pyramid from heads.input_grads, then
    backward_from of the encoder from the sum of their input_grads["memory"]: bit for bit, dropout on; the shared res5 leaf holds the
    pyramid's and the encoder's paths summed"""
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, f32, pos, targets, enc, dec, pyr, heads = _chain(device)
    try:
        before = {k: v.clone() for k, v in pyr.buffers.items()}
        losses, _ = enc.losses(heads, dec, pyr, f32, targets, p=0.1, seed=3, step=2)
        chained = enc.backward(losses)
        assert len(chained) == 235 and sorted(chained) == sorted({**enc.params, **dec.params, **pyr.params, **heads.params})
        assert all(chained[k] is t.grads[k] for t in (enc, dec, pyr, heads) for k in t.params)
        assert set(enc.input_grads) == {"res5"} and "memory" in dec.input_grads and "memory" in pyr.input_grads and "res5" in pyr.input_grads
        assert all(float(g.abs().max()) > 0 for k, g in chained.items() if not k.endswith("context2plane_decoder.layers.0.norm1.weight"))
        total_res5 = enc.input_grads["res5"].clone()
        assert torch.equal(total_res5, pyr.input_grads["res5"])                # one leaf: both trainers report the sum
        mem_grads = (dec.input_grads["memory"].clone(), pyr.input_grads["memory"].clone())
        keep = {k: g.clone() for k, g in chained.items()}
        # the same step, trainer by trainer (the running statistics restart from the same values)
        for k, v in before.items():
            pyr.buffers[k].copy_(v)
        memory = enc.forward(f32["res5"], 2, 0.1, 3, 2)
        leaf = memory.detach().clone()
        hs = dec.forward(leaf, pos, 2, 0.1, 3, 2)
        p1 = pyr.forward(f32, leaf, 2)
        heads.backward(heads.losses(hs.detach().clone().requires_grad_(True), p1.detach().clone().requires_grad_(True), targets)[0])
        split = dict(heads.grads)
        split.update(dec.backward_from(heads.input_grads["hs"]))
        d_dec = dec.input_grads["memory"].clone()
        split.update(pyr.backward_from(heads.input_grads["p1"]))
        d_pyr, res5_pyr = pyr.input_grads["memory"].clone(), pyr.input_grads["res5"].clone()
        assert torch.equal(d_dec, mem_grads[0]) and torch.equal(d_pyr, mem_grads[1])
        split.update(enc.backward_from(d_dec + d_pyr))
        assert len(split) == 235 and all(torch.equal(split[k], keep[k]) for k in keep), [k for k in keep if not torch.equal(split[k], keep[k])]
        a, b = res5_pyr, enc.input_grads["res5"]
        assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0 and torch.equal(a + b, total_res5)
    finally:
        model.load_state_dict(synth_state_dict(NQ))


def test_twenty_steps_of_the_whole_head_lower_the_loss_and_write_back(device):
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, f32, pos, targets, enc, dec, pyr, heads = _chain(device)
    try:
        weighted = lambda losses: float(sum(v.detach() for v in heads.criterion.weighted(losses).values()))
        history = []
        for it in range(20):
            losses, _ = enc.losses(heads, dec, pyr, f32, targets, p=0.0, seed=1, step=it)
            history.append(weighted(losses))
            enc.backward(losses)
            for t in (enc, dec, pyr, heads):
                t.step(lr=1e-4)
        with torch.no_grad():
            memory = enc.forward(f32["res5"], 2)
            hs = dec.forward(memory, pos, 2)
            final = weighted(heads.criterion(heads.forward(hs, pyr.forward(f32, memory, 2, batch_stats=False)), targets)[0])
            last = weighted(enc.losses(heads, dec, pyr, f32, targets, p=0.0, seed=1, step=20)[0])
        print("weighted loss: %.5f -> %.5f (batch statistics), %.5f (stored statistics)" % (history[0], last, final))
        assert last < history[0]
        for t in (enc, dec, pyr, heads):
            t.write_back(head)
        assert torch.equal(head.decoder_training_inputs(feats)[0], memory)
        assert torch.equal(head.training_inputs(feats)[0], hs)
    finally:
        model.load_state_dict(synth_state_dict(NQ))
