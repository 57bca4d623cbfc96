"""PlanePyramidTrainer on the device (nopesac_amd/training.py; csrc/pyramid_train.hip): forward, running statistics and gradients against
the reference's top_down in train mode (tests/golden/L_plane_pyramid_6x8.npz) and, every element of all 24 parameter gradients, of the
gradients at the memory and at the four backbone maps, of p1 and of the 16 running statistics, within the per-element allowance of the
float64 restatement of the whole pyramid (tests/plane_pyramid_forms.py); the stored-statistics forward is the inference head's p1
within the rule and leaves the buffers alone; the chain pyramid -> instance heads -> PlaneCriterion is backward_from bit for bit; the
memory shared with PlaneDecoderTrainer receives both paths; ten optimiser steps write back parameters and running statistics."""
import functools

import pytest
import torch

from tests import golden_inputs as GI
from tests import plane_pyramid_forms as P
from tests.test_plane_heads_training_gpu import _head_targets
from tests.util import make_model, nhwc

pytestmark = pytest.mark.gpu
KEY = P.PYR_CASES[0]                         # (2, 6, 8): the fixture's case
NQ = 7


def _trainer(c, device, **kw):
    from nopesac_amd.training import PlanePyramidTrainer
    from nopesac_amd.synth import synth_state_dict
    full = synth_state_dict(NQ)
    sd = dict({k: v for k, v in full.items() if k.startswith(P.PREFIX)}, **c["sd"], **c["bufs"])
    return PlanePyramidTrainer.from_state_dict(sd, device, **kw)


def _run(c, device):
    """One batch-statistics forward and backward_from of a fresh trainer -> (trainer, results with pyramid_run's keys, on the CPU)."""
    tr = _trainer(c, device, feature_grads=True)
    feats = {k: v.to(device) for k, v in c["feats"].items()}
    p1 = tr.forward(feats, c["memory"].to(device), c["B"])
    grads = tr.backward_from(c["d_p1"].to(device))
    assert sorted(grads) == sorted(c["sd"]) and len(grads) == 24 and set(tr.input_grads) == {"memory", "res2", "res3", "res4", "res5"}
    got = {k: g.cpu() for k, g in grads.items()}
    got.update({k: g.cpu() for k, g in tr.input_grads.items()})
    got["p1"] = p1.detach().cpu()
    got.update({k: tr.buffers[k].cpu() for k in c["bufs"]})
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    return tr, got


@functools.lru_cache(maxsize=None)
def _fixture_run(device):
    return _run(P.pyramid_inputs(KEY), device)


def _report(tag, w, lim):
    top = sorted(w.items(), key=lambda kv: -kv[1])[:5]
    print("%s: worst error / (limit x A): %s" % (tag, [(k.replace(P.PREFIX, ""), "%.3f" % (q / lim)) for k, q in top]))
    bad = {k: q for k, q in w.items() if not q <= lim}
    assert not bad, (tag, bad, lim)


def test_forward_statistics_and_gradients_are_the_references(device):
    """against the fixture: |trainer - reference| <= limit x A on every stored element, A from the float64 restatement; counters exact"""
    tr, got = _fixture_run(str(device))
    gold = P.golden(KEY[1], KEY[2])
    _, A = P.reference("pyramid", KEY)
    view, av = P.fixture_view(got), P.fixture_view(A)
    w = {}
    for k in view:
        ref = torch.from_numpy(gold[k]).double()
        assert tuple(view[k].shape) == tuple(ref.shape), k
        w[k] = float(P.ratios(view[k], ref, av[k]).max())
    assert len(w) == 43
    _report("fixture", w, P.limit("pyramid"))
    counters = [k for k in tr.buffers if k.endswith("num_batches_tracked")]
    assert len(counters) == 8 and all(int(tr.buffers[k]) == int(gold[k]) == 1 and tr.buffers[k].dtype == torch.int64 for k in counters)


def test_all_gradients_against_the_float64_pyramid(device):
    tr, got = _fixture_run(str(device))
    w = {k: q for k, (q, _) in P.worst_ratio("pyramid", KEY, got).items()}
    assert len(w) == 46
    _report("pyramid %s" % (KEY,), w, P.limit("pyramid"))
    # deterministic: a second trainer gives the same bits
    _, again = _run(P.pyramid_inputs(KEY), device)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_production_size_tie_in(device):
    """15 x 20 -> 120 x 160, B = 1: every output against the float64 pyramid, whose restatement and draws run on the GPU at this size"""
    c = P.pyramid_inputs(P.PYR_TIE_IN, str(device))
    _, got = _run(c, device)
    w = {k: q for k, (q, _) in P.worst_ratio("pyramid", P.PYR_TIE_IN, got, str(device)).items()}
    assert len(w) == 46 and tuple(got["p1"].shape) == (1, 120, 160, 256)
    _report("pyramid %s" % (P.PYR_TIE_IN,), w, P.limit("pyramid"))


def _private(device):
    """(model, head) of a private instance whose top_down holds the fixture case's settled biases; the caller restores the checkpoint"""
    model = make_model(device, overrides=("SOLVER.SEM_SEG_HEAD_MULTIPLIER", 1.0), nq=NQ)
    head = model.sem_seg_head
    _trainer(P.pyramid_inputs(KEY), device).write_back(head)
    return model, head


def _features(device):
    return {k: nhwc(v).to(device) for k, v in GI.feature_maps(int(P.golden(KEY[1], KEY[2])["seed"]), KEY[1], KEY[2], batch=KEY[0]).items()}


def _frozen_reference(head_or_trainer_tensors, memory, device):
    """(p1 in float64, its allowance) of the stored-statistics pyramid at the given parameters / buffers and memory"""
    c = dict(P.pyramid_inputs(KEY), memory=memory.detach().cpu())
    c["sd"] = {k: head_or_trainer_tensors[k].detach().cpu().float() for k in c["sd"]}
    c["bufs"] = {k: head_or_trainer_tensors[k].detach().cpu().float() for k in c["bufs"]}
    ref, A = P.pyramid_reference_for(c, str(device), batch_stats=False)
    return ref["p1"], A["p1"]


def test_stored_statistics_forward_is_the_inference_heads(device):
    """forward(batch_stats=False) and PlaneTRHead.training_inputs' p1 both stand within the limit of the float64 pyramid on stored
    statistics (not bit for bit: the head folds the BatchNorm into the conv's epilogue, the trainer applies it in a launch of its own);
    the buffers are untouched"""
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlanePyramidTrainer
    model, head = _private(device)
    try:
        feats = _features(device)
        memory, f32_feats = head.pyramid_training_inputs(feats)
        assert tuple(memory.shape) == (KEY[0] * KEY[1] * KEY[2], 256) and not memory.requires_grad and sorted(f32_feats) == list(P.LEVELS)
        assert torch.equal(memory, head.decoder_training_inputs(feats)[0])
        p1_head = head.training_inputs(feats)[1]
        tr = PlanePyramidTrainer.from_head(head)
        before = {k: v.clone() for k, v in tr.buffers.items()}
        p1 = tr.forward(f32_feats, memory, KEY[0], batch_stats=False)
        assert p1.requires_grad and all(torch.equal(before[k], tr.buffers[k]) for k in before) and len(before) == 24
        ref, A = _frozen_reference(dict(tr.params, **tr.buffers), memory, device)
        lim = P.limit("pyramid")
        w = {"trainer": float(P.ratios(p1.detach().cpu(), ref, A).max()), "head": float(P.ratios(p1_head.cpu(), ref, A).max())}
        _report("stored statistics", w, lim)
        tr.backward_from(torch.ones_like(p1))                              # the stored-statistics backward runs (constants of the backward)
        assert set(tr.input_grads) == {"memory"} and all(bool(torch.isfinite(g).all()) for g in tr.grads.values())
        batch = tr.forward(f32_feats, memory, KEY[0])                      # ... and a batch-statistics forward does move the buffers
        assert not torch.equal(batch, p1) and all(not torch.equal(before[k], tr.buffers[k]) for k in before)
    finally:
        model.load_state_dict(synth_state_dict(NQ))


def _chain(device):
    from nopesac_amd.training import PlaneDecoderTrainer, PlaneInstanceHeadsTrainer, PlanePyramidTrainer
    model, head = _private(device)
    feats = _features(device)
    memory, f32_feats = head.pyramid_training_inputs(feats)
    hs = head.training_inputs(feats)[0]
    targets = _head_targets("border_s4", device, 8 * KEY[1], 8 * KEY[2])
    return (model, head, feats, f32_feats, memory, hs, targets, PlanePyramidTrainer.from_head(head, feature_grads=True),
            PlaneInstanceHeadsTrainer.from_head(head), PlaneDecoderTrainer.from_head(head))


def test_backward_from_is_the_chains_backward(device):
    """pyr.backward_from(heads.input_grads["p1"]) = the chained backward through the instance heads and the criterion, bit for bit; under
    deep supervision p1 feeds all three supervised layers"""
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, f32_feats, memory, hs, targets, pyr, heads, _ = _chain(device)
    try:
        assert hs.shape[0] == 3
        losses, _ = pyr.losses(heads, f32_feats, memory, hs, targets)
        chained = pyr.backward(losses)
        assert len(chained) == 24 + 24 and set(pyr.input_grads) == {"memory", "res2", "res3", "res4", "res5"}
        inputs = {k: g.clone() for k, g in pyr.input_grads.items()}
        p1 = pyr.forward(f32_feats, memory, KEY[0])
        leaf = p1.detach().clone().requires_grad_(True)
        heads.backward(heads.losses(hs, leaf, targets)[0])
        split = pyr.backward_from(heads.input_grads["p1"])
        assert all(torch.equal(split[k], chained[k]) for k in split) and all(torch.equal(pyr.input_grads[k], inputs[k]) for k in inputs)
        assert all(float(g.abs().max()) > 0 for g in split.values())
    finally:
        model.load_state_dict(synth_state_dict(NQ))


def test_shared_memory_receives_both_paths(device):
    """memory as one leaf of PlaneDecoderTrainer (p = 0) and of the pyramid: memory.grad = the two trainers' separate input_grads["memory"]
    summed.  Every path's contribution has the same bits in the joint graph as in its own (same kernels, same inputs); the sides differ
    in the order of float32 additions only, and with the decoder built last its contributions are accumulated first on both sides, so
    that what differs is the one rounding of the last addition: LIMIT_FACTOR x 2^-24 (|decoder's| + |pyramid's|) per element."""
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, f32_feats, memory, hs0, targets, pyr, heads, dec = _chain(device)
    try:
        pos = head.decoder_training_inputs(feats)[1]
        leaf = memory.detach().clone().requires_grad_(True)
        p1 = pyr.forward(f32_feats, leaf, KEY[0])
        hs = dec.forward(leaf, pos, KEY[0])
        assert torch.equal(hs.detach(), hs0)
        heads.backward(heads.losses(hs, p1, targets)[0])
        total = leaf.grad.clone()
        dec.backward(dec.losses(heads, memory, pos, p1.detach(), targets)[0])
        pyr.backward(pyr.losses(heads, f32_feats, memory, hs.detach(), targets)[0])
        a, b = dec.input_grads["memory"].double(), pyr.input_grads["memory"].double()
        assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0
        err, allow = (total.double() - (a + b)).abs(), P.LIMIT_FACTOR * P.EPS24 * (a.abs() + b.abs())
        print("shared memory: worst error / allowance %.3f" % float((err / allow.clamp_min(1e-300)).max()))
        assert bool((err <= allow).all())
    finally:
        model.load_state_dict(synth_state_dict(NQ))


def test_ten_steps_write_back_parameters_and_statistics(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.synth import synth_state_dict
    model, head, feats, f32_feats, memory, hs, targets, pyr, heads, _ = _chain(device)
    try:
        cfg = get_cfg()
        start = {k: v.detach().clone() for k, v in list(pyr.params.items()) + list(pyr.buffers.items())}
        for _ in range(10):
            losses, _ = pyr.losses(heads, f32_feats, memory, hs, targets)
            pyr.backward(losses)
            pyr.step_from_cfg(cfg)
        assert all(not torch.equal(start[k], pyr.params[k].detach()) for k in pyr.params)
        pyr.write_back(head)
        sd = head.state_dict()
        for k, t in pyr.buffers.items():
            assert torch.equal(sd[k[len("sem_seg_head."):]], t) and not torch.equal(t, start[k]), k
            if k.endswith("num_batches_tracked"):
                assert int(t) == 10
        for k, t in pyr.params.items():
            assert torch.equal(sd[k[len("sem_seg_head."):]], t.detach()), k
        p1_head = head.training_inputs(feats)[1]                           # the inference route: stored statistics, BatchNorm folded
        p1 = pyr.forward(f32_feats, memory, KEY[0], batch_stats=False).detach()
        ref, A = _frozen_reference(dict(pyr.params, **pyr.buffers), memory, device)
        w = {"trainer": float(P.ratios(p1.cpu(), ref, A).max()), "head": float(P.ratios(p1_head.cpu(), ref, A).max())}
        _report("after ten steps", w, P.limit("pyramid"))
        assert all(int(pyr.buffers[k]) == 10 for k in pyr.buffers if k.endswith("num_batches_tracked"))
    finally:
        model.load_state_dict(synth_state_dict(NQ))
