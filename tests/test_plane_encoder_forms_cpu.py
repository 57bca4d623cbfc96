"""CPU half of the encoder-training sweep (tests/plane_encoder_forms.py): the case lists cover what the issue names, the stream formula
and its disjointness from the decoder's, the 76 names and the optimiser groups, the float64 restatement stands on the reference's
results (tests/golden/L_plane_encoder_3x4.npz), F32_WORST is what the float32 restatement measures, and a planted error exceeds the
limit."""
import re

import pytest
import torch

from tests import plane_decoder_forms as D
from tests import plane_encoder_forms as E


def _header_macro(name):
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nopesac_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_case_lists():
    assert E.TILE == _header_macro("NPS_LINEAR_BWD_TILE") and E.STAGE == _header_macro("NPS_LINEAR_BWD_STAGE")
    assert set(E.LIN_MS) == {1, 5, E.TILE - 1, E.TILE + 1, 24, 600}
    assert set(E.LIN_KN) == {(256, 512), (256, 256), (256, 1024), (1024, 256), (2048, 256), (4, 4), (132, 260)}
    assert {(g, p) for g, p in E.LIN_GATES} >= {("none", 0.0), ("relu", 0.0), ("drop", 0.1), ("drop", 0.5), ("both", 0.1)}
    assert len(E.LIN_CASES) == len(set(E.LIN_CASES)) == len(E.LIN_MS) * len(E.LIN_KN) * len(E.LIN_GATES)
    for M in E.LIN_MS:
        one, many = E.lin_splits(M)
        assert one == 1 and E.split_ranges(M, 1) == [(0, M)]
        ranges = E.split_ranges(M, many)
        assert sum(b - a for a, b in ranges) == M and ranges[-1][1] - ranges[-1][0] < max(b - a for a, b in ranges)      # short or empty
    assert any(E.split_ranges(M, E.lin_splits(M)[1])[-1] == (M, M) for M in E.LIN_MS)                                    # an empty one
    assert any(0 < E.split_ranges(M, E.lin_splits(M)[1])[-1][1] - E.split_ranges(M, E.lin_splits(M)[1])[-1][0] for M in E.LIN_MS)
    assert E.ENC_CASES == ((2, 3, 4, 0.0), (2, 3, 4, 0.1), (3, 3, 4, 0.1), (2, 15, 20, 0.0), (2, 15, 20, 0.1))
    assert D.FFN == 1024


def test_relu_gate_inputs_hold_both_zeros():
    for key in E.LIN_CASES:
        if key[3] in ("relu", "both"):
            y = E.lin_inputs(key)["y"]
            zeros = y[y == 0]
            assert bool((y >= 0).all()) and bool(torch.signbit(zeros).any()) and bool((~torch.signbit(zeros)).any()), key


def test_stream_formula_and_disjointness():
    from nopesac_amd import ops
    enc, dec = set(), set()
    for step in list(range(0, 1001)):
        for layer in range(8):
            for site in range(4):
                v = ops.encoder_dropout_stream(step, layer, site)
                assert v == E.encoder_dropout_stream(step, layer, site) == -(step * 32 + layer * 4 + site) - 1 < 0
                enc.add(v)
            for site in range(6):
                dec.add(ops.dropout_stream(step, layer, site))
    assert len(enc) == 1001 * 8 * 4 and not (enc & dec) and min(dec) >= 0
    # the keys differ too (dropout_key works modulo 2^64): no encoder stream aliases a decoder stream under one seed
    key = lambda s: D.mix64(s + D.mix64(D.SEED))
    assert not ({key(s) for s in enc} & {key(s) for s in dec})
    for bad in ((-1, 0, 0), (0, 8, 0), (0, 0, 4), (0, -1, 0)):
        with pytest.raises(ops.OpsArgumentError):
            ops.encoder_dropout_stream(*bad)


def test_names_sets_and_groups():
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd import training as T
    from nopesac_amd.training import PlaneEncoderTrainer, parameter_group
    sd = synth_state_dict(50)
    keys = list(sd.keys())
    enc = PlaneEncoderTrainer.from_state_dict(sd, "cpu")
    names = PlaneEncoderTrainer.parameter_names(keys)
    assert names == E.encoder_parameter_names(keys) == sorted(enc.params) and len(names) == 76
    want = [E.IPROJ + ".weight", E.IPROJ + ".bias", E.ENC + ".norm.weight", E.ENC + ".norm.bias"]
    for i in range(6):
        for leaf in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight",
                     "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
            want.append("%s.layers.%d.%s" % (E.ENC, i, leaf))
    assert sorted(want) == names
    with pytest.raises(T.ops.OpsArgumentError):
        PlaneEncoderTrainer({k: sd[k] for k in names[:-1]})
    sets = {"camera_convs": set(T.CameraHeadTrainer.from_state_dict(sd, 50, "cpu", conv_stacks=True).params),
            "matcher": set(T.MatchingHeadTrainer.from_state_dict(sd, 50, "cpu").params), "heads": set(T.PlaneInstanceHeadsTrainer.from_state_dict(sd, 50, "cpu").params),
            "decoder": set(T.PlaneDecoderTrainer.from_state_dict(sd, 50, "cpu").params), "pyramid": set(T.PlanePyramidTrainer.from_state_dict(sd, "cpu").params),
            "encoder": set(names)}
    total = sum(len(s) for s in sets.values())
    assert len(set().union(*sets.values())) == total == 599, {k: len(v) for k, v in sets.items()}
    plane = sets["heads"] | sets["decoder"] | sets["pyramid"] | sets["encoder"]
    assert len(plane) == 235 and plane == {k for k in keys if k.startswith(E.PREFIX) and k.split(".")[-1] not in ("running_mean", "running_var", "num_batches_tracked")}
    groups = {k: parameter_group(k) for k in names}
    norms = sorted(k for k, g in groups.items() if g == "norm")
    assert len(norms) == 26 and all(k.split(".")[-2] in ("norm", "norm1", "norm2") for k in norms)
    assert all(g == "plain" for k, g in groups.items() if k not in norms) and groups[E.IPROJ + ".weight"] == "plain"


@pytest.mark.parametrize("key", E.ENC_CASES, ids=lambda k: "B%d_%dx%d_p%g" % k)
def test_relu_margins_hold(key):
    c = E.encoder_inputs(key)
    m = E.relu_margins(c["sd"], c["res5"], c["pos"], c["B"], c["masks"], c["p"])
    print("%s: smallest margin %.4g" % (key, min(float(v.min()) for v in m.values())))
    assert len(m) == 6 and all(float(v.min()) >= E.RELU_MARGIN for v in m.values())


def test_settling_fails_loudly_when_it_cannot_converge(monkeypatch):
    """with no rounds and no steps allowed, a case that needs settling raises instead of returning marginal inputs"""
    c = E.encoder_inputs((2, 3, 4, 0.1))
    from nopesac_amd.synth import synth_state_dict
    full = synth_state_dict(7)
    sd = {k: full[k].float().clone() for k in c["sd"]}
    assert any(float(v.min()) < E.RELU_MARGIN for v in E.relu_margins(sd, c["res5"], c["pos"], c["B"], c["masks"], c["p"]).values())
    monkeypatch.setattr(E, "SETTLE_ROUNDS", 0)
    monkeypatch.setattr(E, "SETTLE_STEPS", 0)
    with pytest.raises(RuntimeError):
        E.settle_relu_margins(sd, c["res5"], c["pos"], c["B"], c["masks"], c["p"])


@pytest.mark.parametrize("tag", sorted(E.GOLDEN_CASES))
def test_float64_restatement_against_the_fixture(tag):
    """|float64 restatement - reference| <= limit x A on every stored element; the reference ran in float32 on its own modules (train:
    under the materialised masks of encoder_dropout_stream, in the reference's call order and index conventions)"""
    key = E.GOLDEN_CASES[tag]
    gold = E.golden(key[1], key[2])
    assert int(gold["train_mode"]) == 1
    c = E.encoder_inputs(key)
    assert torch.equal(torch.from_numpy(gold[tag + ".pos"]), c["pos"])              # the reference's PositionEmbeddingSine = the head's table
    ref, A = E.reference("encoder", key)
    view, av = E.fixture_view(ref), E.fixture_view(A)
    assert len(view) == 78
    w = {k: float(E.ratios(torch.from_numpy(gold[tag + "." + k]), view[k], av[k]).max()) for k in view}
    lim = E.limit("encoder")
    print("fixture %s: worst error / (limit x A): %s" % (tag, sorted(((round(q / lim, 3), k) for k, q in w.items()), reverse=True)[:4]))
    assert all(q <= lim for q in w.values()), {k: q for k, q in w.items() if not q <= lim}


@pytest.mark.parametrize("family", sorted(E.F32_WORST))
def test_f32_worst_is_what_the_restatement_measures(family):
    got = E.f32_worst(family)
    print("%s: measured %.3g, written %.3g" % (family, got, E.F32_WORST[family]))
    assert E.F32_WORST[family] / 2 <= got <= E.F32_WORST[family] * 2


@pytest.mark.parametrize("plant", E.LIN_PLANTS)
def test_a_planted_linear_error_exceeds_the_limit(plant):
    key = (600, 256, 1024, "both", 0.1)
    clean = E.worst_ratio("linear_bwd", key, E.emulate_linear_backward(key))
    bad = E.worst_ratio("linear_bwd", key, E.emulate_linear_backward(key, plant))
    lim = E.limit("linear_bwd")
    assert all(q <= lim for q, _ in clean.values()), clean
    assert max(q for q, _ in bad.values()) > lim and bad["dw"][0] > lim, bad


@pytest.mark.parametrize("plant", E.ENC_PLANTS)
def test_a_planted_encoder_error_exceeds_the_limit(plant):
    key = (2, 3, 4, 0.1)
    c = E.encoder_inputs(key)
    bad = E.worst_ratio("encoder", key, E.encoder_run(c, E._encoder_x(c), E.F32, plant=plant))
    assert bad["memory"][0] > E.limit("encoder") and sum(q > E.limit("encoder") for q, _ in bad.values()) > 70, bad
