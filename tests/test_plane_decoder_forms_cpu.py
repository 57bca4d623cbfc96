"""CPU half of the decoder-training sweep (tests/plane_decoder_forms.py): the keep mask's integer restatement and its statistics, the case
lists reach the tiles and paths they claim, the inputs meet the conditions the GPU half relies on, the committed float32 constants are
what the module measures, the float64 restatement of the decoder reproduces the oracle, a float32 emulation of the attention kernels'
formulas stays within the limit, and the same emulation with one planted error does not."""
import math

import numpy as np
import pytest
import torch

from tests import plane_decoder_forms as D

F64 = torch.float64


def _worst(family, key, got):
    return max(q for q, _ in D.worst_ratio(family, key, {k: got[k] for k in D.OUTPUTS[family]}).values())


# ---- the mask --------------------------------------------------------------------------------------------------------------------------
def test_mix64_is_splitmix64s_finaliser():
    """SplitMix64 seeded with 0 starts 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F (Vigna's splitmix64.c): its n-th output
    is the finaliser of n golden-ratio increments."""
    gold = 0x9E3779B97F4A7C15
    assert [D.mix64(n * gold) for n in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    z = np.array([gold, 2 * gold % 2 ** 64], dtype=np.uint64)
    assert [int(v) for v in D._mix64_np(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


def test_keep_mask_is_the_scalar_formula_on_every_index():
    p, seed, stream = 0.3, -7, D.dropout_stream(2, 5, 4)
    m = D.keep_mask((3, 5, 7), p, seed, stream).reshape(-1)
    key = D.mix64(stream + D.mix64(seed))
    assert [int(v) for v in m] == [int((D.mix64(i + key) >> 32) >= D.threshold(p)) for i in range(105)]
    assert D.threshold(0.0) == 0 and bool(D.keep_mask((64, 64), 0.0, 1, 2).all()) and D.threshold(0.5) == 2 ** 31
    assert D.dropout_stream(3, 4, 5) == 3 * 64 + 4 * 8 + 5


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_stream_independence(p):
    N = 1 << 20
    a = D.keep_mask((N,), p, D.SEED, D.dropout_stream(0, 0, 0)).double()
    b = D.keep_mask((N,), p, D.SEED, D.dropout_stream(0, 0, 1)).double()
    assert abs(float(a.mean()) - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / N)
    corr = float(((a - a.mean()) * (b - b.mean())).mean() / (a.std(unbiased=False) * b.std(unbiased=False)))
    assert abs(corr) < 6 / math.sqrt(N)
    c = D.keep_mask((N,), p, D.SEED + 1, D.dropout_stream(0, 0, 0)).double()
    assert abs(float(((a - a.mean()) * (c - c.mean())).mean() / (a.std(unbiased=False) * c.std(unbiased=False)))) < 6 / math.sqrt(N)


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
def test_tile_sizes_are_the_headers():
    from nopesac_amd import _lib
    assert (D.TQ, D.TK) == (_lib.H.NPS_ATT_TRAIN_TQ, _lib.H.NPS_ATT_TRAIN_TK)


def test_attention_cases_reach_what_they_claim():
    assert set(D.ATT_SHAPES) >= {(1, 1), (1, 300), (50, 50), (50, 300), (128, 300), (300, 300), (7, 129), (65, 64), (D.TQ - 1, D.TK + 1),
                                 (2 * D.TQ + 3, 2 * D.TK + 3)}
    for shape in D.ATT_SHAPES:
        assert {(shape + ("base", p)) in D.ATT_CASES for p in (0.0, 0.1)} == {True}
    assert (50, 300, "base", 0.5) in D.ATT_CASES and {k[2] for k in D.ATT_CASES} == {"base", "peaked", "nolen", "ragged", "h1"}
    tiles = lambda n, t: (n + t - 1) // t
    assert {tiles(lq, D.TQ) for lq, _ in D.ATT_SHAPES} >= {1, 2, 3, 5} and {tiles(lk, D.TK) for _, lk in D.ATT_SHAPES} >= {1, 2, 3, 5}
    assert any(lk % D.TK == 1 for _, lk in D.ATT_SHAPES) and any(lq % D.TQ == D.TQ - 1 for lq, _ in D.ATT_SHAPES)
    assert any(max(lq, lk) > 128 for lq, lk in D.ATT_SHAPES) and any(max(lq, lk) <= 128 for lq, lk in D.ATT_SHAPES)     # both sides of the small kernel's cap
    packed = padded = 0
    for key in D.ATT_CASES:
        c = D.attention_inputs(key)
        Lq, Lk, tag, p = key
        assert c["heads"] == (1 if tag == "h1" else 3) and c["null_lens"] == (tag == "nolen") and c["lens"][0] == (Lq, Lk)
        assert all(0 <= a <= Lq and 0 <= b <= Lk for a, b in c["lens"])
        if tag == "ragged":
            assert any(b == 0 and a > 0 for a, b in c["lens"]) and any(a == 0 and b > 0 for a, b in c["lens"])
        if tag == "peaked":
            assert float(c["q"].std()) > 3.5 and float(c["k"].std()) > 3.5 and float(c["v"].std()) < 1.5
        if c["packed"]:
            W = c["heads"] * D.HD
            assert Lq == Lk and c["q"].stride(0) == 3 * W and c["k"].data_ptr() == c["qkv"].data_ptr() + 4 * W
        packed, padded = packed + c["packed"], padded + (c["out_pad"] > 0)
        d = c["dout"]
        assert (d < 0).any() and ((d.abs().sum(1) == 0).any() or d.shape[0] < 3)
        assert tuple(c["mask"].shape) == (c["B"], c["heads"], Lq, Lk) and (bool(c["mask"].all()) == (p == 0.0) or c["mask"].numel() < 64)
    assert 0 < packed < len(D.ATT_CASES) and 0 < padded < len(D.ATT_CASES)


def test_peaked_rows_hold_probabilities_that_underflow():
    c = D.attention_inputs((50, 300, "peaked", 0.1))
    q, k = c["q"][:50].view(50, 3, 32), c["k"][:300].view(300, 3, 32)
    s = torch.einsum("lhd,shd->lsh", q, k) * c["scale"]
    p = torch.exp(s - s.max(1, keepdim=True).values)
    assert (p == 0).any() and float(torch.softmax(s.double(), 1).max(1).values.median()) > 0.9


def test_dropout_cases():
    assert {k[1] for k in D.DROP_CASES} == {256, 1024, 2048} and {k[2] for k in D.DROP_CASES} == {0.0, 0.1, 0.5}
    assert any(k[3] for k in D.DROP_CASES) and not any(k[3] for k in D.DROP_CASES if k[1] > 256)
    for key in D.DROP_CASES:
        c = D.dropout_inputs(key)
        assert (c["x"] == 0).any() or c["x"].numel() < 64
        assert (c["x"] < 0).any() == (key[1] == 256 and key[0] > 1) or key[0] == 1


def test_decoder_cases_and_their_relu_margins():
    from nopesac_amd.config import get_cfg
    assert set(D.DEC_CASES) >= {(2, 7, 12, 0.0), (2, 7, 12, 0.1), (2, 50, 35, 0.0), (2, 50, 35, 0.1)} and any(k[0] == 3 for k in D.DEC_CASES)
    assert get_cfg().MODEL.SEM_SEG_HEAD.DEEP_SUPERVISION and D.DEC_LAYERS_OUT == 3
    for key in D.DEC_CASES:
        c = D.decoder_inputs(key)
        assert len(c["sd"]) == 111 and c["sd"][D.DEC + ".layers.0.linear1.weight"].shape == (D.FFN, 256)
        assert sorted(c["sd"]) == D.decoder_parameter_names(c["sd"])
        margins = D.relu_margins(c["sd"], c["memory"], c["pos"], c["B"], c["nq"], c["masks"], c["p"])
        assert len(margins) == 6 and min(float(m.min()) for m in margins.values()) >= D.RELU_MARGIN, key
        assert (c["masks"] is None) == (key[3] == 0.0)
        if c["masks"]:
            assert len(c["masks"]) == 36 and tuple(c["masks"][(2, 2)].shape) == (c["B"], 8, c["nq"], c["Lm"])
            assert tuple(c["masks"][(5, 4)].shape) == (c["B"] * c["nq"], D.FFN)
        assert float(c["d_hs"][:, 0, 1].abs().sum()) == 0 and (c["d_hs"] < 0).any()


def test_the_trainer_holds_the_111_tensors_in_the_references_optimiser_groups():
    """train_NopeSAC.py:88-135: LayerNorm tensors take WEIGHT_DECAY_NORM, the nn.Embedding WEIGHT_DECAY_EMBED, sem_seg_head its multiplier"""
    from nopesac_amd.config import get_cfg
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlaneDecoderTrainer
    sd = synth_state_dict(7)
    tr = PlaneDecoderTrainer.from_state_dict(sd, 7, "cpu")
    assert sorted(tr.params) == D.decoder_parameter_names(sd.keys()) and len(tr.params) == 111 and tr.layers_out == 3
    assert PlaneDecoderTrainer.from_state_dict(sd, 7, "cpu", deep_supervision=False).layers_out == 1
    decay = {k: tr._weight_decay(k, 0.5, 0.25) for k in tr.params}
    norm = [k for k in tr.params if k.split(".")[-2].startswith("norm")]
    assert len(norm) == 6 * 6 + 2 and all(decay[k] == 0.25 for k in norm)
    assert all(v == 0.5 for k, v in decay.items() if k not in norm)
    assert tr._weight_decay(D.PREFIX + "query_embed.weight", 0.5, 0.25, 0.125) == 0.125 and tr._weight_decay(norm[0], 0.5, None) == 0.5
    assert not hasattr(tr, "weight_decay_embed")                                     # an argument of the step, not state carried across calls
    cfg = get_cfg()
    assert tr.lr_multiplier(cfg) == float(cfg.SOLVER.SEM_SEG_HEAD_MULTIPLIER)
    with pytest.raises(Exception):
        PlaneDecoderTrainer({k: v for k, v in list(tr.params.items())[:-1]}, 7)


# ---- references ------------------------------------------------------------------------------------------------------------------------
def test_unmasked_decoder_is_the_oracles():
    """decoder_forward without masks: its last layer is oracle.nopesac_oracle.detr_decoder (sequence-major there, batch-major here)."""
    from oracle import nopesac_oracle as O
    c = D.decoder_inputs((2, 7, 12, 0.0))
    B, nq, Lm = c["B"], c["nq"], c["Lm"]
    sd = {k: v.double() for k, v in c["sd"].items()}
    memory, pos = c["memory"].double(), c["pos"].double()
    hs = D.decoder_forward(sd, memory, pos, B, nq)
    assert hs.shape == (3, B, nq, 256)
    mem_sb = memory.view(B, Lm, 256).transpose(0, 1)
    qpos = sd[D.PREFIX + "query_embed.weight"][:, None].expand(nq, B, 256)
    ref = O.detr_decoder(sd, D.DEC, torch.zeros(nq, B, 256, dtype=F64), mem_sb, pos[:, None].expand(Lm, B, 256), qpos, D.NHEADS)
    assert float((hs[-1] - ref.transpose(0, 1)).abs().max()) < 1e-12
    one = D.decoder_forward(sd, memory, pos, B, nq, layers_out=1)
    assert one.shape == (1, B, nq, 256) and torch.equal(one[0], hs[-1])


def test_masked_decoder_uses_every_site():
    """each of the 36 masks changes hs[-1]: flipping one site's mask to all-ones moves the result"""
    c = D.decoder_inputs((2, 7, 12, 0.1))
    sd = {k: v.double() for k, v in c["sd"].items()}
    run = lambda masks: D.decoder_forward(sd, c["memory"].double(), c["pos"].double(), c["B"], c["nq"], masks, c["p"])[-1]
    with torch.no_grad():
        base = run(c["masks"])
        for site in c["masks"]:
            m = dict(c["masks"])
            m[site] = torch.ones_like(m[site])
            assert float((run(m) - base).abs().max()) > 1e-9, site


def test_reference_magnitudes_dominate_the_results():
    """|ref| <= S for every output (S sums the magnitudes of the terms the result sums with signs)"""
    for family, key in (("attention_bwd", (50, 300, "base", 0.1)), ("attention_fwd", (7, 129, "base", 0.0)), ("dropout", (100, 256, 0.5, True))):
        c = D.INPUTS[family](key)
        x = {k: c[k] for k in D.FLOATS[family] if c[k] is not None}
        ref, S = D.RUN[D._group(family)](c, x, F64), D.MAGS[D._group(family)](c, x)
        for k in D.OUTPUTS[family]:
            assert bool((ref[k].abs() <= S[k] * (1 + 1e-12) + 1e-300).all()), (family, k)
    ref, A = D.reference("decoder", (2, 7, 12, 0.1))
    assert set(ref) == set(A) and len(ref) == 113 and all(bool((A[k] >= 0).all()) for k in A)
    # d_hs reaches every tensor; the one gradient that is identically zero is layer 0's norm1.weight (tgt = 0 there, so xhat = 0)
    assert [k for k in ref if float(ref[k].abs().max()) == 0] == [D.DEC + ".layers.0.norm1.weight"]


def test_zero_probability_attention_matches_the_matcher_sweeps_reference():
    """at p = 0 the restatement is tests/matcher_bwd_forms.py's attention_run on the same inputs"""
    from tests import matcher_bwd_forms as M
    c = D.attention_inputs((50, 50, "ragged", 0.0))
    x = {k: c[k] for k in ("q", "k", "v", "dout")}
    mine, theirs = D.attention_run(c, x, F64), M.attention_run(c, x, F64)
    for k in ("dq", "dk", "dv"):
        assert torch.equal(mine[k], theirs[k]), k


# ---- constants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(D.F32_WORST))
def test_f32_worst_is_what_the_module_measures(family):
    measured = D.f32_worst(family)
    print("%s: committed %.3g, measured %.3g" % (family, D.F32_WORST[family], measured))
    assert D.F32_WORST[family] / 2 <= measured <= D.F32_WORST[family] * 2
    assert D.limit(family) == D.LIMIT_FACTOR * max(D.F32_WORST[family], 1.0)


# ---- sharpness -------------------------------------------------------------------------------------------------------------------------
def test_emulated_attention_kernels_stay_within_the_limit():
    for key in D.ATT_CASES:
        got = D.emulate_attention(key)
        for family in ("attention_fwd", "attention_bwd"):
            assert _worst(family, key, got) <= D.limit(family), (family, key)


@pytest.mark.parametrize("plant", D.ATT_PLANTS)
def test_a_planted_error_breaks_the_limit(plant):
    """every planted error fails the output it touches on every p > 0 case with more than one key (dq_without_scale: on every case)"""
    touched = {"delta_from_unmasked_dp": ("dq", "dk"), "dq_without_scale": ("dq",), "inv_keep_dropped": ("o", "dq", "dk", "dv"),
               "mask_of_the_next_stream": ("o", "dq", "dk", "dv"), "mask_index_transposed": ("o", "dq", "dk", "dv")}[plant]
    hit = 0
    for key in D.ATT_CASES:
        if (key[3] == 0.0 and plant != "dq_without_scale") or min(key[0], key[1]) < 7:
            continue
        got = D.emulate_attention(key, plant)
        for family in ("attention_fwd", "attention_bwd"):
            w = D.worst_ratio(family, key, {k: got[k] for k in D.OUTPUTS[family]})
            for k, (q, _) in w.items():
                if k in touched:
                    assert q > D.limit(family), (plant, key, k, q)
                    hit += 1
                else:
                    assert q <= D.limit(family), (plant, key, k, q)
    assert hit >= 4
