"""CPU half of the pyramid-training sweep (tests/plane_pyramid_forms.py): the case lists are what they say, every ReLU decision keeps its
margin, the float64 restatements are torch's modules in train mode, the adjoint's gather formula is up2's matrix transposed, the
committed float32 constants are what the module measures, a float32 emulation of the kernels' formulas stays within the limit, and the
same emulation with one planted error does not."""
import pytest
import torch
from torch import nn

from tests import plane_pyramid_forms as P

F64 = torch.float64


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
def test_block_size_is_the_headers():
    from nopesac_amd import _lib
    assert P.RPS == _lib.H.NPS_BN_TRAIN_RPS


def test_case_lists_are_what_they_say():
    assert set(P.PLAIN_ROWS) == {2, P.RPS - 1, P.RPS, P.RPS + 1, 2 * P.RPS + 1} and set(P.PLAIN_C) == {4, 12, 64, 256}
    assert all(("plain", r, c, "base") in P.PLAIN_CASES for r in P.PLAIN_ROWS for c in P.PLAIN_C)
    assert set(P.UP_HW) == {(1, 1), (1, 3), (3, 1), (2, 2), (3, 4), (5, 7)} and set(P.UP_B) == {1, 2} and set(P.UP_C) == {4, 12, 256}
    assert all(("up", b, h, w, c, "base") in P.UP_CASES for h, w in P.UP_HW for b in P.UP_B for c in P.UP_C)
    assert set(P.ADJ_CASES) == {(b, h, w, c) for h, w in P.UP_HW for b in P.UP_B for c in P.UP_C}
    for cases in (P.PLAIN_CASES, P.UP_CASES):
        assert {k[-1] for k in cases} == {"base", "offset", "gamma0", "noact", "frozen", "slice"}
    assert any(4 * b * h * w > P.RPS for _, b, h, w, _, _ in P.UP_CASES)                    # the upsampled form reaches a second block
    blocks = lambda n: -(-n // P.RPS)                                                       # ... and both forms a run of two blocks
    assert any(blocks(r) > P.SEGMENTS for _, r, _, _ in P.PLAIN_CASES) and any(blocks(4 * b * h * w) > P.SEGMENTS for _, b, h, w, _, _ in P.UP_CASES)
    assert "frozen" not in {k[-1] for k in P.family_keys("stats")} and len(P.family_keys("backward")) == len(P.BN_CASES)
    addends = 0
    for key in P.BN_CASES:
        c = P.bn_inputs(key)
        tag = key[-1]
        assert c["n"] == (4 if c["up"] else 1) * int(torch.tensor(c["shape"]).prod()) >= 2
        assert tuple(c["g"].shape) == tuple(c["out_shape"]) and (c["g"] == 0).any() or c["g"].numel() < 64
        assert c["relu"] == (tag != "noact") and c["batch_stats"] == (tag != "frozen")
        assert (c["src"].stride(-2) == c["C"] + 8) == (tag == "slice")
        v = P._v(c, c["src"].double())
        ratio = v.mean(0).abs() / v.std(0, unbiased=False)
        if tag == "offset":
            assert float(ratio.min()) > 0.5 * P.OFFSET and float(ratio.max()) < 2 * P.OFFSET
        if tag == "gamma0":
            assert bool((c["gamma"][::3] == 0).all()) and bool((c["gamma"][1::3] != 0).all())
        addends += c["addend"] is not None
    assert 0 < addends < len(P.BN_CASES)


def test_every_relu_decision_keeps_its_margin():
    for key in P.BN_CASES:
        c = P.bn_inputs(key)
        z, margin = P.bn_z(c, c["src"])
        assert bool((margin >= P.MARGIN).all())
        if c["relu"]:
            assert bool((z.abs() > margin).all()), key
    for key in P.PYR_CASES:
        c = P.pyramid_inputs(key)
        m = P.pyramid_margins(c["sd"], c["bufs"], c["feats"], c["memory"], c["B"])
        assert len(m) == 8
        for q, (z, margin) in m.items():
            assert bool((margin >= P.MARGIN).all()) and bool((z.abs() > margin).all()), (key, q)


def test_the_trainer_holds_the_pyramids_tensors_in_the_references_optimiser_groups():
    from nopesac_amd.config import get_cfg
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlanePyramidTrainer
    sd = synth_state_dict(7)
    tr = PlanePyramidTrainer.from_state_dict(sd, "cpu")
    assert sorted(tr.params) == P.pyramid_parameter_names(sd.keys()) and len(tr.params) == 24
    stats = P.pyramid_buffer_names(sd.keys())
    assert len(stats) == 16 and len(tr.buffers) == 24 and set(stats) < set(tr.buffers)
    counters = sorted(set(tr.buffers) - set(stats))
    assert all(k.endswith("num_batches_tracked") and tr.buffers[k].dtype == torch.int64 for k in counters)
    decay = {k: tr._weight_decay(k, 0.5, 0.25) for k in tr.params}
    norm = [k for k in tr.params if ".1." in k]
    assert len(norm) == 16 and all(decay[k] == 0.25 for k in norm) and all(v == 0.5 for k, v in decay.items() if k not in norm)
    assert tr._weight_decay(norm[0], 0.5, None) == 0.5
    cfg = get_cfg()
    assert tr.lr_multiplier(cfg) == float(cfg.SOLVER.SEM_SEG_HEAD_MULTIPLIER)
    with pytest.raises(Exception):
        PlanePyramidTrainer({k: v for k, v in list(tr.params.items())[:-1]}, tr.buffers)


# ---- references ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("plain", 2, 4, "base"), ("plain", P.RPS + 1, 12, "offset"), ("up", 2, 5, 7, 12, "base"), ("up", 1, 1, 3, 4, "base"),
                                 ("up", 2, 5, 7, 12, "frozen")])
def test_batchnorm_restatement_is_torchs_modules(key):
    """bn_run in float64 = nn.Upsample + nn.BatchNorm2d + nn.ReLU modules in train mode (eval mode for `frozen`) under autograd, and the
    module's buffers after one and three calls"""
    c = P.bn_inputs(key)
    x = {k: c[k] for k in P.BN_FLOATS if c[k] is not None}
    mine = P.bn_run(c, x, F64)
    bn = nn.BatchNorm2d(c["C"]).double()
    up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["run_mean"]); bn.running_var.copy_(c["run_var"])
    bn.train(c["batch_stats"])
    src = c["src"].double().clone().requires_grad_(True)
    nchw = src.permute(0, 3, 1, 2) if c["up"] else src.t()[None, :, :, None]
    z = bn(up(nchw) if c["up"] else nchw)
    y = (torch.relu(z) if c["relu"] else z).permute(0, 2, 3, 1).reshape(c["out_shape"])
    if c["addend"] is not None:
        y = y + c["addend"].double()
    (y * c["g"].double()).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max()))
    assert close(mine["y"], y.detach()) and close(mine["dsrc"], src.grad) and close(mine["dgamma"], bn.weight.grad) and close(mine["dbeta"], bn.bias.grad)
    if c["batch_stats"]:
        assert close(mine["run_mean1"], bn.running_mean) and close(mine["run_var1"], bn.running_var) and int(bn.num_batches_tracked) == 1
        with torch.no_grad():
            bn(up(nchw) if c["up"] else nchw); bn(up(nchw) if c["up"] else nchw)
        assert close(mine["run_mean3"], bn.running_mean) and close(mine["run_var3"], bn.running_var) and int(bn.num_batches_tracked) == 3


def test_pyramid_restatement_is_the_reference_modules():
    """pyramid_forward (matrix products over NHWC pixels) = nn.Conv2d + nn.BatchNorm2d + nn.ReLU + nn.Upsample modules in train mode, wired
    as top_down.forward (planeTR_head.py:241-252)"""
    c = P.pyramid_inputs((2, 6, 8))
    B = c["B"]
    mods = {}
    for nm in P.CONVS:
        q = P.PREFIX + nm
        w = c["sd"][q + ".0.weight"]
        m = nn.Sequential(nn.Conv2d(w.shape[1], 256, 1, bias=False), nn.BatchNorm2d(256), nn.ReLU(inplace=True)).double().train()
        m.load_state_dict({"0.weight": w.double(), "1.weight": c["sd"][q + ".1.weight"].double(), "1.bias": c["sd"][q + ".1.bias"].double(),
                           "1.running_mean": c["bufs"][q + ".1.running_mean"].double(), "1.running_var": c["bufs"][q + ".1.running_var"].double(),
                           "1.num_batches_tracked": torch.tensor(0)})
        mods[nm] = m
    up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)
    f = {k: v.double().permute(0, 3, 1, 2) for k, v in c["feats"].items()}
    with torch.no_grad():
        p = mods["c4_conv"](f["res5"]) + mods["m_conv_dict.m4"](c["memory"].double().view(B, 6, 8, 256).permute(0, 3, 1, 2))
        p = mods["up_conv3"](up(p)) + mods["c3_conv"](f["res4"])
        p = mods["up_conv2"](up(p)) + mods["c2_conv"](f["res3"])
        p = mods["up_conv1"](up(p)) + mods["c1_conv"](f["res2"])
    ref, A = P.reference("pyramid", (2, 6, 8))
    assert float((ref["p1"] - p.permute(0, 2, 3, 1)).abs().max()) < 1e-11
    for nm in P.CONVS:
        for leaf in ("running_mean", "running_var"):
            assert float((ref[f"{P.PREFIX}{nm}.1.{leaf}"] - getattr(mods[nm][1], leaf)).abs().max()) < 1e-12
    assert len(ref) == 46 and set(ref) == set(A) and all(bool((A[k] >= 0).all()) for k in A)
    assert tuple(ref["memory"].shape) == (B * 48, 256) and tuple(ref["res5"].shape) == (B, 6, 8, 2048)


def test_the_fixture_is_the_float64_pyramid_within_the_limit():
    """the reference's own float32 run (tests/golden/L_plane_pyramid_6x8.npz: top_down in train mode, on the CPU) stands within the limit
    of the float64 restatement on every element it stores: the restatement is the reference's pyramid; the counters count one forward"""
    gold = P.golden(6, 8)
    w = P.fixture_worst((2, 6, 8), gold)
    lim = P.limit("pyramid")
    print("fixture: worst error / (limit x A) %s" % sorted(((k, "%.3f" % (q / lim)) for k, q in w.items()), key=lambda kv: -float(kv[1]))[:5])
    assert len(w) == 43 and all(q <= lim for q in w.values()), {k: q for k, q in w.items() if q > lim}
    counters = [k for k in gold.files if k.endswith("num_batches_tracked")]
    assert len(counters) == 8 and all(int(gold[k]) == 1 for k in counters)
    assert gold["memory"].shape == (96, 256) and gold["p1_sub"].shape == (2, 12, 16, 256)


def test_adjoint_formula_is_up2s_matrix_transposed():
    """the gather dx[i] = 0.75 (du[2i] + du[2i+1]) + 0.25 (du[2i-1] + du[2i+2]) with the border taps folded back, as a dense matrix at
    3 x 4, is the transpose of up2's matrix (from the source-index rule, and from F.interpolate on the unit maps)"""
    for n in (1, 2, 3, 4, 7):
        assert torch.equal(P.adjoint_axis_matrix(n), P.up2_axis_matrix(n).t())
        assert not torch.equal(P.adjoint_axis_matrix(n, fold=False), P.up2_axis_matrix(n).t())
    H, W = 3, 4
    eye = torch.eye(H * W, dtype=F64).view(H * W, H, W, 1)
    M = P.up2(eye).reshape(H * W, 4 * H * W).t()                              # [4HW, HW]: up2 as a matrix
    K = torch.kron(P.adjoint_axis_matrix(H), P.adjoint_axis_matrix(W))        # [HW, 4HW]
    assert torch.equal(K, M.t())
    du = torch.randn(2, 2 * H, 2 * W, 5, dtype=F64)
    assert float((P.adjoint_by_matrices(du) - P.up2_t(du, (2, H, W, 5))).abs().max()) < 1e-14


def test_reference_magnitudes_dominate_the_results():
    for key in (("plain", P.RPS + 1, 12, "base"), ("up", 2, 5, 7, 12, "base"), ("up", 2, 5, 7, 12, "frozen"), ("plain", P.RPS + 1, 12, "offset")):
        c = P.bn_inputs(key)
        x = {k: c[k] for k in P.BN_FLOATS if c[k] is not None}
        ref, S = P.bn_run(c, x, F64), P.bn_mags(c, x)
        for k in S:
            assert bool((ref[k].abs() <= S[k] * (1 + 1e-12) + 1e-300).all()), (key, k)


# ---- constants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(P.F32_WORST))
def test_f32_worst_is_what_the_module_measures(family):
    measured = P.f32_worst(family)
    print("%s: committed %.3g, measured %.3g" % (family, P.F32_WORST[family], measured))
    assert P.F32_WORST[family] / 2 <= measured <= P.F32_WORST[family] * 2
    assert P.limit(family) == P.LIMIT_FACTOR * max(P.F32_WORST[family], 1.0)


# ---- sharpness -------------------------------------------------------------------------------------------------------------------------
def _worst(family, key, got):
    return {k: q for k, (q, _) in P.worst_ratio(family, key, {k: got[k] for k in P.OUTPUTS[family]}).items()}


def test_emulated_kernels_stay_within_the_limit():
    for key in P.BN_CASES:
        got = P.emulate_bn(key)
        for family in ("stats", "running", "apply", "backward"):
            if key in P.family_keys(family):
                assert max(_worst(family, key, got).values()) <= P.limit(family), (family, key)
    for key in P.ADJ_CASES:
        c = P.adjoint_inputs(key)
        w = P.worst_ratio("adjoint", key, {"dx": P.adjoint_by_matrices(c["du"])})
        assert w["dx"][0] <= P.limit("adjoint"), key


PLANT_CASE = {"one_pass_variance": ("plain", P.RPS + 1, 12, "offset"), "border_foldback_dropped": ("up", 2, 5, 7, 12, "base"),
              "dgamma_term_omitted": ("plain", P.RPS + 1, 12, "base"), "unbiased_variance": ("plain", P.RPS + 1, 12, "base")}
PLANT_BREAKS = {"one_pass_variance": {"stats": ("var", "rstd")}, "border_foldback_dropped": {"backward": ("dsrc",)},
                "dgamma_term_omitted": {"backward": ("dsrc",)}, "unbiased_variance": {"stats": ("rstd",), "apply": ("y",)}}


@pytest.mark.parametrize("plant", P.BN_PLANTS)
def test_a_planted_error_breaks_the_limit(plant):
    key = PLANT_CASE[plant]
    got = P.emulate_bn(key, plant)
    for family, outs in PLANT_BREAKS[plant].items():
        w = _worst(family, key, got)
        for k in outs:
            assert w[k] > P.limit(family), (plant, family, k, w[k])
    clean = P.emulate_bn(key)
    for family in PLANT_BREAKS[plant]:
        assert max(_worst(family, key, clean).values()) <= P.limit(family)
    if plant == "border_foldback_dropped":                                  # ... and the stand-alone adjoint without the fold-back
        akey = (2, 5, 7, 12)
        c = P.adjoint_inputs(akey)
        assert P.worst_ratio("adjoint", akey, {"dx": P.adjoint_by_matrices(c["du"], fold=False)})["dx"][0] > P.limit("adjoint")
