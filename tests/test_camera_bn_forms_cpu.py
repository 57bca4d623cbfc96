"""CPU half of the camera head's grouped-BatchNorm sweep (tests/camera_bn_forms.py): the case lists are what they say, every activation
decision keeps its margin, the float64 restatement is torch's module in train mode called once per group, the committed float32
constants are what the module measures, the launchers refuse what the header says before any HIP call, a float32 emulation of the
kernels' formulas stays within the limit, and the same emulation with one planted error does not."""
import ctypes

import pytest
import torch
from torch import nn

from tests import camera_bn_forms as P

F64 = torch.float64


# ---- constants and case lists ----------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers_and_the_trainers():
    from nopesac_amd import _lib, training
    H = _lib.H
    assert P.RPS == H.NPS_BN_GROUPED_RPS and P.SEGMENTS == H.NPS_BN_GROUPED_SEGMENTS and H.NPS_BN_GROUPED_MAX_GROUPS >= 2
    assert P.ACTS == {"none": H.NPS_ACT_NONE, "relu": H.NPS_ACT_RELU, "leaky": H.NPS_ACT_LEAKY}
    assert (P.EPS, P.MOMENTUM) == (training.BN_EPS, training.BN_MOMENTUM) == (1e-3, 0.01)
    assert P.LEAK == float(torch.tensor(0.01, dtype=torch.float32))


def test_case_lists_are_what_they_say():
    R, S = P.RPS, P.SEGMENTS
    assert set(P.ROWS) == {2, 6, R - 1, R, R + 1, 2 * R + 1, S * R + 1} and set(P.GROUPS) == {1, 2} and set(P.CHANNELS) == {4, 128, 256}
    assert all((n, G, C, "leaky") in P.CASES for n in P.ROWS for G in P.GROUPS for C in P.CHANNELS)
    assert {k[-1] for k in P.CASES} == {"leaky", "relu", "none", "offset", "gamma0", "neggamma"} and len(set(P.CASES)) == len(P.CASES)
    assert all(k[:3] == P.TAG_SHAPE for k in P.CASES if k[-1] != "leaky") and P.TAG_SHAPE[1] == 2 and P.TAG_SHAPE[0] > R
    assert any(-(-n // R) > S for n, _, _, _ in P.CASES)                       # one block more than the finishing pass's runs
    assert max(n * G for n, G, _, _ in P.CASES) < 10000
    for key in P.CASES:
        n, G, C, tag = key
        c = P.bn_inputs(key)
        assert tuple(c["src"].shape) == tuple(c["g"].shape) == (G * n, C) and c["src"].is_contiguous()
        assert c["act"] == {"relu": "relu", "none": "none"}.get(tag, "leaky")
        v = c["src"].double().view(G, n, C)
        mean, std = v.mean(1), v.std(1, unbiased=False)
        if tag == "offset":
            ratio = mean.abs() / std
            assert float(ratio.min()) > 0.4 * P.OFFSET and float(ratio.max()) < 2.5 * P.OFFSET
        if tag == "gamma0":
            assert bool((c["gamma"][::3] == 0).all()) and bool((c["gamma"][1::3] != 0).all())
        if tag == "neggamma":
            assert bool((c["gamma"] < 0).all())
        elif tag != "gamma0":
            assert bool((c["gamma"] < 0).any()) or C == 4
        if G == 2 and n >= P.RPS - 1:                                         # the second group: another mean and another scale per channel
            assert tag == "offset" or float(((mean[0] - mean[1]).abs() / (std[0] + std[1])).min()) > 0.5
            assert float((std[0] / std[1]).log().abs().min()) > 0.2


def test_every_activation_decision_keeps_its_margin():
    for key in P.CASES:
        c = P.bn_inputs(key)
        z, margin = P.bn_z(c, c["src"])
        assert bool((margin >= P.MARGIN).all())
        if c["act"] != "none":
            assert bool(((z.abs() > margin) | (c["gamma"] == 0)).all()) and bool((z.abs() > 0).all()), key


# ---- references ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(2, 1, 4, "leaky"), (6, 2, 128, "leaky"), P.TAG_SHAPE + ("offset",), P.TAG_SHAPE + ("relu",), P.TAG_SHAPE + ("none",)])
def test_restatement_is_torchs_module_called_once_per_group(key):
    """bn_run in float64 = one nn.BatchNorm2d(eps=0.001, momentum=0.01) module in train mode called on group 0, then on group 1 - the
    siamese tower's calls (camera_head.py:646-647) - followed by the activation module, under autograd; the module's buffers and its
    counter after one and after three rounds"""
    c = P.bn_inputs(key)
    n, G, C, _ = key
    mine = P.bn_run(c, {k: c[k] for k in P.BN_FLOATS}, F64)
    bn = nn.BatchNorm2d(C, eps=0.001, momentum=0.01).double().train()
    act = {"leaky": nn.LeakyReLU(P.LEAK), "relu": nn.ReLU(), "none": nn.Identity()}[c["act"]]      # (the slope a float32 run uses: 0.01f)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["run_mean"]); bn.running_var.copy_(c["run_var"])
    src = c["src"].double().clone().requires_grad_(True)
    groups = [src[i * n:(i + 1) * n].t().contiguous()[None, :, :, None] for i in range(G)]        # NCHW, [1, C, n, 1]
    y = torch.cat([act(bn(x))[0, :, :, 0].t() for x in groups])
    (y * c["g"].double()).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max()))
    assert close(mine["y"], y.detach()) and close(mine["dc"], src.grad) and close(mine["dgamma"], bn.weight.grad) and close(mine["dbeta"], bn.bias.grad)
    assert close(mine["run_mean1"], bn.running_mean) and close(mine["run_var1"], bn.running_var) and int(bn.num_batches_tracked) == G
    with torch.no_grad():
        for _ in range(2):
            for x in groups:
                bn(x)
    assert close(mine["run_mean3"], bn.running_mean) and close(mine["run_var3"], bn.running_var) and int(bn.num_batches_tracked) == 3 * G
    assert tuple(mine["mean"].shape) == tuple(mine["rstd"].shape) == (G, C)


def test_reference_magnitudes_dominate_the_results():
    for key in ((6, 2, 128, "leaky"), P.TAG_SHAPE + ("offset",), P.TAG_SHAPE + ("relu",), P.TAG_SHAPE + ("neggamma",)):
        c = P.bn_inputs(key)
        x = {k: c[k] for k in P.BN_FLOATS}
        ref, S = P.bn_run(c, x, F64), P.bn_mags(c, x)
        assert set(S) == set(ref)
        for k in S:
            assert bool((ref[k].abs() <= S[k] * (1 + 1e-12) + 1e-300).all()), (key, k)


@pytest.mark.parametrize("family", sorted(P.F32_WORST))
def test_f32_worst_is_what_the_module_measures(family):
    measured = P.f32_worst(family)
    print("%s: committed %.3g, measured %.3g" % (family, P.F32_WORST[family], measured))
    assert P.F32_WORST[family] / 2 <= measured <= P.F32_WORST[family] * 2
    assert P.limit(family) == P.LIMIT_FACTOR * max(P.F32_WORST[family], 1.0)
    assert set(P.F32_WORST) == set(P.FAMILIES)


# ---- launchers -------------------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from nopesac_amd import _lib
    try:
        return _lib, _lib.load()
    except RuntimeError as e:            # pragma: no cover - the library is built by build()
        pytest.skip(str(e))


def _aligned_floats(n):
    """(keep-alive, address) of n floats on a 16-byte boundary"""
    buf = (ctypes.c_float * (n + 4))()
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


def test_workspace_entry_is_the_macro_and_a_status():
    """G (ceil(n / RPS) + 1) 2 C floats: the blocks' partials and, behind them, the backward's per-group sums; a status entry that
    writes the value through a pointer, 0 with NPS_E_ARG for arguments the launchers refuse"""
    from nopesac_amd import ops
    lib, L = _lib_or_skip()
    macro = lambda G, n, C: G * (-(-n // P.RPS) + 1) * 2 * C
    assert "nopesac_bn_train_grouped_workspace_floats" in lib.STATUS
    for args in ((1, 2, 4), (2, P.RPS, 8), (2, P.RPS + 1, 128), (2, 8 * 4800, 256), (1, 48, 128), (64, 6, 4)):
        assert ops.bn_train_grouped_workspace_floats(*args) == macro(*args) > 0, args
    out = ctypes.c_int64(-5)
    for bad in ((0, 300, 16), (-1, 300, 16), (65, 300, 16), (2, 0, 16), (2, -3, 16), (2, 300, 0), (2, 300, 6), (2, 1 << 40, 16)):
        assert L.nopesac_bn_train_grouped_workspace_floats(*bad, ctypes.addressof(out)) == lib.H.NPS_E_ARG and out.value == 0, bad
        with pytest.raises(lib.HipKernelError):
            ops.bn_train_grouped_workspace_floats(*bad)
    assert L.nopesac_bn_train_grouped_workspace_floats(1, 2, 4, None) == lib.H.NPS_E_ARG


def test_launchers_refuse_before_any_hip_call():
    """NPS_E_ARG with no device: a null pointer, G < 1, n < 2, C % 4 != 0, a pointer off the 16-byte grid, a workspace a float short, one
    running buffer without the other, eps / momentum out of range, an unknown activation"""
    lib, L = _lib_or_skip()
    E = lib.H.NPS_E_ARG
    keep, p = _aligned_floats(64)
    need = 2 * 3 * 2 * 16
    stats = lambda c=p, G=2, n=300, C=16, eps=1e-3, mom=0.01, mean=p, rm=None, rv=None, ws=p, wsn=need: \
        L.nopesac_bn_train_grouped_stats_f32(c, G, n, C, eps, mom, mean, p, p, rm, rv, ws, wsn, None)
    for kw in (dict(c=None), dict(mean=None), dict(ws=None), dict(G=0), dict(G=lib.H.NPS_BN_GROUPED_MAX_GROUPS + 1), dict(n=1), dict(n=0), dict(C=6),
               dict(C=0), dict(c=p + 4), dict(ws=p + 8), dict(wsn=need - 1), dict(rm=p), dict(rv=p), dict(eps=0.0), dict(mom=1.5), dict(mom=-0.1),
               dict(n=1 << 31)):
        assert stats(**kw) == E and L.nopesac_last_error(), kw
    apply = lambda c=p, G=2, n=300, C=16, gamma=p, mean=p, act=2, y=p: L.nopesac_bn_train_grouped_apply_f32(c, G, n, C, gamma, p, mean, p, act, y, None)
    for kw in (dict(c=None), dict(y=None), dict(G=0), dict(n=0), dict(C=10), dict(gamma=p + 4), dict(mean=p + 12), dict(y=p + 4), dict(act=3), dict(act=-1),
               dict(act=0x102)):
        assert apply(**kw) == E, kw
    bwd = lambda dy=p, G=2, n=300, C=16, rstd=p, act=2, dc=p, dg=p, ws=p, wsn=need: \
        L.nopesac_bn_train_grouped_backward_f32(dy, p, G, n, C, p, p, p, rstd, act, 1, dc, dg, p, ws, wsn, None)
    for kw in (dict(dy=None), dict(dc=None), dict(dg=None), dict(ws=None), dict(G=0), dict(n=0), dict(C=18), dict(rstd=p + 4), dict(dg=p + 4), dict(act=3),
               dict(wsn=need - 1), dict(wsn=0)):
        assert bwd(**kw) == E, kw


def test_wrappers_have_no_cpu_path():
    from nopesac_amd import ops
    t, v = torch.zeros(8, 4), torch.zeros(4)
    with pytest.raises(ops.OpsArgumentError):
        ops.bn_train_grouped_stats(t, 2, eps=P.EPS, momentum=P.MOMENTUM)
    with pytest.raises(ops.OpsArgumentError):
        ops.bn_train_grouped_apply(t, v, v, v, v, ops.ACT_LEAKY, 1)
    with pytest.raises(ops.OpsArgumentError):
        ops.bn_train_grouped_backward(t, t, v, v, v, v, ops.ACT_LEAKY, 1)


def test_trainer_flag_needs_the_conv_stacks_and_builds_the_buffers():
    """batch_stats=True: refused without conv_stacks; 179 parameters as before, 36 running statistics (f32 clones) and 18 int64
    counters; the default keeps the 36 statistics it had"""
    from nopesac_amd import ops
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import BACKBONE_CONVS, PREFIX, CameraHeadTrainer
    sd = synth_state_dict(50)
    with pytest.raises(ops.OpsArgumentError):
        CameraHeadTrainer.from_state_dict(sd, 50, "cpu", batch_stats=True)
    tr = CameraHeadTrainer.from_state_dict(sd, 50, "cpu", conv_stacks=True, batch_stats=True)
    old = CameraHeadTrainer.from_state_dict(sd, 50, "cpu", conv_stacks=True)
    assert tr.batch_stats and not old.batch_stats and sorted(tr.params) == sorted(old.params) and len(tr.params) == 179
    stats = [k for k in tr.buffers if not k.endswith("num_batches_tracked")]
    counters = [k for k in tr.buffers if k.endswith("num_batches_tracked")]
    assert len(stats) == 36 and len(counters) == 18 and sorted(stats) == sorted(old.buffers)
    assert all(tr.buffers[k].dtype == torch.float32 and tr.buffers[k].data_ptr() != sd[k].data_ptr() and torch.equal(tr.buffers[k], sd[k].float()) for k in stats)
    assert all(tr.buffers[k].dtype == torch.int64 and tr.buffers[k].data_ptr() != sd[k].data_ptr() for k in counters)
    layers = {k[len(PREFIX):].rsplit(".", 2)[0] for k in counters}
    assert layers == {"convs_backbone.%d" % i for i in BACKBONE_CONVS} | {"%s.%d" % (b, i) for b in ("convs_trans", "convs_rots") for i in range(6)}
    short = {k: v for k, v in tr.buffers.items() if k != counters[0]}
    with pytest.raises(ops.OpsArgumentError):
        CameraHeadTrainer(tr.params, 50, buffers=short, conv_stacks=True, batch_stats=True)


# ---- the trainer's reference -----------------------------------------------------------------------------------------------------------
def test_trainer_f32_figures_are_what_the_module_measures():
    """the float32 torch run of the training-mode head under batch statistics against the float64 run with its decisions: the stored
    figures within 2x, every other tensor below GRAD_FLOOR / LIMIT_FACTOR - the conv stacks' 71 tensors among them"""
    fig = P.trainer_f32_figures()
    assert len(fig) == 179 and set(P.TRAINER_F32) < set(fig)
    for k, v in fig.items():
        if k in P.TRAINER_F32:
            assert P.TRAINER_F32[k] / 2 <= v <= P.TRAINER_F32[k] * 2, (k, v, P.TRAINER_F32[k])
            assert P.grad_bound(k) == P.LIMIT_FACTOR * P.TRAINER_F32[k] > P.GRAD_FLOOR
        else:
            assert v * P.LIMIT_FACTOR <= P.GRAD_FLOOR == P.grad_bound(k), (k, v)
    assert not any("convs_" in k or "pixel_decoder" in k for k in P.TRAINER_F32)


def test_the_stand_in_block_is_the_reference_module_in_train_mode():
    """BatchStatBlock = nn.Conv2d(bias=False) + nn.BatchNorm2d(eps=0.001, momentum=0.01) + nn.LeakyReLU in train mode, buffers included;
    with `rec` a pre-activation within TIE of 0 takes the recorded side, every other one its own"""
    g = torch.Generator().manual_seed(5)
    p = P.CAM + ".convs_trans.1"
    seq = nn.Sequential(nn.Conv2d(8, 8, 3, 2, 1, bias=False), nn.BatchNorm2d(8, eps=0.001, momentum=0.01), nn.LeakyReLU(P.LEAK)).double().train()
    with torch.no_grad():
        for t in (seq[0].weight, seq[1].weight, seq[1].bias, seq[1].running_mean):
            t.copy_(torch.randn(t.shape, generator=g))
    sd = {p + "." + k: v.detach().clone() for k, v in seq.state_dict().items() if v.is_floating_point()}
    x = torch.randn(2, 8, 6, 8, generator=g).double()
    block = P.BatchStatBlock()
    y = block(x, sd, p, 2)
    want = seq(x)
    assert float((y - want).abs().max()) < 1e-13 and tuple(y.shape) == (2, 8, 3, 4)
    assert float((sd[p + ".1.running_mean"] - seq[1].running_mean).abs().max()) < 1e-15 and float((sd[p + ".1.running_var"] - seq[1].running_var).abs().max()) < 1e-15
    mean, var, _ = block.stats["convs_trans.1"][0]
    prog = P.running_progress((seq.state_dict()["1.running_mean"] * 0, torch.ones(8).double()), [(mean, var)], (1,))
    # (one step from the module's fresh buffers 0 / 1: the closed form of the update)
    fresh = nn.BatchNorm2d(8, eps=0.001, momentum=0.01).double().train()
    fresh(seq[0](x))
    assert float((prog[1][0] - fresh.running_mean).abs().max()) < 1e-15 and float((prog[1][1] - fresh.running_var).abs().max()) < 1e-15
    # the recorded side decides within TIE of the kink only
    z = torch.where(y.detach() > 0, y.detach(), y.detach() / P.LEAK)
    small = z.abs() <= P.TIE * z.abs().max()
    flipped = P.BatchStatBlock({"convs_trans.1": -y.detach()})(x, dict(sd), p, 2)
    assert bool(((flipped == y) | small).all())


def test_the_consistent_pool_takes_the_float32_winner_within_the_tie_only():
    x = torch.tensor([[1.0, 1.0 + 1e-9, 5.0, 2.0], [0.5, 0.25, 4.0, 3.0]], dtype=F64).view(1, 1, 2, 4).requires_grad_(True)
    ref = x.detach().clone()
    ref[0, 0, 0, 0] = 1.0 + 1e-7                             # the float32 forward saw the first element as the winner of window 0 ...
    ref[0, 0, 1, 3] = 9.0                                   # ... and (wrongly, far beyond a tie) the last one as the winner of window 1
    rec = {"convs_backbone.1": ref, "convs_backbone.4": ref}
    y = P.ConsistentPool(rec, B=1)(x, 2, 2)
    assert y.flatten().tolist() == [1.0, 5.0]
    y.sum().backward()
    assert x.grad.flatten().tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    pool = P.ConsistentPool(rec, B=1)
    assert torch.equal(pool(x.detach(), 3, 2, 1), torch.nn.functional.max_pool2d(x.detach(), 3, 2, 1)) and pool.calls == 0


# ---- sharpness -------------------------------------------------------------------------------------------------------------------------
def _worst(family, key, got):
    return {k: q for k, (q, _) in P.worst_ratio(family, key, {k: got[k] for k in P.OUTPUTS[family]}).items()}


def test_emulated_kernels_stay_within_the_limit():
    for key in P.CASES:
        got = P.emulate(key)
        for family in P.FAMILIES:
            assert max(_worst(family, key, got).values()) <= P.limit(family), (family, key)


PLANT_CASE = {"one_pass_variance": P.TAG_SHAPE + ("offset",), "dgamma_term_omitted": P.TAG_SHAPE + ("leaky",), "unbiased_variance": P.TAG_SHAPE + ("leaky",),
              "pooled_groups": P.TAG_SHAPE + ("leaky",), "running_order_reversed": P.TAG_SHAPE + ("leaky",), "leaky_as_relu": P.TAG_SHAPE + ("leaky",)}
PLANT_BREAKS = {"one_pass_variance": {"stats": ("var", "rstd")}, "dgamma_term_omitted": {"backward": ("dc",)},
                "unbiased_variance": {"stats": ("rstd",), "apply": ("y",)}, "pooled_groups": {"stats": ("mean", "var", "rstd"), "apply": ("y",), "backward": ("dc",)},
                "running_order_reversed": {"running": ("run_mean1", "run_var1", "run_mean3", "run_var3")},
                "leaky_as_relu": {"apply": ("y",), "backward": ("dc", "dgamma", "dbeta")}}


@pytest.mark.parametrize("plant", P.PLANTS)
def test_a_planted_error_breaks_the_limit(plant):
    key = PLANT_CASE[plant]
    got, clean = P.emulate(key, plant), P.emulate(key)
    for family, outs in PLANT_BREAKS[plant].items():
        w = _worst(family, key, got)
        for k in outs:
            assert w[k] > P.limit(family), (plant, family, k, w[k])
        assert max(_worst(family, key, clean).values()) <= P.limit(family)
