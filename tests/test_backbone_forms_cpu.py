"""tests/backbone_forms.py without a GPU: its case lists reach every boundary of the strided dgrad's tile (from the header's
NPS_DGRAD_S2_* constants), its references are torch's autograd, the committed float32 figures are what the CPU measures, the bound is
sharp enough to see a wrong tap and a missing zero fill, and BackboneTrainer's keys, groups and multiplier are the reference's."""
import re

import pytest
import torch

from tests import backbone_forms as BF
from tests.util import ROOT


def test_the_constants_are_the_headers():
    text = open(ROOT + "/include/nopesac_hip.h").read()
    vals = {n: int(v) for n, v in re.findall(r"#define NPS_DGRAD_S2_(\w+) (\d+)", text)}
    assert vals == {"PIXELS": BF.PIXELS, "CHANNELS": BF.CHANNELS, "STAGE": BF.STAGE}
    assert BF.PIXELS % 2 == 0 and BF.CHANNELS % 4 == 0 and BF.STAGE % 4 == 0
    # the workspace macro is the weights' own size in bytes, which is what ops.conv2d_dgrad_strided asks scratch() for
    m = re.search(r"#define NPS_DGRAD_S2_WORKSPACE_BYTES\(Cin, Cout, KH, KW\) \(\(int64_t\)\(Cin\) \* \(Cout\) \* \(KH\) \* \(KW\) \* 4\)", text)
    src = open(ROOT + "/nopesac_amd/ops.py").read()
    assert m and "scratch(dy.device, 4 * w.numel())" in src[src.index("def conv2d_dgrad_strided"):src.index("def maxpool3x3s2_backward")]


def test_the_case_lists_reach_every_boundary():
    cases = BF.DGRAD_CASES
    assert len(set(cases)) == len(cases)
    base = {c[:6] for c in cases if c[-1] == "base"}
    assert all((k, b, h, w, ci, co) in base for k in (1, 3) for h, w in ((1, 1), (2, 2), (3, 3), (4, 6), (5, 9), (7, 10)) for b in (1, 2)
               for ci, co in ((4, 4), (12, 8), (64, 132), (132, 64)))
    for k in (1, 3):
        mine = [c for c in cases if c[0] == k]
        # every parity class at the tile's pixels - 1, exactly, + 1
        counts = {cls: {BF.class_pixels(c[1], c[2], c[3])[cls] for c in mine} for cls in ((0, 0), (0, 1), (1, 0), (1, 1))}
        assert all({BF.PIXELS - 1, BF.PIXELS, BF.PIXELS + 1} <= n for n in counts.values()), counts
        # more than one pixel tile and more than one channel tile; Cin at the channel tile +- 4
        assert any(max(BF.class_pixels(c[1], c[2], c[3]).values()) > BF.PIXELS for c in mine)
        assert {BF.CHANNELS - 4, BF.CHANNELS, BF.CHANNELS + 4} <= {c[4] for c in mine}
        # K = taps x Cout of some class: one LDS stage exactly, and crossed by one float4
        ks = {len(BF.class_taps(k, ph)) * len(BF.class_taps(k, pw)) * c[5] for c in mine for ph in (0, 1) for pw in (0, 1)}
        assert {BF.STAGE - 4, BF.STAGE, BF.STAGE + 4} <= ks
        assert any(c[-1] == "slice" for c in mine)
    assert [len(BF.class_taps(3, p)) for p in (0, 1)] == [1, 2] and [len(BF.class_taps(1, p)) for p in (0, 1)] == [1, 0]
    # odd and even sizes, a last odd row whose kh = 0 tap has no output row (even H), empty classes (H = 1)
    assert {c[2] % 2 for c in cases} == {0, 1} and {c[3] % 2 for c in cases} == {0, 1} and any(c[2] == 1 for c in cases)
    prod = {(c[0], c[2], c[3], c[4], c[5]) for c in BF.PRODUCTION_CASES}
    assert prod == {(3, 120, 160, 128, 128), (3, 60, 80, 256, 256), (3, 30, 40, 512, 512), (1, 120, 160, 256, 512), (1, 60, 80, 512, 1024),
                    (1, 30, 40, 1024, 2048)}
    assert all(c[1] == 1 for c in BF.PRODUCTION_CASES) and BF.IDENTITY_CASE in cases
    assert {(k[1], k[2]) for k in BF.POOL_CASES} == {(1, 1), (2, 2), (3, 3), (4, 5), (5, 4), (7, 9), (8, 8)}
    assert {k[3] for k in BF.POOL_CASES} == {4, 64, 68} and {k[0] for k in BF.POOL_CASES} == {1, 2} and BF.POOL_PRODUCTION[1:4] == (240, 320, 64)
    assert {k[0] for k in BF.GATE_CASES} == {1, 255, 256, 257, 1000} and {k[1] for k in BF.GATE_CASES} == {4, 64, 68, 2048}
    assert {k[2:] for k in BF.GATE_CASES} >= {(r, d, False) for r in (True, False) for d in (True, False)} | {(True, True, True), (True, False, True)}


@pytest.mark.parametrize("key", [c for c in BF.DGRAD_CASES if c[4] <= 12 or c[2:4] == (5, 9)][::3], ids=str)
def test_the_dgrad_reference_is_conv2ds_autograd(key):
    c = BF.dgrad_inputs(key)
    assert (c["OH"], c["OW"]) == tuple(torch.nn.functional.conv2d(torch.zeros(1, 1, c["H"], c["W"]), torch.zeros(1, 1, c["k"], c["k"]), stride=2,
                                                                    padding=c["pad"]).shape[2:])
    ref, A = BF.dgrad_reference(key)
    auto = BF.dgrad_autograd(c["dy"].double(), c["w"].double(), c["H"], c["W"])
    assert float((ref - auto).abs().max()) <= 1e-13 * max(float(ref.abs().max()), 1.0)
    assert bool((A > 0).all()) or bool((ref[A == 0] == 0).all())
    # the emulation of the kernel's decomposition stands within the limit and writes every element
    got = BF.emulate_dgrad(key)
    assert not bool(torch.isnan(got).any()) and BF.dgrad_worst(key, got)[0] <= BF.limit()


def test_the_committed_f32_figures_are_measured():
    got = BF.f32_worst()
    assert BF.F32_WORST["dgrad"] / 2 <= got <= BF.F32_WORST["dgrad"] * 2, got


def test_the_bound_sees_a_wrong_tap_and_a_missing_zero_fill():
    k3 = [c for c in BF.DGRAD_CASES if c[0] == 3 and c[2] >= 2]
    k1 = [c for c in BF.DGRAD_CASES if c[0] == 1 and c[2] * c[3] > 1]
    assert k3 and k1
    for key in k3[::5]:
        assert BF.dgrad_worst(key, BF.emulate_dgrad(key, "wrong_tap"))[0] > BF.limit(), key
    for key in k1[::5]:
        got = BF.emulate_dgrad(key, "missing_zero_fill")
        assert bool(torch.isnan(got).any()) and BF.dgrad_worst(key, got)[0] == float("inf"), key
        assert BF.dgrad_worst(key, torch.nan_to_num(got, nan=BF.FILL))[0] > BF.limit(), key


def test_the_pool_reference_follows_max_pool2ds_rule():
    """strict >, first maximum in row-major order, padding never wins: stated by hand on three small cases"""
    x = torch.zeros(1, 3, 3, 1)                               # one window, every tap ties: the first in-bounds tap takes it all
    dy = torch.tensor([2.0, 3.0, 5.0, 7.0]).view(1, 2, 2, 1)
    got = BF.pool_backward(x, dy)[0, :, :, 0]
    assert got.tolist() == [[2.0, 3.0, 0.0], [5.0, 7.0, 0.0], [0.0, 0.0, 0.0]]
    x = -torch.ones(1, 1, 1, 1)                               # all negative: the zero padding must not win
    assert BF.pool_backward(x, torch.ones(1, 1, 1, 1)).item() == 1.0
    for key in ((1, 4, 5, 4, "increasing"), (1, 4, 5, 4, "decreasing"), (2, 7, 9, 4, "ties")):
        c = BF.pool_inputs(key)
        got = BF.pool_backward(c["x"], c["dy_int"])
        assert float(got.sum()) == float(c["dy_int"].sum())
        if key[-1] == "ties":
            assert float((c["x"] == 0).float().mean()) > 0.35


def test_the_gate_inputs_hold_both_zeros():
    for key in BF.GATE_CASES[:8]:
        c = BF.gate_inputs(key)
        bits = c["y"].contiguous().view(torch.int32)
        if c["y"].numel() >= 64:
            assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any()) and bool((c["y"] < 0).any()) and bool((c["y"] > 0).any())
        dc, dz = BF.gate_reference(c)
        assert dc.shape == c["g"].shape == dz.shape


def test_the_backbone_restatement_and_its_committed_figures():
    assert set(BF.F32_NORM_ERR) == {(c, w) for c in BF.NET_CASES for w in BF.COTANGENTS}
    for (case, which), committed in BF.F32_NORM_ERR.items():
        got = BF.f32_norm_err(case, which)
        assert set(got) == set(committed) == {"stem"} | set(BF.MAPS)
        for fam, v in got.items():
            if BF.LIMIT_FACTOR * 2 * committed[fam] <= BF.NORM_FLOOR:
                # rounding only: the bound is the floor, and stays the floor at twice the committed figure; the last bits of a
                # 1e-6 figure follow the host's summation order, so what is held is that the floor still governs
                assert 0 < v and BF.LIMIT_FACTOR * v <= BF.NORM_FLOOR, (case, which, fam, v)
            else:
                assert committed[fam] / 2 <= v <= committed[fam] * 2, (case, which, fam, v)
    # the odd-sized case is rounding only in every family: it is held to the floor, where a wrong operand or a lost factor shows
    assert all(BF.norm_bound(BF.NET_CASES[1], w, BF.PREFIX + f) == BF.NORM_FLOOR for w in BF.COTANGENTS for f in ("stem",) + BF.MAPS)
    for case in BF.NET_CASES:
        m64, m32 = BF.backbone_reference(case, "all")[0], BF.backbone_reference(case, "all", BF.F32)[0]
        assert all(BF.norm_err(m32[k], m64[k]) <= BF.NORM_FLOOR for k in BF.MAPS)
    assert tuple(BF.backbone_reference(BF.NET_CASES[1], "res5")[0]["res3"].shape[1:3]) == (5, 9)
    assert tuple(BF.backbone_reference(BF.NET_CASES[1], "res5")[0]["res5"].shape[1:3]) == (2, 3)


def test_the_trainers_keys_groups_and_multiplier():
    from nopesac_amd import training as T
    from nopesac_amd.config import get_cfg
    from nopesac_amd.synth import state_dict_spec
    names = T.BackboneTrainer.parameter_names(state_dict_spec(50))
    assert len(names) == 53 and sorted(names) == sorted(BF.PREFIX + n + ".weight" for n in BF.conv_names())
    assert all(T.parameter_group(k) == "plain" for k in names)
    assert issubclass(T.BackboneTrainer, T.HeadTrainer) and not issubclass(T.BackboneTrainer, T.ChainedTrainer)
    assert (T.BackboneTrainer.KEY_PREFIX, T.BackboneTrainer.LR_MULTIPLIER) == ("backbone.", "BACKBONE_MULTIPLIER")
    for m in ("step", "clip_grad_norm", "step_from_cfg", "write_back", "lr_multiplier", "backward"):
        assert m not in T.BackboneTrainer.__dict__
    cfg = get_cfg()
    cfg.SOLVER.BACKBONE_MULTIPLIER = 0.25
    tr = T.BackboneTrainer.from_state_dict(BF.backbone_state_dict(), "cpu")
    assert tr.lr_multiplier(cfg) == 0.25 and len(tr.params) == 53 and len(tr.norms) == 53
    assert all(s.shape == b.shape == (tr.params[k + ".weight"].shape[0],) for k, (s, b) in tr.norms.items())
