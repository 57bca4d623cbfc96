"""CPU half of the stream sweep (tests/stream_forms.py): the dispatch mirrors return every form and the GPU case tables reach each of
them, on both sides of every threshold; the float64 references agree with torch.nn.functional / torch.optim where those exist; the
generated inputs keep every activation decision off its margin; the floors (plain f32 formulations against float64) are computed and
printed.  Runs without a GPU."""
import itertools

import pytest
import torch
from torch.nn import functional as F

from tests import stream_forms as S

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


# ---------------------------------------------------------------------------------------------------------------------------- tables
def test_every_pool_form_has_a_case_on_both_sides_of_each_remainder():
    reached = {S.pool_form(dt, C, mis is None) for dt, C, mis in S.POOL_CASES}
    assert reached == set(S.POOL_FORMS)
    by = lambda dt: [(C, mis) for d, C, mis in S.POOL_CASES if d == dt]
    assert any(C % 4 == 0 for C, _ in by(F32)) and any(C % 4 for C, _ in by(F32))
    assert any(C % 8 == 0 for C, _ in by(BF16)) and any(C % 8 and C % 4 == 0 for C, _ in by(BF16))
    for dt in (F32, BF16):                                          # the scalar build by alignment alone: x, and only the second operand
        assert {mis for C, mis in by(dt) if S.pool_form(dt, C, True) != S.pool_form(dt, C, False)} == {None, "x", "other"}
    dt, C, H, W = S.POOL_GRID_CASE
    assert S.pool_form(dt, C, True) == "f32x1" and S.GRID_LIMIT < 4 * H * W * C < 1.1 * S.GRID_LIMIT
    assert max(2 * S.POOL_B * 4 * H * W * C for _, C, _ in S.POOL_CASES for H, W in S.POOL_HW) < S.GRID_LIMIT
    assert {(1, 1), (1, 5), (5, 1), (7, 9)} <= set(S.POOL_HW) and {(3, 2, 1), (2, 2, 0), (3, 1, 1)} <= set(S.POOL_KSP)
    assert S.pool_out(7, 3, 2, 1) == 4 and S.pool_out(7, 2, 2, 0) == 3 and S.pool_out(1, 2, 2, 0) is None        # 7: a partial last window


def test_groupnorm_form_table():
    for C, G in S.GN_SPLIT_CG:
        assert S.groupnorm_form(C, G) == "split"
        assert S.groupnorm_form(C, G, workspace=False) != "split"
    forms = {cg: S.groupnorm_form(*cg) for cg in S.GN_GENERIC_CG}
    assert forms == {(12, 3): "generic(1)", (96, 6): "generic(1)", (48, 3): "generic(1)", (24, 6): "generic(2)"}
    assert any(C % 8 for C, _ in S.GN_GENERIC_CG) and any(C % 8 == 0 and 256 % (C // 8) for C, _ in S.GN_GENERIC_CG)
    C, G, HW, B = S.GN_MISALIGNED
    assert S.groupnorm_form(C, G) == "split" and S.groupnorm_form(C, G, aligned=False).startswith("generic(")
    for C, G in S.GN_REFUSED_CG:
        assert S.groupnorm_form(C, G) == S.REFUSED and 256 % (C // G)
    # every accepted generic tiling covers every group: gpb divides G, and a workgroup's channels divide its 256 threads
    seen = set()
    for C in range(1, 600):
        for G in (g for g in range(1, C + 1) if C % g == 0):
            f = S.groupnorm_form(C, G, workspace=False)
            if f != S.REFUSED:
                gpb = int(f[8:-1])
                assert 1 <= gpb <= 32 and G % gpb == 0 and 256 % ((C // G) * gpb) == 0, (C, G, f)
                assert gpb == max(k for k in range(1, max(256 // (C // G) // 16, 1) + 1) if G % k == 0 and 256 % ((C // G) * k) == 0)
                seen.add(gpb)
    assert {1, 2, 4, 8, 16} <= seen
    assert min(S.GN_HW) == 1 and any(hw < S.GN_SPLITS for hw in S.GN_HW) and any(hw % S.GN_SPLITS for hw in S.GN_HW if hw > S.GN_SPLITS)
    assert set(S.GN_RATIOS) == {0.0, 2.5, 30.0} and set(S.GN_B) == {1, 3}
    assert {S.groupnorm_form(c[0], c[1], c[4]).split("(")[0] for c in S.gn_cases()} == {"split", "generic"}


def test_sumsq_form_thresholds():
    assert S.sumsq_form(16384) == "one_wg" and S.sumsq_form(16385) == ("two_stage", 4096, 5)
    assert S.sumsq_form(1048576) == ("two_stage", 4096, 256) and S.sumsq_form(1048577) == ("two_stage", 8192, 129)
    forms = [S.sumsq_form(n) for n in S.CLIP_N]
    assert "one_wg" in forms and any(f != "one_wg" and f[2] == 256 for f in forms) and any(f != "one_wg" and f[1] == 8192 for f in forms)
    for n in (16385, 20000, 1048576, 1048577, 5000000):
        _, chunk, nb = S.sumsq_form(n)
        assert chunk % 4096 == 0 and nb <= 256 and (nb - 1) * chunk < n <= nb * chunk
    assert {1, 255, 257} <= set(S.CLIP_N) and {1, 255, 257, 1048577} <= set(S.STEP_N)                  # one workgroup of 256 with a tail
    assert {(n, w > 0, m > 0) for n, w, m in S.STEP_CONFIGS} == {("ADAMW", False, False), ("ADAMW", True, False), ("SGD", False, False),
                                                                  ("SGD", True, False), ("SGD", False, True), ("SGD", True, True)}


def test_softmax_layernorm_and_relayout_tables():
    assert {S.softmax_form(*c) for c in S.SM_CASES} == {"plain", "pad<f32>", "pad<bf16>"}
    assert {1, 63, 64, 65, 300, 1023, 1024} <= set(S.SM_D) and (300, 304, F32) in S.SM_CASES
    for D in (64, 65):                                              # the output row spans more 64-lane trips than the input row
        assert (D, 1024, F32) in S.SM_CASES and (D, 1024, BF16) in S.SM_CASES
    for D, rows in itertools.product(S.SM_D, S.SM_ROWS):
        x = S.sm_inputs(D, rows)
        assert bool(torch.isfinite(x.max(-1).values).all()) and (D == 1 or bool(torch.isinf(x[-1]).any()))
    assert set(S.LN_D) == {64, 256, 1024} and {1, 3, 5, 77} <= set(S.LN_ROWS) and any(r % 4 for r in S.LN_ROWS)
    assert set(S.LN_ADDEND_ROWS) == {None, 1, 11} and any(r > 11 for r in S.LN_ROWS) and all(D % 64 or D > 1024 for D in S.LN_REFUSED_D)
    tiles32 = {(r % 32 == 0, c % 32 == 0) for r, c in S.TRANSPOSE_SHAPES}
    assert (True, True) in tiles32 and (False, False) in tiles32 and any(c > 64 for _, c in S.TRANSPOSE_SHAPES) and (1, 1) in S.TRANSPOSE_SHAPES
    assert any(ld > c for _, c, ld in S.col_sum_cases()) and any(ld == c for _, c, ld in S.col_sum_cases())
    assert {n % 16 == 0 for n in S.U8_N} == {True, False} and min(S.U8_N) < 16 < max(S.U8_N)
    assert max(S.NONFINITE_N) > S.NONFINITE_SINGLE_LIMIT > S.NONFINITE_BATCH_LIMIT and all(r % b for r, _, b in S.ADD_ROWS_BF16_CASES)
    for n in S.NONFINITE_N:
        x, bad = S.nonfinite_input(n)
        assert bad >= 1 and (not torch.isfinite(x[0]) or float(x[0].abs()) in (torch.finfo(F32).max, 1e-45) or float(x[0].abs()) < S.F32_MIN_NORMAL)
        assert n == 1 or not torch.isfinite(x[-1]) or float(x[-1].abs()) == torch.finfo(F32).max or float(x[-1].abs()) < S.F32_MIN_NORMAL
        assert bad == int(torch.isnan(x).sum() + torch.isinf(x).sum())
    x, _ = S.nonfinite_input(max(S.NONFINITE_N))
    assert float(x.abs()[torch.isfinite(x)].max()) == torch.finfo(F32).max and bool(((x != 0) & (x.abs() < S.F32_MIN_NORMAL)).any())


# ---------------------------------------------------------------------------------------------------------------------------- references
def test_pool_references_agree_with_torch():
    nchw, nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1))
    for dtype, C, _ in S.POOL_CASES[:4]:
        for H, W in S.POOL_HW:
            x, addend = S.pool_inputs(dtype, C, H, W)
            for k, s, p in S.POOL_KSP:
                if S.pool_out(H, k, s, p) is None or S.pool_out(W, k, s, p) is None:
                    continue
                assert torch.equal(S.maxpool_ref(x, k, s, p), nhwc(F.max_pool2d(nchw(x.double()), k, s, p)))
            z = nhwc(F.interpolate(nchw(x.double()), scale_factor=2, mode="bilinear", align_corners=False))
            for act, add in S.bilinear_variants():
                y, Sm, zz = S.bilinear_ref(x, addend if add else None, act)
                want = (z.relu() if act == S.ACT_RELU else z) + (addend.double() if add else 0)
                assert float((y - want).abs().max()) <= 1e-15 and bool((Sm >= y.abs() - 1e-15).all())
                assert float(zz.abs().min()) > S.MARGIN                                       # no ReLU decision on its margin
            ref, _ = S.nearest_add_ref(x, addend)
            assert torch.equal(ref, nhwc(F.interpolate(nchw(x.double()), scale_factor=2, mode="nearest")) + addend.double())
            if dtype == F32:                                       # the f32 add the bit-exact comparison uses is the rounded f64 sum
                assert torch.equal((S.up2(x) + addend).double(), ref.float().double())


@pytest.mark.parametrize("case", [c for c in S.gn_cases() if c[2] in (5, 63)], ids=S.gn_case_id)
def test_groupnorm_reference_and_margins(case):
    C, G, HW, B, _ = case
    for dtype, ratio in itertools.product((F32, BF16), S.GN_RATIOS):
        x, gamma, beta = S.gn_inputs(C, G, HW, B, dtype, ratio)
        assert x.dtype == dtype
        y, Sm, z = S.groupnorm_ref(x, gamma, beta, G, S.ACT_RELU)
        want = F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), S.GN_EPS).permute(0, 2, 1).relu()
        assert float(((y - want).abs() / Sm).max()) <= 1e-13
        assert float(z.abs().min()) > S.MARGIN and bool((Sm >= z.abs() * (1 - 1e-12)).all())
        x4 = x.double().view(B, HW, G, C // G)
        got_ratio = x4.mean((1, 3)).abs() / x4.var((1, 3), unbiased=False).sqrt().clamp_min(1e-30)
        if HW * (C // G) >= 60:
            assert bool(((got_ratio - ratio).abs() <= 0.5 + 0.3 * ratio).all()), (ratio, got_ratio)


def test_layernorm_softmax_and_normalize_references_agree_with_torch():
    for D, rows in itertools.product(S.LN_D, S.LN_ROWS):
        c = S.ln_inputs(D, rows)
        y, Sm, y2, S2 = S.layernorm_ref(c["x"], c["res"], c["gamma"], c["beta"], c[11])
        want = F.layer_norm((c["x"] + c["res"].double()), (D,), c["gamma"].double(), c["beta"].double(), S.LN_EPS)
        assert float(((y - want).abs() / Sm).max()) <= 1e-13
        assert torch.equal(y2, y + c[11].double()[torch.arange(rows) % 11])
    for D in S.NORMALIZE_D:
        x, g = S.normalize_inputs(D)
        assert float(x[:, 0].abs().min()) > S.MARGIN
        for canon in (False, True):
            ref = S.normalize_rows_ref(x, canon)
            want = F.normalize(x.double(), dim=-1)
            want = torch.where((want[:, :1] < 0) & canon, -want, want)
            assert float((ref - want).abs().max()) <= 1e-15
            assert float((S.normalize_rows_f32(x, canon).double() - ref).abs().max()) <= 4 * S.EPS32       # the bit-exact yardstick is right
    z = torch.zeros(2, 4)
    assert torch.equal(S.normalize_rows_f32(z, True), z)


def test_optimiser_and_clip_references_agree_with_torch():
    n = 257
    grads = [S.grad_input(n, k + 1) for k in range(S.STEPS)]
    for name, wd, mom in S.STEP_CONFIGS:
        ref, Sm = S.optimiser_steps(S.grad_input(n), grads, name, wd, mom)
        want = S.torch_optimiser_steps(S.grad_input(n), grads, name, wd, mom, F64)
        assert float(((ref - want).abs() / Sm).max()) <= 1e-14, (name, wd, mom)
    g = S.grad_input(n)
    for max_norm in (0.5, 1e3):
        p = torch.nn.Parameter(torch.zeros(n, dtype=F64))
        p.grad = g.double().clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        _, nref, coef, scaled = S.clip_ref(g, max_norm)
        assert abs(float(norm - nref)) <= 1e-12 and float((p.grad - scaled).abs().max()) <= 1e-14 and (float(coef) < 1) == (max_norm < 1)


# ---------------------------------------------------------------------------------------------------------------------------- backward families
def test_backward_tables_sit_on_both_sides_of_every_threshold():
    splits = {S.bn_grid(r, 4)[1] for r in S.BN_ROWS}
    assert S.bn_grid(255, 4)[1] == S.bn_grid(256, 4)[1] == 1 and S.bn_grid(257, 4)[1] == 2 and {1, 2, 4} <= splits     # 256-row splits
    assert S.bn_grid(1, 64)[0] == 1 and S.bn_grid(1, 65)[0] == 2 and any(C < 64 for C in S.BN_C) and any(C % 64 and C > 64 for C in S.BN_C)
    assert {1, 255, 256, 257, 1000} <= set(S.BN_ROWS) and {4, 64, 65, 96} <= set(S.BN_C) and set(S.BN_ACTS) == {0, 1, 2}
    cpg = {C // G for C, G in S.GNB_CG}
    assert cpg == {1, 4, 8, 256} and all(256 % k == 0 for k in cpg)                                   # 256, 64, 32 and 1 pixel lanes
    assert {1, 5, 300} <= set(S.GNB_HW) and any(hw < 256 // max(cpg) + 1 for hw in S.GNB_HW) and set(S.GNB_B) == {1, 3}
    P = [h * w for h, w in S.CORR_HW]
    assert any(p < 64 for p in P) and 64 in P and any(p > 64 and p % 64 for p in P) and all(S.corr_pad(p) > p for p in P)   # C % 64
    assert {(2, 2), (5, 7), (6, 10)} <= set(S.MPB_HW) and any(H % 2 for H, _ in S.MPB_HW) and any(W % 2 for _, W in S.MPB_HW)
    assert {(1, 1, 1, 1), (2, 3, 5, 7)} <= set(S.UPB_SHAPES)
    assert len(S.dgrad_cases()) == 2 * 4 * 2 * 2 and {(3, 1), (1, 0)} == set(S.DGRAD_KP) and set(S.DGRAD_CIN) == {1, 5} and set(S.DGRAD_COUT) == {1, 7}


def test_wgrad_grid_reaches_every_tail():
    g = S.wgrad_grid(36, 132, 3, 154, 2)
    assert g["grid"] == (3, 2, 2) and g["chunk"] == 80 and g["empty_splits"] == 0 and g["split_tail"] and g["n_tail"] and g["m_tail"]
    assert S.wgrad_grid(4, 4, 1, 1, 4) == {"grid": (1, 1, 4), "chunk": 16, "empty_splits": 3, "n_tail": True, "m_tail": True,
                                           "stage_tail": True, "split_tail": False}
    assert S.wgrad_grid(128, 128, 1, 32, 2)["chunk"] == 16 and not S.wgrad_grid(128, 128, 1, 32, 2)["n_tail"]
    grids = [S.wgrad_grid(ch[0], ch[2], ks[0], P, sp) for ch, ks, P in S.wgrad_cases() for sp in S.wgrad_splits(P)]
    assert {g["grid"][0] for g in grids} >= {1, 3, 22} and {g["grid"][1] for g in grids} == {1, 2}            # one and several tiles each way
    assert any(g["empty_splits"] for g in grids) and any(g["split_tail"] for g in grids) and any(g["stage_tail"] for g in grids)
    assert any(g["grid"][2] == 1 for g in grids) and any(g["grid"][2] == 2 for g in grids) and any(g["grid"][2] == 157 for g in grids)
    assert {c[0] for c in S.WGRAD_CH} == {4, 36, 300} and (300, 304, 8) in S.WGRAD_CH and set(S.WGRAD_P) == {1, 17, 154}
    assert set(S.WGRAD_KS) == {(1, 1), (1, 2), (3, 1), (3, 2)} and all(set(S.wgrad_splits(P)) == {1, 2, P + 3} for P in S.WGRAD_P)


def test_backward_references_agree_with_autograd_and_margins_hold():
    for rows, C in ((257, 65), (1, 4)):
        ins = S.bn_inputs(rows, C)
        c, dy, gamma, beta, mean, var = (t.double() for t in ins)
        for act in S.BN_ACTS:
            r = S.bn_ref(*ins, act)
            assert float(r["z"].abs().min()) > S.MARGIN
            cr, gr, br = (t.clone().requires_grad_(True) for t in (c, gamma, beta))
            z = F.batch_norm(cr.view(rows, C, 1, 1), mean, var, gr, br, False, 0.0, S.BN_EPS).view(rows, C)
            y = z if act == S.ACT_NONE else (F.relu(z) if act == S.ACT_RELU else F.leaky_relu(z, 0.01))
            y.backward(dy)
            for k, want in (("y", y.detach()), ("dc", cr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
                assert float(((r[k] - want).abs() / r["S" + k].clamp_min(1e-300)).max()) <= 1e-12, (rows, C, act, k)
    for case in ((128, 32, 5, 3), (256, 1, 5, 1), (32, 32, 5, 1)):
        C, G, HW, B = case
        x, dy, gamma, beta = S.gnb_inputs(*case)
        for relu in (False, True):
            r = S.gnb_ref(x, dy, gamma, beta, G, relu)
            xr, gr, br = (t.double().clone().requires_grad_(True) for t in (x, gamma, beta))
            y = F.group_norm(xr.permute(0, 2, 1), G, gr, br, S.GN_EPS)
            (F.relu(y) if relu else y).backward(dy.double().permute(0, 2, 1))
            for k, want in (("dx", xr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
                assert float(((r[k] - want).abs() / r["S" + k].clamp_min(1e-300)).max()) <= 1e-11, (case, relu, k)
    for H, W in S.MPB_HW:
        assert bool(S.mpb_unique(S.mpb_inputs(H, W, False)[0]).all())                       # every max-pool window has a unique maximum
        assert not bool(S.mpb_unique(S.mpb_inputs(H, W, True)[0]).all())
    for h, w in S.CORR_HW:
        c = S.corr_inputs(h, w)
        x1, x2 = c["x1"].double().requires_grad_(True), c["x2"].double().requires_grad_(True)
        p, _ = S.corr_ref(x1, x2)
        p.backward(c["da"].double())
        r1, r2, S1, S2 = S.corr_bwd_ref(p.detach(), c["da"], c["x1"], c["x2"])
        assert float(((r1 - x1.grad).abs() / S1).max()) <= 1e-12 and float(((r2 - x2.grad).abs() / S2).max()) <= 1e-12
        assert abs(float(p.sum(-1).min()) - 1) <= 1e-12
    dy = S.randn(S.gen(1), 2, 6, 10, 7).float()
    want = F.avg_pool2d(dy.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4
    assert float((S.upb_f32(dy).double() - want).abs().max()) <= 1e-6
    x, w, dyw = S.dgrad_inputs(3, 1, (7, 9), 5, 7)
    dx, Sdx, dw, Sdw = S.conv_grad_ref(x, w, dyw[..., :7], 2, 1)
    want = F.conv_transpose2d(dyw[..., :7].double().permute(0, 3, 1, 2), w.double(), None, 2, 1, output_padding=0).permute(0, 2, 3, 1)
    xr, wr = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, 2, 1).backward(dyw[..., :7].double().permute(0, 3, 1, 2))
    assert float((dx - xr.grad.permute(0, 2, 3, 1)).abs().max()) <= 1e-13 and float((dw - wr.grad).abs().max()) <= 1e-12
    assert float((dx - want).abs().max()) <= 1e-13 and bool((Sdx >= dx.abs() - 1e-13).all()) and bool((Sdw >= dw.abs() - 1e-13).all())


# ---------------------------------------------------------------------------------------------------------------------------- floors
def test_floors_are_computed_and_printed(capsys):
    floors = {"bilinear f32": S.floor_bilinear(), "layernorm": S.floor_layernorm(), "softmax_rows": S.floor_softmax(),
              "normalize_rows backward": S.floor_normalize_bwd(), "sumsq": S.floor_sumsq(), "col_sum": S.floor_col_sum(),
              "optimiser ADAMW": S.floor_optimiser("ADAMW"), "optimiser SGD": S.floor_optimiser("SGD")}
    floors.update({"groupnorm %s ratio %g" % k: v for k, v in S.floors_groupnorm().items()})
    floors.update({"clipped gradient": S.floor_clipped_gradient(), "corr_softmax forward": S.floors_corr()[0], "corr_softmax backward": S.floors_corr()[1],
                   "conv2d_dgrad stride 2": S.floors_conv_grad()[0], "conv2d_wgrad": S.floors_conv_grad()[1]})
    floors.update({"bn_act " + k: v for k, v in S.floors_bn().items()})
    floors.update({"groupnorm_backward " + k: v for k, v in S.floors_gnb().items()})
    with capsys.disabled():
        print("\nstream sweep: f32 floor and bound (%g x floor) per family" % S.FLOOR_FACTOR)
        for k in sorted(floors):
            print("  %-32s %.3g  %.3g" % (k, floors[k], S.FLOOR_FACTOR * floors[k]))
    # a floor is f32 rounding noise: at least half an ulp, and (the split GroupNorm's cancellation at |mean| = 30 std aside) a few ulps
    assert all(v >= S.EPS32 for v in floors.values())
    assert all(v <= 64 * S.EPS32 for k, v in floors.items() if not k.startswith("groupnorm split") and k not in ("softmax_rows", "corr_softmax forward"))
    assert floors["softmax_rows"] <= 128 * 30 * S.EPS32               # |x - max| up to ~ 30 x 8: its rounding scales the exponential
    assert floors["groupnorm split ratio 0"] <= 64 * S.EPS32 and floors["groupnorm split ratio 30"] <= 900 * 16 * S.EPS32
