"""Every kernel of csrc/plane_criterion.hip against the float64 restatement, element by element (tests/plane_criterion_forms.py has the
cases, the references and the allowances; tests/test_plane_criterion_forms_cpu.py proves them).  The raw entries are called through
ops.PlaneCriterionCall on buffers of the test's own: every output NaN-prefilled (0x7f bytes for the integer ones) with a guard tail, the
workspace exactly nopesac_plane_criterion_workspace_floats long plus the tail and NaN-filled before the cost entry and before the loss
entry.  The match handed to the loss entries is the test's, not the optimum; nopesac_plane_assign is tested on hand-made costs."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import plane_criterion_forms as P
from tests import plane_criterion_ref as R

pytestmark = pytest.mark.gpu

WORST = {}                                     # family -> (worst error / (limit x A), case): printed by the last test of the module
FILL = {torch.float32: float("nan"), torch.int32: 0x7F7F7F7F, torch.uint8: 0x7F}


def _guarded(numel, dtype, device):
    return torch.full((numel + P.GUARD,), FILL[dtype], dtype=dtype, device=device)


def _is_fill(t):
    return torch.isnan(t) if t.dtype == torch.float32 else t == FILL[t.dtype]


def _taken(st, numel, what):
    """The first numel elements of a guarded buffer, all written, on the host; the tail untouched."""
    st = st.cpu()
    assert bool(_is_fill(st[numel:]).all()), "%s: a write past the extent" % what
    assert not bool(_is_fill(st[:numel]).any()), "%s: an element left unwritten" % what
    return st[:numel].clone()


def _layout(t, kind, device):
    """[N, C, h, w] on the device in one of the three stride orders -> (view, storage); the gaps of the padded order are NaN"""
    t = t.to(device)
    if kind == "pm":
        st = t.contiguous()
        return st, st
    N, C, h, w = t.shape
    st = torch.full((N, h, w, C + (3 if kind == "pad" else 0)), float("nan"), device=device)
    st[..., :C] = t.permute(0, 2, 3, 1)
    return st[..., :C].permute(0, 3, 1, 2), st


def _strided_out(view, storage, device):
    """a NaN-filled buffer with the strides of `view` over a copy of its storage's extent, plus the guard tail"""
    st = _guarded(storage.numel(), torch.float32, device)
    return st.as_strided(view.shape, view.stride()), st


def _strided_taken(out, st, what):
    got = out.cpu()
    assert not bool(torch.isnan(got).any()), "%s: an element left unwritten" % what
    assert int((~torch.isnan(st)).sum()) == out.numel(), "%s: a write into a stride gap or past the extent" % what
    return got.contiguous()


def run(name, device, layout="pm", own_match=False):
    """costs -> (assign) -> losses -> one backward per cotangent vector, on guarded buffers -> every output on the host"""
    from nopesac_amd import ops
    case = P.CASES[name]
    x = P.inputs(name)
    L, B, nq, nmax, h, w = case.L, case.B, case.nq, case.nmax, case.h, case.w
    H, W, LB = case.s * h, case.s * w, L * B
    dev = lambda k: x[k].to(device).contiguous()
    ml, ml_st = _layout(x["mlog"], layout, device)
    px, px_st = _layout(x["pixc"], layout, device) if case.pixel else (None, None)
    preds = {"pred_logits": dev("logits"), "pred_mask_logits": ml, "pred_centers": dev("centers"), "pred_params": dev("params"), "pixel_centers": px}
    n_host = torch.tensor(case.n, dtype=torch.int32)
    targets = {"masks": dev("masks"), "n": n_host.to(device), "n_host": n_host, "plane_centers": dev("tcenters"), "plane_params": dev("tparams"),
               "pixel_centers": dev("tpixel"), "depth": dev("depth"), "k_inv_dot_xy1": dev("kinv")}
    call = ops.PlaneCriterionCall(L, preds, targets, P.WTS, case.num_masks)
    a = call.args
    sizes = {"cost": (LB * nq * nmax, torch.float32), "match_q": (LB * nmax, torch.int32), "match_gt": (LB * nq, torch.int32),
             "losses": (6 * L + 2, torch.float32), "mask_stats": (LB * nmax * 4, torch.float32), "q_valid": (B * H * W, torch.uint8),
             "q_stats": (B * 2, torch.float32), "ws": (int(a.ws_floats), torch.float32)}
    assert int(a.ws_floats) == int(ops._C.nopesac_plane_criterion_workspace_floats(L, B, nq, nmax, h, w)) > 0
    buf = {k: _guarded(numel, dtype, device) for k, (numel, dtype) in sizes.items()}
    for k, t in buf.items():
        setattr(a, k, t.data_ptr())
    take = lambda k: _taken(buf[k], sizes[k][0], k)
    out = {}
    buf["ws"].fill_(float("nan"))
    ops.plane_match_costs(call)
    out["cost"] = take("cost").view(LB, nq, nmax)
    if own_match:
        ops._C.nopesac_plane_assign(buf["cost"].data_ptr(), n_host.data_ptr(), targets["n"].data_ptr(), L, B, nq, nmax, buf["match_q"].data_ptr(),
                                    buf["match_gt"].data_ptr(), ops._stream())
    else:
        buf["match_q"][:LB * nmax] = x["match_q"].flatten().to(device)
        buf["match_gt"][:LB * nq] = x["match_gt"].flatten().to(device)
    out["match_q"], out["match_gt"] = take("match_q").view(LB, nmax), take("match_gt").view(LB, nq)
    buf["ws"].fill_(float("nan"))
    ops.plane_losses(call)
    out.update(losses=take("losses"), mask_stats=take("mask_stats").view(LB, nmax, 4), q_valid=take("q_valid").view(B, H, W),
               q_stats=take("q_stats").view(B, 2))
    out["grads"] = []
    for g in x["gs"]:                                                            # the workspace is NOT refilled: its content must survive
        gd = g.to(device)
        small = {"d_logits": _guarded(LB * nq * 2, torch.float32, device), "d_centers": _guarded(LB * nq * 2, torch.float32, device),
                 "d_params": _guarded(LB * nq * 3, torch.float32, device)}
        dml, dml_st = _strided_out(ml, ml_st, device)
        dpx, dpx_st = _strided_out(px, px_st, device) if case.pixel else (None, None)
        a.g_losses, a.d_mask_logits, a.d_pixel_centers = gd.data_ptr(), dml.data_ptr(), (dpx.data_ptr() if case.pixel else None)
        for k, t in small.items():
            setattr(a, k, t.data_ptr())
        ops._C.nopesac_plane_losses_backward(ctypes.byref(a), ops._stream())
        gr = {"d_logits": _taken(small["d_logits"], LB * nq * 2, "d_logits").view(LB, nq, 2),
              "d_centers": _taken(small["d_centers"], LB * nq * 2, "d_centers").view(LB, nq, 2),
              "d_params": _taken(small["d_params"], LB * nq * 3, "d_params").view(LB, nq, 3),
              "d_mask_logits": _strided_taken(dml, dml_st, "d_mask_logits"),
              "d_pixel_centers": _strided_taken(dpx, dpx_st, "d_pixel_centers") if case.pixel else torch.zeros(B, 2, h, w)}
        out["grads"].append(gr)
    assert bool(torch.isnan(buf["ws"][sizes["ws"][0]:]).all()), "a write past the workspace"
    return out


def same_bits(a, b):
    eq = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32)) if u.dtype == torch.float32 else torch.equal(u, v)
    for k in ("cost", "losses", "mask_stats", "q_valid", "q_stats", "match_q", "match_gt"):
        assert eq(a[k], b[k]), k
    for ga, gb in zip(a["grads"], b["grads"]):
        for k in ga:
            assert eq(ga[k], gb[k]), k


def judge(name, got, ref, A, label=None):
    """every element of every float output within limit x A; the integer-valued ones exact; unmatched queries exactly 0"""
    case, name = P.CASES[name], label or name
    assert torch.equal(got["q_valid"], ref["q_valid"]), name
    assert torch.equal(got["mask_stats"][..., 3].double(), ref["mask_stats"][..., 3]) and torch.equal(got["q_stats"][:, 1].double(), ref["q_stats"][:, 1])
    free = got["match_gt"] < 0
    for gr in got["grads"]:
        for k in ("d_mask_logits", "d_centers", "d_params"):
            assert not bool((gr[k][free] != 0).any()), (name, k)
    x = P.inputs(case.name)
    for gr, rr in zip(got["grads"], ref["grads"]):                              # the promised subgradient 0 at distance exactly 0
        for i, q, b, j in x["tied"]["centers"]:
            if int(got["match_gt"][i, q]) == j:
                assert not bool(rr["d_centers"][i, q].any()) and not bool(gr["d_centers"][i, q].any()), (name, i, q)
    bad = []
    for fam, q in P.worst(got, ref, A, case).items():
        rel = q / P.limit(fam)
        print("plane-forms %-18s %-16s error / (limit x A) = %.3g" % (name, fam, rel))
        if rel > WORST.get(fam, (0.0, ""))[0]:
            WORST[fam] = (rel, name)
        if not rel <= 1.0:
            bad.append((fam, rel))
    assert not bad, (name, bad)


def sweep(name, device):
    ref, A = P.reference(name)
    got = run(name, device)
    judge(name, got, ref, A)
    same_bits(got, run(name, device))                                           # two launches give the same bits
    for layout in ("nhwc",) + (("pad",) if name in P.PADDED else ()):           # and so do the three stride orders
        same_bits(got, run(name, device, layout))


@pytest.mark.parametrize("name", [c.name for c in P.COST_CASES + P.Q_CASES])
def test_cost_and_q_cases(device, name):
    sweep(name, device)


@pytest.mark.parametrize("h", P.MASK_HS)
@pytest.mark.parametrize("s", P.MASK_SS)
def test_mask_sweep(device, h, s):
    for w in P.MASK_WS:
        sweep("mask_%dx%d_s%d" % (h, w, s), device)


def test_mask_seam_at_the_model_width(device):
    sweep("mask_9x160_s4", device)


@pytest.mark.parametrize("name", P.CHAIN)
def test_chain_on_the_kernels_own_match(device, name):
    """costs -> assign -> losses -> backward as training runs them; the reference takes the kernel's match"""
    case = P.CASES[name]
    got = run(name, device, own_match=True)
    mq, mg = got["match_q"], got["match_gt"]
    for i in range(case.L * case.B):
        n = case.n[i % case.B]
        C = got["cost"][i, :, :n].numpy()
        mine = P.check_match(mq[i].numpy(), mg[i].numpy(), C)
        q, j = P.scipy_assign(C)
        best = float(C.astype(np.float64)[q, j].sum())
        assert abs(mine - best) <= 1e-9 * max(abs(best), 1.0), (name, i, mine, best)
        eq, eg, failed = P.assign_emulate(C)
        assert not failed and np.array_equal(eq, mq[i, :n].numpy()) and np.array_equal(eg, mg[i].numpy()), (name, i)
    x = dict(P.inputs(name), match_q=mq, match_gt=mg)
    ref, A = P.build_reference(x, case)
    judge(name, got, ref, A, label=name + "+own")


@pytest.mark.parametrize("name", list(P.TARGET_CASES))
def test_targets(device, name):
    got_c, got_p, masks, n = _targets(name, device, False)
    exact = P.exact_centroids(masks, n)
    for b in range(masks.shape[0]):
        for j in range(masks.shape[1]):
            for c in range(2):
                v = Fraction(float(got_c[b, j, c]))
                if exact[b][j] is None:
                    assert v == 0
                else:                                                            # float32(float64 quotient): half an ulp and the double rounding
                    assert abs(v - exact[b][j][c]) <= Fraction(2) ** -24 * exact[b][j][c] * (1 + Fraction(1, 10 ** 6)), (name, b, j, c)
    assert torch.equal(got_p.view(torch.int32), P.centre_map_f32(masks, n, got_c).view(torch.int32))


def _targets(name, device, empty):
    from nopesac_amd import ops
    masks, n = P.target_inputs(name, empty)
    B, nmax, H, W = masks.shape
    n_host = torch.tensor(n, dtype=torch.int32)
    md, nd = masks.to(device), n_host.to(device)
    c, p = _guarded(B * nmax * 2, torch.float32, device), _guarded(B * 2 * H * W, torch.float32, device)
    ops._C.nopesac_plane_targets(md.data_ptr(), n_host.data_ptr(), nd.data_ptr(), B, nmax, H, W, c.data_ptr(), p.data_ptr(), ops._stream())
    pc = p.cpu()
    assert bool(torch.isnan(pc[B * 2 * H * W:]).all()) and not bool(torch.isnan(pc[:B * 2 * H * W]).any())
    cc = c.cpu()
    assert bool(torch.isnan(cc[B * nmax * 2:]).all())
    return cc[:B * nmax * 2].view(B, nmax, 2).clone(), pc[:B * 2 * H * W].view(B, 2, H, W).clone(), masks, n


def test_targets_empty_mask_gives_nan(device):
    """the documented 0 / 0 of an empty mask, in a launch of its own: NaN in exactly that centre, the centre map unharmed"""
    got_c, got_p, masks, n = _targets("3x5", device, True)
    want = torch.zeros_like(got_c, dtype=torch.bool)
    want[0, 1] = True
    assert torch.equal(torch.isnan(got_c), want)
    assert torch.equal(got_p.view(torch.int32), P.centre_map_f32(masks, n, torch.nan_to_num(got_c, nan=123.0)).view(torch.int32))


def _assign(cost, n, nq, nmax, device):
    from nopesac_amd import ops
    B = cost.shape[0]
    n_host = torch.tensor(n, dtype=torch.int32)
    cd, nd = cost.to(device).contiguous(), n_host.to(device)
    mq, mg = _guarded(B * nmax, torch.int32, device), _guarded(B * nq, torch.int32, device)
    ops._C.nopesac_plane_assign(cd.data_ptr(), n_host.data_ptr(), nd.data_ptr(), 1, B, nq, nmax, mq.data_ptr(), mg.data_ptr(), ops._stream())
    return _taken(mq, B * nmax, "match_q").view(B, nmax).numpy(), _taken(mg, B * nq, "match_gt").view(B, nq).numpy()


@pytest.mark.parametrize("name", list(P.assign_launches()))
def test_assign(device, name):
    nq, nmax, images = P.assign_launches()[name]
    cost, n = P.pack_costs(nq, nmax, images)
    mq, mg = _assign(cost, n, nq, nmax, device)
    for b, (kind, C) in enumerate(images):
        C = C.numpy()
        total = P.check_match(mq[b], mg[b], C)
        q, j = P.scipy_assign(C)
        assert total == float(C.astype(np.float64)[q, j].sum()) or kind == "continuous", (name, b, kind)
        if kind == "continuous":                                                 # a unique optimum (the CPU half shows it): scipy's match
            want = -np.ones(nmax, dtype=np.int64)
            want[j] = q
            assert np.array_equal(mq[b], want), (name, b)
        eq, eg, failed = P.assign_emulate(C)
        assert not failed and np.array_equal(eq, mq[b, :C.shape[1]]) and np.array_equal(eg, mg[b]), (name, b, kind)


def test_assign_refuses_non_finite_costs_and_returns(device):
    """Every loop of pc_assign_kernel has a fixed bound (nr rows, nq + 1 scan steps, nr + 1 path steps) and the refusal is decided on a
    wave-uniform value, so these inputs can only end; the numpy emulation shows the same on the CPU before the GPU sees them."""
    nq, nmax, images = P.refusal_launch()
    for (kind, fail), C in images:
        assert P.assign_emulate(C.numpy())[2] == (fail is not None)
    cost, n = P.pack_costs(nq, nmax, images)
    mq, mg = _assign(cost, n, nq, nmax, device)
    for b, ((kind, fail), C) in enumerate(images):
        C = C.numpy()
        total = P.check_match(mq[b], mg[b], np.nan_to_num(C, nan=0.0, posinf=1e30), upto=fail)
        if fail is None:
            q, j = P.scipy_assign(np.where(np.isinf(C), 1e30, C))
            assert abs(total - float(np.where(np.isinf(C), 1e30, C).astype(np.float64)[q, j].sum())) < 1e-9, (kind, total)
            assert total < 1e20                                                  # the optimum avoids the column of +inf
        eq, eg, _ = P.assign_emulate(C)
        assert np.array_equal(eq, mq[b, :C.shape[1]]) and np.array_equal(eg, mg[b]), kind
    sound = [k for k, ((_, fail), _) in enumerate(images) if fail is None]
    cost2, n2 = P.pack_costs(nq, nmax, [images[k] for k in sound])
    mq2, mg2 = _assign(cost2, n2, nq, nmax, device)
    assert np.array_equal(mq2, mq[sound]) and np.array_equal(mg2, mg[sound])     # the other images: as in a launch without the refused ones


@pytest.mark.parametrize("name", list(P.corr_cases()))
def test_corr_matrix(device, name):
    from nopesac_amd import ops
    nq, nmax = P.corr_cases()[name][:2]
    corrs, pad, m1, m2, idx1, idx2 = P.corr_inputs(name)
    want = R.plane_corr_matrix(corrs, idx1, idx2, nq)
    B, K, S = pad.shape[0], pad.shape[1], nq + 1
    out = _guarded(B * S * S, torch.uint8, device)
    keep = [pad.to(device), m1.to(device), m2.to(device)]
    ops._C.nopesac_plane_corr_matrix(keep[0].data_ptr(), K, keep[1].data_ptr(), keep[2].data_ptr(), B, nq, nmax, out.data_ptr(), ops._stream())
    got = _taken(out, B * S * S, "corr").view(B, S, S)
    assert torch.equal(got, want.to(torch.uint8)), name
    assert torch.equal(ops.plane_corr_matrix(*keep, nq).cpu(), got)


def test_zz_report():
    """the worst error / (limit x A) per family over the module (docs/kernels.md quotes it)"""
    for fam in sorted(WORST):
        print("plane-forms WORST %-16s %.3g  (%s)" % (fam, WORST[fam][0], WORST[fam][1]))
