"""GPU half of the view-group sweeps (tests/train_step_forms.py).  One pass over G groups of images must give every group the BITS an
ungrouped call on that group's images alone gives - losses, kept statistics and all gradients of the criterion (csrc/plane_criterion.hip),
statistics, running buffers, output and gradients of the pyramid's BatchNorm (csrc/pyramid_train.hip) - and the ungrouped calls are
existing code, held to float64 by tests/test_plane_criterion_forms_gpu.py and tests/test_plane_pyramid_forms_gpu.py.  Then the two
trainers: PlaneCriterion(groups=G) returns the mean over groups, PlanePyramidTrainer.forward(groups=2) is the two per-view forwards."""
import functools

import pytest
import torch

from tests import plane_criterion_forms as P
from tests import plane_pyramid_forms as Y
from tests import train_step_forms as T

pytestmark = pytest.mark.gpu
TAIL = 64
NAN = float("nan")


def _bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _guarded(device, *shape):
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + TAIL,), NAN, device=device, dtype=torch.float32)
    return buf, buf[:n].view(*shape)


def _written(buf, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-TAIL:]).all()), "%s: a write past the extent" % what
    assert not bool(torch.isnan(buf[:-TAIL]).any()), "%s: an element left unwritten" % what


# ===================================================================================================================== the criterion
def _criterion_run(x, case, device, layout, pixel, num_masks, groups, cots):
    """loss entry and one backward per cotangent through ops.PlaneCriterionCall with the test's own match -> every output"""
    from nopesac_amd import ops
    L, B = case.L, case.B
    dev = lambda k: x[k].to(device).contiguous()
    ml = dev("mlog") if layout == "pm" else dev("mlog").permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # the head's [i, h, w, q] order
    px = None if not pixel else (dev("pixc") if layout == "pm" else dev("pixc").permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    preds = {"pred_logits": dev("logits"), "pred_mask_logits": ml, "pred_centers": dev("centers"), "pred_params": dev("params"), "pixel_centers": px}
    n_host = torch.tensor(case.n, dtype=torch.int32)
    targets = {"masks": dev("masks"), "n": n_host.to(device), "n_host": n_host, "plane_centers": dev("tcenters"), "plane_params": dev("tparams"),
               "pixel_centers": dev("tpixel"), "depth": dev("depth"), "k_inv_dot_xy1": dev("kinv")}
    call = ops.PlaneCriterionCall(L, preds, targets, P.WTS, num_masks, **({} if groups is None else {"groups": groups}))
    G = groups or 1
    assert tuple(call.losses.shape) == ((6 * L + 2,) if G == 1 else (G, 6 * L + 2))
    call.match_q.copy_(x["match_q"].to(device))
    call.match_gt.copy_(x["match_gt"].to(device))
    buf, losses = _guarded(device, G, 6 * L + 2)
    call.args.losses = losses.data_ptr()
    ops.plane_losses(call)
    _written(buf, "losses")
    out = {"losses": losses.cpu(), "mask_stats": call.mask_stats.cpu(), "q_stats": call.q_stats.cpu(), "q_valid": call.q_valid.cpu(), "grads": []}
    for g in cots:
        got = ops.plane_losses_backward(call, g.to(device).contiguous())
        assert got[1].stride() == ml.stride() and (px is None or got[4].stride() == px.stride())
        out["grads"].append([None if t is None else t.cpu().contiguous() for t in got])
    return out


@pytest.mark.parametrize("kind", T.NUM_MASKS)
@pytest.mark.parametrize("name", list(T.CRITERION_CASES))
def test_criterion_group_has_the_bits_of_a_call_on_its_images(device, name, kind):
    case, G = T.CRITERION_CASES[name]
    x = T.criterion_inputs(name)
    grouped_nm, per_group = T.num_masks_of(kind, G)
    cots = [T.group_cotangents(x, G, launch) for launch in range(2)]
    for layout in ("pm", "nhwc"):
        for pixel in (True, False):
            got = _criterion_run(x, case, device, layout, pixel, grouped_nm, G, cots)
            for grp in range(G):
                sub, sub_case = T.group_slice(x, case, G, grp)
                bs, rows = T.group_images(case, G, grp)
                ref = _criterion_run(sub, sub_case, device, layout, pixel, per_group[grp], None, [c[grp] for c in cots])
                what = (name, kind, layout, pixel, grp)
                assert _bits(got["losses"][grp], ref["losses"][0]), what
                assert _bits(got["mask_stats"][rows], ref["mask_stats"]) and _bits(got["q_stats"][bs], ref["q_stats"]), what
                assert torch.equal(got["q_valid"][bs], ref["q_valid"]), what
                empty = all(b in case.no_valid for b in bs)
                assert (float(ref["losses"][0, 6 * case.L + 1]) == 0.0) == empty, what        # the group without a valid pixel, and only it
                for launch in range(2):
                    d_lg, d_ml, d_ce, d_pa, d_px = got["grads"][launch]
                    r_lg, r_ml, r_ce, r_pa, r_px = ref["grads"][launch]
                    assert _bits(d_lg[rows], r_lg) and _bits(d_ml[rows], r_ml) and _bits(d_ce[rows], r_ce) and _bits(d_pa[rows], r_pa), what + (launch,)
                    assert (d_px is None and r_px is None) if not pixel else _bits(d_px[bs], r_px), what + (launch,)
                    assert bool(torch.isfinite(d_ml).all()) and float(d_pa.abs().max()) > 0


def test_criterion_groups_1_is_the_call_without_the_argument(device):
    for name in ("g2_L1", "g3_L3"):
        case, _ = T.CRITERION_CASES[name]
        x = T.criterion_inputs(name)
        cots = [x["gs"][0], x["gs"][1]]
        for nm in (0.0, 2.5):
            a = _criterion_run(x, case, device, "nhwc", True, nm, None, cots)
            for groups, per in ((1, nm), (1, [nm])):
                b = _criterion_run(x, case, device, "nhwc", True, per, groups, cots)
                assert all(_bits(a[k], b[k]) for k in ("losses", "mask_stats", "q_stats", "q_valid"))
                assert all(_bits(u, v) for ga, gb in zip(a["grads"], b["grads"]) for u, v in zip(ga, gb))


def _criterion_dicts(name, device, images=None):
    """(outputs with leaves that require grad, targets) of PlaneCriterion for a case, or for the batch elements `images` of it"""
    case, _ = T.CRITERION_CASES[name]
    x = T.criterion_inputs(name)
    if images is not None:
        x, case = T.group_slice(x, case, case.B // len(images), images[0] // len(images))
    L, B = case.L, case.B
    leaf = lambda k: x[k].to(device).requires_grad_(True)
    lv = {k: leaf(k) for k in ("logits", "mlog", "centers", "params", "pixc")}
    layer = lambda l: {"pred_logits": lv["logits"][l * B:(l + 1) * B], "pred_mask_logits": lv["mlog"][l * B:(l + 1) * B],
                       "pred_centers": lv["centers"][l * B:(l + 1) * B], "pred_params": lv["params"][l * B:(l + 1) * B]}
    out = dict(layer(0), pixel_centers=lv["pixc"])
    if L > 1:
        out["aux_outputs"] = [layer(l) for l in range(1, L)]
    targets = {"masks": x["masks"].to(device), "n": list(case.n), "plane_params": x["tparams"].to(device), "depth": x["depth"].to(device),
               "k_inv_dot_xy1": x["kinv"].to(device)}
    return out, targets, lv, case


@pytest.mark.parametrize("name", ["g2_L3", "g3_L1"])
def test_plane_criterion_returns_the_mean_over_groups(device, name):
    """PlaneCriterion(groups=G): every loss is ((l_0 + l_1) + ...) / G of last["group_losses"], each of which has the bits of the
    criterion called on that group alone; groups=1 is the call without the argument; with two groups the gradient at every leaf is
    half the per-view gradient, exactly (a power of two)."""
    from nopesac_amd.training import PlaneCriterion
    crit = PlaneCriterion.from_cfg(_cfg())
    case, G = T.CRITERION_CASES[name]
    out, targets, lv, _ = _criterion_dicts(name, device)
    losses, idx = crit(out, targets, groups=G)
    per = crit.last["group_losses"]
    assert len(per) == G and all(set(p) == set(losses) for p in per) and len(losses) == 6 * case.L + 2
    Bg = case.B // G
    views = []
    for grp in range(G):
        o, t, leaves, _ = _criterion_dicts(name, device, list(range(grp * Bg, (grp + 1) * Bg)))
        l, i = crit(o, t)
        views.append((l, leaves))
        assert all(_bits(per[grp][k], l[k].detach()) for k in l), (name, grp)
        assert torch.equal(idx["match_q"][:, grp * Bg:(grp + 1) * Bg], i["match_q"])
    for k in losses:
        acc = per[0][k]
        for grp in range(1, G):
            acc = acc + per[grp][k]
        assert _bits(losses[k].detach(), acc / G), k
    w = crit.weighted(losses)
    assert set(w) == set(losses) and all(_bits(w[k].detach(), losses[k].detach() * crit.weight_dict[k]) for k in w)
    if G == 2:
        sum(w.values()).backward()
        for grp, (l, leaves) in enumerate(views):
            sum(crit.weighted(l).values()).backward()
            for k, t in leaves.items():
                rows = T.group_images(case, G, grp)[0 if k == "pixc" else 1]
                assert _bits(lv[k].grad[rows], 0.5 * t.grad), (name, grp, k)
    o1, t1, _, _ = _criterion_dicts(name, device)
    o2, t2, _, _ = _criterion_dicts(name, device)
    a, b = crit(o1, t1)[0], crit(o2, t2, groups=1)[0]
    assert all(_bits(a[k].detach(), b[k].detach()) for k in a)


def test_unequal_plane_counts_are_the_point(device):
    """n = (1, 1 | 8, 8): the ungrouped 2B value of loss_param_l1 is (2 m1 + 16 m2) / 18, the grouped one the reference's (m1 + m2) / 2"""
    from nopesac_amd.training import PlaneCriterion
    crit = PlaneCriterion.from_cfg(_cfg())
    name = "g2_L1"
    pooled = crit(*_criterion_dicts(name, device)[:2])[0]["loss_param_l1"].detach()
    grouped = crit(*_criterion_dicts(name, device)[:2], groups=2)[0]["loss_param_l1"].detach()
    m = [crit(*_criterion_dicts(name, device, bs)[:2])[0]["loss_param_l1"].detach() for bs in ([0, 1], [2, 3])]
    print("loss_param_l1: views %.6f %.6f, grouped %.6f, pooled over 2B %.6f" % (float(m[0]), float(m[1]), float(grouped), float(pooled)))
    assert _bits(grouped, (m[0] + m[1]) / 2)
    assert abs(float(pooled) - float(grouped)) > 1e-3 * float(grouped)
    assert abs(float(pooled) - (2 * float(m[0]) + 16 * float(m[1])) / 18) < 1e-5 * float(pooled)


def test_criterion_refusals(device):
    from nopesac_amd import ops
    from nopesac_amd.training import PlaneCriterion
    case, _ = T.CRITERION_CASES["g2_L1"]
    x = T.criterion_inputs("g2_L1")
    for groups, nm in ((3, 0.0), (8, 0.0), (0, 0.0), (2, [1.0]), (2, [1.0, 2.0, 3.0]), (1, [1.0, 2.0])):
        with pytest.raises(ops.OpsArgumentError):
            _criterion_run(x, case, device, "pm", True, nm, groups, [])
    crit = PlaneCriterion.from_cfg(_cfg())
    out, targets = _criterion_dicts("g2_L1", device)[:2]
    with pytest.raises(ops.OpsArgumentError):
        crit(out, targets, groups=3)
    with pytest.raises(ops.OpsArgumentError):
        crit(out, targets, num_masks=[1.0, 2.0, 3.0], groups=2)
    call_losses, _ = crit(out, targets, num_masks=[3.0, 5.0], groups=2)            # and the per-group override reaches the kernels
    default, _ = crit(out, targets, groups=2)
    assert not _bits(call_losses["loss_mask"].detach(), default["loss_mask"].detach())
    assert _bits(call_losses["loss_ce"].detach(), default["loss_ce"].detach())


@functools.lru_cache(maxsize=None)
def _cfg():
    from nopesac_amd.config import get_cfg
    return get_cfg()


# ===================================================================================================================== the pyramid's BatchNorm
def _lib():
    from nopesac_amd import _lib
    return _lib, _lib.load()


def _call(name, *args):
    lib, L = _lib()
    lib.check(getattr(L, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream), name)


def _bn_src(c, device):
    if c["tag"] == "slice":
        src = c["buf"].to(device)[..., 4:4 + c["C"]]
        assert src.stride(-2) == c["C"] + 8 and src.data_ptr() % 16 == 0
        return src
    return c["src"].contiguous().to(device)


def _dims(src, up):
    return tuple(src.shape[:3]) if src.dim() == 4 else (src.shape[0], 1, 1)


def _bn_round(device, src, up, G, C, relu, gamma, beta, g, addend, run, grouped_entries):
    """stats (running buffers updated in place) -> apply -> backward on guarded buffers through the raw entry points: the grouped
    entries with G, or the ungrouped ones (G = 1)"""
    from nopesac_amd import ops
    B, H, W = _dims(src, up)
    n = B * H * W * (4 if up else 1)
    out_shape = tuple(g.shape)
    sb, (mean, var, rstd) = zip(*[_guarded(device, G, C) for _ in range(3)])
    floats = ops.bn_train_groups_workspace_floats(G, n, C) if grouped_entries else ops.bn_train_workspace_floats(n, C)
    assert floats == G * -(-(n // G) // T.RPS) * 2 * C
    wsb, ws = _guarded(device, floats)
    yb, y = _guarded(device, *out_shape)
    db, dsrc = _guarded(device, *src.shape)
    gb, dg = _guarded(device, C)
    bb, dbeta = _guarded(device, C)
    cs = src.stride(-2)
    if grouped_entries:
        smb, sums = _guarded(device, G, 2, C)
        _call("nopesac_bn_train_groups_stats_f32", src, int(up), B, H, W, C, cs, G, T.EPS, T.MOMENTUM, mean, var, rstd, run[0], run[1], ws, ws.numel())
        _call("nopesac_bn_train_groups_apply_f32", src, int(up), B, H, W, C, cs, G, gamma, beta, mean, rstd, int(relu), addend, y)
        _call("nopesac_bn_train_groups_backward_f32", g, src, int(up), B, H, W, C, cs, G, gamma, beta, mean, rstd, int(relu), 1, dsrc, dg, dbeta,
              sums if G > 1 else None, ws, ws.numel())
        if G > 1:
            _written(smb, "group_sums")
        else:
            sums = torch.stack([dg, dbeta])[None]
    else:
        _call("nopesac_bn_train_stats_f32", src, int(up), B, H, W, C, cs, T.EPS, T.MOMENTUM, mean, var, rstd, run[0], run[1], ws, ws.numel())
        _call("nopesac_bn_train_apply_f32", src, int(up), B, H, W, C, cs, gamma, beta, mean, rstd, int(relu), addend, y)
        _call("nopesac_bn_train_backward_f32", g, src, int(up), B, H, W, C, cs, gamma, beta, mean, rstd, int(relu), 1, dsrc, dg, dbeta, ws, ws.numel())
        sums = torch.stack([dg, dbeta])[None]
    for b, what in zip(sb + (yb, db, gb, bb), ("mean", "var", "rstd", "y", "dsrc", "dgamma", "dbeta")):
        _written(b, what)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wsb[-TAIL:]).all()), "a write past the workspace"
    return {"mean": mean, "var": var, "rstd": rstd, "y": y, "dsrc": dsrc, "dgamma": dg, "dbeta": dbeta, "sums": sums}


@pytest.mark.parametrize("key", T.bn_cases(), ids=T.bn_id)
def test_bn_group_has_the_bits_of_a_call_on_its_rows(device, key):
    c = T.bn_inputs(key)
    G, C, up, relu = c["G"], c["C"], c["up"], c["relu"]
    src = _bn_src(c, device)
    gamma, beta, g = (c[k].to(device) for k in ("gamma", "beta", "g"))
    addend = None if c["addend"] is None else c["addend"].to(device)
    run = [c["run_mean"].to(device), c["run_var"].to(device)]
    got = _bn_round(device, src, up, G, C, relu, gamma, beta, g, addend, run, True)
    per = src.shape[0] // G
    run1 = [c["run_mean"].to(device), c["run_var"].to(device)]
    dg = db = None
    for grp in range(G):
        sl = slice(grp * per, (grp + 1) * per)
        ref = _bn_round(device, src[sl], up, 1, C, relu, gamma, beta, g[sl].contiguous(), None if addend is None else addend[sl].contiguous(), run1, False)
        for k in ("mean", "var", "rstd"):
            assert _bits(got[k][grp], ref[k][0]), (key, grp, k)
        assert _bits(got["y"][sl], ref["y"]) and _bits(got["dsrc"][sl], ref["dsrc"]), (key, grp)
        assert _bits(got["sums"][grp], ref["sums"][0]), (key, grp)                             # S2_g = sum dz xhat, S1_g = sum dz
        dg, db = (ref["dgamma"].clone(), ref["dbeta"].clone()) if grp == 0 else (dg + ref["dgamma"], db + ref["dbeta"])
    assert _bits(run[0], run1[0]) and _bits(run[1], run1[1]), key                              # G consecutive calls in group order
    assert not _bits(run[0], c["run_mean"].to(device))
    assert _bits(got["dgamma"], dg) and _bits(got["dbeta"], db), key
    assert not _bits(got["mean"][0], got["mean"][1])
    again = _bn_round(device, src, up, G, C, relu, gamma, beta, g, addend, [c["run_mean"].to(device), c["run_var"].to(device)], True)
    assert all(_bits(got[k], again[k]) for k in got), "two launches differ"


@pytest.mark.parametrize("key", [k for k in T.bn_cases() if k[1] == 2 and (k[2] in (None, 257)) and k[3] != 4], ids=T.bn_id)
def test_bn_groups_1_is_the_ungrouped_entry_and_the_wrappers_follow(device, key):
    from nopesac_amd import ops
    c = T.bn_inputs(key)
    G, C, up, relu = c["G"], c["C"], c["up"], c["relu"]
    src = _bn_src(c, device)
    gamma, beta, g = (c[k].to(device) for k in ("gamma", "beta", "g"))
    addend = None if c["addend"] is None else c["addend"].to(device)
    fresh = lambda: [c["run_mean"].to(device), c["run_var"].to(device)]
    r0, r1 = fresh(), fresh()
    a = _bn_round(device, src, up, 1, C, relu, gamma, beta, g, addend, r0, False)
    b = _bn_round(device, src, up, 1, C, relu, gamma, beta, g, addend, r1, True)
    assert all(_bits(a[k], b[k]) for k in a) and _bits(r0[0], r1[0]) and _bits(r0[1], r1[1])
    # the wrappers: groups=G is the raw grouped entries, groups=1 the ungrouped ones
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    for groups, want, entries in ((G, None, True), (1, a, False)):
        rw, rr = fresh(), fresh()
        want = want or _bn_round(device, src, up, groups, C, relu, gamma, beta, g, addend, rr, True)
        mean, var, rstd = ops.bn_train_stats(src, up=up, eps=T.EPS, momentum=T.MOMENTUM, running_mean=rw[0], running_var=rw[1], groups=groups)
        assert tuple(mean.shape) == ((C,) if groups == 1 else (groups, C))
        y = ops.bn_train_apply(src, gamma, beta, mean, rstd, act, addend, up=up, groups=groups)
        dsrc, dgm, dbt, sums = ops.bn_train_backward(g, src, gamma, beta, mean, rstd, act, up=up, groups=groups, group_sums=True)
        for t, k in ((mean, "mean"), (var, "var"), (rstd, "rstd"), (y, "y"), (dsrc, "dsrc"), (dgm, "dgamma"), (dbt, "dbeta"), (sums, "sums")):
            assert _bits(t.reshape(want[k].shape), want[k]), (key, groups, k)
    for bad in (3, 0, 9, True):
        if src.shape[0] % 3 == 0 and bad == 3:
            continue
        with pytest.raises(ops.OpsArgumentError):
            ops.bn_train_stats(src, up=up, groups=bad)


# ===================================================================================================================== the pyramid trainer
PYR_KEY = (4, 3, 4)        # 2 pairs = 2 x 2 images, res5 at 3 x 4 and p1 at 24 x 32: the smallest maps on which all four levels differ in
                           # size, no level is a single pixel and a group's res5 BatchNorm has 24 rows; its float64 pyramid takes 2 s on the CPU


@functools.lru_cache(maxsize=None)
def _pyramid_case():
    """pyramid_inputs for 4 images, its BatchNorm biases settled for BOTH views' statistics (the gates of a view's forward must not sit
    within rounding of 0 for that view's z), and the two per-view cases"""
    c = Y.pyramid_inputs(PYR_KEY)
    B, h, w = PYR_KEY
    Bg = B // 2

    def view(v):
        sl = slice(v * Bg, (v + 1) * Bg)
        return dict(c, key=(Bg, h, w), B=Bg, feats={k: t[sl].contiguous() for k, t in c["feats"].items()},
                    memory=c["memory"][v * Bg * h * w:(v + 1) * Bg * h * w].contiguous(), d_p1=c["d_p1"][sl].contiguous())
    sd = {k: v.clone() for k, v in c["sd"].items()}
    for _ in range(16):
        before = {k: v.clone() for k, v in sd.items()}
        for v in range(2):
            cv = view(v)
            Y.settle_biases(sd, cv["bufs"], cv["feats"], cv["memory"], Bg)
        if all(torch.equal(before[k], sd[k]) for k in sd):
            break
    else:
        raise AssertionError("the ReLU margins of the two views did not settle together")
    c = dict(c, sd=sd)
    return c, [dict(view(v), sd=sd) for v in range(2)]


def _pyramid_trainer(c, device):
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import PlanePyramidTrainer
    full = synth_state_dict(7)
    sd = dict({k: v for k, v in full.items() if k.startswith(Y.PREFIX)}, **c["sd"], **c["bufs"])
    return PlanePyramidTrainer.from_state_dict(sd, device, feature_grads=True)


def _pyramid_pass(tr, c, device, **kw):
    p1 = tr.forward({k: v.to(device) for k, v in c["feats"].items()}, c["memory"].to(device), c["B"], **kw)
    grads = tr.backward_from(c["d_p1"].to(device))
    return p1.detach(), {k: v.clone() for k, v in grads.items()}, {k: v.clone() for k, v in tr.input_grads.items()}


def test_pyramid_trainer_groups_are_the_two_views(device):
    """forward(groups=2) on 2 x 2 images: p1, the running statistics and the gradients at memory and res2 .. res5 have the bits of the two
    per-view forwards (same trainer: its buffers take view 1, then view 2); the counters advance by 2; the 16 BatchNorm affine gradients
    are the views' sum in view order.  The 8 conv weights' gradients are NOT bit-equal: one wgrad call over 2B images walks its K
    dimension (the pixels) in another order than two calls over B images whose results are added.  They are held to the float64
    pyramid instead - the sum of the two views' float64 gradients under tests/plane_pyramid_forms.py's allowance, each view's A
    unchanged and added."""
    c, views = _pyramid_case()
    one = _pyramid_trainer(c, device)
    p1, grads, ins = _pyramid_pass(one, c, device, groups=2)
    two = _pyramid_trainer(c, device)
    per = [_pyramid_pass(two, cv, device) for cv in views]
    Bg, h, w = views[0]["B"], c["h"], c["w"]
    assert _bits(p1, torch.cat([per[0][0], per[1][0]]))
    for k in one.buffers:
        if k.endswith("num_batches_tracked"):
            assert int(one.buffers[k]) == int(two.buffers[k]) == 2
        else:
            assert _bits(one.buffers[k], two.buffers[k]), k
    assert set(ins) == {"memory", "res2", "res3", "res4", "res5"}
    for k in ins:
        assert _bits(ins[k], torch.cat([per[0][2][k], per[1][2][k]])), k
    conv = [k for k in grads if k.endswith(".0.weight")]
    assert len(conv) == 8 and len(grads) == 24
    for k in grads:
        if k not in conv:
            assert _bits(grads[k], per[0][1][k] + per[1][1][k]), k
    worst = {}
    refs = [Y.pyramid_reference_for(cv) for cv in views]
    for k in conv:
        ref, A = refs[0][0][k] + refs[1][0][k], refs[0][1][k] + refs[1][1][k]
        worst[k] = float(Y.ratios(grads[k].cpu(), ref, A).max())
        assert worst[k] <= Y.limit("pyramid"), (k, worst[k], Y.limit("pyramid"))
        assert float(Y.ratios((per[0][1][k] + per[1][1][k]).cpu(), ref, A).max()) <= Y.limit("pyramid"), k
    print("pyramid groups: conv weight gradients, worst error / (limit x A): %s" % {k.replace(Y.PREFIX, ""): "%.3f" % (q / Y.limit("pyramid")) for k, q in worst.items()})
    # the ungrouped pass over the same four images is something else: its statistics pool the views
    pooled = _pyramid_pass(_pyramid_trainer(c, device), c, device)[0]
    assert not _bits(pooled, p1)
    # groups=1 is the call without the argument; stored statistics ignore the groups and leave the buffers alone
    a = _pyramid_pass(_pyramid_trainer(c, device), c, device, groups=1)
    assert _bits(a[0], pooled)
    fz = _pyramid_trainer(c, device)
    stored = {k: v.clone() for k, v in fz.buffers.items()}
    f1 = _pyramid_pass(fz, c, device, batch_stats=False, groups=2)[0]
    f2 = _pyramid_pass(_pyramid_trainer(c, device), c, device, batch_stats=False)[0]
    assert _bits(f1, f2) and all(torch.equal(stored[k], v) for k, v in fz.buffers.items())
    from nopesac_amd import ops
    with pytest.raises(ops.OpsArgumentError):
        _pyramid_pass(_pyramid_trainer(c, device), c, device, groups=3)


def test_the_trainers_losses_pass_groups_on(device):
    """encoder.losses / decoder.losses / pyramid.losses with groups=2 are the step-by-step composition with groups=2 at the pyramid's
    forward and at the criterion, bit for bit (B = 2: one image per view, res5 at 3 x 4, no dropout); the pyramid's counters advance by 2
    per forward; the chain's backward fills all 235 gradients.  The grouped losses differ from the ungrouped ones."""
    from nopesac_amd.synth import synth_state_dict
    from tests.test_plane_encoder_training_gpu import NQ, _chain
    model, head, feats, f32, pos, targets, enc, dec, pyr, heads = _chain(device)
    try:
        stored = {k: v.clone() for k, v in pyr.buffers.items()}

        def restart():
            for k, v in stored.items():
                pyr.buffers[k].copy_(v)
        counter = [k for k in pyr.buffers if k.endswith("num_batches_tracked")]
        losses, idx = enc.losses(heads, dec, pyr, f32, targets, groups=2)
        assert len(counter) == 8 and all(int(pyr.buffers[k]) == int(stored[k]) + 2 for k in counter)
        per = heads.criterion.last["group_losses"]
        assert len(per) == 2 and all(_bits(losses[k].detach(), (per[0][k] + per[1][k]) / 2) for k in losses)
        grads = enc.backward(losses)
        assert len(grads) == 235 and all(bool(torch.isfinite(g).all()) for g in grads.values())
        restart()
        memory = enc.forward(f32["res5"], 2).detach()
        hs = dec.forward(memory, pos, 2).detach()
        p1 = pyr.forward(f32, memory, 2, groups=2).detach()
        want, _ = heads.losses(hs, p1, targets, groups=2)
        assert set(want) == set(losses) and all(_bits(want[k].detach(), losses[k].detach()) for k in want)
        restart()
        a, _ = dec.losses(heads, memory, pos, p1, targets, groups=2)
        b, _ = pyr.losses(heads, f32, memory, hs, targets, groups=2)
        assert all(_bits(a[k].detach(), want[k].detach()) and _bits(b[k].detach(), want[k].detach()) for k in want)
        restart()
        pooled, _ = enc.losses(heads, dec, pyr, f32, targets)
        assert all(int(pyr.buffers[k]) == int(stored[k]) + 1 for k in counter)
        assert not all(_bits(pooled[k].detach(), losses[k].detach()) for k in losses)
    finally:
        model.load_state_dict(synth_state_dict(NQ))
