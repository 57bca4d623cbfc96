"""GPU: the model-wide optimiser (nopesac_amd/optim.py over csrc/optimizer.hip).  The per-tensor path - ops.scale_by + ops.adamw_step /
ops.sgd_step, HeadTrainer.step_from_cfg - is the yardstick for bits; float64 restatements (tests/model_optimizer_forms.py on
tests/stream_forms.py) are the yardstick wherever the full-model norm changes the numbers, under the project's rule: FLOOR_FACTOR x the
error of the plain-f32 formulation, per element against S, never below 2^-24."""
import pytest
import torch

from tests import model_optimizer_forms as M
from tests import stream_forms as S

pytestmark = pytest.mark.gpu
WORST = {}


def _note(family, q, tag):
    if q > WORST.get(family, (0.0, ""))[0]:
        WORST[family] = (q, tag)
    print("model optimiser: %-28s error / bound %.3f  (%s)" % (family, q, tag))


def _toy(device, sizes, seed, cls=None, prefix="", guard=False):
    """A toy trainer over `sizes` with keys of every group.  guard: its parameters are moved into prefilled buffers, every second one
    a float off a 16-byte boundary -> (trainer, [(buffer, n, misaligned)])."""
    Head, _ = M.toy_classes()
    tr = (cls or Head)({prefix + M.key_for(i): M.values(n, seed + i).to(device) for i, n in enumerate(sizes)})
    bufs = []
    if guard:
        for i, (k, p) in enumerate(list(tr.params.items())):
            buf, view = M.guarded(p.detach(), device, misalign=i % 2 == 1)
            tr.params[k] = view.requires_grad_(True)
            bufs.append((buf, p.numel(), i % 2 == 1))
    return tr, bufs


def _set_grads(trainers, step, device, scale=1.0, skip=()):
    i = 0
    for tr in trainers:
        for k, p in tr.params.items():
            p.grad = None if k in skip else (M.values(p.numel(), 1000 + 17 * step + i) * scale).to(device).view(p.shape)
            i += 1


def _params_equal(a_trainers, b_trainers):
    for a, b in zip(a_trainers, b_trainers):
        for k in a.params:
            assert M.same_bits(a.params[k], b.params[k]), k


def _arenas_clean(opt):
    for arena in (opt.G, opt.M1, opt.M2):
        if arena is not None:
            assert M.padding_is_zero(opt.layout, arena)


# ---------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_gather_bits(misalign, device):
    from nopesac_amd import ops
    params = [torch.zeros(n, device=device) for n in M.SIZES]
    layout = ops.OptLayout(params, [0] * len(params))
    G = layout.arena()
    srcs = [M.guarded(M.values(n, 40 + i), device, misalign) for i, n in enumerate(M.SIZES)]
    for present in ([True] * len(params), [i % 3 != 1 for i in range(len(params))], [i % 3 == 1 for i in range(len(params))]):
        grads = [v if here else None for (_, v), here in zip(srcs, present)]
        ops.opt_gather(layout, layout.sources(grads), G)
        want = torch.zeros(layout.arena_floats)
        for i, (g, o) in enumerate(zip(grads, layout.offsets.tolist())):
            if g is not None:
                want[o:o + g.numel()] = g.cpu()
        assert M.same_bits(G, want), present                                            # sources at their offsets, +0 everywhere else
        assert all(M.guards_intact(buf, v.numel(), misalign) for buf, v in srcs)
    with pytest.raises(ops.OpsArgumentError):                                           # a strided gradient never reaches the table
        layout.sources([torch.zeros(2 * n, device=device)[::2] for n in M.SIZES])


def test_gather_takes_a_non_contiguous_grad(device):
    from nopesac_amd.optim import ModelOptimizer
    Head, _ = M.toy_classes()
    tr = Head({"toy.w": M.values(7 * 9, 1).view(7, 9).to(device), "toy.b": M.values(5, 2).to(device)})
    g = M.values(7 * 9, 3).view(9, 7).to(device).t()
    assert not g.is_contiguous()
    tr.params["toy.w"].grad = g
    opt = ModelOptimizer([tr], optimizer="SGD", momentum=0.0, weight_decay=0.0)
    opt.step(lr=0.1)
    assert M.same_bits(opt.layout.view(opt.G, 0), g.contiguous()) and M.same_bits(opt.layout.view(opt.G, 1), torch.zeros(5))
    assert M.same_bits(tr.params["toy.b"], M.values(5, 2))                              # no gradient: not stepped


@pytest.mark.parametrize("coef", [0.37, 1.0, None])
@pytest.mark.parametrize("config", S.STEP_CONFIGS, ids=lambda c: "%s_wd%g_mom%g" % c)
def test_step_bits_against_the_per_tensor_kernels(config, coef, device):
    """Three steps of ops.opt_step over the boundary sizes, two groups with their own lr and decay, parameters inside guarded buffers
    (every second one misaligned) == ops.scale_by + ops.adamw_step / ops.sgd_step per tensor on copies: parameters and both moments."""
    from nopesac_amd import ops
    name, wd, mom = config
    lr = S.STEP_LR[name]
    groups = [(lr, wd), (0.3 * lr, wd + 0.02)]
    held = [M.guarded(M.values(n, i), device, misalign=i % 2 == 1) for i, n in enumerate(M.SIZES)]
    params = [v for _, v in held]
    gidx = [(i // 2) % 2 for i in range(len(params))]
    layout = ops.OptLayout(params, gidx)
    G, M1, M2 = layout.arena(), layout.arena(), layout.arena()
    ref = [p.clone() for p in params]
    r1, r2 = [torch.zeros_like(p) for p in ref], [torch.zeros_like(p) for p in ref]
    cdev = None if coef is None else torch.full((1,), coef, device=device)
    for t in range(1, S.STEPS + 1):
        grads = [M.values(p.numel(), 100 * t + i).to(device) for i, p in enumerate(params)]
        src = layout.sources(grads, first=[t == 1] * len(params))
        ops.opt_gather(layout, src, G)
        ops.opt_step(layout, src, G, M1 if (name == "ADAMW" or mom) else None, M2 if name == "ADAMW" else None, cdev, name, groups, t,
                     S.ADAM_BETAS, S.ADAM_EPS, mom)
        for i, g in enumerate(grads):
            g = g.clone()
            if cdev is not None:
                ops.scale_by(g, cdev)
            glr, gwd = groups[gidx[i]]
            if name == "ADAMW":
                ops.adamw_step(ref[i], g, r1[i], r2[i], glr, S.ADAM_BETAS[0], S.ADAM_BETAS[1], S.ADAM_EPS, gwd, t)
            else:
                ops.sgd_step(ref[i], g, r1[i], glr, mom, gwd, t == 1)
    for i, p in enumerate(params):
        assert M.same_bits(p, ref[i]), ("param", M.SIZES[i])
        if name == "ADAMW" or mom:
            assert M.same_bits(layout.view(M1, i), r1[i]), ("moment 1", M.SIZES[i])
        if name == "ADAMW":
            assert M.same_bits(layout.view(M2, i), r2[i]), ("moment 2", M.SIZES[i])
        assert M.guards_intact(held[i][0], p.numel(), i % 2 == 1), M.SIZES[i]
    assert all(M.padding_is_zero(layout, a) for a in (G, M1, M2))
    if name == "SGD":
        assert not bool(M2.any()) and (mom or not bool(M1.any()))                      # arenas the mode does not use are never written


# ---------------------------------------------------------------------------------------------------------------------------- ModelOptimizer
@pytest.mark.parametrize("name", ["ADAMW", "SGD"])
def test_model_step_without_clipping_is_step_from_cfg(name, device):
    """Three steps, multipliers 0.1 and 1, all three decay groups, parameters partly misaligned: the bits of every trainer's own
    step_from_cfg on copies - parameters and optimiser state."""
    from nopesac_amd.optim import ModelOptimizer
    _, Backbone = M.toy_classes()
    cfg = M.solver_cfg("SOLVER.OPTIMIZER", name)
    a, bufs_a = _toy(device, M.SIZES, 0, guard=True)
    b, bufs_b = _toy(device, (5, 4097, 300), 50, cls=Backbone, prefix="backbone.", guard=True)
    a2, _ = _toy(device, M.SIZES, 0)
    b2, _ = _toy(device, (5, 4097, 300), 50, cls=Backbone, prefix="backbone.")
    opt = ModelOptimizer.from_cfg([a, b], cfg)
    assert opt.max_norm is None and len(opt.groups) == 4 and opt.reduce is None
    for t in range(3):
        _set_grads([a, b], t, device)
        _set_grads([a2, b2], t, device)
        coef = opt.step(lr=float(cfg.SOLVER.BASE_LR))
        assert float(coef) == 1.0
        a2.step_from_cfg(cfg)
        b2.step_from_cfg(cfg)
    _params_equal([a, b], [a2, b2])
    assert opt.steps == 3 == a2.steps
    for i, k in enumerate(opt.keys):
        st = (a2 if k in a2.params else b2).state[k]
        if name == "ADAMW":
            assert M.same_bits(opt.layout.view(opt.M1, i), st["m1"]) and M.same_bits(opt.layout.view(opt.M2, i), st["m2"]), k
        else:
            assert M.same_bits(opt.layout.view(opt.M1, i), st["mom"]), k
    assert all(M.guards_intact(*b_) for b_ in bufs_a + bufs_b)
    _arenas_clean(opt)


def _unit_norm_grads(trainer, norm, seed, device):
    gs = [M.values(p.numel(), seed + i).double() for i, p in enumerate(trainer.params.values())]
    total = torch.cat(gs).norm()
    gs = [(g * (norm / total)).float() for g in gs]
    for p, g in zip(trainer.params.values(), gs):
        p.grad = g.to(device).view(p.shape)
    return gs


@pytest.mark.parametrize("name", ["ADAMW", "SGD"])
def test_full_model_clip_over_two_trainers(name, device):
    """Two trainers whose gradient norms are 0.8 c each: the model's norm is 1.13 c, so the reference scales both by 1 / 1.13.  Each
    trainer's own clip (what step_from_cfg runs) sees 0.8 c and leaves its gradients alone - the behaviour ModelOptimizer corrects."""
    from nopesac_amd.optim import ModelOptimizer
    from nopesac_amd.training import HeadTrainer
    c = 0.5
    mom = 0.9 if name == "SGD" else 0.0
    solver = ("SOLVER.OPTIMIZER", name, "SOLVER.BASE_LR", S.STEP_LR[name], "SOLVER.MOMENTUM", mom)
    cfg = M.solver_cfg(*solver, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model",
                       "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", c)
    sizes_a, sizes_b = (257, 4097, 3), (16385, 1, 255)
    sets = []
    for _ in range(3):
        a, _b = _toy(device, sizes_a, 0)
        b, _b = _toy(device, sizes_b, 20, prefix="second.")
        ga, gb = _unit_norm_grads(a, 0.8 * c, 300, device), _unit_norm_grads(b, 0.8 * c, 400, device)
        sets.append((a, b))
    (a, b), (a2, b2), (a3, b3) = sets
    p0 = [p.detach().cpu().clone() for tr in (a, b) for p in tr.params.values()]
    wds = [HeadTrainer._weight_decay(k, float(cfg.SOLVER.WEIGHT_DECAY), float(cfg.SOLVER.WEIGHT_DECAY_NORM), float(cfg.SOLVER.WEIGHT_DECAY_EMBED))
           for tr in (a, b) for k in tr.params]
    opt = ModelOptimizer.from_cfg([a, b], cfg)
    coef = opt.step(lr=S.STEP_LR[name])
    ref, Sm, coefs = M.clipped_steps_ref(p0, [ga + gb], name, wds, mom, c)
    ss = S.clip_ref(torch.cat(ga + gb), c)[0]
    assert float(coefs[0]) < 0.9 and float(coef) < 1.0 and abs(float(coefs[0]) - 1 / (0.8 * 2 ** 0.5)) < 1e-3
    q = abs(float(coef) - float(coefs[0])) / float(coefs[0]) / M.coef_bound()
    _note("full-model clip coefficient", q, "two trainers at 0.8 c")
    assert q <= 1.0
    assert abs(float(opt.grad_norm_sq) - float(ss)) / float(ss) <= M.coef_bound()
    bound = M.clipped_step_bound(name)
    for p, r, s_, k in zip(opt.params, ref, Sm, opt.keys):
        q = S.quotient(p.detach(), r, s_) / bound
        _note("clipped step " + name, q, "two trainers, %s n%d" % (k, p.numel()))
        assert q <= 1.0, (k, q)
    # the per-trainer path on the same gradients: neither trainer clips (coefficient exactly 1), and its step is the UNCLIPPED step
    assert float(a2.clip_grad_norm(c)) == 1.0 and float(b2.clip_grad_norm(c)) == 1.0
    a2.step_from_cfg(cfg)
    b2.step_from_cfg(cfg)
    cfg_off = M.solver_cfg(*solver)
    ModelOptimizer.from_cfg([a3, b3], cfg_off).step(lr=S.STEP_LR[name])
    _params_equal([a2, b2], [a3, b3])
    if name == "SGD":                                    # (AdamW's step is scale-invariant up to eps: there the coefficient is the witness)
        assert not M.same_bits(a.params[M.key_for(1)], a2.params[M.key_for(1)])


@pytest.mark.parametrize("name,mom", [("ADAMW", 0.0), ("SGD", 0.9)], ids=["ADAMW", "SGD_momentum"])
def test_three_clipped_steps_against_f64(name, mom, device):
    from nopesac_amd.optim import ModelOptimizer
    from nopesac_amd.training import HeadTrainer
    tr, _ = _toy(device, M.SIZES, 0)
    grads = [[M.values(n, 500 + 31 * t + i) for i, n in enumerate(M.SIZES)] for t in range(S.STEPS)]
    max_norm = 0.5 * float(torch.cat(grads[0]).double().norm())
    cfg = M.solver_cfg("SOLVER.OPTIMIZER", name, "SOLVER.BASE_LR", S.STEP_LR[name], "SOLVER.MOMENTUM", mom, "SOLVER.CLIP_GRADIENTS.ENABLED", True,
                       "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", max_norm)
    p0 = [p.detach().cpu().clone() for p in tr.params.values()]
    wds = [HeadTrainer._weight_decay(k, float(cfg.SOLVER.WEIGHT_DECAY), float(cfg.SOLVER.WEIGHT_DECAY_NORM), float(cfg.SOLVER.WEIGHT_DECAY_EMBED))
           for k in tr.params]
    assert len(set(wds)) == 3
    opt = ModelOptimizer.from_cfg([tr], cfg)
    got_coefs = []
    for t in range(S.STEPS):
        for p, g in zip(tr.params.values(), grads[t]):
            p.grad = g.to(device)
        got_coefs.append(opt.step(lr=S.STEP_LR[name]).cpu())
    ref, Sm, coefs = M.clipped_steps_ref(p0, grads, name, wds, mom, max_norm)
    for t in range(S.STEPS):
        assert float(coefs[t]) < 1.0 and float(got_coefs[t]) < 1.0
        q = abs(float(got_coefs[t]) - float(coefs[t])) / float(coefs[t]) / M.coef_bound()
        _note("clip coefficient", q, "%s step %d" % (name, t))
        assert q <= 1.0
    bound = M.clipped_step_bound(name)
    for p, r, s_, n in zip(tr.params.values(), ref, Sm, M.SIZES):
        q = S.quotient(p.detach(), r, s_) / bound
        _note("three clipped steps " + name, q, "n%d" % n)
        assert q <= 1.0, (name, n, q)
    _arenas_clean(opt)


def test_absent_gradient_without_reduce(device):
    """No .grad, no reduce: the tensor and its moments do not move, the norm is that of the rest, and its first momentum step - two
    steps later - is a FIRST step (buffer = gradient, whatever the buffer held)."""
    from nopesac_amd import ops
    from nopesac_amd.optim import ModelOptimizer
    tr, _ = _toy(device, (257, 4097, 5), 0)
    keys = list(tr.params)
    lone = keys[1]
    before = tr.params[lone].detach().clone()
    opt = ModelOptimizer([tr], optimizer="SGD", momentum=0.9, weight_decay=0.01, max_norm=1.0)
    for t in range(2):
        _set_grads([tr], t, device, skip=(lone,))
        opt.step(lr=0.1)
        rest = torch.cat([p.grad.reshape(-1).cpu() for k, p in tr.params.items() if k != lone])
        ss = S.clip_ref(rest, 1.0)[0]
        assert abs(float(opt.grad_norm_sq) - float(ss)) / float(ss) <= M.coef_bound()
        assert M.same_bits(tr.params[lone], before) and not bool(opt.layout.view(opt.M1, 1).any())
    assert opt.stepped == [True, False, True] and opt.steps == 2
    opt.layout.view(opt.M1, 1).fill_(7.0)                                               # a first step must not read the buffer
    _set_grads([tr], 2, device)
    coef = opt.step(lr=0.1)
    g = tr.params[lone].grad.clone()
    ops.scale_by(g, coef)
    want, buf = before.clone(), torch.full_like(before, 7.0)
    ops.sgd_step(want, g, buf, 0.1, 0.9, 0.01, True)
    assert M.same_bits(tr.params[lone], want) and M.same_bits(opt.layout.view(opt.M1, 1), buf)
    assert opt.stepped == [True, True, True]


def test_absent_gradient_with_reduce_is_stepped_with_zeros(device):
    from nopesac_amd import ops
    from nopesac_amd.optim import ModelOptimizer
    tr, _ = _toy(device, (257, 4097, 5), 0)
    lone = list(tr.params)[1]
    before = tr.params[lone].detach().clone()
    seen = []
    opt = ModelOptimizer([tr], optimizer="ADAMW", weight_decay=0.05, reduce=lambda G: seen.append(G.data_ptr()))
    _set_grads([tr], 0, device, skip=(lone,))
    opt.step(lr=0.01)
    assert seen == [opt.G.data_ptr()] and not bool(opt.layout.view(opt.G, 1).any())
    want, m1, m2 = before.clone(), torch.zeros_like(before), torch.zeros_like(before)
    ops.adamw_step(want, torch.zeros_like(before), m1, m2, 0.01, 0.9, 0.999, 1e-8, 0.05, 1)
    assert M.same_bits(tr.params[lone], want) and not M.same_bits(want, before)
    assert opt.stepped == [True, True, True]


def test_reduce_hook_equals_averaged_gradients(device):
    """A reduce that adds a second rank's gradients and halves == a run fed (g1 + g2) * 0.5, formed with the same f32 operations."""
    from nopesac_amd.optim import ModelOptimizer
    sizes = (257, 4097, 5, 16385)
    a, _ = _toy(device, sizes, 0)
    b, _ = _toy(device, sizes, 0)
    g1 = [M.values(n, 600 + i).to(device) for i, n in enumerate(sizes)]
    g2 = [M.values(n, 700 + i).to(device) for i, n in enumerate(sizes)]
    opt_a = ModelOptimizer([a], weight_decay=0.05, weight_decay_norm=0.5, max_norm=1.0)
    other = opt_a.layout.arena()
    for i, g in enumerate(g2):
        opt_a.layout.view(other, i).copy_(g)
    opt_a.reduce = lambda G: G.add_(other).mul_(0.5)
    opt_b = ModelOptimizer([b], weight_decay=0.05, weight_decay_norm=0.5, max_norm=1.0)
    for p, q, x, y in zip(a.params.values(), b.params.values(), g1, g2):
        p.grad, q.grad = x, (x + y) * 0.5
    ca, cb = opt_a.step(lr=0.01), opt_b.step(lr=0.01)
    assert M.same_bits(ca, cb) and float(ca) < 1.0 and M.same_bits(opt_a.grad_norm_sq, opt_b.grad_norm_sq)
    _params_equal([a], [b])
    _arenas_clean(opt_a)


def test_schedule_in_the_loop(device):
    from nopesac_amd.optim import ModelOptimizer, lr_at
    cfg = M.solver_cfg("SOLVER.WARMUP_ITERS", 2, "SOLVER.STEPS", (3,))
    lrs = [lr_at(cfg, k) for k in range(5)]
    assert lrs[0] < lrs[1] < lrs[2] == float(cfg.SOLVER.BASE_LR) and lrs[3] == lrs[4] == pytest.approx(lrs[2] * float(cfg.SOLVER.GAMMA))
    a, _ = _toy(device, (257, 5, 4097), 0)
    b, _ = _toy(device, (257, 5, 4097), 0)
    c, _ = _toy(device, (257, 5, 4097), 0)
    oa, ob, oc = (ModelOptimizer.from_cfg([t], cfg) for t in (a, b, c))
    for k in range(5):
        _set_grads([a], k, device); _set_grads([b], k, device); _set_grads([c], k, device)
        oa.step()
        ob.step(lr=lrs[k])
        oc.step(lr=float(cfg.SOLVER.BASE_LR))
    _params_equal([a], [b])
    assert oa.steps == 5 and not M.same_bits(a.params["toy.w0"], c.params["toy.w0"])
    with pytest.raises(ValueError, match="learning rate"):
        ModelOptimizer([c]).step()


@pytest.mark.parametrize("name", ["ADAMW", "SGD"])
def test_resume_is_bitwise(name, device, tmp_path):
    from nopesac_amd.optim import ModelOptimizer
    Head, _ = M.toy_classes()
    kw = dict(optimizer=name, momentum=0.9, weight_decay=0.05, weight_decay_embed=0.25, max_norm=1.0)
    sizes = (257, 4097, 5)
    a, _ = _toy(device, sizes, 0)
    b, _ = _toy(device, sizes, 0)
    oa, ob = ModelOptimizer([a], **kw), ModelOptimizer([b], **kw)
    skip = (list(a.params)[2],)                                                         # one tensor has not stepped at save time
    for t in range(2):
        _set_grads([a], t, device, skip=skip); _set_grads([b], t, device, skip=skip)
        oa.step(lr=0.01); ob.step(lr=0.01)
    path = str(tmp_path / "optimizer.pt")
    ob.save(path)
    sd = ob.state_dict()
    assert sd["steps"] == 2 and sd["optimizer"] == name and set(sd["state"]) == set(b.params)
    assert all(not t.is_cuda for e in sd["state"].values() for t in e.values() if torch.is_tensor(t))
    assert [sd["state"][k]["stepped"] for k in b.params] == [True, True, False]
    assert set(sd["state"][skip[0]]) == ({"exp_avg", "exp_avg_sq", "stepped"} if name == "ADAMW" else {"momentum_buffer", "stepped"})
    c = Head({k: p.detach().clone() for k, p in b.params.items()})
    oc = ModelOptimizer([c], **kw)
    oc.load(path)
    assert oc.steps == 2 and oc.stepped == ob.stepped
    _set_grads([a], 2, device); _set_grads([c], 2, device)
    ca, cc = oa.step(lr=0.01), oc.step(lr=0.01)
    assert M.same_bits(ca, cc)
    _params_equal([a], [c])
    assert M.same_bits(oa.M1, oc.M1)
    other = Head({"toy.other": torch.zeros(3, device=device)})
    with pytest.raises(ValueError, match="keys differ"):
        ModelOptimizer([other], **kw).load(path)
    wrong = ob.state_dict()
    first = list(wrong["state"])[0]
    wrong["state"][first] = {k: (v[:-1] if torch.is_tensor(v) else v) for k, v in wrong["state"][first].items()}
    with pytest.raises(ValueError, match="shape"):
        oc.load_state_dict(wrong)
    with pytest.raises(ValueError, match="optimizer"):
        ModelOptimizer([other], optimizer="SGD" if name == "ADAMW" else "ADAMW").load_state_dict(sd)


def test_real_tensors_once(device, sd50):
    """The matching head's and the instance heads' tensors of the synthetic checkpoint (209 tensors, 12.5 M floats, bin_score at n = 1,
    sizes not divisible by 4) under seeded gradients: clipping off == step_from_cfg, bit for bit; clipping on against float64."""
    from nopesac_amd import training as T
    from nopesac_amd.optim import ModelOptimizer

    def trainers():
        return [T.MatchingHeadTrainer.from_state_dict(sd50, 50, device), T.PlaneInstanceHeadsTrainer.from_state_dict(sd50, 50, device)]

    def seeded_grads(trs):
        g = torch.Generator(device="cpu")
        g.manual_seed(20240)
        out = []
        for tr in trs:
            for p in tr.params.values():
                out.append(torch.randn(p.shape, generator=g, dtype=torch.float32))
                p.grad = out[-1].to(device)
        return out
    a, b, c = trainers(), trainers(), trainers()
    sizes = [p.numel() for tr in a for p in tr.params.values()]
    assert len(sizes) == 209 and 12.4e6 < sum(sizes) < 12.6e6 and min(sizes) == 1 and sum(1 for n in sizes if n % 4) >= 5
    cfg = M.solver_cfg()
    seeded_grads(a); seeded_grads(b)
    ModelOptimizer.from_cfg(a, cfg).step(lr=float(cfg.SOLVER.BASE_LR))
    for tr in b:
        tr.step_from_cfg(cfg)
    _params_equal(a, b)
    grads = seeded_grads(c)
    max_norm = 0.5 * float(torch.cat([g.reshape(-1) for g in grads]).double().norm())
    cfg_on = M.solver_cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", max_norm)
    assert all(tr.lr_multiplier(cfg_on) == 1.0 for tr in c) and float(cfg_on.SOLVER.BASE_LR) == S.STEP_LR["ADAMW"]
    p0 = [p.detach().cpu().clone().reshape(-1) for tr in c for p in tr.params.values()]
    wds = [T.HeadTrainer._weight_decay(k, float(cfg.SOLVER.WEIGHT_DECAY), float(cfg.SOLVER.WEIGHT_DECAY_NORM), float(cfg.SOLVER.WEIGHT_DECAY_EMBED))
           for tr in c for k in tr.params]
    opt = ModelOptimizer.from_cfg(c, cfg_on)
    coef = opt.step(lr=S.STEP_LR["ADAMW"])
    ref, Sm, coefs = M.clipped_steps_ref(p0, [[g.reshape(-1) for g in grads]], "ADAMW", wds, 0.0, max_norm)
    q = abs(float(coef) - float(coefs[0])) / float(coefs[0]) / M.coef_bound()
    _note("clip coefficient", q, "209 real tensors")
    assert q <= 1.0 and float(coef) < 1.0
    bound = M.clipped_step_bound("ADAMW")
    worst = max(S.quotient(p.detach(), r, s_) for p, r, s_ in zip(opt.params, ref, Sm)) / bound
    _note("clipped step ADAMW", worst, "209 real tensors")
    assert worst <= 1.0
