"""The backward half of the matching head (reference matching_net/matching_head.py:43-139, transformer/gnn.py): the kernels of
csrc/matcher_bwd.hip (ragged attention, LayerNorm, the unrolled log-Sinkhorn + embedding loss, the descriptor dot) and
nopesac_amd/training.py::MatchingHeadTrainer against float64 torch.autograd on the oracle's functions (O.matcher_scores, O.log_sinkhorn,
O.gnn_layer, O.layer_norm - pinned to the imported reference in the forward direction, oracle/gen_golden.py stage E).  The three loss
lines of embedding_loss_forward (:136-138) are restated here."""
import pytest
import torch
from torch.nn import functional as F

from tests import golden_inputs as GI
from tests.util import make_model

pytestmark = pytest.mark.gpu

HEAD_CASES = [(7, 5, 11), (1, 3, 12), (32, 33, 13), (50, 50, 14), (2, 2, 15)]
MP = "matching_head."


def _pad(t, nq):
    out = torch.zeros(nq, *t.shape[1:], dtype=t.dtype)
    out[: t.shape[0]] = t
    return out


def gt_corr_case(n1, n2, seed, nq):
    """uint8 [nq+1, nq+1], dustbin at index nq: min(n1, n2) // 2 random matches, every other live row / column goes to the dustbin."""
    g = torch.Generator().manual_seed(seed)
    m = min(n1, n2) // 2
    r = torch.randperm(n1, generator=g)[:m]
    c = torch.randperm(n2, generator=g)[:m]
    gt = torch.zeros(nq + 1, nq + 1, dtype=torch.uint8)
    gt[r, c] = 1
    for i in sorted(set(range(n1)) - set(r.tolist())):
        gt[i, nq] = 1
    for j in sorted(set(range(n2)) - set(c.tolist())):
        gt[nq, j] = 1
    return gt


def _live(t, n1, n2, nq):
    """The live block of a padded [nq+1, nq+1] matrix in the oracle's compact layout [n1+1, n2+1]."""
    ri = torch.tensor(list(range(n1)) + [nq])
    ci = torch.tensor(list(range(n2)) + [nq])
    return t[ri][:, ci]


def _emb_loss(selected):
    """embedding_loss_forward (matching_head.py:136-138) on the selected entries of the whole batch."""
    return torch.mean(-torch.clamp(selected, max=0.0)) * 2


def _f64(fn):
    torch.set_default_dtype(torch.float64)                    # (the oracle creates a few constants in the default dtype)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


_HEAD = {}


def _head_batch():
    """The batch of the whole-head tests (generated once, in the default dtype, before any float64 section)."""
    if not _HEAD:
        nq = 50
        cases = [GI.matcher_case(n1, n2, s) for n1, n2, s in HEAD_CASES]
        _HEAD.update(nq=nq, cases=cases, gts=[gt_corr_case(n1, n2, s, nq) for n1, n2, s in HEAD_CASES],
                     app=torch.stack([_pad(c[0], nq) for c in cases] + [_pad(c[1], nq) for c in cases]),
                     n_all=torch.tensor([c[0] for c in HEAD_CASES] + [c[1] for c in HEAD_CASES], dtype=torch.int32),
                     cam7=torch.stack([c[2] for c in cases]), p1=torch.stack([_pad(c[3], nq) for c in cases]),
                     p2=torch.stack([_pad(c[4], nq) for c in cases]))
        _HEAD["gt"] = torch.stack(_HEAD["gts"])
    return _HEAD


def _oracle_head(sd_or_params, sd, iters, names, want_app=True):
    """float64: loss, parameter gradients, app gradients (padded [2B, nq, 256]) and the selected scores, from O.matcher_scores +
    O.log_sinkhorn + the loss lines.  `sd_or_params`: {name: float64 leaf} to use instead of sd's tensors (the optimiser test)."""
    from oracle import nopesac_oracle as O
    H = _head_batch()
    nq = H["nq"]

    def run():
        sdg = {k: v.double() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
        for k in names:
            sdg[k] = sd_or_params[k] if sd_or_params is not None else sdg[k].clone().requires_grad_(True)
        apps = [(c[0].double().requires_grad_(want_app), c[1].double().requires_grad_(want_app)) for c in H["cases"]]
        sel = []
        for b, (c, (n1, n2, _)) in enumerate(zip(H["cases"], HEAD_CASES)):
            s = O.matcher_scores(sdg, apps[b][0], apps[b][1], c[2].double(), c[3].double(), c[4].double(), O.OracleConfig(num_queries=nq))
            Z = O.log_sinkhorn(s, sdg[MP + "bin_score"], iters)
            sel.append(Z[_live(H["gts"][b], n1, n2, nq) > 0])
        sel = torch.cat(sel)
        loss = _emb_loss(sel)
        loss.backward()
        g_app = None
        if want_app:
            g_app = torch.stack([_pad(a[0].grad, nq) for a in apps] + [_pad(a[1].grad, nq) for a in apps])
        return loss.detach(), {k: sdg[k].grad for k in names}, g_app, sel.detach()
    return _f64(run)


def _run_trainer(tr, device, iters, app_grad=True):
    H = _head_batch()
    dv = lambda k: H[k].to(device)
    app = dv("app").requires_grad_(app_grad)
    losses = tr.matching_losses(app, dv("n_all"), dv("cam7"), dv("p1"), dv("p2"), dv("gt"), suffix="t", iterations=iters)
    assert list(losses) == ["losses_emb_t"]
    return losses, tr.backward(losses)


@pytest.mark.parametrize("iters", [200, 3])
def test_matching_head_gradients_match_autograd_on_the_oracle(device, sd50, iters):
    """All 185 parameter gradients and d app of the whole head for losses_emb, five ragged pairs in one batch.  At 3 iterations some
    selected scores are still positive (the clamp's zero-gradient branch), and the unrolled gradient differs from the fixed point's."""
    from nopesac_amd.training import MatchingHeadTrainer
    H = _head_batch()
    nq = H["nq"]
    tr = MatchingHeadTrainer.from_state_dict(sd50, nq, device)
    names = list(tr.params)
    assert len(names) == 185
    losses, grads = _run_trainer(tr, device, iters)
    o_loss, o_grads, o_app, o_sel = _oracle_head(None, sd50, iters, names)
    n_pos = int((o_sel > 0).sum())
    print("iters", iters, "selected", o_sel.numel(), "positive", n_pos, "loss", float(losses["losses_emb_t"].detach()), float(o_loss))
    if iters == 3:
        assert n_pos >= 1, "no selected score is positive: the clamp's zero-gradient branch is not exercised"
    mine = float(losses["losses_emb_t"].detach())
    assert abs(mine - float(o_loss)) < 2e-4 * abs(float(o_loss)), (mine, float(o_loss))
    gmax = max(float(o_grads[k].abs().max()) for k in names)
    report = []
    for k in names:
        ref = o_grads[k].float()
        assert float(ref.abs().max()) > 0, k                       # (no gradient is identically zero in the reference)
        assert torch.isfinite(grads[k]).all() and grads[k].shape == tr.params[k].shape, k
        report.append((float((grads[k].cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax), k))
    report.sort(reverse=True)
    print("worst parameter gradients", report[:4])
    assert report[0][0] < 2e-3, report[:6]
    g_app = tr.input_grads["app"].cpu()
    ref = o_app.float()
    err = float((g_app - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
    print("app gradient", err)
    assert float(ref.abs().max()) > 0 and err < 2e-3, err
    for s, n in enumerate(H["n_all"].tolist()):
        assert float(g_app[s, n:].abs().max()) == 0.0 if n < nq else True, s
    # run-to-run: no atomics anywhere
    losses2, grads2 = _run_trainer(tr, device, iters)
    assert torch.equal(losses["losses_emb_t"], losses2["losses_emb_t"]) and all(torch.equal(grads[k], grads2[k]) for k in names)
    assert torch.equal(g_app, tr.input_grads["app"].cpu())


def _sinkhorn_pairs(nq):
    k = 5
    pairs = [(nq, nq), (1, 1), (nq, 2), (3, nq), (nq - 1, nq // 3 + 1), (0, k), (k, 0)]
    return pairs + [p for p in [(63, 64), (64, 63), (65, nq)] if max(p) <= nq]


_SINK = {}


def _sinkhorn_inputs(nq):
    if nq not in _SINK:
        pairs = _sinkhorn_pairs(nq)
        g = torch.Generator().manual_seed(1000 + nq)
        geo = [GI.matcher_case(max(n1, 1), max(n2, 1), 300 + 7 * i + nq) for i, (n1, n2) in enumerate(pairs)]
        _SINK[nq] = dict(pairs=pairs, dd=torch.randn(len(pairs), nq, nq, generator=g) * 2, cam7=torch.stack([c[2] for c in geo]),
                         p1=torch.stack([_pad(c[3], nq) for c in geo]), p2=torch.stack([_pad(c[4], nq) for c in geo]),
                         gt=torch.stack([gt_corr_case(n1, n2, 40 + i, nq) for i, (n1, n2) in enumerate(pairs)]),
                         bin=torch.tensor(0.7))
    return _SINK[nq]


def _sinkhorn_autograd(S, nq, iters, dtype):
    """(loss, d desc_dot [B, nq, nq], d bin_score) of O.log_sinkhorn with the geometric terms as constants, in `dtype` on the CPU."""
    from oracle import nopesac_oracle as O

    def run():
        dd = S["dd"].to(dtype).clone().requires_grad_(True)
        bs = S["bin"].to(dtype).clone().requires_grad_(True)
        sel = []
        for b, (n1, n2) in enumerate(S["pairs"]):
            if n1 == 0 or n2 == 0:
                continue
            with torch.no_grad():
                ang, off = O._geometric_dists(S["p1"][b, :n1].to(dtype), S["p2"][b, :n2].to(dtype), S["cam7"][b, 3:].to(dtype),
                                              S["cam7"][b, :3].to(dtype), 1e-10, 5.0)
            Z = O.log_sinkhorn(dd[b, :n1, :n2] - off / 4.0 - ang / 8.0, bs, iters)
            sel.append(Z[_live(S["gt"][b], n1, n2, nq) > 0])
        loss = _emb_loss(torch.cat(sel))
        loss.backward()
        return loss.detach(), dd.grad, bs.grad
    return _f64(run) if dtype == torch.float64 else run()


@pytest.mark.parametrize("iters", [1, 3, 200])
@pytest.mark.parametrize("nq", [50, 64, 128])
def test_sinkhorn_loss_backward_matches_autograd(device, nq, iters):
    """The raw training twin and its backward: d desc_dot on the live blocks and d bin_score against float64 autograd of the unrolled
    iterations, at the row / column counts where a 64-lane reduction or the LDS layout can go wrong; exact zeros outside the live
    block and for empty pairs.  Tolerance: 10 x the error of float32 torch autograd on the same graph (floored at 1e-6 of the tensor)."""
    from nopesac_amd import _lib
    S = _sinkhorn_inputs(nq)
    B = len(S["pairs"])
    L = _lib.load()
    f32 = dict(device=device, dtype=torch.float32)
    d = {k: S[k].to(device).contiguous() for k in ("dd", "cam7", "p1", "p2", "gt")}
    n1 = torch.tensor([p[0] for p in S["pairs"]], dtype=torch.int32, device=device)
    n2 = torch.tensor([p[1] for p in S["pairs"]], dtype=torch.int32, device=device)
    bs = S["bin"].reshape(1).to(device)
    ls, uv = torch.empty(B, nq + 1, nq + 1, **f32), torch.empty(B, iters, 2, nq + 1, **f32)
    stats, loss, g = torch.empty(B, 2, **f32), torch.empty(2, **f32), torch.ones(1, **f32)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def run():
        gd, gb = torch.full((B, nq, nq), float("nan"), **f32), torch.full((B,), float("nan"), **f32)
        _lib.check(L.nopesac_matcher_sinkhorn_train(p(d["dd"]), p(d["p1"]), p(d["p2"]), p(d["cam7"]), p(n1), p(n2), p(bs), 4.0, 8.0, iters,
                                                    p(d["gt"]), B, nq, p(ls), p(uv), p(stats), p(loss), st), "nopesac_matcher_sinkhorn_train")
        _lib.check(L.nopesac_matcher_sinkhorn_train_backward(p(d["dd"]), p(d["p1"]), p(d["p2"]), p(d["cam7"]), p(n1), p(n2), p(bs), 4.0, 8.0,
                                                             iters, p(d["gt"]), p(uv), p(loss), p(g), B, nq, p(gd), p(gb), st),
                   "nopesac_matcher_sinkhorn_train_backward")
        return loss.cpu().clone(), gd.cpu(), gb.cpu()
    k_loss, k_gd, k_gb = run()
    l64, gd64, gb64 = _sinkhorn_autograd(S, nq, iters, torch.float64)
    l32, gd32, gb32 = _sinkhorn_autograd(S, nq, iters, torch.float32)
    assert abs(float(k_loss[0]) - float(l64)) < 2e-5 * abs(float(l64)), (float(k_loss[0]), float(l64))
    n_sel = sum(int((_live(S["gt"][b], a, c, nq) > 0).sum()) for b, (a, c) in enumerate(S["pairs"]) if a > 0 and c > 0)
    assert float(k_loss[1]) == n_sel
    e32 = float((gd32.double() - gd64).abs().max())
    ek = float((k_gd.double() - gd64).abs().max())
    tol = max(10 * e32, 1e-6 * float(gd64.abs().max()))
    print("nq", nq, "iters", iters, "d desc_dot: kernel", ek, "f32 autograd", e32, "tol", tol)
    assert float(gd64.abs().max()) > 0 and ek <= tol, ("d desc_dot", ek, e32, tol)
    e32b = abs(float(gb32) - float(gb64))
    ekb = abs(float(k_gb.double().sum()) - float(gb64))
    tolb = max(10 * e32b, 1e-6 * abs(float(gb64)))
    print("d bin_score: kernel", ekb, "f32 autograd", e32b, "tol", tolb)
    assert ekb <= tolb, ("d bin_score", ekb, e32b, tolb)
    for b, (a, c) in enumerate(S["pairs"]):
        assert float(k_gd[b, a:].abs().max() if a < nq else 0.0) == 0.0 and float(k_gd[b, :, c:].abs().max() if c < nq else 0.0) == 0.0, b
        if a == 0 or c == 0:
            assert float(k_gb[b]) == 0.0 and float(k_gd[b].abs().max()) == 0.0, b
    r_loss, r_gd, r_gb = run()
    assert torch.equal(k_loss, r_loss) and torch.equal(k_gd, r_gd) and torch.equal(k_gb, r_gb)


def _attention_autograd(q, k, v, w, B, L, qlen, klen, dtype):
    """Masked-softmax attention (8 heads of 32, scale 32^-0.5) per set on the live rows / keys; loss = sum(o * w)."""
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    total = 0
    for b in range(B):
        ql, kl = qlen[b], klen[b]
        qb = q[b * L: b * L + ql].view(ql, 8, 32)
        kb = k[b * L: b * L + kl].view(kl, 8, 32)
        vb = v[b * L: b * L + kl].view(kl, 8, 32)
        a = torch.softmax(torch.einsum("lhd,shd->lsh", qb, kb) * 32 ** -0.5, dim=1)
        o = torch.einsum("lsh,shd->lhd", a, vb).reshape(ql, 256)
        total = total + (o * w[b * L: b * L + ql].to(dtype)).sum()
    total.backward()
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("nq", [50, 128])
def test_attention_backward_matches_autograd(device, nq, packed):
    """dq, dk, dv of the ragged attention against float64 autograd: q / k / v as column slices of one [rows, 768] matrix (the self
    layers) and as separate matrices (the cross layers), query and key lengths that differ; exact zeros beyond the lengths."""
    from nopesac_amd.training import _Attention
    B, L = 4, nq
    qlen, klen = (nq, 1, 7, nq - 1), (nq, 3, 1, 65 if nq > 65 else 5)
    g = torch.Generator().manual_seed(5 + nq)
    qkv = torch.randn(B * L, 768, generator=g)
    w = torch.randn(B * L, 256, generator=g)
    q, k, v = qkv[:, :256], qkv[:, 256:512], qkv[:, 512:]
    ql, kl = (torch.tensor(t, dtype=torch.int32, device=device) for t in (qlen, klen))

    def run():
        if packed:
            x = qkv.to(device).requires_grad_(True)
            o = _Attention.apply(x[:, :256], x[:, 256:512], x[:, 512:], B, L, L, 8, 32 ** -0.5, ql, kl)
            o.backward(w.to(device))
            return x.grad[:, :256].cpu(), x.grad[:, 256:512].cpu(), x.grad[:, 512:].cpu()
        xs = [t.contiguous().to(device).requires_grad_(True) for t in (q, k, v)]
        o = _Attention.apply(*xs, B, L, L, 8, 32 ** -0.5, ql, kl)
        o.backward(w.to(device))
        return tuple(t.grad.cpu() for t in xs)
    mine = run()
    ref = _f64(lambda: _attention_autograd(q, k, v, w, B, L, qlen, klen, torch.float64))
    r32 = _attention_autograd(q, k, v, w, B, L, qlen, klen, torch.float32)
    for name, m, r, r3, lens in zip(("dq", "dk", "dv"), mine, ref, r32, (qlen, klen, klen)):
        e32 = float((r3.double() - r).abs().max())
        ek = float((m.double() - r).abs().max())
        tol = max(10 * e32, 1e-6 * float(r.abs().max()))
        print(name, "nq", nq, "packed", packed, "kernel", ek, "f32 autograd", e32, "tol", tol)
        assert ek <= tol, (name, ek, e32, tol)
        for b in range(B):
            if lens[b] < L:
                assert float(m[b * L + lens[b]: (b + 1) * L].abs().max()) == 0.0, (name, b)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(mine, again))


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("rows", [1, 50, 257])
def test_layernorm_backward_matches_autograd(device, rows, with_addend):
    from nopesac_amd.training import _LayerNorm
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 256, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(256, generator=g), torch.randn(256, generator=g)
    add, w = torch.randn(rows, 256, generator=g), torch.randn(rows, 256, generator=g)

    def autograd(dtype):
        xs = [t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta)]
        y = F.layer_norm(xs[0], (256,), xs[1], xs[2], 1e-5)
        (y * w.to(dtype)).sum().backward()
        return [t.grad for t in xs]

    def run():
        xs = [t.to(device).requires_grad_(True) for t in (x, gamma, beta)]
        a = add.to(device).requires_grad_(True) if with_addend else None
        y = _LayerNorm.apply(xs[0], xs[1], xs[2], a)
        y.backward(w.to(device))
        return [t.grad.cpu() for t in xs], (a.grad.cpu() if with_addend else None), y.detach().cpu()
    mine, g_add, y = run()
    ref, r32 = _f64(lambda: autograd(torch.float64)), autograd(torch.float32)
    y_ref = F.layer_norm(x.double(), (256,), gamma.double(), beta.double(), 1e-5) + (add.double() if with_addend else 0)
    assert float((y.double() - y_ref).abs().max()) < 1e-5
    for name, m, r, r3 in zip(("dx", "dgamma", "dbeta"), mine, ref, r32):
        e32 = float((r3.double() - r).abs().max())
        ek = float((m.double() - r).abs().max())
        tol = max(10 * e32, 1e-6 * float(r.abs().max()))
        print(name, "rows", rows, "kernel", ek, "f32 autograd", e32, "tol", tol)
        assert ek <= tol, (name, ek, e32, tol)
    if with_addend:
        assert torch.equal(g_add, w)
    again, _, _ = run()
    assert all(torch.equal(a, b) for a, b in zip(mine, again))


def test_matching_head_training_steps_match_torch_optim(device, sd50):
    """Five AdamW steps on the batch of the whole-head test: the first two losses against torch.optim.AdamW on the float64 oracle, and
    the loss goes down (later steps are not compared: Adam moves parameters whose gradient is rounding noise by +-lr, see
    test_refine_head_training_steps_match_torch_optim)."""
    from nopesac_amd.training import MatchingHeadTrainer
    H = _head_batch()
    tr = MatchingHeadTrainer.from_state_dict(sd50, H["nq"], device)
    names = list(tr.params)
    ref_p = {k: sd50[k].clone().double().requires_grad_(True) for k in names}
    opt = torch.optim.AdamW([ref_p[k] for k in names], lr=2e-4, weight_decay=0.01)
    mine, theirs = [], []
    for it in range(5):
        losses, _ = _run_trainer(tr, device, 200, app_grad=False)
        mine.append(float(losses["losses_emb_t"].detach()))
        tr.step(lr=2e-4, optimizer="ADAMW", weight_decay=0.01)
        if it < 2:
            opt.zero_grad()
            o_loss, _, _, _ = _oracle_head(ref_p, sd50, 200, names, want_app=False)
            theirs.append(float(o_loss))
            opt.step()
    print("losses", mine, theirs)
    assert abs(mine[0] - theirs[0]) < 1e-4 * abs(theirs[0]) and abs(mine[1] - theirs[1]) < 2e-3 * abs(theirs[1]), (mine, theirs)
    assert mine[-1] < mine[0], mine


def _live_blocks(ls, nq):
    return [_live(ls[b], n1, n2, nq) for b, (n1, n2, _) in enumerate(HEAD_CASES)]


def test_trained_matcher_reaches_the_inference_head(device, sd50):
    """The trainer's forward is the inference head's f32 forward (same parameters -> log scores within 1e-5 absolute on the live
    blocks), and after one step and write_back() the inference head runs on the updated parameters.  (The trainer groups its GEMMs as
    MatchingHead._gnn_layer does and launches the inference Sinkhorn kernel itself; one GEMM per tensor and a Sinkhorn kernel of its
    own were 2.3e-5 away - f32 rounding on scores up to 16, measured - which is why it does.)"""
    from nopesac_amd.training import MatchingHeadTrainer
    H = _head_batch()
    nq = H["nq"]
    model = make_model(device)
    head = model.matching_head
    tr = MatchingHeadTrainer.from_head(head)
    assert len(tr.params) == 185 and tr.sinkhorn_iterations == 200
    dv = lambda k: H[k].to(device)

    def inference():
        with torch.no_grad():
            return head(dv("app"), dv("n_all"), dv("cam7"), dv("p1"), dv("p2"), 0.2)[0].cpu()

    def worst(ls_a, ls_b):
        return max(float((a - b).abs().max()) for a, b in zip(_live_blocks(ls_a, nq), _live_blocks(ls_b, nq)))
    try:
        before = inference()
        _run_trainer(tr, device, None, app_grad=False)
        w_before = worst(before, tr.last["log_scores_padded"].cpu())
        tr.step(lr=1e-3)
        tr.write_back(head)
        after = inference()
        changed = worst(before, after)
        _run_trainer(tr, device, None, app_grad=False)
        w_after = worst(after, tr.last["log_scores_padded"].cpu())
    finally:                                                  # (tests/util.make_model caches the model: hand it back with its checkpoint)
        model.load_state_dict(sd50)
    print("trainer vs inference log scores: before", w_before, "after one step", w_after, "moved by", changed)
    assert changed > 1e-4, changed
    assert w_before < 1e-5 and w_after < 1e-5, (w_before, w_after)


def test_empty_batch_gives_zero_loss_and_zero_gradients(device, sd50):
    """Every pair has n1 == 0: nothing is selected, the loss is 0 (the reference's mean of nothing is NaN) and every gradient is 0."""
    from nopesac_amd.training import MatchingHeadTrainer
    H = _head_batch()
    nq, B = H["nq"], len(HEAD_CASES)
    tr = MatchingHeadTrainer.from_state_dict(sd50, nq, device)
    n_all = torch.tensor([0] * B + [0, 3, 50, 1, 7], dtype=torch.int32, device=device)
    dv = lambda k: H[k].to(device)
    app = dv("app").requires_grad_(True)
    losses = tr.matching_losses(app, n_all, dv("cam7"), dv("p1"), dv("p2"), dv("gt"), suffix="t")
    grads = tr.backward(losses)
    assert float(losses["losses_emb_t"].detach()) == 0.0
    for k, gk in grads.items():
        assert torch.isfinite(gk).all() and float(gk.abs().max()) == 0.0, k
    ga = tr.input_grads["app"]
    assert torch.isfinite(ga).all() and float(ga.abs().max()) == 0.0
