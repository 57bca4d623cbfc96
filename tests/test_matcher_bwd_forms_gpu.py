"""GPU half of the matching head's backward sweep (tests/matcher_bwd_forms.py): the kernels of csrc/matcher_bwd.hip through the raw
library, every element of every output against the float64 reference within limit x (2^-24 S + C) - nothing normalised by a tensor
maximum.  Outputs are NaN-prefilled with a guard tail: every element the header promises is written, the tail and the gaps of a padded
row stride stay; exact zeros (and the exact -1e30 padding) where the header promises them; two launches give the same bits."""
import pytest
import torch

from tests import matcher_bwd_forms as M

pytestmark = pytest.mark.gpu
WORST = {}           # (family, output) -> (worst error / (limit x A), case)
TAIL = 64
NAN = float("nan")


def _lib():
    from nopesac_amd import _lib
    return _lib, _lib.load()


def _call(name, *args):
    lib, L = _lib()
    lib.check(getattr(L, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream), name)


def _guarded(device, *shape, dtype=torch.float32):
    """A NaN-prefilled output (uint8: 255) with a guard tail -> (the whole buffer, the output view)."""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + TAIL,), NAN if dtype.is_floating_point else 255, device=device, dtype=dtype)
    return buf, buf[:n].view(*shape)


def _tail_untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b[-TAIL:]).all()) for b in bufs)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, got, case):
    w = M.worst_ratio(family, key, got)
    lim = M.limit(family)
    print("%s %s: error / (limit x A) %s" % (family, case, {k: "%.3f" % (q / lim) for k, (q, _) in w.items()}))
    for k, (q, i) in w.items():
        if q / lim > WORST.get((family, k), (-1.0, ""))[0]:
            WORST[(family, k)] = (q / lim, "%s [%d]" % (case, i))
    assert all(q <= lim for q, _ in w.values()), (case, w, lim)


# ---- attention -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.ATT_CASES, ids=lambda k: "%dx%d_%s" % k)
def test_attention_backward_against_f64(key, device):
    c = M.attention_inputs(key)
    B, Lq, Lk, H = c["B"], c["Lq"], c["Lk"], c["heads"]
    W = H * M.HD
    if c["packed"]:
        qkv = c["qkv"].to(device)
        q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
    else:
        q, k, v = (c[n].contiguous().to(device) for n in ("q", "k", "v"))
    assert q.stride(0) == (3 * W if c["packed"] else W)
    dout = c["dout"].to(device)
    ql = kl = None                                                                                  # null pointers
    if not c["null_lens"]:
        ql, kl = (torch.tensor([p[i] for p in c["lens"]], dtype=torch.int32, device=device) for i in (0, 1))
    ld = W + c["out_pad"]

    def run():
        bufs = [_guarded(device, B * L, ld) for L in (Lq, Lk, Lk)]
        (dq, dk, dv) = (b[1] for b in bufs)
        _call("nopesac_attention_small_backward", q, q.stride(0), k, k.stride(0), v, v.stride(0), dout, W, B, Lq, Lk, H, c["scale"], ql, kl,
              dq, ld, dk, ld, dv, ld)
        assert _tail_untouched(*[b[0] for b in bufs]), "wrote past the end of an output"
        return dq, dk, dv
    outs, again = run(), run()
    assert all(_same_bits(a[:, :W], b[:, :W]) for a, b in zip(outs, again))
    got = {}
    for n, o in zip(("dq", "dk", "dv"), outs):
        assert bool(torch.isnan(o[:, W:]).all()), (n, "the gap of the padded row stride was written")
        got[n] = o[:, :W].cpu()
        assert not bool(torch.isnan(got[n]).any()), (n, "an element was not written")
    _judge("attention", key, got, "%dx%d %s" % key)
    for b, (a, s) in enumerate(c["lens"]):                                                          # exact zeros beyond the lengths, and for an empty side
        dead_q = a if s else 0
        assert float(got["dq"][b * Lq + dead_q:(b + 1) * Lq].abs().sum()) == 0, b
        dead_k = s if a else 0
        for n in ("dk", "dv"):
            assert float(got[n][b * Lk + dead_k:(b + 1) * Lk].abs().sum()) == 0, (n, b)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.family_keys("layernorm"), ids=lambda k: "rows%d_ratio%g" % k)
def test_layernorm_backward_against_f64(key, device):
    _, L = _lib()
    c = M.layernorm_inputs(key)
    rows = c["rows"]
    x, gamma, dy = (c[n].to(device) for n in ("x", "gamma", "dy"))
    ws_floats = int(L.nopesac_layernorm_backward_workspace_floats(rows))
    assert ws_floats == 512 * ((rows + M.LN_BLOCK - 1) // M.LN_BLOCK)

    def run():
        bufs = [_guarded(device, rows, 256), _guarded(device, 256), _guarded(device, 256), _guarded(device, ws_floats)]
        dx, dg, db, ws = (b[1] for b in bufs)
        _call("nopesac_layernorm_backward", x, gamma, dy, rows, 256, M.LN_EPS, dx, dg, db, ws, ws_floats)
        assert _tail_untouched(*[b[0] for b in bufs]), "wrote past the end of an output or of the workspace"
        return dx, dg, db
    outs, again = run(), run()
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    got = {n: o.cpu() for n, o in zip(("dx", "dgamma", "dbeta"), outs)}
    assert not any(bool(torch.isnan(v).any()) for v in got.values())
    _judge("layernorm", key, got, "rows %d mean/std %g" % key)


# ---- Sinkhorn twin ---------------------------------------------------------------------------------------------------------------------
_TWIN = {}


def _twin(key, device):
    """The twin and its backward on one case, twice -> outputs on the CPU (cached: three tests judge them)."""
    if key in _TWIN:
        return _TWIN[key]
    c = M.sink_problem(key)
    nq, iters, B, R = c["nq"], c["iters"], len(c["pairs"]), c["nq"] + 1
    d = {n: c[n].contiguous().to(device) for n in ("dd", "p1", "p2", "cam7", "n1", "n2", "bin", "gt", "g_loss")}
    head = [d["dd"], d["p1"], d["p2"], d["cam7"], d["n1"], d["n2"], d["bin"], M.OFFSET_MULT, M.NORMAL_MULT, iters, d["gt"]]

    def run():
        bufs = [_guarded(device, B, R, R), _guarded(device, B, iters, 2, R), _guarded(device, B, 2), _guarded(device, 2),
                _guarded(device, B, nq, nq), _guarded(device, B)]
        ls, uv, stats, loss, gd, gb = (b[1] for b in bufs)
        _call("nopesac_matcher_sinkhorn_train", *head, B, nq, ls, uv, stats, loss)
        _call("nopesac_matcher_sinkhorn_train_backward", *head, uv, loss, d["g_loss"], B, nq, gd, gb)
        assert _tail_untouched(*[b[0] for b in bufs]), "wrote past the end of an output"
        return {"log_scores": ls, "uv": uv, "pair_stats": stats, "loss": loss, "d_desc_dot": gd, "d_bin_pairs": gb}
    a, b = run(), run()
    assert all(_same_bits(a[n], b[n]) for n in a), key
    _TWIN[key] = {n: v.cpu() for n, v in a.items()}
    return _TWIN[key]


@pytest.mark.parametrize("key", M.sink_cases(), ids=str)
def test_sinkhorn_twin_forward_against_f64(key, device):
    got = _twin(key, device)
    c = M.sink_problem(key)
    ref, _ = M.reference("sinkhorn_fwd", key)
    ls, uv = got["log_scores"], got["uv"]
    assert not bool(torch.isnan(ls).any()) and bool((ls[ref["log_scores"] < -1e29] == M.NEG_PAD).all())         # the padding exactly
    assert torch.equal(torch.isnan(uv), torch.isnan(ref["uv"])), "uv: written beyond a pair's compact range, or not written inside it"
    assert torch.equal(got["pair_stats"][:, 1].double(), ref["pair_stats"][:, 1]) and float(got["loss"][1]) == float(ref["loss"][1])
    for b, (n1, n2) in enumerate(c["pairs"]):
        if n1 == 0 or n2 == 0:
            assert float(got["pair_stats"][b].abs().sum()) == 0 and bool((ls[b] == M.NEG_PAD).all()), b
    if key[3] == "none_selected":
        assert float(got["loss"].abs().sum()) == 0 and float(got["pair_stats"].abs().sum()) == 0
    _judge("sinkhorn_fwd", key, {k: got[k] for k in M.OUTPUTS["sinkhorn_fwd"]}, "nq%d iters%d g%g %s" % key)


@pytest.mark.parametrize("key", M.sink_cases(), ids=str)
def test_sinkhorn_twin_backward_against_f64(key, device):
    got = _twin(key, device)
    c = M.sink_problem(key)
    gd, gb = got["d_desc_dot"], got["d_bin_pairs"]
    assert not bool(torch.isnan(gd).any()) and not bool(torch.isnan(gb).any()), "an element was not written"
    _judge("sinkhorn_bwd", key, {"d_desc_dot": gd, "d_bin_pairs": gb}, "nq%d iters%d g%g %s" % key)               # d_bin_pairs per pair
    for b, (n1, n2) in enumerate(c["pairs"]):
        live = min(n1, n2) > 0
        assert float(gd[b, n1 if live else 0:].abs().sum()) == 0 and float(gd[b, :, n2 if live else 0:].abs().sum()) == 0, b
        if not live or int(M._sel_mask(c, b).sum()) == 0:                                            # an empty pair, a pair with nothing selected
            assert float(gd[b].abs().sum()) == 0 and float(gb[b]) == 0, b
    if key[2] == 0.0 or key[3] == "none_selected":                                                   # g_loss = 0; count = 0
        assert float(gd.abs().sum()) == 0 and float(gb.abs().sum()) == 0


@pytest.mark.parametrize("key", [k for k in M.sink_cases() if k[1] in (3, 200)], ids=str)
def test_twin_and_inference_kernel_agree_within_the_f64_allowance(key, device):
    """nopesac_matcher_sinkhorn (the build each nq routes to) on the twin's inputs: its log scores sit inside the same float64 allowance,
    and `score <= 0` on every selected entry is the decision the twin and the reference make."""
    from nopesac_amd import ops
    got = _twin(key, device)
    c = M.sink_problem(key)
    nq = c["nq"]
    d = [c[n].contiguous().to(device) for n in ("dd", "p1", "p2", "cam7", "n1", "n2", "bin")]
    inf_ls = ops.matcher_sinkhorn(*d, M.OFFSET_MULT, M.NORMAL_MULT, c["iters"], 0.2)[0].cpu()
    ref, A = M.reference("sinkhorn_fwd", key)
    live = ref["log_scores"] > -1e29
    for name, ls in (("twin", got["log_scores"]), ("inference", inf_ls)):
        q = M.ratios(torch.where(live, ls.double(), ref["log_scores"]), ref["log_scores"], A["log_scores"])
        print(name, "nq", nq, "iters", c["iters"], "log_scores error / (limit x A)", float(q.max()) / M.limit("sinkhorn_fwd"))
        assert float(q.max()) <= M.limit("sinkhorn_fwd"), (name, key)
    for b, (n1, n2) in enumerate(c["pairs"]):
        if n1 and n2:
            m = M._sel_mask(c, b)
            sides = [M.live_block(t[b], n1, n2, nq)[m] <= 0 for t in (ref["log_scores"], got["log_scores"], inf_ls)]
            assert torch.equal(sides[0], sides[1]) and torch.equal(sides[0], sides[2]), (key, b)


# ---- embedding loss, descriptor dot ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.EMB_CASES, ids=lambda k: "%s%d" % k)
def test_embedding_loss_against_f64(key, device):
    c = M.emb_inputs(key)
    B = len(c["pairs"])
    ls, gt, n1, n2 = (c[n].contiguous().to(device) for n in ("ls", "gt", "n1", "n2"))

    def run():
        bufs = [_guarded(device, B, 2), _guarded(device, 2)]
        _call("nopesac_matcher_emb_loss", ls, gt, n1, n2, B, c["nq"], bufs[0][1], bufs[1][1])
        assert _tail_untouched(*[b[0] for b in bufs])
        return bufs[0][1], bufs[1][1]
    outs, again = run(), run()
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    got = {"pair_stats": outs[0].cpu(), "loss": outs[1].cpu()}
    assert not any(bool(torch.isnan(v).any()) for v in got.values())
    ref, _ = M.reference("emb_loss", key)
    assert torch.equal(got["pair_stats"][:, 1].double(), ref["pair_stats"][:, 1]) and float(got["loss"][1]) == float(ref["loss"][1])      # counts exactly
    _judge("emb_loss", key, got, "%s %d" % key)


@pytest.mark.parametrize("nq", M.DOT_NQS)
def test_descriptor_dot_backward_against_f64(nq, device):
    c = M.dot_inputs(nq)
    B = len(c["pairs"])
    G, d0, d1, n1, n2 = (c[n].to(device) for n in ("G", "d0", "d1", "n1", "n2"))

    def run():
        bufs = [_guarded(device, B, nq, 256), _guarded(device, B, nq, 256)]
        _call("nopesac_desc_dot_backward", G, d0, d1, n1, n2, B, nq, 256, bufs[0][1], bufs[1][1])
        assert _tail_untouched(*[b[0] for b in bufs])
        return bufs[0][1], bufs[1][1]
    outs, again = run(), run()
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    got = {"dd0": outs[0].cpu(), "dd1": outs[1].cpu()}
    assert not any(bool(torch.isnan(v).any()) for v in got.values())
    _judge("desc_dot", nq, got, "nq%d" % nq)
    for b, (a, s) in enumerate(c["pairs"]):                                                         # rows >= n exactly zero
        assert float(got["dd0"][b, a:].abs().sum()) == 0 and float(got["dd1"][b, s:].abs().sum()) == 0, b
        if a == 0 or s == 0:
            assert float(got["dd0"][b].abs().sum()) == 0 and float(got["dd1"][b].abs().sum()) == 0, b


def test_zz_worst_ratio_per_family_and_output(capsys):
    with capsys.disabled():
        print("\nmatching head backward sweep: worst |kernel - f64| / (limit x (2^-24 S + C)) per family and output")
        for fam, k in sorted(WORST):
            q, case = WORST[(fam, k)]
            print("  %-13s %-12s %.3f  %s   (limit %.3g)" % (fam, k, q, case, M.limit(fam)))
    assert len({f for f, _ in WORST}) == len(M.F32_WORST) and all(q <= 1.0 for q, _ in WORST.values())
