"""GPU half of the two-view training forms (tests/two_view_forms.py): the kernels of csrc/two_view_train.hip through the raw library.
The two backward kernels: every element against the float64 VJP within limit x (2^-24 S + C), exact zeros where the header promises
them, the same bits from two launches, outputs between guard floats that stay untouched.  match_compact / its backward / corr_compact:
bit-equal to the numpy restatement on guarded, unaligned buffers, the three kinds of bad input flagged, and the identity case through
MatchingHeadTrainer.matching_losses."""
import numpy as np
import pytest
import torch

from tests import two_view_forms as T

pytestmark = pytest.mark.gpu
GUARD = 64
DTYPES = {torch.float32: float("nan"), torch.int32: -77, torch.uint8: 0xA5}


def _raw(name, *args):
    from nopesac_amd import ops
    lib = ops._L()
    rc = getattr(lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._stream())
    assert rc == 0, (name, rc, lib.nopesac_last_error())


class Guarded:
    """Output tensors that sit between guard elements (`shift` extra elements in front make the tensor's address unaligned)."""

    def __init__(self, shapes, device, dtypes=None, shift=0):
        self.bufs, self.outs, self.shift = [], [], shift
        for i, s in enumerate(shapes):
            dt = (dtypes or [torch.float32] * len(shapes))[i]
            n = int(torch.Size(s).numel())
            b = torch.full((GUARD + shift + n + GUARD,), DTYPES[dt], device=device, dtype=dt)
            self.bufs.append(b)
            self.outs.append(b[GUARD + shift:GUARD + shift + n].view(*s))

    def check(self, what):
        torch.cuda.synchronize()
        for b, o in zip(self.bufs, self.outs):
            fill = torch.full((1,), DTYPES[b.dtype], dtype=b.dtype, device=b.device)
            for g in (b[:GUARD + self.shift], b[b.numel() - GUARD:]):
                same = torch.isnan(g) if b.dtype == torch.float32 else g == fill
                assert bool(same.all()), what + ": a guard element was written"
            if b.dtype == torch.float32:
                assert not bool(torch.isnan(o).any()), what + ": an element was not written"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, got, case):
    w = T.worst_ratio(family, key, got)
    print("%s %s: error / (limit x A) %s" % (family, case, {k: "%.3f" % (q / T.limit(family)) for k, (q, _) in w.items()}))
    assert all(q <= T.limit(family) for q, _ in w.values()), (case, w, T.limit(family))


@pytest.mark.parametrize("nq", T.NQS)
def test_score_maps_backward_geo_against_f64(nq, device):
    c = T.inputs(nq)
    B = len(c["kinds"])
    d = lambda *ks: [c[k].to(device) for k in ks]
    args = d("geo_local", "rot_raw", "trans_raw", "init_rot", "init_trans", "m") + [B, nq] + d(*T.FAMILIES["score_maps_geo"]["cots"])
    runs = []
    for _ in range(2):
        g = Guarded([(B, nq, 6)], device)
        _raw("nopesac_refine_score_maps_backward_geo", *args, *g.outs)
        g.check("refine_score_maps_backward_geo nq%d" % nq)
        runs.append(g.outs[0])
    assert _same_bits(*runs)
    got = runs[0].cpu()
    _judge("score_maps_geo", nq, {"g_geo_local": got}, "nq%d" % nq)
    z0, _, _ = T.expected_zero(nq)
    assert bool((got[z0] == 0).all()), "rows j >= m (the m = 0 pair included) must be exact zeros"
    assert bool((got[~z0].abs().sum(-1) > 0).all())


@pytest.mark.parametrize("warp_in_ref", T.WARPS)
@pytest.mark.parametrize("nq", T.NQS)
def test_geo_sequence_backward_against_f64(nq, warp_in_ref, device):
    from nopesac_amd import ops
    c = T.inputs(nq)
    B = len(c["kinds"])
    d = lambda *ks: [c[k].to(device) for k in ks]
    fwd = ops.geo_sequence(*d("A", "planes1", "planes2", "n1", "n2", "init_trans", "init_rot"), warp_in_ref=warp_in_ref)
    assert fwd[4].cpu().tolist() == c["m"].tolist()                                        # the forward kernel counts what the restatement counts
    args = d("A", "planes1", "planes2", "n1", "n2", "init_trans", "init_rot") + [B, nq, int(warp_in_ref)] + d("g_geo_local", "g_geo_enc")
    runs = []
    for _ in range(2):
        g = Guarded([(B, nq, 3), (B, nq, 3)], device)
        _raw("nopesac_geo_sequence_backward", *args, *g.outs)
        g.check("geo_sequence_backward nq%d" % nq)
        runs.append(g.outs)
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    got = {"g_planes1": runs[0][0].cpu(), "g_planes2": runs[0][1].cpu()}
    _judge("geo_sequence", (nq, warp_in_ref), got, "nq%d warp%d" % (nq, warp_in_ref))
    _, z1, z2 = T.expected_zero(nq)                            # unmatched planes, planes beyond n1 / n2, rows beyond the cut, the m = 0 pair
    assert bool((got["g_planes1"][z1] == 0).all()) and bool((got["g_planes2"][z2] == 0).all())
    assert bool((got["g_planes1"][~z1].abs().sum(-1) > 0).all()) and bool((got["g_planes2"][~z2].abs().sum(-1) > 0).all())


def _compact(c, device, shift):
    N, nq, _ = c["x"].shape
    nmax = c["match_q"].shape[1]
    g = Guarded([(N, nq, 256), (N, nq, 3), (N, nq), (N, nq), (N,)], device, [torch.float32, torch.float32, torch.int32, torch.int32, torch.int32], shift)
    src = Guarded([(N, nq, 256), (N, nq, 3)], device, shift=shift)                         # the inputs at unaligned addresses as well
    src.outs[0].copy_(torch.from_numpy(c["x"]))
    src.outs[1].copy_(torch.from_numpy(c["params"]))
    _raw("nopesac_match_compact", src.outs[0], src.outs[1], torch.from_numpy(c["match_q"]).to(device), torch.from_numpy(c["n"]).to(device),
         N, nq, nmax, *g.outs)
    g.check("match_compact")
    return [o.cpu().numpy() for o in g.outs]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("nq,nmax", [(2, 2), (50, 20), (50, 50), (128, 50), (128, 128)])
def test_match_compact_and_backward_equal_numpy(nq, nmax, shift, device):
    c = T.compact_case(nq, nmax)
    got = _compact(c, device, shift)
    want = T.match_compact_np(c["x"], c["params"], c["match_q"], c["n"])
    for name, a, b in zip(("x_c", "params_c", "order", "rank", "bad"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    assert not got[4].any()
    # the backward: an exact copy through rank, zero rows for unmatched queries
    N = len(c["n"])
    rng = np.random.default_rng(5)
    g_c = rng.standard_normal((N, nq, 256)).astype(np.float32)
    g = Guarded([(N, nq, 256)], device, shift=shift)
    _raw("nopesac_match_compact_backward", torch.from_numpy(g_c).to(device), torch.from_numpy(got[3]).to(device), N, nq, *g.outs)
    g.check("match_compact_backward")
    want_g = np.zeros_like(g_c)
    for i in range(N):
        for q in range(nq):
            if want[3][i, q] >= 0:
                want_g[i, q] = g_c[i, want[3][i, q]]
    assert np.array_equal(g.outs[0].cpu().numpy().view(np.int32), want_g.view(np.int32))


def test_match_compact_flags_bad_input(device):
    """An index outside [0, nq), a query named twice, n outside [0, min(nq, nmax)]: the flag, n = 0 treatment, untouched guards; the
    good images of the same launch are not affected; the wrapper raises ValueError on request."""
    from nopesac_amd import ops
    nq, nmax = 50, 20
    c = T.compact_case(nq, nmax, orders=("random",))
    base = c["match_q"][2].copy()                                                          # the image with n = nmax
    rows, ns = [base.copy() for _ in range(7)], [nmax] * 7
    rows[0][3] = nq                  # past the end
    rows[1][0] = -1                  # negative inside the live prefix
    rows[2][5] = 1 << 30             # far outside
    rows[3][7] = rows[3][2]          # a query named twice
    ns[4] = nmax + 1                 # n > nmax
    ns[5] = -3                       # n < 0
    g = np.random.default_rng(1)
    c = {"x": g.standard_normal((7, nq, 256)).astype(np.float32), "params": g.standard_normal((7, nq, 3)).astype(np.float32),
         "match_q": np.stack(rows).astype(np.int32), "n": np.array(ns, np.int32)}
    got = _compact(c, device, 0)
    want = T.match_compact_np(c["x"], c["params"], c["match_q"], c["n"])
    assert want[4].tolist() == [1, 1, 1, 1, 1, 1, 0]
    for name, a, b in zip(("x_c", "params_c", "order", "rank", "bad"), got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name
    assert (got[0][:6] == 0).all() and (got[2][:6] == -1).all() and (got[3][:6] == -1).all() and (got[2][6, :nmax] >= 0).all()
    dv = lambda k: torch.from_numpy(c[k]).to(device)
    out = ops.match_compact(dv("x"), dv("params"), dv("match_q"), dv("n"))                # no sync, no raise: the flag comes back
    assert out[4].cpu().tolist() == [1, 1, 1, 1, 1, 1, 0]
    with pytest.raises(ValueError, match="match_compact"):
        ops.match_compact(dv("x"), dv("params"), dv("match_q"), dv("n"), check=True)
    with pytest.raises(ValueError, match="match_compact"):
        ops.match_compact_check(out[4])
    # nq = 128 with n > nq where nmax allows it
    c2 = T.compact_case(2, 2)
    c2["n"][:] = 3
    assert _compact(c2, device, 0)[4].all()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("nq,nmax", [(2, 2), (50, 20), (128, 50)])
def test_corr_compact_equals_numpy(nq, nmax, shift, device):
    c1, c2 = T.compact_case(nq, nmax, seed=1), T.compact_case(nq, nmax, seed=2)
    B = len(c1["n"])
    c2["n"] = c2["n"][::-1].copy()                                                        # every (n1, n2) combination of (0, 1, nmax) occurs
    c2["match_q"] = c2["match_q"][::-1].copy()
    o1, o2 = (T.match_compact_np(c["x"], c["params"], c["match_q"], c["n"])[2] for c in (c1, c2))
    rng = np.random.default_rng(9)
    gt = (rng.random((B, nq + 1, nq + 1)) < 0.3).astype(np.uint8)
    g = Guarded([(B, nq + 1, nq + 1)], device, [torch.uint8], shift)
    src = Guarded([(B, nq + 1, nq + 1)], device, [torch.uint8], shift)
    src.outs[0].copy_(torch.from_numpy(gt))
    dv = lambda a: torch.from_numpy(a).to(device)
    _raw("nopesac_corr_compact", src.outs[0], dv(o1), dv(o2), dv(c1["n"]), dv(c2["n"]), B, nq, *g.outs)
    g.check("corr_compact")
    want = T.corr_compact_np(gt, o1, o2, c1["n"], c2["n"])
    assert np.array_equal(g.outs[0].cpu().numpy(), want) and want.any()
    # order entries that break the contract read nothing out of bounds and give zeros
    bad = np.full_like(o1, 1 << 20)
    g = Guarded([(B, nq + 1, nq + 1)], device, [torch.uint8], shift)
    _raw("nopesac_corr_compact", src.outs[0], dv(bad), dv(o2), dv(np.full(B, nq + 5, np.int32)), dv(c2["n"]), B, nq, *g.outs)
    g.check("corr_compact (bad order)")
    assert np.array_equal(g.outs[0].cpu().numpy(), T.corr_compact_np(gt, bad, o2, np.full(B, nq, np.int32), c2["n"]))


def test_identity_case_through_the_matching_trainer(device, sd50):
    """nq = nmax = 50, every query matched: the compacted call of matching_losses gives bit for bit the loss and the gradient at the queries
    of the uncompacted call on plane_corr_matrix's output."""
    from nopesac_amd import ops
    from nopesac_amd.training import MatchingHeadTrainer, _MatchCompact, plane_corr_matrix
    nq, B = 50, 2
    g = torch.Generator().manual_seed(17)
    mq = torch.stack([torch.randperm(nq, generator=g) for _ in range(2 * B)]).to(torch.int32).to(device)
    n_all = torch.full((2 * B,), nq, dtype=torch.int32, device=device)
    corrs = torch.stack([torch.stack([torch.randperm(nq, generator=g)[:12], torch.randperm(nq, generator=g)[:12]], -1) for _ in range(B)])
    gt = plane_corr_matrix(corrs.to(torch.int32).to(device), mq[:B], mq[B:], nq)
    planes = (torch.nn.functional.normalize(torch.randn(2 * B, nq, 3, generator=g), dim=-1) * (1 + torch.rand(2 * B, nq, 1, generator=g))).to(device)
    cam7 = torch.cat([0.3 * torch.randn(B, 3, generator=g), torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)], 1).to(device)
    app0 = torch.randn(2 * B, nq, 256, generator=g).to(device)
    tr = MatchingHeadTrainer.from_state_dict(sd50, nq, device)
    app = app0.clone().requires_grad_(True)
    loss = tr.matching_losses(app, n_all, cam7, planes[:B], planes[B:], gt, suffix="0", iterations=20)
    grads = tr.backward(loss)
    app2 = app0.clone().requires_grad_(True)
    x_c, p_c, order, rank, bad = _MatchCompact.apply(app2, planes, mq, n_all)
    assert not bool(bad.any()) and torch.equal(order, torch.arange(nq, device=device, dtype=torch.int32).expand(2 * B, nq))
    gt_c = ops.corr_compact(gt, order[:B].contiguous(), order[B:].contiguous(), n_all[:B].contiguous(), n_all[B:].contiguous())
    assert torch.equal(gt_c, gt)
    loss2 = tr.matching_losses(x_c, n_all, cam7, p_c[:B], p_c[B:], gt_c, suffix="0", iterations=20)
    grads2 = tr.backward(loss2)
    assert float(loss["losses_emb_0"].detach()) > 0 and _same_bits(loss["losses_emb_0"].detach().view(1), loss2["losses_emb_0"].detach().view(1))
    assert float(app.grad.abs().max()) > 0 and _same_bits(app.grad, app2.grad) and _same_bits(tr.input_grads["app"], app2.grad)
    assert all(_same_bits(grads[k], grads2[k]) for k in grads)
