"""GPU half of the fused sweep: the fused stem (all three entry points), the pose-net branch tail, the chained MLP kernel and the fused mask
head (both plane builds, every flag of the entry point) at the smallest shapes that reach each path of their tile arithmetic and once at
the workload's size - each against a float64 reference with a per-element error bound (tests/fused_forms.py), every element compared.  The
CPU half shows that correct f32 arithmetic reaches the bound and that one planted error per kernel feature does not."""
import pytest
import torch

from tests import fused_forms as FF

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = {}           # family -> (worst ratio, case)


def _note(fam, q, case):
    if q > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (q, case)


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------------------- stem
_stem_id = lambda c: "%dx%d_B%d_%s%s" % (c[0], c[1], c[2], "pos" if c[3] > 0 else "neg", "_frac" if c[4] else "")


@pytest.mark.parametrize("case", FF.stem_cases(), ids=_stem_id)
def test_stem_builds_against_f64(case, device):
    """ops.preprocess + ops.stem_fused (build 0, judged on the bf16 image preprocess wrote), ops.stem_fused_raw (build 1) and
    ops.stem_fused_raw_shifted (build 2, operands from ops.fold_stem_normalisation) on the same pixels; builds 0 and 1 give the same bits."""
    from nopesac_amd import ops
    c = FF.stem_case(*case)
    d = lambda t: t.to(device)
    raw, mean, std, scale = d(c.raw), d(c.mean), d(c.std), d(c.scale)
    x4 = ops.preprocess(raw, mean, std, 4, BF)
    ys = {0: ops.stem_fused(x4, d(c.w224), scale, d(c.bias)),
          1: ops.stem_fused_raw(raw, mean, std, d(c.w224), scale, d(c.bias)),
          2: ops.stem_fused_raw_shifted(raw, d(c.pad3), d(c.w224f), scale, d(c.biasf))}
    again = ops.stem_fused_raw_shifted(raw, d(c.pad3), d(c.w224f), scale, d(c.biasf))
    torch.cuda.synchronize()
    CH, CW, PH, PW = FF.stem_dims(case[0], case[1])
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), "preprocess + stem_fused differs from stem_fused_raw"
    assert torch.equal(ys[2].view(torch.int16), again.view(torch.int16)), "repeat"
    for build, y in ys.items():
        assert y.shape == (case[2], PH, PW, 64)
        ref = FF.stem_reference(c, build, x4=x4.cpu() if build == 0 else None)
        q = FF.stem_ratio(y, ref)
        print("stem build %d %-18s worst / tol %.3f" % (build, _stem_id(case), q))
        _note("stem build %d" % build, q, _stem_id(case))
        assert q <= 1.0, (build, q)


# ---------------------------------------------------------------------------------------------------------------------------- pose-net
@pytest.mark.parametrize("case", FF.PB_CASES + FF.PB_ISO_CASES, ids=lambda c: "B%d_%s" % c)
def test_posenet_branch_tail_against_f64(case, device):
    """The whole tail on random and border-only inputs, and one layer at a time (the other four layers exact pass-throughs: that layer's
    own 2^-20 A plus one rounding point, on the near, far and mixed routings of its output pixels)."""
    from nopesac_amd import ops
    from nopesac_amd.modeling.params import ConvW
    c = FF.pb_case(*case)
    convs = [[ConvW(c.w[br][i].float().to(device), c.scale[br][i].to(device), c.bias[br][i].to(device)) for i in range(5)] for br in range(2)]
    packed = ops.PoseBranchTail(convs[0], convs[1])
    xs = [c.x[br].to(device) for br in range(2)]
    ys = ops.posenet_branch_tail(xs[0], xs[1], packed)
    ys2 = ops.posenet_branch_tail(xs[0], xs[1], packed)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys, ys2)), "repeat"
    assert all(y.shape == (case[0], 2, 3, 128) and y.dtype == torch.float32 for y in ys)
    q = FF.pb_ratio(ys, FF.pb_forward(c))
    print("pose-net branch tail B%d_%-7s worst / tol %.3f" % (case + (q,)))
    _note("pose-net branch tail" + (", one layer" if case in FF.PB_ISO_CASES else ""), q, "B%d_%s" % case)
    assert q <= 1.0, q


# ---------------------------------------------------------------------------------------------------------------------------- MLP chain
@pytest.mark.parametrize("name", sorted(FF.MLP_CASES))
def test_mlp_chain_against_f64(name, device):
    """Taps go into column slices of NaN-filled buffers with spare rows: nothing outside a slice may be written."""
    from nopesac_amd import ops
    c = FF.mlp_case(name)
    x = c.xbuf.to(device)[:, c.x_off:c.x_off + c.kx]
    xb = None if c.xb is None else c.xb.to(device)
    layers = [ops.MlpLayer(w.to(device), None if b is None else b.to(device)) for w, b in zip(c.w, c.b)]
    acts = [getattr(ops, "ACT_" + l[1].upper()) for l in c.layers]
    restarts = [l[3] for l in c.layers]

    def run():
        bufs = FF.mlp_buffers(c, device)
        ops.mlp_chain(x, layers, acts, [None if t is None else t[1] for t in bufs], x_bcast=xb, rows_per=c.rows_per,
                      restarts=restarts if any(restarts) else None)
        return bufs
    bufs, bufs2 = run(), run()
    torch.cuda.synchronize()
    for t, t2 in zip(bufs, bufs2):
        assert t is None or torch.equal(t[0].view(torch.int32), t2[0].view(torch.int32)), "repeat"
    q, per = FF.mlp_ratio(c, bufs)
    print("mlp chain %-22s worst / tol %.3f  per tap %s" % (name, q, " ".join("%d:%.3f" % p for p in per)))
    _note("mlp chain", q, name)
    assert q <= 1.0, (name, per)


# ---------------------------------------------------------------------------------------------------------------------------- mask head
_mh_id = lambda c: "B%d_%dx%d_nq%d" % c


@pytest.mark.parametrize("case", FF.MH_CASES, ids=_mh_id)
def test_mask_head_against_f64(case, device):
    """Every flag of the entry point on one set of inputs: probabilities, logits with p1, the planar layout (the same values), the
    per-pixel bilinear form, the persistent pipelined form (the dispatch falls back to the default kernel where W % 4 != 0) and the
    operands straight from the folded plane embeddings."""
    from nopesac_amd import ops
    B, H, W, nq = case
    c = FF.mh_case(*case)
    ref = FF.mh_reference(c)
    d = lambda t: t.to(device)
    args = (d(c.c1), d(c.t1), ops.mfma_fragment_major(d(c.wl)), d(c.sc), d(c.bi))
    mw, mb, fold = d(c.mask_w), d(c.mask_b), d(c.fold)
    prob = ops.mask_head(*args, mw, mb)
    logit, p1 = ops.mask_head(*args, mw, mb, sigmoid=False, want_p1=True)
    planar = ops.mask_head(*args, mw, mb, planar=True)
    planar_logit, planar_p1 = ops.mask_head(*args, mw, mb, sigmoid=False, planar=True, want_p1=True)
    taps_prob, taps_p1 = ops.mask_head(*args, mw, mb, taps1=True, want_p1=True)
    pipe_prob, pipe_p1 = ops.mask_head(*args, mw, mb, pipe=True, want_p1=True)
    pipe_logit = ops.mask_head(*args, mw, mb, sigmoid=False, pipe=True)
    fold_prob = ops.mask_head(*args, None, None, fold=fold)
    fold_logit, fold_p1 = ops.mask_head(*args, None, None, sigmoid=False, want_p1=True, fold=fold)
    torch.cuda.synchronize()
    assert prob.shape == (B, H, W, nq) and planar.shape == (B, nq, H, W) and p1.shape == (B, H, W, 256) and p1.dtype == BF
    assert torch.equal(planar.permute(0, 2, 3, 1), prob) and torch.equal(planar_logit.permute(0, 2, 3, 1), logit), "planar holds other values"
    for form, kw in (("default", dict(prob=prob, logit=logit, p1=p1)), ("planar", dict(prob=planar.permute(0, 2, 3, 1), p1=planar_p1)),
                     ("taps1", dict(prob=taps_prob, p1=taps_p1)), ("pipe", dict(prob=pipe_prob, logit=pipe_logit, p1=pipe_p1)),
                     ("fold", dict(prob=fold_prob, logit=fold_logit, p1=fold_p1))):
        for k, t in kw.items():
            q = FF.mh_ratio(ref, **{k: t})
            print("mask head %-7s %-5s %-18s worst / tol %.3f" % (form, k, _mh_id(case), q))
            _note("mask head %s %s (%d planes)" % (form, k, 64 if nq <= 64 else 128), q, _mh_id(case))
            assert q <= 1.0, (form, k, q)
        # the mask GEMM alone, on the p1 this form stored (launches of one form with and without p1 compute the same tile)
        q = FF.mh_own_p1_ratio(c, kw["p1"], **{k: t for k, t in kw.items() if k != "p1"})
        print("mask head %-7s GEMM on own p1 %-12s worst / tol %.3f" % (form, _mh_id(case), q))
        _note("mask head %s GEMM on own p1 (%d planes)" % (form, 64 if nq <= 64 else 128), q, _mh_id(case))
        assert q <= 1.0, (form, "own p1", q)


def test_zz_worst_ratio_per_family(capsys, device):
    with capsys.disabled():
        print("\nfused sweep: worst |kernel - f64| / tolerance per family")
        for fam in sorted(WORST):
            print("  %-36s %.3f  %s" % ((fam,) + WORST[fam]))
    assert WORST and all(q <= 1.0 for q, _ in WORST.values())
