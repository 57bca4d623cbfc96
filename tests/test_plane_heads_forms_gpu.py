"""The two launches of csrc/plane_head_bwd.hip (ops.mask_product_backward) held, element by element, to the float64 VJPs of
tests/plane_heads_forms.py: |kernel - f64| <= limit(family) x A_k over every case; two runs bit-identical; argument errors are refused
before any launch."""
import pytest
import torch

from tests import plane_heads_forms as H

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


def run_kernels(name, device):
    """-> {output: tensor on the CPU}; d_fold / d_beta are written into columns 0..255 / 256 of a sentinel-filled [rows, 264] matrix, as
    the trainer's backward has them, and the columns behind stay sentinels."""
    from nopesac_amd import ops
    L, B, nq, h, w, centre, splits, flags, _ = H.CASES[name]
    x = H.inputs(name)
    dev = lambda t: None if t is None else t.to(device)
    p1 = x["p1"].view(B, h, w, H.C)
    if "slice" in flags:
        wide = torch.full((B, h, w, H.SLICE_WIDTH), 3.0, device=device)
        wide[..., H.SLICE_OFFSET:H.SLICE_OFFSET + H.C] = p1.to(device)
        p1d = wide[..., H.SLICE_OFFSET:H.SLICE_OFFSET + H.C]
        assert not p1d.is_contiguous()
    else:
        p1d = p1.to(device)
    rows = L * B * nq
    gw = torch.full((rows, 264), SENTINEL, device=device)
    r = ops.mask_product_backward(x["dM"].view(L, B, nq, h, w).to(device), x["F"].view(rows, H.C).to(device), p1d,
                                  None if not centre else x["dZ"].view(B, 2, h, w).to(device), dev(x["wc"]), splits=splits,
                                  d_fold=gw[:, :256], d_beta=gw[:, 256])
    assert bool((gw[:, 257:] == SENTINEL).all()), "wrote behind the bias column"
    out = {"d_fold": gw[:, :256].cpu().view(L, B, nq, H.C), "d_beta": gw[:, 256].cpu().view(L, B, nq), "d_p1": r[2].cpu().view(B, h * w, H.C)}
    if centre:
        out["d_wc"], out["d_bc"] = r[3].cpu(), r[4].cpu()
    assert len(r) == (5 if centre else 3)
    return out


@pytest.mark.parametrize("name", list(H.CASES))
def test_every_element_within_its_allowance_and_deterministic(device, name):
    got = run_kernels(name, device)
    ratios = H.ratios(got, name)
    ref = H.reference(name)
    assert set(got) == set(ref["g"])
    for fam, keys in H.FAMILIES.items():
        for k in keys:
            if k in ratios:
                print("%-26s %-7s worst |err| / A = %.3f  (limit %.2f)" % (name, k, ratios[k], H.limit(fam)))
    for fam, keys in H.FAMILIES.items():
        for k in keys:
            if k in ratios:
                assert ratios[k] <= H.limit(fam), (name, k, ratios[k], H.limit(fam))
    if "zero_rows" in H.CASES[name][7]:                           # rows of exact zeros give exact zeros
        assert float(got["d_fold"][:, :, 1::2].abs().max()) == 0.0 and float(got["d_beta"][:, :, 1::2].abs().max()) == 0.0
    again = run_kernels(name, device)
    for k, v in got.items():
        assert torch.equal(v, again[k]), (name, k)


def test_single_launches_give_the_same_bits(device):
    from nopesac_amd import ops
    name = "q21_6x8_b3"
    L, B, nq, h, w = H.CASES[name][:5]
    x = H.inputs(name)
    a = [x["dM"].view(L, B, nq, h, w).to(device), x["F"].to(device), x["p1"].view(B, h, w, H.C).to(device), x["dZ"].view(B, 2, h, w).to(device),
         x["wc"].to(device)]
    both = ops.mask_product_backward(*a)
    wg = ops.mask_product_backward(*a, which="wgrad")
    dg = ops.mask_product_backward(*a, which="dgrad")
    assert wg[2] is None and dg[0] is None and dg[1] is None and dg[3] is None
    for i in (0, 1, 3, 4):
        assert torch.equal(both[i], wg[i])
    assert torch.equal(both[2], dg[2])
    no_centre = ops.mask_product_backward(a[0], a[1], a[2])
    assert len(no_centre) == 3 and torch.equal(no_centre[0], both[0]) and torch.equal(no_centre[1], both[1])


def test_argument_errors_are_refused_before_any_launch(device):
    """C != 256, nq outside 1..128, L outside 1..3, a workspace that is too small, a null pointer and a non-dense p1: NPS_E_ARG from the
    entry points themselves, every output still holding its sentinel."""
    from nopesac_amd import _lib, ops
    lib = ops._L()
    L, B, nq, h, w, C = 2, 2, 7, 6, 8, 256
    hw = h * w
    f = lambda *s: torch.randn(*s, device=device)
    dM, dZ, p1, F, wc = f(L, B, nq, hw), f(B, 2, hw), f(B, hw, C), f(L * B * nq, C), f(2, C)
    outs = {k: torch.full(s, SENTINEL, device=device) for k, s in (("d_fold", (L * B * nq, C)), ("d_beta", (L * B * nq,)), ("d_wc", (2, C)),
                                                                   ("d_bc", (2,)), ("d_p1", (B, hw, C)))}
    S = 2
    n_ws = ops.mask_product_workspace_floats(L, B, nq, 2, S)
    assert n_ws == S * B * (L * nq + 2) * 257
    ws = torch.full((n_ws,), SENTINEL, device=device)
    p = lambda t: None if t is None else t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def wgrad(dM=dM, dZ=dZ, p1=p1, d_fold=outs["d_fold"], d_wc=outs["d_wc"], ws_floats=n_ws, L=L, nq=nq, C=C, ps=C, bs=hw * C, S=S):
        return lib.nopesac_mask_product_wgrad_f32(p(dM), p(dZ), p(p1), p(d_fold), C, p(outs["d_beta"]), 1, p(d_wc), p(outs["d_bc"]), p(ws), ws_floats,
                                                  L, B, nq, h, w, C, ps, bs, S, stream)

    def dgrad(dM=dM, dZ=dZ, F=F, wc=wc, d_p1=outs["d_p1"], L=L, nq=nq, C=C, ps=C, bs=hw * C, ld=C):
        return lib.nopesac_mask_product_dgrad_f32(p(dM), p(dZ), p(F), ld, p(wc), p(d_p1), L, B, nq, h, w, C, ps, bs, stream)

    E = _lib.H.NPS_E_ARG
    bad = [wgrad(C=128), wgrad(nq=0), wgrad(nq=129), wgrad(L=0), wgrad(L=4), wgrad(ws_floats=n_ws - 1), wgrad(dM=None), wgrad(p1=None),
           wgrad(d_fold=None), wgrad(d_wc=None), wgrad(bs=hw * C + 4), wgrad(ps=C - 4), wgrad(ps=C + 2, bs=hw * (C + 2)), wgrad(S=0), wgrad(S=1025),
           dgrad(C=128), dgrad(nq=0), dgrad(nq=129), dgrad(L=0), dgrad(L=4), dgrad(dM=None), dgrad(F=None), dgrad(d_p1=None), dgrad(wc=None),
           dgrad(bs=hw * C + 4), dgrad(ps=C - 4), dgrad(ld=C + 2)]
    assert bad == [E] * len(bad), bad
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + [("ws", ws)]:
        assert bool((t == SENTINEL).all()), k
    # ... and through the checked wrapper: the same refusals raise
    d5 = dM.view(L, B, nq, h, w)
    with pytest.raises(_lib.HipKernelError):
        ops.mask_product_backward(d5, f(L * B * nq, 128), f(B, h, w, 128))
    with pytest.raises((_lib.HipKernelError, ops.OpsArgumentError)):
        ops.mask_product_backward(d5, F, f(B, h + 1, w, C)[:, :h])                # rows of another image between the images
    with pytest.raises(ops.OpsArgumentError):
        ops.mask_product_backward(d5, F, p1.view(B, h, w, C), dZ.view(B, 2, h, w), None)
    with pytest.raises(_lib.HipKernelError):
        ops.mask_product_backward(d5, F, p1.view(B, h, w, C), splits=2000)
    assert wgrad() == 0 and dgrad() == 0                                           # the same arguments, unspoilt, are taken
    torch.cuda.synchronize()
    assert not bool((outs["d_p1"] == SENTINEL).any()) and not bool((outs["d_fold"] == SENTINEL).any())
