"""GPU half of the decoder-training sweep (tests/plane_decoder_forms.py): the kernels of csrc/decoder_train.hip through the raw library,
every element of every output against the float64 reference within limit x (2^-24 S + C).  Outputs are NaN-prefilled with a guard tail
and, on every other case, a padded row stride: every element the header promises is written, the tail and the gaps stay; exact zeros
where the header promises them; two launches give the same bits.  The materialised mask is the integer restatement's, bit for bit, and
the mask the attention kernels apply is the materialised one."""
import math

import pytest
import torch

from tests import plane_decoder_forms as D

pytestmark = pytest.mark.gpu
TAIL = 64
NAN = float("nan")


def _lib():
    from nopesac_amd import _lib
    return _lib, _lib.load()


def _call(name, *args):
    lib, L = _lib()
    lib.check(getattr(L, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream), name)


def _guarded(device, *shape):
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + TAIL,), NAN, device=device, dtype=torch.float32)
    return buf, buf[:n].view(*shape)


def _tail_untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b[-TAIL:]).all()) for b in bufs)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, got, case):
    w = D.worst_ratio(family, key, got)
    lim = D.limit(family)
    print("%s %s: error / (limit x A) %s" % (family, case, {k: "%.3f" % (q / lim) for k, (q, _) in w.items()}))
    assert all(q <= lim for q, _ in w.values()), (case, w, lim)


def _operands(c, device):
    W = c["heads"] * D.HD
    if c["packed"]:
        qkv = c["qkv"].to(device)
        q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
    else:
        q, k, v = (c[n].contiguous().to(device) for n in ("q", "k", "v"))
    assert q.stride(0) == (3 * W if c["packed"] else W)
    ql = kl = None                                                                                      # null pointers
    if not c["null_lens"]:
        ql, kl = (torch.tensor([p[i] for p in c["lens"]], dtype=torch.int32, device=device) for i in (0, 1))
    return q, k, v, c["dout"].to(device), ql, kl, W


# ---- the mask --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, p, seed, stream", [((3, 5, 7), 0.3, -7, 172), ((2, 8, 50, 300), 0.1, D.SEED, D.ATT_STREAM), ((1 << 20,), 0.5, 1, 0),
                                                    ((64, 64), 0.0, 5, 9), ((100, 2048), 0.1, 2 ** 40 + 3, 2 ** 33 + 5)])
def test_keep_mask_is_the_integer_restatement(device, shape, p, seed, stream):
    from nopesac_amd import ops
    got = ops.dropout_keep_mask(shape, p, seed, stream, device=device)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert torch.equal(got.cpu(), D.keep_mask(shape, p, seed, stream))
    if p == 0.0:
        assert bool(got.all())


def test_keep_rate_and_stream_independence(device):
    from nopesac_amd import ops
    N, p = 1 << 22, 0.1
    a = ops.dropout_keep_mask((N,), p, D.SEED, D.dropout_stream(7, 0, 0), device=device).double()
    b = ops.dropout_keep_mask((N,), p, D.SEED, D.dropout_stream(7, 0, 1), device=device).double()
    assert abs(float(a.mean()) - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / N)
    corr = float(((a - a.mean()) * (b - b.mean())).mean() / (a.std(unbiased=False) * b.std(unbiased=False)))
    assert abs(corr) < 6 / math.sqrt(N)


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_a_rate_outside_the_unit_interval_raises(device, p):
    from nopesac_amd import ops
    from nopesac_amd._lib import HipKernelError
    x = torch.ones(4, 256, device=device)
    q = torch.ones(4, 32, device=device)
    with pytest.raises(HipKernelError):
        ops.dropout_keep_mask((4,), p, 0, 0, device=device)
    with pytest.raises(HipKernelError):
        ops.dropout(x, p, 0, 0)
    with pytest.raises(HipKernelError):
        ops.attention_train(q, q, q, 1, 4, 4, 1, 1.0, p=p)
    with pytest.raises(HipKernelError):
        ops.attention_train_backward(q, q, q, q, 1, 4, 4, 1, 1.0, p=p)


@pytest.mark.parametrize("Lq, Lk, p", [(50, 300, 0.1), (131, 131, 0.5), (7, 129, 0.1)])
def test_the_attention_kernels_apply_the_materialised_mask(device, Lq, Lk, p):
    """uniform scores (q = 0) and V = identity columns reveal the mask: with the 32 keys of one window owning one column each and every
    other key's values zero, O[b, i, h, d] = keep[b, h, i, j0 + d] / (Lk (1 - p)) - the zeros of O are the zeros of the mask, exactly."""
    from nopesac_amd import ops
    B, H = 2, 3
    W = H * 32
    seed, stream = D.SEED, D.dropout_stream(1, 2, 2)
    mask = ops.dropout_keep_mask((B, H, Lq, Lk), p, seed, stream, device=device)
    q = torch.zeros(B * Lq, W, device=device)
    k = torch.randn(B * Lk, W, device=device)
    # forward: one window of 32 keys at a time gets the identity as its values, every other key zero: O's zeros are that window's mask zeros
    for j0 in range(0, Lk, 32):
        n = min(32, Lk - j0)
        v = torch.zeros(B, Lk, H, 32, device=device)
        v[:, j0:j0 + n] = torch.eye(32, device=device)[:n].view(1, n, 1, 32)
        o = ops.attention_train(q, k, v.view(B * Lk, W), B, Lq, Lk, H, 32 ** -0.5, p=p, seed=seed, stream=stream).view(B, Lq, H, 32)
        got = (o[..., :n] != 0).permute(0, 2, 1, 3)                                                     # [B, H, Lq, n]
        assert torch.equal(got, mask[..., j0:j0 + n] != 0), j0
        assert float(o[..., n:].abs().sum()) == 0
    # backward: with d_out = e_0 on every row and v_j = (1, 0, ...), dv_j[0] = sum_i keep_ij P_ij / (1 - p): a key column whose mask is
    # all zero over the queries gets exactly 0, any other a positive value; and with d_out = e_0 on ONE row the zeros of dv[:, 0] are that row's mask
    v = torch.zeros(B * Lk, W, device=device)
    for i in (0, Lq - 1):
        g = torch.zeros(B, Lq, H, 32, device=device)
        g[:, i, :, 0] = 1.0
        _, _, dv = ops.attention_train_backward(q, k, v, g.view(B * Lq, W), B, Lq, Lk, H, 32 ** -0.5, p=p, seed=seed, stream=stream)
        got = (dv.view(B, Lk, H, 32)[..., 0] != 0).permute(0, 2, 1)                                     # [B, H, Lk]
        assert torch.equal(got, mask[:, :, i, :] != 0), i


# ---- attention -------------------------------------------------------------------------------------------------------------------------
_ids = lambda k: "%dx%d_%s_p%g" % k


@pytest.mark.parametrize("key", D.ATT_CASES, ids=_ids)
def test_attention_forward_against_f64(key, device):
    c = D.attention_inputs(key)
    B, Lq, Lk, H = c["B"], c["Lq"], c["Lk"], c["heads"]
    q, k, v, _, ql, kl, W = _operands(c, device)
    ld = W + c["out_pad"]

    def run():
        buf, o = _guarded(device, B * Lq, ld)
        _call("nopesac_attention_train_forward", q, q.stride(0), k, k.stride(0), v, v.stride(0), o, ld, B, Lq, Lk, H, c["scale"], ql, kl,
              float(c["p"]), D.SEED, D.ATT_STREAM)
        assert _tail_untouched(buf), "wrote past the end of the output"
        return o
    o, again = run(), run()
    assert _same_bits(o[:, :W], again[:, :W])
    assert bool(torch.isnan(o[:, W:]).all()), "the gap of the padded row stride was written"
    got = {"o": o[:, :W].cpu()}
    assert not bool(torch.isnan(got["o"]).any()), "an element was not written"
    _judge("attention_fwd", key, got, _ids(key))
    for b, (a, s) in enumerate(c["lens"]):                                                              # exact zeros beyond the lengths
        assert float(got["o"][b * Lq + (a if s else 0):(b + 1) * Lq].abs().sum()) == 0, b
    if c["p"] == 0.0 and max(Lq, Lk) <= 128:                                                            # the small kernel on the same reference
        buf, o2 = _guarded(device, B * Lq, ld)
        _call("nopesac_attention_small", q, q.stride(0), k, k.stride(0), v, v.stride(0), o2, ld, B, Lq, Lk, H, c["scale"], ql, kl)
        _judge("attention_fwd", key, {"o": o2[:, :W].cpu()}, _ids(key) + " (attention_small)")


@pytest.mark.parametrize("key", D.ATT_CASES, ids=_ids)
def test_attention_backward_against_f64(key, device):
    lib, _ = _lib()
    c = D.attention_inputs(key)
    B, Lq, Lk, H = c["B"], c["Lq"], c["Lk"], c["heads"]
    q, k, v, dout, ql, kl, W = _operands(c, device)
    ld = W + c["out_pad"]
    ws_floats = lib.H.NPS_ATT_TRAIN_WS_ROW_FLOATS * B * H * Lq                                          # NPS_ATT_TRAIN_BACKWARD_WORKSPACE_FLOATS

    def run(entry="nopesac_attention_train_backward"):
        bufs = [_guarded(device, B * n, ld) for n in (Lq, Lk, Lk)]
        (dq, dk, dv) = (b[1] for b in bufs)
        if entry == "nopesac_attention_train_backward":
            wsb, ws = _guarded(device, ws_floats)
            _call(entry, q, q.stride(0), k, k.stride(0), v, v.stride(0), dout, W, B, Lq, Lk, H, c["scale"], ql, kl, float(c["p"]), D.SEED,
                  D.ATT_STREAM, dq, ld, dk, ld, dv, ld, ws, ws_floats)
            bufs.append((wsb, ws))
        else:
            _call(entry, q, q.stride(0), k, k.stride(0), v, v.stride(0), dout, W, B, Lq, Lk, H, c["scale"], ql, kl, dq, ld, dk, ld, dv, ld)
        assert _tail_untouched(*[b[0] for b in bufs]), "wrote past the end of an output or of the workspace"
        return dq, dk, dv

    def collect(outs):
        got = {}
        for n, o in zip(("dq", "dk", "dv"), outs):
            assert bool(torch.isnan(o[:, W:]).all()), (n, "the gap of the padded row stride was written")
            got[n] = o[:, :W].cpu()
            assert not bool(torch.isnan(got[n]).any()), (n, "an element was not written")
        return got
    outs, again = run(), run()
    assert all(_same_bits(a[:, :W], b[:, :W]) for a, b in zip(outs, again))
    got = collect(outs)
    _judge("attention_bwd", key, got, _ids(key))
    for b, (a, s) in enumerate(c["lens"]):                                                              # exact zeros beyond the lengths, and for an empty side
        assert float(got["dq"][b * Lq + (a if s else 0):(b + 1) * Lq].abs().sum()) == 0, b
        for n in ("dk", "dv"):
            assert float(got[n][b * Lk + (s if a else 0):(b + 1) * Lk].abs().sum()) == 0, (n, b)
    if c["p"] == 0.0 and max(Lq, Lk) <= 128:                                                            # the small kernel, held to the same reference
        _judge("attention_bwd", key, collect(run("nopesac_attention_small_backward")), _ids(key) + " (attention_small_backward)")


def test_the_wrappers_take_the_forward_and_backward_through_column_slices(device):
    """ops.attention_train / _backward on q | k | v slices of one matrix and `out` slices of another: the raw entry points' results"""
    from nopesac_amd import ops
    key = (50, 50, "ragged", 0.0)
    c = D.attention_inputs(key)
    q, k, v, dout, ql, kl, W = _operands(c, device)
    B, L, H = c["B"], c["Lq"], c["heads"]
    o = ops.attention_train(q, k, v, B, L, L, H, c["scale"], ql, kl)
    _judge("attention_fwd", key, {"o": o.cpu()}, "wrapper")
    packed = torch.full((B * L, 3 * W), NAN, device=device)
    ops.attention_train_backward(q, k, v, dout, B, L, L, H, c["scale"], ql, kl, out=(packed[:, :W], packed[:, W:2 * W], packed[:, 2 * W:]))
    _judge("attention_bwd", key, {"dq": packed[:, :W].cpu(), "dk": packed[:, W:2 * W].cpu(), "dv": packed[:, 2 * W:].cpu()}, "wrapper")


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", D.DROP_CASES, ids=lambda k: "%dx%d_p%g_%s" % (k[0], k[1], k[2], "res" if k[3] else "plain"))
def test_dropout_against_f64(key, device):
    from nopesac_amd import ops
    c = D.dropout_inputs(key)
    rows, Dm, p = c["rows"], c["D"], c["p"]
    x = c["x"].to(device)
    r = None if c["residual"] is None else c["residual"].to(device)
    buf, y = _guarded(device, rows, Dm)
    _call("nopesac_dropout_f32", x, r, y, rows * Dm, float(p), D.SEED, D.DROP_STREAM)
    assert _tail_untouched(buf)
    got = y.cpu()
    _judge("dropout", key, {"y": got}, str(key))
    if r is None:
        assert torch.equal(got == 0, (c["mask"] == 0) | (c["x"] == 0))                                  # dropped elements are exact zeros
        if p == 0.0:
            assert torch.equal(got, c["x"])
    w = ops.dropout(x, p, D.SEED, D.DROP_STREAM, residual=r)
    assert _same_bits(w, y)
