"""GPU half of the encoder-training sweep (tests/plane_encoder_forms.py): ops.linear_backward / nopesac_linear_backward_f32
(csrc/linear_bwd.hip) through the raw library, every element of dx, dW and db against the float64 reference within limit x (2^-24 S + C)
at both split counts of every case.  Outputs and the workspace are NaN-prefilled with a guard tail: every element the header promises
is written, the tail stays; two launches give the same bits.  Then the gates against ops.dropout, column-slice operands, each output
switched off, the argument errors, and the encoder's dropout streams."""
import pytest
import torch

from tests import plane_decoder_forms as D
from tests import plane_encoder_forms as E

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


def _raw(c, device, S, x=None, g=None, y=None, dx=None, want=(True, True, True)):
    """One raw launch on the case's operands (or the given device tensors, which may be column slices) -> (dx, dw, db, guard buffers)."""
    M, K, N, p = c["M"], c["K"], c["N"], c["p"]
    x = c["x"].to(device) if x is None else x
    g = c["g"].to(device) if g is None else g
    if y is None and c["y"] is not None:
        y = c["y"].to(device)
    w = c["w"].to(device)
    bufs = []
    if dx is None and want[0]:
        b, dx = _guarded(device, M, K)
        bufs.append(b)
    dw = db = None
    if want[1]:
        b, dw = _guarded(device, N, K)
        bufs.append(b)
    if want[2]:
        b, db = _guarded(device, N)
        bufs.append(b)
    n_ws = S * (N * K + N)
    wsb, ws = _guarded(device, n_ws)
    bufs.append(wsb)
    _call("nopesac_linear_backward_f32", x if want[1] else None, x.stride(0), w, g, g.stride(0), y, 0 if y is None else y.stride(0), float(p), D.SEED,
          E.LIN_STREAM, dx if want[0] else None, dx.stride(0) if want[0] else 0, dw, db, ws, n_ws, M, K, N, S)
    return (dx if want[0] else None), dw, db, bufs


def _judge(key, got, case):
    w = E.worst_ratio("linear_bwd", key, got)
    lim = E.limit("linear_bwd")
    print("linear_bwd %s: error / (limit x A) %s" % (case, {k: "%.3f" % (q / lim) for k, (q, _) in w.items()}))
    assert all(q <= lim for q, _ in w.values()), (case, w, lim)


@pytest.mark.parametrize("key", E.LIN_CASES, ids=lambda k: "M%d_K%d_N%d_%s_p%g" % k)
def test_linear_backward_against_float64(device, key):
    c = E.lin_inputs(key)
    for S in E.lin_splits(c["M"]):
        dx, dw, db, bufs = _raw(c, device, S)
        assert _tail_untouched(*bufs)
        got = {"dx": dx.cpu(), "dw": dw.cpu(), "db": db.cpu()}
        assert all(bool(torch.isfinite(t).all()) for t in got.values())
        _judge(key, got, (key, S))
        dx2, dw2, db2, _ = _raw(c, device, S)                                   # the same inputs give the same bits
        assert _same_bits(dx, dx2) and _same_bits(dw, dw2) and _same_bits(db, db2)


@pytest.mark.parametrize("key", [(600, 256, 1024, "drop", 0.1), (129, 132, 260, "drop", 0.5), (24, 1024, 256, "both", 0.1)],
                         ids=lambda k: "M%d_K%d_N%d_%s_p%g" % k)
def test_the_dropout_gate_is_ops_dropout_on_the_gradient(device, key):
    """the gated call = the ungated call on ops.dropout(g, ...) (both gates: on the ReLU-gated gradient): bit for bit, and both within the
    allowance"""
    from nopesac_amd import ops
    c = E.lin_inputs(key)
    x, w, g = (c[n].to(device) for n in ("x", "w", "g"))
    y = None if c["y"] is None else c["y"].to(device)
    gated = ops.linear_backward(x, w, g, y=y, p=c["p"], seed=D.SEED, stream=E.LIN_STREAM, splits=3)
    dropped = ops.dropout(g if y is None else ops.relu_backward(g, y), c["p"], D.SEED, E.LIN_STREAM)
    assert torch.equal(dropped != 0, (g != 0) & c["mask"].to(device).bool() & (torch.ones_like(g, dtype=torch.bool) if y is None else y > 0))
    plain = ops.linear_backward(x, w, dropped, splits=3)
    # the same g' reaches the same MFMAs in the same order: the two calls agree bit for bit, not only within the allowance
    assert all(_same_bits(a, b) for a, b in zip(gated, plain))
    _judge(key, dict(zip(("dx", "dw", "db"), (t.cpu() for t in gated))), (key, "gated"))
    _judge(key, dict(zip(("dx", "dw", "db"), (t.cpu() for t in plain))), (key, "ops.dropout"))


@pytest.mark.parametrize("key", [(129, 256, 512, "both", 0.1), (5, 132, 260, "relu", 0.0), (600, 4, 4, "drop", 0.5)], ids=lambda k: "M%d_K%d_N%d_%s_p%g" % k)
def test_column_slices_of_wider_buffers(device, key):
    """x, g, y and dx as column slices (offset 4 floats, wider rows): the results are the dense call's bits, dx's gaps stay untouched"""
    c = E.lin_inputs(key)
    M, K, N = c["M"], c["K"], c["N"]

    def wide(t, cols):
        buf = torch.full((M, cols + 12), NAN, device=device)
        buf[:, 4:4 + cols] = t.to(device)
        return buf[:, 4:4 + cols]
    xs, gs, ys = wide(c["x"], K), wide(c["g"], N), (None if c["y"] is None else wide(c["y"], N))
    dxb = torch.full((M, K + 12), NAN, device=device)
    dx, dw, db, bufs = _raw(c, device, 3, x=xs, g=gs, y=ys, dx=dxb[:, 4:4 + K])
    assert _tail_untouched(*bufs) and bool(torch.isnan(dxb[:, :4]).all()) and bool(torch.isnan(dxb[:, 4 + K:]).all())
    dense = _raw(c, device, 3)
    assert _same_bits(dx, dense[0]) and _same_bits(dw, dense[1]) and _same_bits(db, dense[2])
    _judge(key, {"dx": dx.cpu(), "dw": dw.cpu(), "db": db.cpu()}, (key, "slices"))
    from nopesac_amd import ops
    o = ops.linear_backward(xs, c["w"].to(device), gs, y=ys, p=c["p"], seed=D.SEED, stream=E.LIN_STREAM, splits=3, dx=dxb[:, 4:4 + K])
    assert o[0].data_ptr() == dxb[:, 4:4 + K].data_ptr() and all(_same_bits(a, b) for a, b in zip(o, dense[:3]))


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)])
def test_each_output_can_be_switched_off(device, want):
    from nopesac_amd import ops
    key = (129, 132, 260, "both", 0.1)
    c = E.lin_inputs(key)
    full = _raw(c, device, 3)
    part = _raw(c, device, 3, want=want)
    assert _tail_untouched(*part[3])
    for on, a, b in zip(want, part[:3], full[:3]):
        assert (a is None) if not on else _same_bits(a, b)
    o = ops.linear_backward(c["x"].to(device) if want[1] else None, c["w"].to(device), c["g"].to(device), y=c["y"].to(device), p=c["p"], seed=D.SEED,
                            stream=E.LIN_STREAM, want=want, splits=3)
    for on, a, b in zip(want, o, full[:3]):
        assert (a is None) if not on else _same_bits(a, b)


def test_argument_errors_raise(device):
    from nopesac_amd import ops
    from nopesac_amd._lib import HipKernelError
    M = 8
    x, w, g = torch.ones(M, 8, device=device), torch.ones(8, 8, device=device), torch.ones(M, 8, device=device)
    assert ops.linear_backward(x, w, g)[2].tolist() == [float(M)] * 8
    with pytest.raises(HipKernelError):                                           # K is not a multiple of 4
        ops.linear_backward(torch.ones(M, 6, device=device), torch.ones(8, 6, device=device), g)
    with pytest.raises(HipKernelError):                                           # N is not a multiple of 4
        ops.linear_backward(x, torch.ones(6, 8, device=device), torch.ones(M, 6, device=device))
    with pytest.raises(HipKernelError):                                           # a short workspace
        ops.linear_backward(x, w, g, splits=2, ws=torch.empty(2 * (64 + 8) - 1, device=device))
    for p in (1.0, -0.1, float("nan")):
        with pytest.raises(HipKernelError):
            ops.linear_backward(x, w, g, p=p)
    with pytest.raises(HipKernelError):                                           # a row stride that is no multiple of 4
        ops.linear_backward(x, w, torch.ones(M, 10, device=device)[:, :8])
    with pytest.raises(HipKernelError):
        ops.linear_backward(x, w, g, splits=1025)
    with pytest.raises(ops.OpsArgumentError):
        ops.linear_backward(x, torch.ones(8, 4, device=device), g)                # x does not match w


def test_encoder_streams_and_their_masks(device):
    from nopesac_amd import ops
    for step, layer, site in ((0, 0, 0), (3, 5, 2), (1000, 7, 3)):
        s = ops.encoder_dropout_stream(step, layer, site)
        assert s == E.encoder_dropout_stream(step, layer, site) < 0
        mask = ops.dropout_keep_mask((64, 256), 0.1, D.SEED, s, device=device)
        assert torch.equal(mask.cpu(), D.keep_mask((64, 256), 0.1, D.SEED, s))
        # the decoder's stream of the same (seed, step, layer, site) draws another mask
        assert not torch.equal(mask, ops.dropout_keep_mask((64, 256), 0.1, D.SEED, ops.dropout_stream(step, layer, site), device=device))
