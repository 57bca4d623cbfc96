"""GPU half of the pyramid-training sweep (tests/plane_pyramid_forms.py): the kernels of csrc/pyramid_train.hip through the raw library,
every element of every output against the float64 reference within limit x (2^-24 S + C).  Outputs are NaN-prefilled with a guard tail:
every element the header promises is written and the tail stays; two launches give the same bits; the running statistics after one and
after three calls are F.batch_norm's; the adjoint satisfies <up2(x), g> = <x, up2^T(g)> with the forward kernel already in use; the
wrappers of nopesac_amd/ops.py equal the raw entry points bit for bit and refuse what they must
(tests/test_training_wrappers_gpu.py's conventions)."""
import pytest
import torch

from tests import plane_pyramid_forms as P

pytestmark = pytest.mark.gpu
TAIL = 64
NAN = float("nan")


def _lib():
    from nopesac_amd import _lib
    return _lib, _lib.load()


def _rc(name, *args):
    _, L = _lib()
    return getattr(L, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    _lib()[0].check(_rc(name, *args), name)


def _guarded(device, *shape):
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + TAIL,), NAN, device=device, dtype=torch.float32)
    return buf, buf[:n].view(*shape)


def _tail_untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b[-TAIL:]).all()) for b in bufs)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, got):
    w = P.worst_ratio(family, key, got)
    lim = P.limit(family)
    print("%s %s: error / (limit x A) %s" % (family, key, {k: "%.3f" % (q / lim) for k, (q, _) in w.items()}))
    assert all(q <= lim for q, _ in w.values()), (family, key, w, lim)


def _dims(c):
    """(B, H, W) of the entry points for a case (plain: rows as B)."""
    return tuple(c["shape"]) if c["up"] else (c["shape"][0], 1, 1)


def _src(c, device):
    """The source on the device with the case's channel stride (a channel slice of the wider buffer for `slice`)."""
    if c["tag"] == "slice":
        src = c["buf"].to(device)[..., 4:4 + c["C"]]
        assert src.stride(-2) == c["C"] + 8
        return src
    return c["src"].contiguous().to(device)


def _ws(device, c):
    from nopesac_amd import ops
    n = ops.bn_train_workspace_floats(c["n"], c["C"])
    assert n == -(-c["n"] // P.RPS) * 2 * c["C"]
    return _guarded(device, n)


def _stats(device, c, src, run=None):
    """One launch pair of bn_train_stats -> (mean, var, rstd), every buffer guarded."""
    B, H, W = _dims(c)
    C = c["C"]
    bufs, outs = zip(*[_guarded(device, C) for _ in range(3)])
    wsb, ws = _ws(device, c)
    rm, rv = run if run is not None else (None, None)
    _call("nopesac_bn_train_stats_f32", src, int(c["up"]), B, H, W, C, src.stride(-2), P.EPS, P.MOMENTUM, *outs, rm, rv, ws, ws.numel())
    assert _tail_untouched(wsb, *bufs)
    return outs


def _backward(device, c, src, g, gamma, beta, mean, rstd):
    B, H, W = _dims(c)
    C = c["C"]
    db, dsrc = _guarded(device, *c["src"].shape)
    gb, dg = _guarded(device, C)
    bb, dbeta = _guarded(device, C)
    wsb, ws = _ws(device, c)
    _call("nopesac_bn_train_backward_f32", g, src, int(c["up"]), B, H, W, C, src.stride(-2), gamma, beta, mean, rstd, int(c["relu"]),
          int(c["batch_stats"]), dsrc, dg, dbeta, ws, ws.numel())
    assert _tail_untouched(db, gb, bb, wsb)
    return {"dsrc": dsrc, "dgamma": dg, "dbeta": dbeta}


@pytest.mark.parametrize("key", P.BN_CASES, ids=lambda k: "-".join(map(str, k)))
def test_batchnorm_kernels_against_float64(device, key):
    """statistics (and the running buffers after one and three calls), apply and backward of one case, per element"""
    c = P.bn_inputs(key)
    C = c["C"]
    src = _src(c, device)
    gamma, beta, g = (c[k].to(device) for k in ("gamma", "beta", "g"))
    addend = None if c["addend"] is None else c["addend"].to(device)
    if c["batch_stats"]:
        rmb, rm = _guarded(device, C)
        rvb, rv = _guarded(device, C)
        rm.copy_(c["run_mean"]); rv.copy_(c["run_var"])
        running = {}
        for k in range(1, max(P.RUNNING_CALLS) + 1):
            mean, var, rstd = _stats(device, c, src, (rm, rv))
            if k in P.RUNNING_CALLS:
                running["run_mean%d" % k], running["run_var%d" % k] = rm.clone(), rv.clone()
        assert _tail_untouched(rmb, rvb)
        _judge("stats", key, {"mean": mean, "var": var, "rstd": rstd})
        _judge("running", key, running)
        again = _stats(device, c, src)                                          # without running buffers: the same statistics
        assert all(_same_bits(a, b) for a, b in zip(again, (mean, var, rstd)))
    else:
        mean, rstd = c["run_mean"].to(device), torch.rsqrt(c["run_var"].double() + P.EPS).float().to(device)
    B, H, W = _dims(c)
    yb, y = _guarded(device, *c["out_shape"])
    _call("nopesac_bn_train_apply_f32", src, int(c["up"]), B, H, W, C, src.stride(-2), gamma, beta, mean, rstd, int(c["relu"]), addend, y)
    assert _tail_untouched(yb)
    _judge("apply", key, {"y": y})
    got = _backward(device, c, src, g, gamma, beta, mean, rstd)
    _judge("backward", key, got)
    again = _backward(device, c, src, g, gamma, beta, mean, rstd)
    assert all(_same_bits(got[k], again[k]) for k in got), "two backward launches differ"
    if c["tag"] == "gamma0":
        assert float(got["dsrc"][..., ::3].abs().max()) == 0.0


def test_upsampled_form_has_the_forward_kernels_bits(device):
    """v = up2(t) inside the kernels is ops.upsample2x_bilinear(t) bit for bit: with gamma = 1, beta = 0, mean = 0, rstd = 1 and no ReLU
    bn_train_apply writes it out"""
    from nopesac_amd import ops
    for key in (("up", 2, 5, 7, 12, "base"), ("up", 1, 1, 3, 256, "base"), ("up", 2, 3, 4, 256, "slice")):
        c = P.bn_inputs(key)
        src = _src(c, device)
        one, zero = torch.ones(c["C"], device=device), torch.zeros(c["C"], device=device)
        assert _same_bits(ops.bn_train_apply(src, one, zero, zero, one, ops.ACT_NONE, up=True), ops.upsample2x_bilinear(src.contiguous()))


@pytest.mark.parametrize("key", P.ADJ_CASES, ids=lambda k: "-".join(map(str, k)))
def test_bilinear_adjoint_against_float64_and_the_forward_kernel(device, key):
    from nopesac_amd import ops
    c = P.adjoint_inputs(key)
    B, H, W, C = key
    du, x = c["du"].to(device), c["x"].to(device)
    buf, dx = _guarded(device, B, H, W, C)
    _call("nopesac_upsample2x_bilinear_backward_f32", du, dx, B, H, W, C)
    assert _tail_untouched(buf)
    _judge("adjoint", key, {"dx": dx})
    buf2, dx2 = _guarded(device, B, H, W, C)
    _call("nopesac_upsample2x_bilinear_backward_f32", du, dx2, B, H, W, C)
    assert _same_bits(dx, dx2)
    # <up2(x), g> = <x, up2^T(g)> with the forward kernel in use: both sides are sums of B 4HW C products; each side's allowance is
    # limit x (2^-24 sum of the products' magnitudes + the elementwise allowances of its kernel output weighed by the other factor)
    up = ops.upsample2x_bilinear(x)
    lhs, rhs = float((up.double() * du.double()).sum()), float((x.double() * dx.double()).sum())
    _, A = P.reference("adjoint", key)
    S_up = P.up2(c["x"].double().abs())
    allow = P.limit("adjoint") * float(P.EPS24 * (S_up * c["du"].double().abs()).sum() * 2 + (A["dx"] * c["x"].double().abs()).sum())
    print("adjoint identity %s: |lhs - rhs| / allowance %.3f" % (key, abs(lhs - rhs) / allow))
    assert abs(lhs - rhs) <= allow


def test_one_value_per_channel_is_refused(device):
    """rows = 1 (torch refuses it too): NPS_E_ARG from the raw entry point, OpsArgumentError from the wrapper; nothing is written"""
    from nopesac_amd import ops
    lib, _ = _lib()
    src = torch.randn(1, 12, device=device)
    bufs, outs = zip(*[_guarded(device, 12) for _ in range(3)])
    ws = torch.empty(64, device=device)
    rc = _rc("nopesac_bn_train_stats_f32", src, 0, 1, 1, 1, 12, 12, P.EPS, P.MOMENTUM, *outs, None, None, ws, ws.numel())
    assert rc == lib.H.NPS_E_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs)
    with pytest.raises(ops.OpsArgumentError):
        ops.bn_train_stats(src)
    with pytest.raises(ValueError):
        torch.nn.functional.batch_norm(src.cpu(), None, None, training=True)
    # a workspace one float short, one running buffer without the other
    src = torch.randn(300, 12, device=device)
    assert _rc("nopesac_bn_train_stats_f32", src, 0, 300, 1, 1, 12, 12, P.EPS, P.MOMENTUM, *outs, None, None, ws, 2 * 2 * 12 - 1) == lib.H.NPS_E_ARG
    assert _rc("nopesac_bn_train_stats_f32", src, 0, 300, 1, 1, 12, 12, P.EPS, P.MOMENTUM, *outs, outs[0], None, ws, ws.numel()) == lib.H.NPS_E_ARG


def test_channel_quads_are_required(device):
    """a thread works on four channels: C or a channel stride that is no multiple of 4, and a pointer off the 16-byte grid, are refused
    (NPS_E_ARG from the raw entry points, OpsArgumentError from the wrappers)"""
    from nopesac_amd import ops
    lib, _ = _lib()
    E = lib.H.NPS_E_ARG
    buf = torch.randn(300 * 16 + 8, device=device)
    outs = [torch.empty(16, device=device) for _ in range(3)]
    ws = torch.empty(256, device=device)
    stats = lambda src, C, cs: _rc("nopesac_bn_train_stats_f32", src, 0, 300, 1, 1, C, cs, P.EPS, P.MOMENTUM, *outs, None, None, ws, ws.numel())
    assert stats(buf, 12, 12) == 0
    assert stats(buf, 6, 6) == E and stats(buf, 12, 14) == E and stats(buf[1:], 12, 12) == E and stats(buf[4:], 12, 12) == 0
    du, dx = torch.randn(2 * 6 * 8 * 6 + 4, device=device), torch.empty(2 * 3 * 4 * 6 + 4, device=device)
    assert _rc("nopesac_upsample2x_bilinear_backward_f32", du, dx, 2, 3, 4, 6) == E
    assert _rc("nopesac_upsample2x_bilinear_backward_f32", du[1:], dx, 1, 3, 4, 4) == E
    assert _rc("nopesac_upsample2x_bilinear_backward_f32", du, dx, 1, 3, 4, 4) == 0
    torch.cuda.synchronize()
    for bad in (torch.randn(8, 6, device=device), torch.randn(8, 14, device=device)[:, :12], torch.randn(2, 3, 4, 6, device=device)):
        with pytest.raises(ops.OpsArgumentError):
            ops.bn_train_stats(bad)
    with pytest.raises(ops.OpsArgumentError):
        ops.upsample2x_bilinear_backward(torch.randn(1, 4, 4, 6, device=device))


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
WRAP_KEYS = (("plain", P.RPS + 1, 12, "base"), ("up", 2, 3, 4, 256, "slice"), ("plain", P.RPS + 1, 12, "frozen"))


@pytest.mark.parametrize("key", WRAP_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_wrappers_equal_the_raw_entry_points(device, key):
    from nopesac_amd import ops
    c = P.bn_inputs(key)
    C, up = c["C"], c["up"]
    src = _src(c, device)
    gamma, beta, g = (c[k].to(device) for k in ("gamma", "beta", "g"))
    addend = None if c["addend"] is None else c["addend"].to(device)
    act = ops.ACT_RELU if c["relu"] else ops.ACT_NONE
    if c["batch_stats"]:
        rm, rv = c["run_mean"].to(device), c["run_var"].to(device)
        rm2, rv2 = rm.clone(), rv.clone()
        mean, var, rstd = ops.bn_train_stats(src, up=up, eps=P.EPS, momentum=P.MOMENTUM, running_mean=rm, running_var=rv)
        raw = _stats(device, c, src, (rm2, rv2))
        assert all(_same_bits(a, b) for a, b in zip((mean, var, rstd, rm, rv), raw + (rm2, rv2)))
        assert not _same_bits(rm, c["run_mean"].to(device))
    else:
        mean, rstd = c["run_mean"].to(device), torch.rsqrt(c["run_var"].to(device) + P.EPS)
    y = ops.bn_train_apply(src, gamma, beta, mean, rstd, act, addend, up=up)
    B, H, W = _dims(c)
    _, y2 = _guarded(device, *c["out_shape"])
    _call("nopesac_bn_train_apply_f32", src, int(up), B, H, W, C, src.stride(-2), gamma, beta, mean, rstd, int(c["relu"]), addend, y2)
    assert tuple(y.shape) == tuple(c["out_shape"]) and _same_bits(y, y2)
    got = ops.bn_train_backward(g, src, gamma, beta, mean, rstd, act, up=up, batch_stats=c["batch_stats"])
    raw = _backward(device, c, src, g, gamma, beta, mean, rstd)
    assert tuple(got[0].shape) == tuple(c["src"].shape) and all(_same_bits(a, raw[k]) for a, k in zip(got, ("dsrc", "dgamma", "dbeta")))
    if up:
        du = c["g"].to(device)
        _, dx = _guarded(device, *c["src"].shape)
        _call("nopesac_upsample2x_bilinear_backward_f32", du, dx, B, H, W, C)
        assert _same_bits(ops.upsample2x_bilinear_backward(du), dx)


def test_wrappers_refuse_wrong_dtype_strided_and_short_tensors(device):
    from nopesac_amd import ops
    E = ops.OpsArgumentError
    c = P.bn_inputs(("up", 2, 3, 4, 256, "base"))
    t, gamma, beta, g = (c[k].to(device) for k in ("src", "gamma", "beta", "g"))
    mean, var, rstd = ops.bn_train_stats(t, up=True)
    short = lambda v: v.reshape(-1)[:-1]
    for bad in (t.double(), t.cpu(), t.permute(0, 2, 1, 3), t[:, ::2], t[..., ::2]):
        with pytest.raises(E):
            ops.bn_train_stats(bad, up=True)
    with pytest.raises(E):
        ops.bn_train_stats(t.view(-1, 256), up=True)                      # the upsampled form needs the NHWC geometry
    with pytest.raises(E):
        ops.bn_train_stats(t, up=True, running_mean=mean)                 # one running buffer without the other
    with pytest.raises(E):
        ops.bn_train_stats(t, up=True, running_mean=short(mean), running_var=var)
    for args in ((gamma.double(), beta, mean, rstd), (short(gamma), beta, mean, rstd), (gamma, beta[::2], mean, rstd), (gamma, beta, mean, short(rstd)),
                 (gamma, beta, mean.half(), rstd)):
        with pytest.raises(E):
            ops.bn_train_apply(t, *args, ops.ACT_RELU, up=True)
        with pytest.raises(E):
            ops.bn_train_backward(g, t, *args, ops.ACT_RELU, up=True)
    with pytest.raises(E):
        ops.bn_train_apply(t, gamma, beta, mean, rstd, ops.ACT_LEAKY, up=True)
    with pytest.raises(E):
        ops.bn_train_apply(t, gamma, beta, mean, rstd, ops.ACT_RELU, g[:, :-1], up=True)          # an addend one row short
    with pytest.raises(E):
        ops.bn_train_apply(t, gamma, beta, mean, rstd, ops.ACT_RELU, g.double(), up=True)
    for bad in (g.double(), g[:, :-1], g.permute(0, 2, 1, 3), g[..., ::2], up_shape_of(t)):
        with pytest.raises(E):
            ops.bn_train_backward(bad, t, gamma, beta, mean, rstd, ops.ACT_RELU, up=True)
    for bad in (g.double(), g[:, :-1], g.permute(0, 2, 1, 3), g.cpu(), g.reshape(-1)):
        with pytest.raises(E):
            ops.upsample2x_bilinear_backward(bad)


def up_shape_of(t):
    """a cotangent of t's own shape where the upsampled form expects [B, 2H, 2W, C]"""
    return torch.zeros_like(t)
