"""GPU half of the camera head's grouped-BatchNorm sweep (tests/camera_bn_forms.py): the kernels of csrc/camera_bn_train.hip through the
raw library, every element of every output against the float64 reference within limit x (2^-24 S + C).  Every output and the workspace
lie between sentinel floats that stay intact, and every element the header promises is written (the outputs are NaN-prefilled); two
launches give the same bits; the running statistics after one and after three calls are F.batch_norm's over the groups in order; a
G = 2 call has, per group, the bits of G = 1 calls on the halves; the backward's LeakyReLU side is the forward's; the wrappers of
nopesac_amd/ops.py equal the raw entry points bit for bit and refuse what they must."""
import pytest
import torch

from tests import camera_bn_forms as P

pytestmark = pytest.mark.gpu
PAD = 64                                     # sentinel floats on either side (a multiple of 4: the payload stays 16-byte aligned)
NAN = float("nan")
SENTINEL = -7.25


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
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=device, dtype=torch.float32)
    buf[PAD:PAD + n] = NAN
    return buf, buf[PAD:PAD + n].view(*shape)


def _intact(*bufs):
    torch.cuda.synchronize()
    return all(bool((b[:PAD] == SENTINEL).all()) and bool((b[-PAD:] == SENTINEL).all()) for b in bufs)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, got):
    w = P.worst_ratio(family, key, got)
    lim = P.limit(family)
    print("%s %s: error / (limit x A) %s" % (family, key, {k: "%.3f" % (q / lim) for k, (q, _) in w.items()}))
    assert all(q <= lim for q, _ in w.values()), (family, key, w, lim)


def _ws(device, G, n, C):
    from nopesac_amd import ops
    floats = ops.bn_train_grouped_workspace_floats(G, n, C)
    assert floats == G * (-(-n // P.RPS) + 1) * 2 * C
    return _guarded(device, floats)


def _stats(device, src, G, n, C, run=None):
    """One bn_train_grouped_stats call -> (mean, var, rstd) [G, C], every buffer between sentinels."""
    bufs, outs = zip(*[_guarded(device, G, C) for _ in range(3)])
    wsb, ws = _ws(device, G, n, C)
    rm, rv = run if run is not None else (None, None)
    _call("nopesac_bn_train_grouped_stats_f32", src, G, n, C, P.EPS, P.MOMENTUM, *outs, rm, rv, ws, ws.numel())
    assert _intact(wsb, *bufs)
    return outs


def _apply(device, src, G, n, C, gamma, beta, mean, rstd, act):
    yb, y = _guarded(device, G * n, C)
    _call("nopesac_bn_train_grouped_apply_f32", src, G, n, C, gamma, beta, mean, rstd, act, y)
    assert _intact(yb)
    return y


def _backward(device, g, src, G, n, C, gamma, beta, mean, rstd, act, batch_stats=1):
    db, dc = _guarded(device, G * n, C)
    gb, dg = _guarded(device, C)
    bb, dbeta = _guarded(device, C)
    wsb, ws = _ws(device, G, n, C)
    _call("nopesac_bn_train_grouped_backward_f32", g, src, G, n, C, gamma, beta, mean, rstd, act, batch_stats, dc, dg, dbeta, ws, ws.numel())
    assert _intact(db, gb, bb, wsb)
    return {"dc": dc, "dgamma": dg, "dbeta": dbeta}


def _running(device, c, src, G, n, C, calls):
    """The running buffers (between sentinels) after `calls` stats calls from the case's start -> (run_mean, run_var, last statistics)."""
    rmb, rm = _guarded(device, C)
    rvb, rv = _guarded(device, C)
    rm.copy_(c["run_mean"]); rv.copy_(c["run_var"])
    for _ in range(calls):
        st = _stats(device, src, G, n, C, (rm, rv))
    assert _intact(rmb, rvb)
    return rm, rv, st


@pytest.mark.parametrize("key", P.CASES, ids=lambda k: "-".join(map(str, k)))
def test_grouped_batchnorm_kernels_against_float64(device, key):
    """statistics (and the running buffers after one and three calls), apply and backward of one case, per element; with G = 2 the
    groups bit for bit against G = 1 calls on the halves"""
    c = P.bn_inputs(key)
    n, G, C, tag = key
    act = P.ACTS[c["act"]]
    src, gamma, beta, g = (c[k].to(device) for k in ("src", "gamma", "beta", "g"))
    running = {}
    rm1, rv1, _ = _running(device, c, src, G, n, C, 1)
    running["run_mean1"], running["run_var1"] = rm1, rv1
    rm3, rv3, (mean, var, rstd) = _running(device, c, src, G, n, C, 3)
    running["run_mean3"], running["run_var3"] = rm3, rv3
    _judge("stats", key, {"mean": mean, "var": var, "rstd": rstd})
    _judge("running", key, running)
    again = _stats(device, src, G, n, C)                                      # without running buffers: the same statistics
    assert all(_same_bits(a, b) for a, b in zip(again, (mean, var, rstd)))
    y = _apply(device, src, G, n, C, gamma, beta, mean, rstd, act)
    _judge("apply", key, {"y": y})
    got = _backward(device, g, src, G, n, C, gamma, beta, mean, rstd, act)
    _judge("backward", key, got)
    twice = _backward(device, g, src, G, n, C, gamma, beta, mean, rstd, act)
    assert all(_same_bits(got[k], twice[k]) for k in got), "two backward launches differ"
    assert _same_bits(y, _apply(device, src, G, n, C, gamma, beta, mean, rstd, act))
    if tag == "gamma0":
        assert float(got["dc"][:, ::3].abs().max()) == 0.0
    if G == 2:
        # ---- the groups, bit for bit: every per-group result is the G = 1 call's on that half; the running buffers are two G = 1
        # calls in view order; dgamma / dbeta are the f32 sums (group 0 + group 1) of the halves' results
        rmb, rm = _guarded(device, C)
        rvb, rv = _guarded(device, C)
        rm.copy_(c["run_mean"]); rv.copy_(c["run_var"])
        dg, db = [], []
        for grp in range(2):
            half, gh = src[grp * n:(grp + 1) * n], g[grp * n:(grp + 1) * n]
            m1, v1, r1 = _stats(device, half, 1, n, C, (rm, rv))
            assert _same_bits(m1[0], mean[grp]) and _same_bits(v1[0], var[grp]) and _same_bits(r1[0], rstd[grp]), grp
            assert _same_bits(_apply(device, half, 1, n, C, gamma, beta, m1, r1, act), y[grp * n:(grp + 1) * n]), grp
            h = _backward(device, gh, half, 1, n, C, gamma, beta, m1, r1, act)
            assert _same_bits(h["dc"], got["dc"][grp * n:(grp + 1) * n]), grp
            dg.append(h["dgamma"]); db.append(h["dbeta"])
        assert _intact(rmb, rvb) and _same_bits(rm, rm1) and _same_bits(rv, rv1)
        assert _same_bits(dg[0] + dg[1], got["dgamma"]) and _same_bits(db[0] + db[1], got["dbeta"])
        assert not _same_bits(mean[0], mean[1])


@pytest.mark.parametrize("key", [P.TAG_SHAPE + ("leaky",), (6, 1, 128, "leaky"), (2 * P.RPS + 1, 2, 256, "leaky")], ids=lambda k: "-".join(map(str, k)))
def test_the_backwards_leaky_side_is_the_forwards(device, key):
    """gamma = 1, dy = 1 and the statistics passed as constants (batch_stats = 0, rstd = 1): dc is dz / dy itself - exactly 1 where the
    forward's y > 0 and exactly the slope elsewhere, z = 0 included (the mean is a row of the group itself)."""
    n, G, C, _ = key
    c = P.bn_inputs(key)
    src = c["src"].to(device)
    one, zero = torch.ones(C, device=device), torch.zeros(C, device=device)
    mean = src.view(G, n, C)[:, 0].contiguous()                               # the first row of every group: z = 0 there
    rstd = torch.ones(G, C, device=device)
    act = P.ACTS["leaky"]
    y = _apply(device, src, G, n, C, one, zero, mean, rstd, act)
    got = _backward(device, torch.ones_like(src), src, G, n, C, one, zero, mean, rstd, act, batch_stats=0)
    slope = torch.tensor(0.01, dtype=torch.float32, device=device)
    want = torch.where(y > 0, torch.ones_like(y), slope.expand_as(y))
    assert _same_bits(got["dc"], want)
    assert bool((y == 0).any()) and bool((y > 0).any()) and bool((y < 0).any())
    assert torch.isfinite(got["dgamma"]).all() and torch.isfinite(got["dbeta"]).all()


def test_what_the_entry_points_refuse(device):
    """n < 2, C % 4, G < 1, a pointer off the 16-byte grid, a short workspace, one running buffer without the other, an unknown
    activation: NPS_E_ARG and nothing written"""
    lib, _ = _lib()
    E = lib.H.NPS_E_ARG
    buf = torch.randn(600 * 16 + 8, device=device)
    bufs, outs = zip(*[_guarded(device, 2, 16) for _ in range(3)])
    ws = torch.empty(4096, device=device)
    stats = lambda src, G, n, C, rm=None, rv=None, wsn=4096: _rc("nopesac_bn_train_grouped_stats_f32", src, G, n, C, P.EPS, P.MOMENTUM, *outs, rm, rv, ws, wsn)
    assert stats(buf, 2, 1, 16) == E and stats(buf, 1, 1, 16) == E and stats(buf, 0, 300, 16) == E and stats(buf, 2, 300, 6) == E
    assert stats(buf, 2, 300, 14) == E and stats(buf[1:], 2, 300, 16) == E and stats(buf, 2, 300, 16, outs[0][0]) == E
    assert stats(buf, lib.H.NPS_BN_GROUPED_MAX_GROUPS + 1, 2, 16) == E
    need = 2 * 3 * 2 * 16
    assert stats(buf, 2, 300, 16, wsn=need - 1) == E
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b[PAD:-PAD]).all()) for b in bufs)
    assert stats(buf, 2, 300, 16, wsn=need) == 0 and stats(buf[4:], 2, 300, 16) == 0
    v = torch.ones(32, device=device)
    y = torch.empty(600 * 16, device=device)
    apply = lambda act, C=16, m=v: _rc("nopesac_bn_train_grouped_apply_f32", buf, 2, 300, C, v, v, m, v, act, y)
    assert apply(3) == E and apply(-1) == E and apply(2, 6) == E and apply(2, 16, v[1:]) == E and apply(2) == 0 and apply(0) == 0 and apply(1) == 0
    bwd = lambda act, wsn=4096, n=300: _rc("nopesac_bn_train_grouped_backward_f32", y, buf, 2, n, 16, v, v, v, v, act, 1, y.clone(), v.clone(), v.clone(), ws, wsn)
    assert bwd(3) == E and bwd(2, need - 1) == E and bwd(2, need, 0) == E and bwd(2, need) == 0
    torch.cuda.synchronize()


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [P.TAG_SHAPE + ("leaky",), (P.RPS, 1, 4, "leaky"), P.TAG_SHAPE + ("relu",)], ids=lambda k: "-".join(map(str, k)))
def test_wrappers_equal_the_raw_entry_points(device, key):
    from nopesac_amd import ops
    c = P.bn_inputs(key)
    n, G, C, _ = key
    act = P.ACTS[c["act"]]
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY) == (P.ACTS["none"], P.ACTS["relu"], P.ACTS["leaky"])
    src, gamma, beta, g = (c[k].to(device) for k in ("src", "gamma", "beta", "g"))
    rm, rv = c["run_mean"].to(device), c["run_var"].to(device)
    rm2, rv2 = rm.clone(), rv.clone()
    src4 = src.view(G, n, 1, C)                                               # any contiguous [..., C] shape
    mean, var, rstd = ops.bn_train_grouped_stats(src4, G, eps=P.EPS, momentum=P.MOMENTUM, running_mean=rm, running_var=rv)
    raw = _stats(device, src, G, n, C, (rm2, rv2))
    assert tuple(mean.shape) == (G, C) and all(_same_bits(a, b) for a, b in zip((mean, var, rstd, rm, rv), raw + (rm2, rv2)))
    assert not _same_bits(rm, c["run_mean"].to(device))
    y = ops.bn_train_grouped_apply(src4, gamma, beta, mean, rstd, act, G)
    assert tuple(y.shape) == tuple(src4.shape) and _same_bits(y.view(G * n, C), _apply(device, src, G, n, C, gamma, beta, mean, rstd, act))
    got = ops.bn_train_grouped_backward(g.view_as(src4), src4, gamma, beta, mean, rstd, act, G)
    raw = _backward(device, g, src, G, n, C, gamma, beta, mean, rstd, act)
    assert tuple(got[0].shape) == tuple(src4.shape) and all(_same_bits(a.reshape(raw[k].shape), raw[k]) for a, k in zip(got, ("dc", "dgamma", "dbeta")))
    frozen = ops.bn_train_grouped_backward(g, src, gamma, beta, mean, rstd, act, G, batch_stats=False)
    raw = _backward(device, g, src, G, n, C, gamma, beta, mean, rstd, act, batch_stats=0)
    assert all(_same_bits(a, raw[k]) for a, k in zip(frozen, ("dc", "dgamma", "dbeta"))) and not _same_bits(frozen[0], got[0].view(G * n, C))


def test_wrappers_refuse_before_any_launch(device):
    """a row count not divisible by groups, n < 2, C % 4 != 0, a wrong dtype, non-contiguous input, mismatched vector lengths, a CPU
    tensor, an unknown activation"""
    from nopesac_amd import ops
    E = ops.OpsArgumentError
    c = P.bn_inputs(P.TAG_SHAPE + ("leaky",))
    n, G, C, _ = c["key"]
    t, gamma, beta, g = (c[k].to(device) for k in ("src", "gamma", "beta", "g"))
    mean, var, rstd = ops.bn_train_grouped_stats(t, G, eps=P.EPS, momentum=P.MOMENTUM)
    short = lambda v: v.reshape(-1)[:-1]
    kw = dict(eps=P.EPS, momentum=P.MOMENTUM)
    for bad, groups in ((t[:-1], 2), (t[:2], 2), (t[:1], 1), (t[:, :6].contiguous(), 2), (t.double(), 2), (t.cpu(), 2), (t[:, ::2], 2), (t.t(), 2),
                        (t, 0), (t, 3), (t, 2.0), (t.view(-1), 2)):
        with pytest.raises(E):
            ops.bn_train_grouped_stats(bad, groups, **kw)
    with pytest.raises(E):
        ops.bn_train_grouped_stats(t, G, running_mean=mean[0], **kw)                      # one running buffer without the other
    with pytest.raises(E):
        ops.bn_train_grouped_stats(t, G, running_mean=short(mean[0]), running_var=var[0].clone(), **kw)
    with pytest.raises(E):
        ops.bn_train_grouped_stats(t, G, running_mean=mean[0].double(), running_var=var[0].double(), **kw)
    for args in ((gamma.double(), beta, mean, rstd), (short(gamma), beta, mean, rstd), (gamma, beta[::2], mean, rstd), (gamma, beta, mean, short(rstd)),
                 (gamma, beta, mean[0], rstd), (gamma, beta, mean.half(), rstd), (gamma, beta, mean, rstd[:, ::2])):
        with pytest.raises(E):
            ops.bn_train_grouped_apply(t, *args, ops.ACT_LEAKY, G)
        with pytest.raises(E):
            ops.bn_train_grouped_backward(g, t, *args, ops.ACT_LEAKY, G)
    with pytest.raises(E):
        ops.bn_train_grouped_apply(t, gamma, beta, mean, rstd, ops.ACT_SIGMOID, G)
    with pytest.raises(E):
        ops.bn_train_grouped_apply(t, gamma, beta, mean, rstd, ops.ACT_LEAKY, 1)           # [2, C] statistics for one group
    for bad in (g.double(), g[:-1], g.t(), g[:, ::2], g.cpu()):
        with pytest.raises(E):
            ops.bn_train_grouped_backward(bad, t, gamma, beta, mean, rstd, ops.ACT_LEAKY, G)
