"""ops.scratch - the one arena kernel workspaces come from - and the wrappers that draw on it.

  * eager: one buffer per (device, stream), grown and kept; under capture a fresh buffer of the capture's own pool, never cached;
  * every wrapper that takes its partials from the arena gives, with the arena holding the previous op's partials (and NaNs), the bits of
    the same call made through the raw C ABI with a private NaN-prefilled workspace of exactly the size entry's length;
  * a graph that holds layernorm_backward and sumsq_accumulate, captured twice on two streams and both replayed, gives the eager bits.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _raw(name, *args):
    """The entry point `name` of the raw library on the current stream; tensors go in as their device address."""
    from nopesac_amd import ops
    lib = ops._L()
    rc = getattr(lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._stream())
    assert rc == 0, (name, rc, lib.nopesac_last_error())


def _private(dev, entry, *args, unit=1):
    """A private workspace of exactly the size entry's length (`unit` bytes per count: 4 for a *_bytes entry), NaN-prefilled."""
    from nopesac_amd import ops
    n = int(getattr(ops._L(), entry)(*args))
    assert n > 0 and n % unit == 0, (entry, args, n)
    return torch.full((n // unit,), NAN, device=dev)


def _out(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- the arena itself
def test_scratch_is_one_buffer_per_stream_grown_and_kept(device):
    from nopesac_amd import ops
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a, b = ops.scratch(device, 1024), ops.scratch(device, 1024)
        assert a.data_ptr() == b.data_ptr() and a.dtype == torch.float32 and a.numel() * 4 >= 1024 and a.data_ptr() % 16 == 0
        big = ops.scratch(device, 1 << 20)
        small = ops.scratch(device, 1024)
        assert big.numel() * 4 >= 1 << 20 and small.data_ptr() == big.data_ptr()                    # it grew, and is kept
        assert ops.scratch(device, 1 << 20).data_ptr() == big.data_ptr()
        assert ops.scratch(device, 1021).numel() * 4 >= 1021
    with torch.cuda.stream(s2):
        other = ops.scratch(device, 1024)
        assert other.data_ptr() != big.data_ptr()
        lo, hi = big.data_ptr(), big.data_ptr() + (1 << 20)
        assert not (lo <= other.data_ptr() < hi)                                                      # another buffer, not a slice
    torch.cuda.synchronize()


def test_scratch_under_capture_is_fresh_and_never_cached(device):
    from nopesac_amd import ops
    eager = ops.scratch(device, 1024).data_ptr()
    graphs, ptrs = [], []
    for _ in range(2):
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(g, stream=s):
            t = ops.scratch(device, 1024)
            t.zero_()                                      # (a node, so that the capture is not empty)
            ptrs.append(t.data_ptr())
        graphs.append((g, s, t))                           # the graphs, and with them their private pools, stay alive
    assert ptrs[0] != ptrs[1] and eager not in ptrs
    after = [ops.scratch(device, 1024).data_ptr(), ops.scratch(device, 1 << 16).data_ptr()]
    for _, s, _ in graphs:                                 # the capture streams' own arenas hold no capture pointer either
        with torch.cuda.stream(s):
            after.append(ops.scratch(device, 1024).data_ptr())
    assert after[0] == eager and not set(after) & set(ptrs)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- reuse between ops
class _Ops:
    """The ops of the issue's list: `wrapped()` through the ops wrappers (workspace from the arena), `raw()` through the C ABI with a
    private NaN-prefilled workspace of exactly the size entry's length.  Both return the same tuple of output tensors."""

    def __init__(self, dev):
        from nopesac_amd import ops
        self.dev, self.ops = dev, ops
        d = lambda t: t.to(dev)
        self.ln = tuple(d(t) for t in (_rand(1, 33, 256), _rand(2, 256), _rand(3, 33, 256)))
        self.bn = {False: (d(_rand(4, 130, 8)), d(_rand(5, 130, 8))), True: (d(_rand(6, 1, 3, 5, 8)), d(_rand(7, 1, 6, 10, 8)))}
        self.bn_affine = (d(_rand(8, 8)), d(_rand(9, 8)))
        self.lin = (d(_rand(10, 257, 132)), d(_rand(11, 128, 132)), d(_rand(12, 257, 128)))
        self.att = tuple(d(t) for t in (_rand(13, 2 * 5, 64), _rand(14, 2 * 70, 64), _rand(15, 2 * 70, 64), _rand(16, 2 * 5, 64)))
        self.mp = (d(_rand(17, 1, 2, 3, 16, 16)), d(_rand(18, 6, 256)), d(_rand(19, 2, 16, 16, 256)))
        self.gn = (d(_rand(20, 2, 4, 4, 64)), d(_rand(21, 2, 4, 4, 64)), d(_rand(22, 64)), d(_rand(23, 64)))
        self.wg = (d(_rand(24, 2, 8, 8, 4)), d(_rand(25, 2, 8, 8, 8)))
        self.ss = {n: d(_rand(26, n)) for n in (16385, 4096 * 256, 4096 * 256 + 1)}          # 5, 256 and 129 slices

    # ---- layernorm_backward, rows = 33
    def layernorm(self, raw):
        x, gamma, dy = self.ln
        if not raw:
            return self.ops.layernorm_backward(x, gamma, dy, 1e-5)
        dx, dg, db = _out(self.dev, 33, 256), _out(self.dev, 256), _out(self.dev, 256)
        ws = _private(self.dev, "nopesac_layernorm_backward_workspace_floats", 33)
        _raw("nopesac_layernorm_backward", x, gamma, dy, 33, 256, 1e-5, dx, dg, db, ws, ws.numel())
        return dx, dg, db

    # ---- bn_train_stats + bn_train_backward: [130, 8] plain, [1, 3, 5, 8] upsampled
    def _bn(self, raw, up):
        ops, dev = self.ops, self.dev
        src, dy = self.bn[up]
        gamma, beta = self.bn_affine
        if not raw:
            mean, var, rstd = ops.bn_train_stats(src, up=up)
            return (mean, var, rstd) + tuple(ops.bn_train_backward(dy, src, gamma, beta, mean, rstd, ops.ACT_RELU, up=up))
        B, H, W, n = (1, 3, 5, 60) if up else (130, 1, 1, 130)
        mean, var, rstd, dg, db = (_out(dev, 8) for _ in range(5))
        dsrc = _out(dev, *src.shape)
        ws = _private(dev, "nopesac_bn_train_workspace_floats", n, 8)
        _raw("nopesac_bn_train_stats_f32", src, int(up), B, H, W, 8, 8, 1e-5, 0.1, mean, var, rstd, None, None, ws, ws.numel())
        ws = _private(dev, "nopesac_bn_train_workspace_floats", n, 8)
        _raw("nopesac_bn_train_backward_f32", dy, src, int(up), B, H, W, 8, 8, gamma, beta, mean, rstd, ops.ACT_RELU, 1, dsrc, dg, db, ws, ws.numel())
        return mean, var, rstd, dsrc, dg, db

    def bn_plain(self, raw):
        return self._bn(raw, False)

    def bn_up(self, raw):
        return self._bn(raw, True)

    # ---- linear_backward, M = 257, K = 132, N = 128, default splits
    def linear(self, raw):
        ops, dev = self.ops, self.dev
        x, w, g = self.lin
        if not raw:
            return ops.linear_backward(x, w, g)
        M, K, N = 257, 132, 128
        S = ops.linear_backward_splits(M, K, N)
        dx, dw, db = _out(dev, M, K), _out(dev, N, K), _out(dev, N)
        ws = _private(dev, "nopesac_linear_backward_workspace_floats", N, K, S)
        _raw("nopesac_linear_backward_f32", x, K, w, g, N, None, 0, 0.0, 0, 0, dx, K, dw, db, ws, ws.numel(), M, K, N, S)
        return dx, dw, db

    # ---- attention_train_backward, B = 2, Lq = 5, Lk = 70, heads = 2
    def attention(self, raw):
        ops, dev = self.ops, self.dev
        q, k, v, d_out = self.att
        B, Lq, Lk, heads, scale = 2, 5, 70, 2, 1.0 / math.sqrt(32.0)
        if not raw:
            return ops.attention_train_backward(q, k, v, d_out, B, Lq, Lk, heads, scale)
        dq, dk, dv = _out(dev, B * Lq, 64), _out(dev, B * Lk, 64), _out(dev, B * Lk, 64)
        ws = _private(dev, "nopesac_attention_train_backward_workspace_floats", B, heads, Lq)
        _raw("nopesac_attention_train_backward", q, 64, k, 64, v, 64, d_out, 64, B, Lq, Lk, heads, scale, None, None, 0.0, 0, 0, dq, 64, dk, 64,
             dv, 64, ws, ws.numel())
        return dq, dk, dv

    # ---- mask_product_backward's wgrad launch, L = 1, B = 2, nq = 3, 16 x 16
    def mask_product(self, raw):
        ops, dev = self.ops, self.dev
        d_logits, fold, p1 = self.mp
        L, B, nq, h, w, C = 1, 2, 3, 16, 16, 256
        if not raw:
            d_fold, d_beta, _ = ops.mask_product_backward(d_logits, fold, p1, which="wgrad")
            return d_fold.view(L * B * nq, C), d_beta.view(L * B * nq)
        S = ops.mask_product_splits(L, B, nq, h * w, 0)
        d_fold, d_beta = _out(dev, L * B * nq, C), _out(dev, L * B * nq)
        ws = _private(dev, "nopesac_mask_product_wgrad_workspace_floats", L, B, nq, 0, S)
        _raw("nopesac_mask_product_wgrad_f32", d_logits, None, p1, d_fold, C, d_beta, 1, None, None, ws, ws.numel(), L, B, nq, h, w, C, C, h * w * C, S)
        return d_fold, d_beta

    # ---- groupnorm_backward, [2, 4, 4, 64], 32 groups
    def groupnorm_bwd(self, raw):
        ops, dev = self.ops, self.dev
        x, dy, gamma, beta = self.gn
        if not raw:
            return ops.groupnorm_backward(x, dy, gamma, beta, 32, 1e-5)
        dx, dg, db = _out(dev, 2, 4, 4, 64), _out(dev, 64), _out(dev, 64)
        ws = _private(dev, "nopesac_groupnorm_backward_workspace_floats", 2, 64)
        _raw("nopesac_groupnorm_backward_f32", x, dy, gamma, beta, 2, 16, 64, 32, 1e-5, 0, dx, dg, db, ws, ws.numel())
        return dx, dg, db

    # ---- conv2d_wgrad, 3 x 3, Cin = 4, Cout = 8, 8 x 8
    def wgrad(self, raw):
        ops, dev = self.ops, self.dev
        x, dy = self.wg
        if not raw:
            return (ops.conv2d_wgrad(x, dy, 3, pad=1),)
        S = ops.wgrad_splits(2 * 8 * 8, 8, 3 * 3 * 4)
        dw = _out(dev, 8, 4, 3, 3)
        ws = _private(dev, "nopesac_conv2d_wgrad_workspace_bytes", 8, 4, 3, 3, S, unit=4)
        _raw("nopesac_conv2d_wgrad_f32", x, dy, dw, ws, ws.numel() * 4, 2, 8, 8, 4, 8, 3, 3, 1, 1, 4, 8, S)
        return (dw,)

    # ---- sumsq_accumulate, 5 / 256 / 129 slices
    def _sumsq(self, raw, n):
        x = self.ss[n]
        if not raw:
            return (self.ops.sumsq_accumulate(x),)
        acc = torch.zeros(1, device=self.dev)
        ws = _private(self.dev, "nopesac_sumsq_workspace_floats", n)
        _raw("nopesac_sumsq_accumulate_f32", x, n, acc, ws, ws.numel())
        return (acc,)

    def sumsq_5(self, raw):
        return self._sumsq(raw, 16385)

    def sumsq_256(self, raw):
        return self._sumsq(raw, 4096 * 256)

    def sumsq_129(self, raw):
        return self._sumsq(raw, 4096 * 256 + 1)


SEQUENCE = ("layernorm", "bn_plain", "bn_up", "linear", "attention", "mask_product", "groupnorm_bwd", "wgrad", "sumsq_5", "sumsq_256", "sumsq_129")


def test_reuse_does_not_leak_between_ops(device):
    """The sequence twice on one stream through the wrappers: every op inherits the previous op's partials (the first one NaNs) in the
    arena.  A kernel that reads scratch it did not write shows as a NaN or a bit that differs from the private-workspace call."""
    from nopesac_amd import ops
    o = _Ops(device)
    L = ops._L()
    assert [int(L.nopesac_sumsq_workspace_floats(n)) for n in sorted(o.ss)] == [5, 256, 129]
    ref = {name: getattr(o, name)(True) for name in SEQUENCE}
    ops.scratch(device, 1 << 20).fill_(NAN)
    arena = ops.scratch(device, 4).data_ptr()
    got = [{name: getattr(o, name)(False) for name in SEQUENCE} for _ in range(2)]
    assert ops.scratch(device, 4).data_ptr() == arena                        # every op drew on the one buffer (none needs more than 1 MB)
    torch.cuda.synchronize()
    for rnd, outs in enumerate(got):
        for name in SEQUENCE:
            assert len(outs[name]) == len(ref[name])
            for i, (a, b) in enumerate(zip(outs[name], ref[name])):
                assert bool(torch.isfinite(b).all()), (name, i)
                assert _same_bits(a, b), (rnd, name, i, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- captured replay
def test_captured_replay_equals_eager(device):
    """layernorm_backward (rows = 33) then sumsq_accumulate (n = 16385: the two-stage form) in one graph, captured twice on two streams,
    both replayed: the eager bits.  (The sum of squares used to allocate inside the library and could not be captured.)"""
    from nopesac_amd import ops
    o = _Ops(device)
    x = o.ss[16385]

    def body():
        return tuple(ops.layernorm_backward(*o.ln, 1e-5)) + (ops.sumsq_accumulate(x),)
    eager = body()
    torch.cuda.synchronize()
    caps = []
    for _ in range(2):
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(g, stream=s):
            outs = body()
        caps.append((g, s, outs))
    for g, s, _ in caps:                                   # each on its own stream: the two replays are in flight together
        with torch.cuda.stream(s):
            g.replay()
    torch.cuda.synchronize()
    for _, _, outs in caps:
        for i, (a, b) in enumerate(zip(outs, eager)):
            assert _same_bits(a, b), i


# ---------------------------------------------------------------------------------------------------------------- forward users
def _dirty_arena(device):
    """A larger scratch user on this stream first: the arena is 1 MB of NaNs under the Linear backward's partials."""
    from nopesac_amd import ops
    ops.scratch(device, 1 << 20).fill_(NAN)
    ops.linear_backward(_rand(30, 257, 132).to(device), _rand(31, 128, 132).to(device), _rand(32, 257, 128).to(device))


def test_p8n_split_k_from_a_used_arena(device, monkeypatch):
    """ops.conv2d routed to the split-K form (one 63-row tile, 8 slices of Cin = 512) after a larger scratch user, against the raw call
    with a private NaN-prefilled workspace of the size entry's length."""
    from nopesac_amd import ops
    B, H, W, Cin, Cout = 1, 9, 7, 512, 128
    x = _rand(33, B, H, W, Cin).to(device, torch.bfloat16)
    w = (_rand(34, Cout, 3, 3, Cin) / math.sqrt(9 * Cin)).to(device, torch.bfloat16)
    asked = []
    real = ops.scratch
    monkeypatch.setattr(ops, "scratch", lambda dev, nbytes: asked.append(nbytes) or real(dev, nbytes))
    monkeypatch.setattr(ops.TUNER, "measuring", True)
    monkeypatch.setattr(ops.TUNER, "choose", lambda key, launch, extra=(): ops.CFG_P8N_SPLIT if ops.CFG_P8N_SPLIT in extra else 0)
    _dirty_arena(device)
    del asked[:]
    y = ops.conv2d(x, w, None, None, pad=1)
    assert ops.LAST_CONV_CFG[0] == ops.CFG_P8N_SPLIT and len(asked) == 1
    splits, rest = divmod(asked[0], B * H * W * Cout * 4)
    assert rest == 0 and 2 <= splits <= Cin // 64
    ref = torch.full_like(y, NAN)
    ws = _private(device, "nopesac_conv2d_p8n_splitk_workspace_bytes", splits, B * H * W, Cout, unit=4)
    assert ws.numel() * 4 == asked[0]
    _raw("nopesac_conv2d_nhwc_p8n_splitk", x, w, None, None, ref, B, H, W, Cin, Cout, 3, 3, 1, 1, Cin, Cout, ops.ACT_NONE, 32, splits, ws, ws.numel() * 4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref.float()).all()) and torch.equal(y.view(torch.int16), ref.view(torch.int16))


def test_groupnorm_forward_from_a_used_arena(device):
    """ops.groupnorm in its split-statistics form ([2, 4, 4, 64], 32 groups) after a larger scratch user, against the raw call with a
    private NaN-prefilled workspace of the size entry's length."""
    from nopesac_amd import ops
    x, gamma, beta = _rand(35, 2, 4, 4, 64).to(device), _rand(36, 64).to(device), _rand(37, 64).to(device)
    _dirty_arena(device)
    y = ops.groupnorm(x, gamma, beta, 32, 1e-5, ops.ACT_RELU)
    ref = torch.full_like(y, NAN)
    ws = _private(device, "nopesac_groupnorm_workspace_floats", 2, 32)
    assert ws.numel() == 2 * 16 * 32 * 2
    _raw("nopesac_groupnorm_nhwc", x, gamma, beta, ref, 2, 16, 64, 32, 1e-5, ops.ACT_RELU, ops.F32, ws)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all()) and _same_bits(y, ref)
