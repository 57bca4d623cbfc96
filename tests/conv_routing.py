"""Shared helpers of the conv routing sweep (tests/test_conv_routing_*.py): the routed shapes of the committed routing files, the call
each routing key came from, a deterministic row sampler and a float64 reference of ops.conv2d at the sampled output rows.

A routing key is ConvTuner.key_str of the tuple conv2d hands the tuner; its field order is the files' meta.note:
dtype|w dtype|out dtype|B|H|W|Cin|Cout|KH|KW|stride|pad|residual|x_cs|y_cs|batched|scale|bias|act|bfrag_ok|halo_ok|p8_ok."""
import json
import math
import os
import zlib
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the routing files a current run can load: bench.py's headline leg and the two legs of its `other_configs`
ROUTING_FILES = ("routing_r5.json", "routing_r5_scannet_k64.json", "routing_r5_fp8_k128.json")
FIELDS = ("x_dtype", "w_dtype", "out_dtype", "B", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "residual", "x_cs", "y_cs",
          "batched", "scale", "bias", "act", "bfrag_ok", "halo_ok", "p8_ok")
_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float8_e4m3fn": torch.float8_e4m3fn}
_SHORT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float8_e4m3fn: "fp8"}
TILE_HEIGHTS = (32, 64, 128, 256)        # output-row tile heights of the conv kernels (64 / 128: conv_igemm, bfrag; 256: p8 / p8n)


def routing_path(name):
    return os.path.join(ROOT, "profiles", name)


def load_routing():
    """{key string: {routing file name: configuration}} over ROUTING_FILES (read only)."""
    keys = {}
    for name in ROUTING_FILES:
        with open(routing_path(name)) as f:
            doc = json.load(f)
        for k, v in doc["routing"].items():
            keys.setdefault(k, {})[name] = int(v)
    return keys


def parse_key(key_str):
    """The call a routing key came from, as a namespace with the FIELDS of the key (dtypes as torch dtypes, flags as bools)."""
    parts = key_str.split("|")
    assert len(parts) == len(FIELDS), key_str
    vals = {}
    for name, s in zip(FIELDS, parts):
        if name.endswith("dtype"):
            vals[name] = _DTYPES[s]
        elif s in ("True", "False"):
            vals[name] = s == "True"
        else:
            vals[name] = int(s)
    return SimpleNamespace(**vals)


def key_tuple(case):
    return tuple(getattr(case, f) for f in FIELDS)


def key_id(key_str):
    """A readable pytest id: dtypes, batch x spatial, Cin-Cout, kernel / stride / pad and the epilogue."""
    c = parse_key(key_str)
    s = "%s%s-%s_b%d_%dx%d_%d-%d_k%dx%ds%dp%d" % (_SHORT[c.x_dtype], "" if c.w_dtype == c.x_dtype else "w" + _SHORT[c.w_dtype],
                                                  _SHORT[c.out_dtype], c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad)
    if c.x_cs != c.Cin or c.y_cs != c.Cout:
        s += "_cs%d-%d" % (c.x_cs, c.y_cs)
    s += "".join(t for t, on in (("_res", c.residual), ("_batched", c.batched), ("_scale", c.scale), ("_bias", c.bias)) if on)
    return s + "_act%d" % c.act


def key_seed(key_str):
    return zlib.crc32(key_str.encode()) & 0x7fffffff


def eligibility(case, aligned=True):
    """ops.conv_eligibility of the key's call (a contiguous residual).  Needs no GPU; it asks the built library."""
    from nopesac_amd import ops
    return ops.conv_eligibility(case.x_dtype, case.w_dtype, case.out_dtype, case.B, case.H, case.W, case.Cin, case.Cout, case.KH, case.KW,
                                case.stride, case.pad, case.residual, case.x_cs, case.y_cs, case.Cout if case.residual else 0, case.batched,
                                case.scale, case.bias, case.act, aligned)


def build_call(case, device, seed):
    """Inputs of the key's call on `device`: x ~ N(0, 1) NHWC (a channel slice of a wider buffer when x_cs > Cin), w ~ N(0, 1 / (KH KW Cin))
    as [Cout, KH, KW, Cin] ([B, Cout, KH, KW, Cin] when batched), scale ~ 1 + 0.1 N, bias ~ 0.1 N, residual ~ N(0, 1) in the output dtype.
    call.new_out() gives a NaN-filled output (a slice of a wider NaN-filled buffer when y_cs > Cout) and the buffer it lives in.
    The shape flags conv2d computes for this call must be the key's last three fields."""
    from nopesac_amd import ops
    c = case
    device = torch.device(device)
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*shape):
        return torch.randn(shape, generator=g, device=device)

    OH = (c.H + 2 * c.pad - c.KH) // c.stride + 1
    OW = (c.W + 2 * c.pad - c.KW) // c.stride + 1
    x = randn(c.B, c.H, c.W, c.x_cs).to(c.x_dtype)[..., :c.Cin]
    w = (randn(*((c.B,) if c.batched else ()), c.Cout, c.KH, c.KW, c.Cin) / math.sqrt(c.KH * c.KW * c.Cin)).to(c.w_dtype)
    scale = 1 + 0.1 * randn(c.Cout) if c.scale else None
    bias = 0.1 * randn(c.Cout) if c.bias else None
    residual = randn(c.B, OH, OW, c.Cout).to(c.out_dtype) if c.residual else None

    def new_out():
        wide = torch.full((c.B, OH, OW, c.y_cs), float("nan"), device=device, dtype=c.out_dtype)
        return wide[..., :c.Cout], wide

    out, _ = new_out()
    aligned = all(t is None or t.data_ptr() % 16 == 0 for t in (x, w, out, residual, scale, bias))
    el = ops.conv_eligibility(c.x_dtype, c.w_dtype, c.out_dtype, c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, residual is not None,
                              x.stride(2), out.stride(2), residual.stride(2) if residual is not None else 0, c.batched, scale is not None,
                              bias is not None, c.act, aligned)
    assert (el.bfrag_ok, el.halo_ok, el.p8_ok) == (c.bfrag_ok, c.halo_ok, c.p8_ok), (key_tuple(c), el)
    return SimpleNamespace(case=c, x=x, w=w, scale=scale, bias=bias, residual=residual, OH=OH, OW=OW, M=c.B * OH * OW, el=el,
                           new_out=new_out, device=device)


def run_conv(call, out):
    """ops.conv2d of the call into `out` (whatever configuration the tuner state in force picks)."""
    from nopesac_amd import ops
    c = call.case
    return ops.conv2d(call.x, call.w, call.scale, call.bias, call.residual, stride=c.stride, pad=c.pad, act=c.act & ~ops.ACT_BIAS_BATCHED,
                      out=out, batched_weights=c.batched)


def sample_rows(M, B, OH, OW, seed, n=1536):
    """About `n` output rows (flat pixel indices b * OH * OW + oh * OW + ow), deterministic in `seed`: rows 0-63 and the last 64 (the M tail),
    the two rows on each side of a few boundaries of every tile height in TILE_HEIGHTS, the corners and edge midpoints of the first, the
    last and one random image (the padding taps), the rest uniform over M.  Sorted, unique, int64."""
    g = torch.Generator().manual_seed(seed)
    rows = set(range(min(64, M))) | set(range(max(0, M - 64), M))
    for t in TILE_HEIGHTS:
        nb = (M - 1) // t                               # boundaries at t, 2t, .., nb * t
        if nb < 1:
            continue
        picks = {1, nb} | {1 + int(v) for v in torch.randint(0, nb, (2,), generator=g)}
        for j in picks:
            rows |= {j * t + d for d in (-2, -1, 0, 1)}
    P = OH * OW
    for b in {0, B - 1, int(torch.randint(0, B, (1,), generator=g))}:
        for oh, ow in ((0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1), (0, OW // 2), (OH - 1, OW // 2), (OH // 2, 0), (OH // 2, OW - 1)):
            rows.add(b * P + oh * OW + ow)
    rows = {r for r in rows if 0 <= r < M}
    rest = max(0, min(n, M) - len(rows))
    if rest:
        cand = torch.randperm(M, generator=g)[: rest + len(rows)].tolist()
        for r in cand:
            if len(rows) >= min(n, M):
                break
            rows.add(r)
    return torch.tensor(sorted(rows), dtype=torch.long)


def _act(v, act):
    from nopesac_amd import ops
    if act == ops.ACT_RELU:
        return v.clamp_min(0)
    if act == ops.ACT_LEAKY:
        return torch.where(v > 0, v, 0.01 * v)
    if act == ops.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def _pixels(t, rows, OH, OW):
    """t[b, oh, ow, :] of the flat output rows (t NHWC, channel-slice views allowed)."""
    rows = rows.to(t.device)
    P = OH * OW
    return t[rows // P, (rows % P) // OW, rows % OW]


def output_rows(call, out, rows):
    """The kernel's output at the sampled rows, float64 on the CPU."""
    return _pixels(out, rows, call.OH, call.OW).float().cpu().double()


def reference_rows(call, rows):
    """float64 reference of every output channel at the sampled rows: (r, A), both [len(rows), Cout] on the CPU.  r is the exact
    act(conv * scale + bias [+ residual]) (the residual before or after the activation as `act` says) of the operand values the kernel
    reads; A = |scale| sum|x w| + |bias| + |residual| is the magnitude the kernel's float32 accumulation is measured against.
    The KH x KW x Cin patches are gathered on the call's device; only the patch matrix goes to the CPU."""
    from nopesac_amd import ops
    c = call.case
    rows_d = rows.to(call.device)
    P = call.OH * call.OW
    b, oh, ow = rows_d // P, (rows_d % P) // call.OW, rows_d % call.OW
    cols = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            ih, iw = oh * c.stride - c.pad + kh, ow * c.stride - c.pad + kw
            ok = (ih >= 0) & (ih < c.H) & (iw >= 0) & (iw < c.W)
            v = call.x[b, ih.clamp(0, c.H - 1), iw.clamp(0, c.W - 1)]
            cols.append(torch.where(ok[:, None], v, torch.zeros((), dtype=v.dtype, device=v.device)))
    patches = torch.cat(cols, 1)                       # [R, KH * KW * Cin], the K order of w.reshape(Cout, -1)
    if c.x_dtype == torch.float32 and c.w_dtype == torch.bfloat16:
        # f32 activations x bf16 weights: conv_igemm_kernel rounds every activation to bf16 as it loads it (csrc/conv_igemm.hip, the
        # `sizeof(TA) != sizeof(T)` branch of the A-tile load: f32_to_bf16 of each value), so the reference multiplies the rounded values
        patches = patches.to(torch.bfloat16)
    Pm = patches.cpu().double()
    del patches, cols
    K = c.KH * c.KW * c.Cin
    w = call.w.float().cpu().double()
    if c.batched:
        acc = torch.empty(Pm.shape[0], c.Cout, dtype=torch.float64)
        mag = torch.empty_like(acc)
        bc = b.cpu()
        for bi in bc.unique().tolist():
            sel = (bc == bi).nonzero().squeeze(1)
            wb = w[bi].reshape(c.Cout, K)
            acc[sel] = Pm[sel] @ wb.T
            mag[sel] = Pm[sel].abs() @ wb.abs().T
    else:
        wm = w.reshape(c.Cout, K)
        acc = Pm @ wm.T
        mag = Pm.abs() @ wm.abs().T
    v, A = acc, mag
    if call.scale is not None:
        s = call.scale.cpu().double()
        v, A = v * s, A * s.abs()
    if call.bias is not None:
        bb = call.bias.cpu().double()
        v, A = v + bb, A + bb.abs()
    act, res_after = c.act & 0xff, bool(c.act & ops.ACT_RES_AFTER)
    if call.residual is not None:
        res = output_rows(call, call.residual, rows)
        A = A + res.abs()
        r = _act(v, act) + res if res_after else _act(v + res, act)
    else:
        r = _act(v, act)
    return r, A


def tolerance(r, A, out_dtype):
    """Allowed |kernel - r| per element: E = 2^-20 A covers the float32 accumulation; the rest is the rounding to the output format
    (round to nearest: 2^-8 relative for bf16, 2^-4 relative + half the smallest subnormal spacing for fp8 e4m3)."""
    E = A * 2.0 ** -20
    if out_dtype == torch.float32:
        return r.abs() * 2.0 ** -22 + E
    if out_dtype == torch.bfloat16:
        return r.abs() * 2.0 ** -8 + 2 * E
    if out_dtype == torch.float8_e4m3fn:
        return r.abs() * 2.0 ** -4 + 2.0 ** -10 + 2 * E
    raise ValueError(out_dtype)


def error_ratio(y, r, A, out_dtype):
    """(worst |y - r| / tolerance, (row index, channel) where it occurs); a non-finite y counts as an infinite ratio."""
    q = (y - r).abs() / tolerance(r, A, out_dtype)
    q = torch.where(torch.isfinite(y), q, torch.full_like(q, math.inf))
    i = int(q.argmax())
    return float(q.flatten()[i]), divmod(i, q.shape[1])


def full_agreement(a, b):
    """Worst ratio of |a - b| to 2^-7 max(|a|, |b|) + 2^-10 rms(b) over two whole outputs of the same call (<= 1: they agree).
    Two configurations sum in different orders, so a bf16 output may differ by one unit in the last place: 2^-7 relative.  For an
    fp8 e4m3 output one unit is 2^-3 relative and the subnormal spacing 2^-9, and the bound is widened to that."""
    a32, b32 = a.float(), b.float()
    rel, floor = (2.0 ** -3, 2.0 ** -9) if a.dtype == torch.float8_e4m3fn else (2.0 ** -7, 0.0)
    rms = float(b32.square().mean().sqrt())
    q = (a32 - b32).abs() / (rel * torch.maximum(a32.abs(), b32.abs()) + 2.0 ** -10 * rms + floor)
    q = torch.where(torch.isfinite(a32) & torch.isfinite(b32), q, torch.full_like(q, math.inf))
    return float(q.max())
