"""Shared helpers of the bottleneck-tail form sweep (tests/test_tail_forms_*.py): the production calls of ops.bottleneck_tail, the sweep's
calls at their stage's production size, their inputs, and float64 references of y and o at sampled rows.  The row sampler, tolerance and
comparators are those of tests/conv_routing.py."""
import math
from types import SimpleNamespace

import torch

# stage of a tail by its C: (OH, OW) of the output, (H2, W2) and stride of the projection source (x2[b, oy * s, ox * s])
STAGES = {64: ((120, 160), (120, 160), 1), 128: ((60, 80), (120, 160), 2), 256: ((30, 40), (60, 80), 2)}
SWEEP_B = (64, 2, 3)            # the benchmark (32 pairs x 2 views), one pair, and an odd batch that takes the M-tail paths
GUARD_ROWS = 128                # NaN rows behind y and o: one whole 128-pixel tile
FP8_S1 = 300.0                  # scale1 of the swept calls: relu(s1 . (y w1) + b1) exceeds e4m3fn's 448 at ~7 % of the elements

# every tail the backbone launches at B images of 480 x 640: name -> ((C, C4, CN, C2), the default form id's name).  res2 / res3 in
# every bf16 step; res4 in fp8 mode (MODEL.AMD.BACKBONE_FP8) and under NOPESAC_TAIL_RES4_FUSED=1
PRODUCTION = {
    "res2.0": ((64, 256, 64, 64), "rt4_proj"), "res2.1": ((64, 256, 64, 0), "rt4"), "res2.2": ((64, 256, 128, 0), "rt4"),
    "res3.0": ((128, 512, 128, 256), "rt4h"), "res3.1": ((128, 512, 128, 0), "rt4"), "res3.2": ((128, 512, 128, 0), "rt4"),
    "res3.3": ((128, 512, 256, 0), "rt4h"),
    "res4.0": ((256, 1024, 256, 512), "wide"), "res4.1": ((256, 1024, 256, 0), "stream"), "res4.2": ((256, 1024, 256, 0), "stream"),
    "res4.3": ((256, 1024, 256, 0), "stream"), "res4.4": ((256, 1024, 256, 0), "stream"), "res4.5": ((256, 1024, 512, 0), "wide"),
}


def stage_call(cfg, B):
    """(B, OH, OW, H2, W2, stride) of the config at its stage's production size (H2 = W2 = 0 for an identity block)."""
    C, C4, CN, C2 = cfg
    (OH, OW), (H2, W2), s = STAGES[C]
    return (B, OH, OW, H2, W2, s) if C2 else (B, OH, OW, 0, 0, 1)


def call_id(cfg, B):
    C, C4, CN, C2 = cfg
    (OH, OW), (H2, W2), s = STAGES[C]
    return "C%d-%d_cn%d_%s_b%d_%dx%d" % (C, C4, CN, ("proj%d_s%d" % (C2, s)) if C2 else "id", B, OH, OW)


def forms_of(mask):
    return [f for f in range(32) if (mask >> f) & 1]


def build_tail(cfg, B, OH, OW, H2, W2, stride, device, seed, s1_scale=FP8_S1):
    """Inputs of one tail call: b, residual / x2 ~ N(0, 1) bf16, weights ~ N(0, 1 / K) bf16 ([N, K] plain; *_f: fragment-major, as the
    kernels read them), BN scales ~ 1 + 0.1 N (s1 times s1_scale) and shifts ~ 0.1 N in f32.  call.new_outputs(o_fp8) gives NaN-filled
    y / o views of buffers with GUARD_ROWS more rows, and those buffers."""
    from nopesac_amd import ops
    C, C4, CN, C2 = cfg
    device = torch.device(device)
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*shape):
        return torch.randn(shape, generator=g, device=device)

    def frag(w):
        return ops.mfma_fragment_major(w) if device.type == "cuda" else w

    c = SimpleNamespace(cfg=cfg, C=C, C4=C4, CN=CN, C2=C2, B=B, OH=OH, OW=OW, H2=H2, W2=W2, stride=stride, M=B * OH * OW, device=device)
    c.b = randn(B, OH, OW, C).to(torch.bfloat16)
    c.w3 = (randn(C4, C) / math.sqrt(C)).to(torch.bfloat16)
    c.s3, c.b3 = 1 + 0.1 * randn(C4), 0.1 * randn(C4)
    c.residual = c.x2 = c.wsc = c.ssc = c.bsc = c.w1 = c.s1 = c.b1 = None
    if C2:
        c.x2 = randn(B, H2, W2, C2).to(torch.bfloat16)
        c.wsc = (randn(C4, C2) / math.sqrt(C2)).to(torch.bfloat16)
        c.ssc, c.bsc = 1 + 0.1 * randn(C4), 0.1 * randn(C4)
    else:
        c.residual = randn(B, OH, OW, C4).to(torch.bfloat16)
    if CN:
        c.w1 = (randn(CN, C4) / math.sqrt(C4)).to(torch.bfloat16)
        c.s1, c.b1 = s1_scale * (1 + 0.1 * randn(CN)), 0.1 * randn(CN)
    c.w3_f, c.wsc_f, c.w1_f = frag(c.w3), (frag(c.wsc) if C2 else None), (frag(c.w1) if CN else None)

    def new_outputs(o_fp8=False):
        ybuf = torch.full((c.M + GUARD_ROWS, C4), float("nan"), device=device, dtype=torch.bfloat16)
        y = ybuf[:c.M].view(B, OH, OW, C4)
        obuf = o = None
        if CN:
            obuf = torch.full((c.M + GUARD_ROWS, CN), float("nan"), device=device).to(torch.float8_e4m3fn if o_fp8 else torch.bfloat16)
            o = obuf[:c.M].view(B, OH, OW, CN)
        return y, o, ybuf, obuf

    c.new_outputs = new_outputs
    return c


def run_tail(c, form, o_fp8=False):
    """ops.bottleneck_tail of the call on `form` (None: the default selection) into fresh NaN-filled buffers: (y, o, ybuf, obuf)."""
    from nopesac_amd import ops
    y, o, ybuf, obuf = c.new_outputs(o_fp8)
    kw = dict(residual=c.residual) if c.C2 == 0 else dict(x2=c.x2, wsc=c.wsc_f, ssc=c.ssc, bsc=c.bsc, stride=c.stride)
    if c.CN:
        kw.update(w1=c.w1_f, s1=c.s1, b1=c.b1)
    ops.bottleneck_tail(c.b, c.w3_f, c.s3, c.b3, o_fp8=o_fp8, form=form, y=y, o=o, **kw)
    return y, o, ybuf, obuf


def rows_of(t, rows):
    """t[rows] of a [B, OH, OW, N] (or [M, N]) tensor as float64 [len(rows), N] on the CPU."""
    return t.reshape(-1, t.shape[-1])[rows.to(t.device)].float().cpu().double()


def source_pixels(c, rows):
    """Flat index into x2 [B * H2 * W2] of the shortcut source of each output row: x2[b, oy * s, ox * s]."""
    P = c.OH * c.OW
    b, oy, ox = rows // P, (rows % P) // c.OW, rows % c.OW
    return (b * c.H2 + oy * c.stride) * c.W2 + ox * c.stride


def _d(t):
    return t.float().cpu().double()


def reference_y(c, rows):
    """float64 y at the sampled rows: (r, A), [len(rows), C4] on the CPU.  r = relu(s3 (b w3) + b3 + shortcut), the shortcut being the bf16
    residual as read or ssc (x2 wsc) + bsc at the strided source pixel; A = |s3| sum|b||w3| + |b3| + the shortcut's own magnitude
    (|residual|, or |ssc| sum|x2||wsc| + |bsc|)."""
    bm, w3 = rows_of(c.b, rows), _d(c.w3)
    s3, b3 = _d(c.s3), _d(c.b3)
    v = (bm @ w3.T) * s3 + b3
    A = (bm.abs() @ w3.abs().T) * s3.abs() + b3.abs()
    if c.C2:
        xm = rows_of(c.x2, source_pixels(c, rows))
        wsc, ssc, bsc = _d(c.wsc), _d(c.ssc), _d(c.bsc)
        v = v + (xm @ wsc.T) * ssc + bsc
        A = A + (xm.abs() @ wsc.abs().T) * ssc.abs() + bsc.abs()
    else:
        res = rows_of(c.residual, rows)
        v, A = v + res, A + res.abs()
    return v.clamp_min(0), A


def reference_o(c, y_rows):
    """float64 o = relu(s1 (y w1) + b1) of the kernel's own bf16 y rows (conv1 is 1 x 1: an o row depends on its y row only): (r, A)."""
    w1, s1, b1 = _d(c.w1), _d(c.s1), _d(c.b1)
    v = (y_rows @ w1.T) * s1 + b1
    A = (y_rows.abs() @ w1.abs().T) * s1.abs() + b1.abs()
    return v.clamp_min(0), A


def q8(t):
    """float -> e4m3fn with the kernels' saturating round-to-nearest-even (f32x8_to_fp8 in csrc/common.h)."""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def fp8_ratio(o8, o16):
    """Worst |o8 - q8(o16)| over 2^-4 |q8(o16)| + 2^-10 (one e4m3 unit in the last place is 2^-3 relative): 0 when o8 is the bf16 o converted
    bit for bit; a non-finite o8 counts as infinite."""
    want, got = q8(o16).float(), o8.float()
    q = (got - want).abs() / (2.0 ** -4 * want.abs() + 2.0 ** -10)
    q = torch.where(torch.isfinite(got), q, torch.full_like(q, math.inf))
    return float(q.max())


def emulate(c, fault=None, o_fp8=False):
    """A CPU float32 'kernel' of the call (c built on the CPU): the GEMMs and epilogues in float32, y and o rounded where the kernels round
    them - with one planted fault.  Returns (y [B, OH, OW, C4] bf16, o or None)."""
    C4, CN = c.C4, c.CN
    bm = c.b.reshape(-1, c.C).float()
    w3 = c.w3.float().clone()
    s3, b3 = c.s3.clone(), c.b3.clone()
    if fault == "conv3_drops_last_16_k":                 # the last 16 input channels of conv3 never accumulated
        w3[:, c.C - 16:] = 0
    acc = bm @ w3.T
    if c.C2:
        ssc, bsc = c.ssc.clone(), c.bsc.clone()
        if fault == "bn_sc_swapped_with_bn3":            # the projection's BN vectors applied to conv3 and the other way round
            s3, b3, ssc, bsc = ssc, bsc, s3, b3
        rows = torch.arange(c.M)
        if fault == "stride2_gather_wrong_row":          # a 64-pixel tile that crosses an image row keeps gathering from its first row
            P = c.OH * c.OW
            t0 = rows // 64 * 64
            same_img = t0 // P == rows // P
            oy0 = (t0 % P) // c.OW
            oy = torch.where(same_img, oy0, (rows % P) // c.OW)
            src = (rows // P * c.H2 + oy * c.stride) * c.W2 + (rows % c.OW) * c.stride
        else:
            src = source_pixels(c, rows)
        xm = c.x2.reshape(-1, c.C2)[src].float()
        v = acc * s3 + b3 + ((xm @ c.wsc.float().T) * ssc + bsc)
        y = v.clamp_min(0)
    else:
        res = c.residual.reshape(-1, C4).float()
        v = acc * s3 + b3
        y = v.clamp_min(0) + res if fault == "residual_after_relu" else (v + res).clamp_min(0)
    y = y.to(torch.bfloat16)
    if fault == "last_tile_y_col_tile_unwritten":       # the last 128-pixel tile's final 32-channel column tile never stored
        y[(c.M - 1) // 128 * 128:, C4 - 32:] = 0
    o = None
    if CN:
        s1, b1 = c.s1.clone(), c.b1.clone()
        if fault == "o_tile_shifted_bn1":                # o channels 0-31 (one column tile) read s1 / b1 one channel on
            s1[0:32], b1[0:32] = c.s1[1:33].clone(), c.b1[1:33].clone()
        o = ((y.float() @ c.w1.float().T) * s1 + b1).clamp_min(0).to(torch.bfloat16)
        if o_fp8:
            o = o.float().to(torch.float8_e4m3fn) if fault == "fp8_o_unsaturated" else q8(o)
        o = o.view(c.B, c.OH, c.OW, CN)
    return y.view(c.B, c.OH, c.OW, C4), o
