"""The backward kernels of the backbone (csrc/backbone_bwd.hip: the stride-2 dgrad by input parity on the f32 MFMA, the 3x3 / stride-2
max-pool backward, the FrozenBN + ReLU gate from the saved output) and BackboneTrainer as data: seeded cases, float64 references in
plain torch, allowances, a float32 emulation of the parity decomposition in which errors can be planted, and a float64 / float32
restatement of the whole ResNet-50.  tests/test_backbone_forms_gpu.py and tests/test_backbone_training_gpu.py hold the kernels and the
trainer to it; tests/test_backbone_forms_cpu.py proves the case lists, the references, the committed constants and the sharpness of the
bound.  Imports without a GPU.

Strided dgrad - the construction of tests/refine_bwd_forms.py and tests/plane_pyramid_forms.py: per element an allowance
A_k = 2^-24 S_k + C_k and the limit LIMIT_FACTOR x max(F32_WORST["dgrad"], 1).
  S_k    the transposed conv of |dy| with |w|: the sum of the magnitudes of the products that make dx_k
  C_k    the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input by 1 +- 2^-23
  F32_WORST  the worst error / A of the float32 torch restatement over DGRAD_CASES (measured on the CPU, never from a kernel)
The float64 reference is the transposed conv stated tap by tap as matrix products (dgrad_run: it runs on any device, so the
production layers' references are evaluated where the test runs); the CPU test holds it to F.conv2d's autograd.

Max-pool backward: float64 autograd of F.max_pool2d(3, 2, 1); with integer dy the kernel's result is exact, with normal dy it is
within 3 x 2^-24 x (the same routing of |dy|): at most four terms, three roundings (derived, not measured).

FrozenBN gate: the float32 torch expression, bit for bit (one rounding).

Whole backbone: per tensor the normalised error max |a - ref| / max |ref| against the float64 restatement, bounded by LIMIT_FACTOR x
the same figure of the float32 restatement ON THE SAME INPUTS (F32_NORM_ERR per case, cotangents and tensor family, measured on the
CPU) with a floor of NORM_FLOOR = 2e-5 (the gate tests/test_conv_backward_gpu.py holds single convs to).  ReLU decisions that flip between float32 and float64 over 50 layers are
part of what float32 does, so the bound comes from the float32 restatement and no element is left out."""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

from nopesac_amd import _lib
from nopesac_amd.synth import RES_STAGES, _g, state_dict_spec, synth_tensor
from tests.refine_bwd_forms import DRAWS, EPS24, F32, F64, LIMIT_FACTOR, _cot, jiggle, ratios

PIXELS, CHANNELS, STAGE = _lib.H.NPS_DGRAD_S2_PIXELS, _lib.H.NPS_DGRAD_S2_CHANNELS, _lib.H.NPS_DGRAD_S2_STAGE     # the kernel's tile

# worst error / A of the float32 torch restatement over DGRAD_CASES.  Printed by
#   python -c "from tests import backbone_forms as B; B.print_f32_worst()"
# and re-measured by tests/test_backbone_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"dgrad": 2.48}
# worst normalised error of the float32 restatement's gradients per (case of NET_CASES, cotangents of COTANGENTS) and tensor family: a
# run is held to the figure of its OWN inputs (same printer).  At 2 x 64 x 96 the figures are per cent, not 1e-6: a few ReLU
# decisions fall the other way in float32, and with 12 pixels at res5 one of them moves a weight gradient by a pixel's whole
# contribution (the maps themselves agree to 1e-6, which the CPU test also holds).  At 1 x 40 x 72 no decision flips, every figure is
# 1e-6, and the bound is the floor.
F32_NORM_ERR = {
    ((2, 64, 96), "all"): {"stem": 0.00402, "res2": 0.0042, "res3": 0.00871, "res4": 0.0115, "res5": 0.0924},
    ((2, 64, 96), "res5"): {"stem": 0.0114, "res2": 0.0112, "res3": 0.017, "res4": 0.017, "res5": 0.0924},
    ((1, 40, 72), "all"): {"stem": 5.99e-07, "res2": 8.21e-07, "res3": 7.97e-07, "res4": 1.04e-06, "res5": 5.67e-07},
    ((1, 40, 72), "res5"): {"stem": 8.54e-07, "res2": 1.02e-06, "res3": 1.06e-06, "res4": 9.19e-07, "res5": 5.67e-07}}
NORM_FLOOR = 2e-5


def limit(family="dgrad"):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


# ===================================================================================================================== strided dgrad
DGRAD_K = (1, 3)
DGRAD_HW = ((1, 1), (2, 2), (3, 3), (4, 6), (5, 9), (7, 10))
DGRAD_B = (1, 2)
DGRAD_CC = ((4, 4), (12, 8), (64, 132), (132, 64))                      # (Cin, Cout)
# (k, B, H, W, Cin, Cout, tag).  base: dense dy and out; slice: both are channel slices of wider buffers filled with FILL
BASE_CASES = tuple((k, b, h, w, ci, co, "base") for k in DGRAD_K for h, w in DGRAD_HW for b in DGRAD_B for ci, co in DGRAD_CC)
# H = 2 gives every row parity one row; W = 2 n puts n pixels into each of the four classes: the tile's pixels - 1, exactly, + 1
PIXEL_CASES = tuple((k, 1, 2, 2 * (PIXELS + d), 8, 8, "base") for k in DGRAD_K for d in (-1, 0, 1))
CHANNEL_CASES = tuple((k, 1, 5, 9, CHANNELS + d, 8, "base") for k in DGRAD_K for d in (-4, 0, 4))
# K = taps x Cout of a class with one tap: a float4 short of one LDS stage, exactly one, one stage and a float4 (the stage crossed by one load)
STAGE_CASES = tuple((k, 1, 5, 9, 8, STAGE + d, "base") for k in DGRAD_K for d in (-4, 0, 4))
SLICE_CASES = tuple((k, b, h, w, ci, co, "slice") for k in DGRAD_K for b, h, w, ci, co in ((2, 5, 9, 12, 8), (1, 7, 10, 132, 64)))
DGRAD_CASES = BASE_CASES + PIXEL_CASES + CHANNEL_CASES + STAGE_CASES + SLICE_CASES
# res3.0 / res4.0 / res5.0: conv2 and the shortcut, B = 1 (their float64 references: about 1.4 GMAC each; not part of F32_WORST)
PRODUCTION_CASES = ((3, 1, 120, 160, 128, 128, "base"), (3, 1, 60, 80, 256, 256, "base"), (3, 1, 30, 40, 512, 512, "base"),
                    (1, 1, 120, 160, 256, 512, "base"), (1, 1, 60, 80, 512, 1024, "base"), (1, 1, 30, 40, 1024, 2048, "base"))
IDENTITY_CASE = (3, 2, 7, 10, 132, 64, "base")
FILL, SLICE_PAD = 7.0, 4                                                # the wider buffers: SLICE_PAD channels of FILL on either side


def out_size(n, k):
    return (n + 2 * ((k - 1) // 2) - k) // 2 + 1


def class_pixels(B, H, W):
    """Pixels of the four parity classes (row parity, column parity) of a B x H x W input."""
    return {(ph, pw): B * ((H - ph + 1) // 2) * ((W - pw + 1) // 2) for ph in (0, 1) for pw in (0, 1)}


def class_taps(k, parity):
    """The taps (along one axis) through which an input coordinate of this parity receives gradient: (parity + pad - tap) even."""
    pad = (k - 1) // 2
    return [t for t in range(k) if (parity + pad - t) % 2 == 0]


@functools.lru_cache(maxsize=None)
def dgrad_inputs(key):
    k, B, H, W, Cin, Cout, tag = key
    g = _g(70000 + 7919 * k + 1009 * B + 131 * H + 17 * W + 3 * Cin + Cout + (500000 if tag == "slice" else 0))
    OH, OW = out_size(H, k), out_size(W, k)
    return dict(key=key, k=k, pad=(k - 1) // 2, B=B, H=H, W=W, Cin=Cin, Cout=Cout, OH=OH, OW=OW, dy=_cot(g, B, OH, OW, Cout),
                w=torch.randn(Cout, Cin, k, k, generator=g) * (Cout * k * k) ** -0.5)


def dgrad_run(dy, w, H, W):
    """The input gradient of the stride-2 conv (pad (k - 1) / 2) in dy's dtype on dy's device, NHWC: every tap's matrix product
    dy [pixels, Cout] @ w[:, :, kh, kw] lands on the padded input rows 2 oh + kh, columns 2 ow + kw."""
    B, OH, OW, Cout = dy.shape
    k = w.shape[2]
    pad = (k - 1) // 2
    dxp = torch.zeros(B, H + 2 * pad + 1, W + 2 * pad + 1, w.shape[1], dtype=dy.dtype, device=dy.device)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] += dy @ w[:, :, kh, kw]
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def dgrad_autograd(dy, w, H, W):
    """The same gradient from F.conv2d's autograd (NCHW inside)."""
    k = w.shape[2]
    x = torch.zeros(dy.shape[0], w.shape[1], H, W, dtype=dy.dtype, requires_grad=True)
    y = F.conv2d(x, w, stride=2, padding=(k - 1) // 2)
    return torch.autograd.grad(y, x, dy.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def dgrad_reference(key, device="cpu"):
    """-> (ref, A) on the CPU: the float64 gradient and the allowance 2^-24 S + C per element, evaluated on `device`."""
    c = dgrad_inputs(key)
    to = lambda t: t.to(device=device, dtype=F64)
    ref = dgrad_run(to(c["dy"]), to(c["w"]), c["H"], c["W"])
    S = dgrad_run(to(c["dy"]).abs(), to(c["w"]).abs(), c["H"], c["W"])
    g = _g(87)
    C = torch.zeros_like(ref)
    for _ in range(DRAWS):
        C = torch.maximum(C, (dgrad_run(jiggle(c["dy"], g).to(device), jiggle(c["w"], g).to(device), c["H"], c["W"]) - ref).abs())
    return ref.cpu(), (EPS24 * S + C).cpu()


def dgrad_worst(key, got, device="cpu"):
    """(worst error / A, flat index) of `got` [B, H, W, Cin]; a NaN counts as inf."""
    ref, A = dgrad_reference(key, device)
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    q = ratios(got.cpu(), ref, A).reshape(-1)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max()), int(q.argmax())


def dgrad_f32(key):
    c = dgrad_inputs(key)
    return dgrad_run(c["dy"], c["w"], c["H"], c["W"])


def f32_worst(family="dgrad"):
    return max(dgrad_worst(key, dgrad_f32(key))[0] for key in DGRAD_CASES)


DGRAD_PLANTS = ("wrong_tap", "missing_zero_fill")


def emulate_dgrad(key, plant=None):
    """The kernel's decomposition in float32: out starts as NaN (an uninitialised buffer); each parity class of input pixels is one
    sum over its taps of dy[oh, ow] @ w[:, :, kh, kw], oh = (ih + pad - kh) / 2, a tap without an output row / column contributing
    zeros; a class without taps is filled with zeros.  Plants: "wrong_tap" - the odd-row / even-column class of a 3x3 conv takes the
    weights of the mirrored row tap (kh 0 <-> 2); "missing_zero_fill" - the classes without taps of a 1x1 conv are left as they were."""
    c = dgrad_inputs(key)
    k, pad, B, H, W, OH, OW = c["k"], c["pad"], c["B"], c["H"], c["W"], c["OH"], c["OW"]
    dy, w = c["dy"], c["w"]
    dx = torch.full((B, H, W, c["Cin"]), float("nan"))
    for ph in (0, 1):
        for pw in (0, 1):
            ih, iw = torch.arange(ph, H, 2), torch.arange(pw, W, 2)
            if not len(ih) or not len(iw):
                continue
            khs, kws = class_taps(k, ph), class_taps(k, pw)
            if not khs or not kws:
                if plant != "missing_zero_fill":
                    dx[:, ph::2, pw::2] = 0.0
                continue
            acc = torch.zeros(B, len(ih), len(iw), c["Cin"])
            for kh in khs:
                for kw in kws:
                    oh, ow = (ih + pad - kh) // 2, (iw + pad - kw) // 2
                    live = ((oh < OH)[:, None] & (ow < OW)[None, :]).float()[None, :, :, None]
                    gth = dy[:, oh.clamp(max=OH - 1)][:, :, ow.clamp(max=OW - 1)] * live
                    wk = w[:, :, (k - 1 - kh) if (plant == "wrong_tap" and (ph, pw) == (1, 0)) else kh, kw]
                    acc = acc + gth @ wk
            dx[:, ph::2, pw::2] = acc
    return dx


# ===================================================================================================================== max-pool backward
POOL_HW = ((1, 1), (2, 2), (3, 3), (4, 5), (5, 4), (7, 9), (8, 8))
POOL_C = (4, 64, 68)
POOL_B = (1, 2)
POOL_VARIANTS = ("ties", "negative", "increasing", "decreasing")
POOL_CASES = tuple((b, h, w, ch, v) for h, w in POOL_HW for ch in POOL_C for b in POOL_B for v in POOL_VARIANTS)
POOL_PRODUCTION = (1, 240, 320, 64, "ties")
POOL_ROUNDINGS = 3                                                       # at most four terms per element: three additions


@functools.lru_cache(maxsize=None)
def pool_inputs(key):
    """x [B, H, W, C] (ties: {0, 1, 2} with about half zeros, so that every window ties; negative: all < 0, so that padding must not
    win; increasing / decreasing: strictly monotonic in row-major order per channel), dy_int (integers in [-3, 3]) and dy (normal)."""
    B, H, W, C, variant = key
    g = _g(71000 + 1009 * B + 131 * H + 17 * W + C + 100003 * POOL_VARIANTS.index(variant))
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if variant == "ties":
        x = torch.where(torch.rand(B, H, W, C, generator=g) < 0.5, torch.zeros(()), torch.randint(1, 3, (B, H, W, C), generator=g).float())
    elif variant == "negative":
        x = -(0.1 + torch.rand(B, H, W, C, generator=g))
    else:
        ramp = (torch.arange(H * W).float().view(1, H, W, 1) + 0.25 * torch.arange(C).float().view(1, 1, 1, C)
                + 1000.0 * torch.arange(B).float().view(B, 1, 1, 1))
        x = ramp if variant == "increasing" else -ramp
    return dict(key=key, x=x.contiguous(), dy_int=torch.randint(-3, 4, (B, OH, OW, C), generator=g).float(), dy=torch.randn(B, OH, OW, C, generator=g))


def pool_backward(x, dy):
    """float64 autograd of F.max_pool2d(x, 3, 2, 1) at dy (NHWC in, NHWC out)."""
    xs = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xs, 3, 2, 1)
    return torch.autograd.grad(y, xs, dy.double().permute(0, 3, 1, 2).contiguous())[0].permute(0, 2, 3, 1).contiguous()


# ===================================================================================================================== FrozenBN gate
GATE_ROWS = (1, 255, 256, 257, 1000)
GATE_C = (4, 64, 68, 2048)
# (rows, C, relu, want_dz, strided)
GATE_CASES = tuple((r, ch, relu, dz, False) for r in GATE_ROWS for ch in GATE_C for relu in (True, False) for dz in (True, False)) + tuple(
    (r, ch, True, dz, True) for r in (257,) for ch in (4, 68) for dz in (True, False))


@functools.lru_cache(maxsize=None)
def gate_inputs(key):
    """g, y [rows, C] (strided: column slices of buffers 8 wider), scale [C]: y is a post-activation map - about half exact zeros, a
    quarter of them -0.0 - with a few negative values ("not > 0" as well), scale has both signs."""
    rows, C, relu, want_dz, strided = key
    gen = _g(72000 + 31 * rows + C + 2 * relu + want_dz + 4 * strided)
    Cb = C + 8 if strided else C
    gb, yb = torch.randn(rows, Cb, generator=gen), torch.randn(rows, Cb, generator=gen)
    u = torch.rand(rows, Cb, generator=gen)
    yb = torch.where(u < 0.375, torch.zeros(()), yb.abs())
    yb = torch.where(u < 0.125, -torch.zeros(()), yb)
    yb = torch.where(u > 0.95, -yb, yb)
    off = 4 if strided else 0
    return dict(key=key, g=gb[:, off:off + C], y=yb[:, off:off + C], scale=torch.randn(C, generator=gen), g_buf=gb, y_buf=yb, off=off)


def gate_reference(c):
    """(dc, dz) of the float32 torch expression."""
    relu = c["key"][2]
    dz = torch.where(c["y"] > 0, c["g"], torch.zeros(())) if relu else c["g"].clone()
    return dz * c["scale"], dz


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ===================================================================================================================== the whole backbone
NET_CASES = ((2, 64, 96), (1, 40, 72))                                   # (N, H, W): the second makes the strided layers see 5 x 9 -> 3 x 5 -> 2 x 3
COTANGENTS = ("all", "res5")                                             # unit-normal cotangents at all four maps / at res5 alone
MAPS = ("res2", "res3", "res4", "res5")
PREFIX = "backbone."
BN_EPS = 1e-5


def conv_names():
    """The 53 convs in forward order, without the prefix."""
    names, cin = ["stem.conv1"], 64
    for name, n, cmid, cout in RES_STAGES:
        for i in range(n):
            names += [f"{name}.{i}.{c}" for c in ("conv1", "conv2", "conv3") + (("shortcut",) if cin != cout else ())]
            cin = cout
    return names


def family_of(key):
    return key[len(PREFIX):].split(".")[0]


@functools.lru_cache(maxsize=None)
def backbone_state_dict():
    """The backbone's tensors of the name-seeded synthetic checkpoint (f32, CPU)."""
    return {k: synth_tensor(k, shape) for k, shape in state_dict_spec(50).items() if k.startswith(PREFIX)}


@functools.lru_cache(maxsize=None)
def net_inputs(case):
    """x [N, H, W, 4] f32 NHWC (unit normal, the fourth channel zero) and a unit-normal cotangent per map."""
    N, H, W = case
    g = _g(73000 + 1000 * N + 7 * H + W)
    x = torch.zeros(N, H, W, 4)
    x[..., :3] = torch.randn(N, H, W, 3, generator=g)
    cots, h, w = {}, (H - 1) // 2 + 1, (W - 1) // 2 + 1                 # the stem
    for i, (name, _, _, cout) in enumerate(RES_STAGES):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1                       # the pool, then every stage's stride-2 block
        cots[name] = torch.randn(N, h, w, cout, generator=g)
    return x, cots


def backbone_run(sd, x, cots, dtype, device="cpu"):
    """The network in plain torch in `dtype`: F.conv2d, the folded FrozenBN, F.relu, F.max_pool2d(3, 2, 1), residuals.  x NHWC
    [N, H, W, 4]; cots: {map: cotangent NHWC} over any subset of the maps -> ({map: NHWC}, {state-dict key: gradient} of the 53
    weights for the sum of <map, cotangent>)."""
    to = lambda t: t.to(device=device, dtype=dtype)
    P = {k: to(v) for k, v in sd.items()}
    Wt = {PREFIX + n + ".weight": P[PREFIX + n + ".weight"].clone().requires_grad_(True) for n in conv_names()}

    def cbn(t, name, stride=1, pad=0, relu=True, residual=None):
        q = PREFIX + name + ".norm."
        scale = P[q + "weight"] * torch.rsqrt(P[q + "running_var"] + BN_EPS)
        shift = P[q + "bias"] - P[q + "running_mean"] * scale
        z = F.conv2d(t, Wt[PREFIX + name + ".weight"], stride=stride, padding=pad) * scale[None, :, None, None] + shift[None, :, None, None]
        if residual is not None:
            z = z + residual
        return F.relu(z) if relu else z
    t = F.max_pool2d(cbn(to(x[..., :3]).permute(0, 3, 1, 2), "stem.conv1", 2, 3), 3, 2, 1)
    maps, cin = {}, 64
    for name, n, cmid, cout in RES_STAGES:
        for i in range(n):
            p = f"{name}.{i}"
            stride = 2 if (i == 0 and name != "res2") else 1
            y = cbn(cbn(t, p + ".conv1"), p + ".conv2", stride, 1)
            sc = cbn(t, p + ".shortcut", stride, 0, relu=False) if cin != cout else t
            t = cbn(y, p + ".conv3", residual=sc)
            cin = cout
        maps[name] = t
    total = sum((maps[k] * to(c).permute(0, 3, 1, 2)).sum() for k, c in cots.items())
    grads = torch.autograd.grad(total, list(Wt.values()))
    return ({k: v.detach().permute(0, 2, 3, 1).contiguous().cpu() for k, v in maps.items()},
            {k: g.detach().cpu() for k, g in zip(Wt, grads)})


@functools.lru_cache(maxsize=None)
def backbone_reference(case, which, dtype=F64):
    """(maps, grads) of the restatement at NET_CASES' `case` under COTANGENTS' `which`."""
    x, cots = net_inputs(case)
    return backbone_run(backbone_state_dict(), x, cots if which == "all" else {"res5": cots["res5"]}, dtype)


def norm_err(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max())


def norm_bound(case, which, key):
    """The bound of one tensor's normalised error in a run at (case, which)."""
    return max(LIMIT_FACTOR * F32_NORM_ERR[(case, which)][family_of(key)], NORM_FLOOR)


def f32_norm_err(case, which):
    """{family: the worst normalised error of the float32 restatement's 53 gradients at (case, which)}."""
    ref, got = backbone_reference(case, which)[1], backbone_reference(case, which, F32)[1]
    out = {}
    for k in ref:
        out[family_of(k)] = max(out.get(family_of(k), 0.0), norm_err(got[k], ref[k]))
    return out


def print_f32_worst():
    print('F32_WORST = {"dgrad": %.3g}' % f32_worst())
    for case in NET_CASES:
        for which in COTANGENTS:
            print("    (%r, %r): {%s}," % (case, which, ", ".join('"%s": %.3g' % kv for kv in f32_norm_err(case, which).items())))
