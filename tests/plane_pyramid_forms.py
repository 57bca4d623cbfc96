"""The training kernels of the plane head's top-down pyramid (csrc/pyramid_train.hip: training-mode BatchNorm statistics, apply and
backward in the plain and in the upsampled-source form, the bilinear 2x adjoint) and PlanePyramidTrainer as data: seeded cases, each
operation restated in plain torch (F.batch_norm(training=True), F.interpolate(scale_factor=2, mode="bilinear", align_corners=False);
float64 is the reference, differentiated with torch.autograd.grad; float32 is the restatement the limits are measured from), a
per-element allowance A_k = 2^-24 S_k + C_k for every element of every output (tests/refine_bwd_forms.py, tests/plane_decoder_forms.py:
the same construction and the same constants), and a float32 emulation of the kernels' formulas in which errors can be planted.
tests/test_plane_pyramid_forms_gpu.py and tests/test_plane_pyramid_training_gpu.py hold the kernels and the trainer to it;
tests/test_plane_pyramid_forms_cpu.py proves case lists, margins, references, constants and the sharpness of the bound.  Imports without
a GPU.

  S_k    the sum of the magnitudes of the terms that make element k, in float64: mean: sum |v| / n; var: the variance itself (its terms
         are squares); rstd: itself; a running statistic: (1 - m) |r| + m |stat|; y: [z > 0] (|gamma xhat| + |beta|) + |addend|;
         dgamma: sum |dz xhat|; dbeta: sum |dz|; dv: |gamma| rstd (|dz| + S_dbeta / n + |xhat| S_dgamma / n); the gradient at t and the
         bilinear adjoint: up2^T of the magnitudes (its weights are positive); where v = up2(t), |v| is up2(|t|).  Whole pyramid: the last
         accumulation of every gradient from the float64 restatement's own intermediates - |dC|^T |X| for a conv weight, the sums above
         for a BatchNorm's affine pair, |dC| |W| for memory and the backbone maps
  C_k    conditioning: the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input by
         1 +- 2^-23, and with them the intermediate tensors a float32 run rounds element by element (plane_decoder_forms.jiggle_tap):
         v = up2(t) of the upsampled form, and in the whole pyramid every intermediate tensor and the gradient arriving at it
  limit  LIMIT_FACTOR x max(F32_WORST[family], 1): the worst error / A of the float32 torch restatement over the cases of the family
         (measured on the CPU, never from a kernel; a CPU test re-measures it)

ReLU decisions: no pre-activation z of a case lies within its margin of 0 in float64 (MARGIN of tests/fused_forms.py, times
1 + |mean| rstd per channel: a float32 run rounds the mean by 2^-24 |mean|, which moves xhat by that times rstd - the "offset" case has
|mean| rstd = 1e3).  Marginal elements get their input moved and the case is evaluated again, statistics included, until none is left."""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g
from tests.fused_forms import MARGIN
from tests.plane_decoder_forms import jiggle_tap
from tests.refine_bwd_forms import DRAWS, EPS23, EPS24, F32, F64, LIMIT_FACTOR, _cot, ratios

RPS = 256                                    # rows per partial block of the new kernels (include/nopesac_hip.h NPS_BN_TRAIN_RPS; a CPU test compares)
SEGMENTS = 16                                # the finishing kernels merge the blocks' partials in this many runs of consecutive blocks: one more
                                             # block than runs (the last "plain" case, the last "up" case) makes a run of two
EPS, MOMENTUM = 1e-5, 0.1                    # nn.BatchNorm2d's defaults
OFFSET = 1e3                                 # |mean| / std of the "offset" case

# worst error / A of the float32 torch restatement over every case of the family.  Printed by
#   python -c "from tests import plane_pyramid_forms as P; P.print_f32_worst()"
# and re-measured by tests/test_plane_pyramid_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"stats": 2.69, "running": 1.77, "apply": 12.0, "backward": 12.2, "adjoint": 1.83, "pyramid": 10.4}


def limit(family):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


# ===================================================================================================================== cases
PLAIN_ROWS = (2, RPS - 1, RPS, RPS + 1, 2 * RPS + 1)
PLAIN_C = (4, 12, 64, 256)
UP_HW = ((1, 1), (1, 3), (3, 1), (2, 2), (3, 4), (5, 7))
UP_B = (1, 2)
UP_C = (4, 12, 256)
# ("plain", rows, C, tag) / ("up", B, H, W, C, tag).  base: ReLU, batch statistics (an addend on every other case); offset: |mean| / std =
# 1e3 in every channel; gamma0: gamma = 0 in every third channel; noact: no ReLU; frozen: stored statistics (batch_stats = False); slice:
# the source is a channel slice of a wider buffer
PLAIN_CASES = tuple(("plain", r, c, "base") for r in PLAIN_ROWS for c in PLAIN_C) + tuple(
    ("plain", RPS + 1, 12, t) for t in ("offset", "gamma0", "noact", "frozen", "slice")) + (
    ("plain", 2 * RPS + 1, 64, "offset"), ("plain", SEGMENTS * RPS + 1, 4, "base"))
UP_CASES = tuple(("up", b, h, w, c, "base") for h, w in UP_HW for b in UP_B for c in UP_C) + tuple(
    ("up", 2, 5, 7, 12, t) for t in ("offset", "gamma0", "noact", "frozen", "slice")) + (("up", 2, 3, 4, 256, "slice"), ("up", 2, 24, 24, 4, "base"))
BN_CASES = PLAIN_CASES + UP_CASES
ADJ_CASES = tuple((b, h, w, c) for h, w in UP_HW for b in UP_B for c in UP_C)
RUNNING_CALLS = (1, 3)


def up2(x):
    """nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) on an NHWC tensor."""
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def up2_t(g, shape):
    """The adjoint of up2 at a cotangent g [B, 2H, 2W, C] (float64 autograd on the linear map)."""
    x = torch.zeros(shape, dtype=g.dtype, requires_grad=True)
    return torch.autograd.grad(up2(x), x, g)[0]


def _v(c, src):
    """v [n, C] of a case from its source tensor."""
    return up2(src).reshape(-1, src.shape[-1]) if c["up"] else src.reshape(-1, src.shape[-1])


def _margin(v):
    """per channel: MARGIN (1 + |mean| rstd) of the float64 statistics of v [n, C]"""
    return MARGIN * (1 + v.mean(0).abs() / torch.sqrt(v.var(0, unbiased=False) + EPS))


def bn_z(c, src, dtype=F64):
    """(z [n, C], per-channel margin) of a case in `dtype`: the pre-activations of its BatchNorm."""
    v = _v(c, src.to(dtype))
    if c["batch_stats"]:
        mean, var = v.mean(0), v.var(0, unbiased=False)
    else:
        mean, var = c["run_mean"].to(dtype), c["run_var"].to(dtype)
    z = (v - mean) / torch.sqrt(var + EPS) * c["gamma"].to(dtype) + c["beta"].to(dtype)
    return z, (_margin(v) if c["batch_stats"] else MARGIN * (1 + mean.abs() / torch.sqrt(var + EPS)))


@functools.lru_cache(maxsize=None)
def bn_inputs(key):
    """One BatchNorm case: src (plain: [rows, C]; up: t [B, H, W, C]; `slice`: a channel slice of `buf`), gamma, beta, the cotangent g at y,
    an addend or None, stored statistics run_mean / run_var (the running buffers' start, and the statistics of `frozen`).  Settled: an
    element of src whose z (plain), or which is the dominant tap (dst // 2) of an output whose z (up), lies within twice the margin of 0
    is moved by a quarter of its channel's standard deviation, until none is left; where a channel holds one distinct value (1 x 1,
    B = 1: z = beta whatever the input) its beta is moved away from 0 instead."""
    up, tag = key[0] == "up", key[-1]
    if up:
        _, B, H, W, C, _ = key
        shape = (B, H, W)
        seed = 61000 + 1000 * B + 131 * H + 17 * W + C
    else:
        _, rows, C, _ = key
        shape = (rows,)
        seed = 60000 + 7 * rows + C
    g = _g(seed + 100003 * ("base", "offset", "gamma0", "noact", "frozen", "slice").index(tag))
    Cb = C + 8 if tag == "slice" else C
    scale = 0.5 + 1.5 * torch.rand(Cb, generator=g)
    shift = torch.randn(Cb, generator=g)
    if tag == "offset":
        shift = OFFSET * scale * (2.0 * torch.randint(0, 2, (Cb,), generator=g).float() - 1)
    buf = torch.randn(*shape, Cb, generator=g) * scale + shift
    src = buf[..., 4:4 + C] if tag == "slice" else buf
    gamma = (0.5 + torch.rand(C, generator=g)) * (2.0 * torch.randint(0, 2, (C,), generator=g).float() - 1)
    if tag == "gamma0":
        gamma[::3] = 0.0
    beta = 0.3 * torch.randn(C, generator=g)
    beta = torch.where(beta < 0, beta - 0.01, beta + 0.01)             # (where gamma = 0, z = beta: it keeps its distance from 0 too)
    n = (4 if up else 1) * int(torch.tensor(shape).prod())
    out_shape = (B, 2 * H, 2 * W, C) if up else (rows, C)
    c = dict(key=key, up=up, tag=tag, C=C, n=n, shape=shape, out_shape=out_shape, buf=buf, src=src, gamma=gamma, beta=beta,
             g=_cot(g, *out_shape), addend=torch.randn(*out_shape, generator=g) if (seed + len(tag)) % 2 else None,
             relu=tag != "noact", batch_stats=tag != "frozen",
             run_mean=(shift + 0.1 * scale * torch.randn(Cb, generator=g))[4 if tag == "slice" else 0:][:C].clone(),
             run_var=((scale * (0.8 + 0.4 * torch.rand(Cb, generator=g))) ** 2)[4 if tag == "slice" else 0:][:C].clone())
    for _ in range(64):
        z, margin = bn_z(c, src)
        bad = (z.abs() <= 2 * margin) & (c["gamma"] != 0)
        if not c["relu"] or not bad.any():
            break
        flat = bad.any(0) & (_v(c, src.double()).var(0, unbiased=False) == 0)      # one distinct value per channel (1 x 1, B = 1): z = beta
        beta[flat] += torch.where(beta < 0, -4 * margin.float(), 4 * margin.float())[flat]
        bad = (bad & ~flat).view(out_shape)
        if up:
            bad = bad.view(B, H, 2, W, 2, C).any(4).any(2)
        src[bad] += (0.25 * scale[4 if tag == "slice" else 0:][:C]).expand(src.shape)[bad]
    else:
        raise AssertionError("bn_inputs%r: the ReLU margins did not settle" % (key,))
    return c


BN_FLOATS = ("src", "gamma", "beta", "g", "addend", "run_mean", "run_var")
STATS_OUT = ("mean", "var", "rstd")
RUNNING_OUT = tuple("%s%d" % (n, k) for k in RUNNING_CALLS for n in ("run_mean", "run_var"))
OUTPUTS = {"stats": STATS_OUT, "running": RUNNING_OUT, "apply": ("y",), "backward": ("dsrc", "dgamma", "dbeta"), "adjoint": ("dx",)}


def bn_run(c, x, dtype, tap=None):
    """Every output of a BatchNorm case from plain torch in `dtype`: the statistics, the running buffers after RUNNING_CALLS calls (batch
    statistics only), y, and the VJP of sum(y g) at src, gamma and beta.  `tap` (the conditioning draws' jiggle_tap) is applied to the
    one intermediate tensor a float32 run rounds element by element before the statistics see it: v = up2(t) of the upsampled form
    (where every output of a channel has the same value - 1 x 1, B = 1 - v - mean is an exact cancellation that survives any change of
    the inputs, and no rounding of v)."""
    src, gamma, beta = (x[k].to(dtype).clone().requires_grad_(True) for k in ("src", "gamma", "beta"))
    v = _v(c, src)
    if tap is not None and c["up"]:
        v = tap(v)
    rm, rv = x["run_mean"].to(dtype).clone(), x["run_var"].to(dtype).clone()
    out = {}
    if c["batch_stats"]:
        with torch.no_grad():
            for k in range(1, max(RUNNING_CALLS) + 1):
                F.batch_norm(v, rm, rv, gamma, beta, True, MOMENTUM, EPS)
                if k in RUNNING_CALLS:
                    out["run_mean%d" % k], out["run_var%d" % k] = rm.clone(), rv.clone()
            out["mean"], out["var"] = v.mean(0), v.var(0, unbiased=False)
            out["rstd"] = 1.0 / torch.sqrt(out["var"] + EPS)
        z = F.batch_norm(v, None, None, gamma, beta, True, MOMENTUM, EPS)
    else:
        z = F.batch_norm(v, rm, rv, gamma, beta, False, MOMENTUM, EPS)
    y = (torch.relu(z) if c["relu"] else z).view(c["out_shape"])
    out["y"] = (y + x["addend"].to(dtype) if c["addend"] is not None else y).detach()
    grads = torch.autograd.grad((y * x["g"].to(dtype)).sum(), [src, gamma, beta])
    out["dsrc"], out["dgamma"], out["dbeta"] = (t.detach() for t in grads)
    return out


def bn_mags(c, x):
    """S of every output of bn_run (float64)."""
    src, gamma, beta, g = (x[k].double() for k in ("src", "gamma", "beta", "g"))
    C, n = c["C"], c["n"]
    v, va = _v(c, src), _v(c, src.abs())
    S = {}
    if c["batch_stats"]:
        mean, var = v.mean(0), v.var(0, unbiased=False)
        S["mean"], S["var"] = va.mean(0), var
        S["rstd"] = 1.0 / torch.sqrt(var + EPS)
        rm, rv, sm, sv = x["run_mean"].double().abs(), x["run_var"].double().abs(), x["run_mean"].double().abs(), x["run_var"].double().abs()
        for k in range(1, max(RUNNING_CALLS) + 1):
            sm = (1 - MOMENTUM) * sm + MOMENTUM * S["mean"]
            sv = (1 - MOMENTUM) * sv + MOMENTUM * var * n / (n - 1)
            if k in RUNNING_CALLS:
                S["run_mean%d" % k], S["run_var%d" % k] = sm, sv
    else:
        mean, var = x["run_mean"].double(), x["run_var"].double()
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (v - mean) * rstd
    z = xh * gamma + beta
    gate = (z > 0).double() if c["relu"] else torch.ones_like(z)
    S["y"] = (gate * ((gamma * xh).abs() + beta.abs())).view(c["out_shape"])
    if c["addend"] is not None:
        S["y"] = S["y"] + x["addend"].double().abs()
    dz = (g.reshape(-1, C) * gate).abs()
    S["dgamma"], S["dbeta"] = (dz * xh.abs()).sum(0), dz.sum(0)
    stat = 1.0 / n if c["batch_stats"] else 0.0
    dv = gamma.abs() * rstd * (dz + stat * S["dbeta"] + stat * xh.abs() * S["dgamma"])
    S["dsrc"] = up2_t(dv.view(c["out_shape"]), tuple(src.shape)) if c["up"] else dv.view(src.shape)
    return S


def adjoint_inputs(key):
    B, H, W, C = key
    g = _g(62000 + 1000 * B + 131 * H + 17 * W + C)
    return dict(key=key, x=torch.randn(B, H, W, C, generator=g), du=_cot(g, B, 2 * H, 2 * W, C))


def adjoint_run(c, x, dtype):
    return {"dx": up2_t(x["du"].to(dtype), tuple(c["x"].shape))}


def adjoint_mags(c, x):
    return {"dx": up2_t(x["du"].double().abs(), tuple(c["x"].shape))}


# ===================================================================================================================== the kernels' formulas
def up2_axis_matrix(n, dtype=F64):
    """[2n, n]: up2 along one axis, from the source-index rule (src = max(0.5 (dst + 0.5) - 0.5, 0), i1 = min(i0 + 1, n - 1))."""
    M = torch.zeros(2 * n, n, dtype=dtype)
    for o in range(2 * n):
        s = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        M[o, i0] += 1.0 - (s - i0)
        M[o, i1] += s - i0
    return M


def adjoint_axis_matrix(n, fold=True, dtype=F64):
    """[n, 2n]: the gather of the adjoint along one axis as the kernel states it: dx[i] = 0.75 (du[2i] + du[2i+1]) + 0.25 (du[2i-1] +
    du[2i+2]), taps outside [0, 2n) dropped and, with `fold`, the clamped border taps folded back in (du[0] and du[2n-1] weigh 1)."""
    M = torch.zeros(n, 2 * n, dtype=dtype)
    for i in range(n):
        for o, w in ((2 * i - 1, 0.25), (2 * i, 0.75), (2 * i + 1, 0.75), (2 * i + 2, 0.25)):
            if 0 <= o < 2 * n:
                M[i, o] = w
    if fold:
        M[0, 0] = 1.0
        M[n - 1, 2 * n - 1] = 1.0
    return M


def adjoint_by_matrices(du, fold=True):
    """up2^T(du) [B, 2H, 2W, C] -> [B, H, W, C] through the two axis matrices (in du's dtype)."""
    H, W = du.shape[1] // 2, du.shape[2] // 2
    return torch.einsum("iy,byxc,jx->bijc", adjoint_axis_matrix(H, fold, du.dtype), du, adjoint_axis_matrix(W, fold, du.dtype))


BN_PLANTS = ("one_pass_variance", "border_foldback_dropped", "dgamma_term_omitted", "unbiased_variance")


def emulate_bn(key, plant=None):
    """The kernels' formulas in f32: two-pass statistics, z = gamma ((v - mean) rstd) + beta, dz = g [z > 0], dgamma = sum dz xhat,
    dbeta = sum dz, dv = gamma rstd ((dz - dbeta / n) - xhat dgamma / n), the gradient at t through the adjoint's axis matrices -
    without the blocks (a change of summation order only)."""
    c = bn_inputs(key)
    n, C = c["n"], c["C"]
    v = _v(c, c["src"])
    out = {}
    if c["batch_stats"]:
        mean = v.mean(0)
        var = ((v * v).mean(0) - mean * mean) if plant == "one_pass_variance" else ((v - mean) ** 2).mean(0)
        out["mean"], out["var"] = mean, var
        norm_var = var * n / (n - 1) if plant == "unbiased_variance" else var
        rm, rv = c["run_mean"].clone(), c["run_var"].clone()
        for k in range(1, max(RUNNING_CALLS) + 1):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1 - MOMENTUM) * rv + MOMENTUM * (var * (n / (n - 1)))
            if k in RUNNING_CALLS:
                out["run_mean%d" % k], out["run_var%d" % k] = rm, rv
    else:
        mean, norm_var = c["run_mean"], c["run_var"]
    rstd = 1.0 / torch.sqrt(norm_var + torch.tensor(EPS, dtype=F32))
    if c["batch_stats"]:
        out["rstd"] = rstd
    xh = (v - mean) * rstd
    z = c["gamma"] * xh + c["beta"]
    y = (torch.relu(z) if c["relu"] else z).view(c["out_shape"])
    out["y"] = y + c["addend"] if c["addend"] is not None else y
    dz = c["g"].reshape(-1, C) * ((z > 0).float() if c["relu"] else 1.0)
    out["dgamma"], out["dbeta"] = (dz * xh).sum(0), dz.sum(0)
    stat = 1.0 / n if c["batch_stats"] else 0.0
    dv = (c["gamma"] * rstd) * ((dz - out["dbeta"] * stat) - (0.0 if plant == "dgamma_term_omitted" else xh * (out["dgamma"] * stat)))
    out["dsrc"] = adjoint_by_matrices(dv.view(c["out_shape"]), plant != "border_foldback_dropped") if c["up"] else dv.view(c["src"].shape)
    return out


# ===================================================================================================================== the whole pyramid
PREFIX = "sem_seg_head.top_down."
CONVS = ("up_conv3", "up_conv2", "up_conv1", "c4_conv", "c3_conv", "c2_conv", "c1_conv", "m_conv_dict.m4")
LEVELS = ("res2", "res3", "res4", "res5")
PYR_CASES = ((2, 6, 8),)                     # (B, res5's h, w): p1 at 8x that
PYR_TIE_IN = (1, 15, 20)                     # the production size: one tie-in of the trainer, its float64 reference evaluated on the GPU


def pyramid_parameter_names(keys):
    return sorted(k for k in keys if k.startswith(PREFIX) and k.split(".")[-1] not in ("running_mean", "running_var", "num_batches_tracked"))


def pyramid_buffer_names(keys):
    return sorted(k for k in keys if k.startswith(PREFIX) and k.split(".")[-1] in ("running_mean", "running_var"))


def cotangent(seed, B, h, w):
    """The seeded gradient at p1 [B, 8h, 8w, 256] NHWC that the golden generator and the tests share."""
    g = _g(63000 + seed)
    d = _cot(g, B, 8 * h, 8 * w, 256) / 16.0
    d[:, 0, 1] = 0.0
    return d


def pyramid_forward(sd, bufs, feats, memory, B, batch_stats=True, rec=None, tap=None):
    """The reference's top_down.forward (planeTR_head.py:241-252) in its own operation order - the up convs run AFTER the upsampling, at
    the high resolution - on NHWC tensors (a 1x1 conv without bias is a matrix product over the pixels; a CPU test compares with the
    nn.Conv2d / nn.BatchNorm2d / nn.Upsample modules) -> p1 NHWC.  sd: the 24 parameters, bufs: the 16 running statistics (updated in
    place by a batch-statistics run, as nn.BatchNorm2d does).  rec(name, x, c, z) sees every conv + BatchNorm (input, conv output and
    pre-activation as [pixels, C] matrices); `tap` every intermediate tensor."""
    tap = tap or (lambda t: t)
    rec = rec or (lambda name, x, c, z: None)

    def cbr(x, nm):
        q = PREFIX + nm
        w = sd[q + ".0.weight"]
        x2 = x.reshape(-1, x.shape[-1])
        c = tap(x2 @ w.view(w.shape[0], -1).t())
        z = tap(F.batch_norm(c, bufs[q + ".1.running_mean"], bufs[q + ".1.running_var"], sd[q + ".1.weight"], sd[q + ".1.bias"], batch_stats,
                             MOMENTUM, EPS))
        rec(q, x2, c, z)
        return tap(torch.relu(z)).view(*x.shape[:-1], w.shape[0])
    hc, wc = feats["res5"].shape[1:3]
    p = tap(cbr(feats["res5"], "c4_conv") + cbr(memory.view(B, hc, wc, 256), "m_conv_dict.m4"))
    for nm, lat, lvl in (("up_conv3", "c3_conv", "res4"), ("up_conv2", "c2_conv", "res3"), ("up_conv1", "c1_conv", "res2")):
        p = tap(cbr(tap(up2(p)), nm) + cbr(feats[lvl], lat))
    return p


def pyramid_margins(sd, bufs, feats, memory, B, batch_stats=True, device="cpu"):
    """{conv: (z [n, C], per channel the margin)} of the float64 forward (evaluated on `device`)."""
    out = {}
    f64 = lambda t: t.to(device=device, dtype=F64)

    def rec(q, x, c, z):
        out[q] = (z.detach(), _margin(c.detach()))
    with torch.no_grad():
        pyramid_forward({k: f64(v) for k, v in sd.items()}, {k: f64(v).clone() for k, v in bufs.items()},
                        {k: f64(v) for k, v in feats.items()}, f64(memory), B, batch_stats, rec=rec)
    return out


def settle_biases(sd, bufs, feats, memory, B, device="cpu"):
    """Move, in place, the BatchNorm bias of every channel of sd that has a z within twice its margin of 0 (the statistics do not depend
    on the bias): by the smallest shift that puts 0 into the middle of a gap of at least six margins between the channel's sorted z
    values; the pass is repeated, coarse levels first, until nothing moves.  `device`: where the float64 passes run."""
    for _ in range(64):
        moved = False
        for q, (z, margin) in pyramid_margins(sd, bufs, feats, memory, B, device=device).items():
            for ch in (z.abs().amin(0) <= 2 * margin).nonzero().flatten().tolist():
                zs = torch.cat([z[:, ch].sort().values, z[:, ch].max().view(1) + 1.0])
                mid, wide = (zs[1:] + zs[:-1]) / 2, (zs[1:] - zs[:-1]) >= 6 * margin[ch]
                sd[q + ".1.bias"][ch] -= float(mid[wide][mid[wide].abs().argmin()])
                moved = True
        if not moved:
            return
    raise AssertionError("settle_biases: the ReLU margins did not settle")


GOLDEN = "L_plane_pyramid_%dx%d.npz"         # tests/golden/: the reference's top_down in train mode (scripts/gen_plane_pyramid_golden.py)


def golden(h, w):
    import os

    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN % (h, w)))


@functools.lru_cache(maxsize=None)
def pyramid_inputs(key, device="cpu"):
    """(sd: the 24 f32 parameters of the name-seeded synthetic checkpoint with settled BatchNorm biases, bufs: its 16 running statistics,
    feats: the backbone maps of tests/golden_inputs.feature_maps as NHWC, memory [B Lm, 256], d_p1).  A key of PYR_CASES is the fixture's
    case: the feature seed, the reference encoder's memory and the biases its generator settled and gave the reference come from the
    fixture; any other key (the tie-in) draws a memory and settles here, on `device`.  The tensors returned are on the CPU."""
    from nopesac_amd.synth import synth_state_dict
    from tests.golden_inputs import feature_maps
    B, h, w = key
    full = synth_state_dict(7)
    sd = {k: full[k].float().clone() for k in pyramid_parameter_names(full.keys())}
    bufs = {k: full[k].float().clone() for k in pyramid_buffer_names(full.keys())}
    if key in PYR_CASES:
        gold = golden(h, w)
        seed = int(gold["seed"])
        memory = torch.from_numpy(gold["memory"]).clone()
        for k in sd:
            if k.endswith(".1.bias"):
                sd[k] = torch.from_numpy(gold["bias." + k]).clone()
    else:
        seed = 1
        memory = torch.randn(B * h * w, 256, generator=_g(64000 + 100 * B + 17 * h + w))
    feats = {k: v.float().permute(0, 2, 3, 1).contiguous() for k, v in feature_maps(seed, h, w, batch=B).items() if k in LEVELS}
    if key not in PYR_CASES:
        settle_biases(sd, bufs, feats, memory, B, device)
    return dict(key=key, B=B, h=h, w=w, sd=sd, bufs=bufs, feats=feats, memory=memory, d_p1=cotangent(seed, B, h, w))


def pyramid_run(c, x, dtype, mags=False, tap=None, batch_stats=True, device="cpu"):
    """p1, the running statistics after one forward, and the VJP of sum(p1 d_p1) at the 24 parameters, the memory and the four backbone
    maps.  x: {"memory", "d_p1", "res2" .. "res5", parameter and buffer keys}.  With `mags` also S.  Plain torch on `device`."""
    to = lambda t: t.to(device=device, dtype=dtype).clone()
    sd = {k: to(x[k]).requires_grad_(True) for k in c["sd"]}
    bufs = {k: to(x[k]) for k in c["bufs"]}
    feats = {k: to(x[k]).requires_grad_(True) for k in LEVELS}
    memory = to(x["memory"]).requires_grad_(True)
    recs = []

    def rec(q, xin, cv, z):
        if mags:
            cv.retain_grad()
            z.retain_grad()
            recs.append((q, xin, cv, z))
    p1 = pyramid_forward(sd, bufs, feats, memory, c["B"], batch_stats, rec=rec, tap=tap)
    (p1 * to(x["d_p1"])).sum().backward()
    out = {k: sd[k].grad.detach() for k in sd}
    out.update({k: feats[k].grad.detach() for k in LEVELS})
    out["memory"] = memory.grad.detach()
    out["p1"] = p1.detach()
    out.update({k: v.detach() for k, v in bufs.items()})
    if not mags:
        return out
    S = {}
    src = {"c4_conv": "res5", "c3_conv": "res4", "c2_conv": "res3", "c1_conv": "res2", "m_conv_dict.m4": "memory"}
    for q, xin, cv, z in recs:
        xa, dc, dz, v = xin.detach().abs(), cv.grad.abs(), z.grad.abs(), cv.detach()
        n = v.shape[0]
        mean, var = v.mean(0), v.var(0, unbiased=False)
        rm, rv = to(x[q + ".1.running_mean"]), to(x[q + ".1.running_var"])
        xh = (v - mean) / torch.sqrt(var + EPS) if batch_stats else (v - rm) / torch.sqrt(rv + EPS)
        w = sd[q + ".0.weight"].detach()
        S[q + ".0.weight"] = (dc.t() @ xa).view(w.shape)
        S[q + ".1.weight"], S[q + ".1.bias"] = (dz * xh.abs()).sum(0), dz.sum(0)
        S[q + ".1.running_mean"] = (1 - MOMENTUM) * rm.abs() + MOMENTUM * v.abs().mean(0) if batch_stats else rm.abs()
        S[q + ".1.running_var"] = (1 - MOMENTUM) * rv.abs() + MOMENTUM * var * n / (n - 1) if batch_stats else rv.abs()
        nm = q[len(PREFIX):]
        if nm in src:
            S[src[nm]] = (dc @ w.view(w.shape[0], -1).abs()).view(out[src[nm]].shape)
        if nm in ("up_conv1", "c1_conv"):
            term = (z.detach() > 0).double() * ((xh * sd[q + ".1.weight"].detach()).abs() + sd[q + ".1.bias"].detach().abs())
            S["p1"] = S.get("p1", 0) + term.view(out["p1"].shape)
    return out, S


def _pyramid_x(c):
    return dict(c["sd"], **c["bufs"], **c["feats"], memory=c["memory"], d_p1=c["d_p1"])


def sign_tap(g, device="cpu"):
    """plane_decoder_forms.jiggle_tap with the signs drawn on `device` from the generator g of that device: every intermediate tensor, and
    the gradient that arrives at it, times 1 +- 2^-23 per element."""
    sign = lambda t: torch.where(torch.randint(0, 2, t.shape, generator=g, device=device, dtype=torch.int8) > 0, 1 + EPS23, 1 - EPS23).to(t.dtype)

    def tap(t):
        y = t * sign(t)
        if y.requires_grad:
            y.register_hook(lambda gr: gr * sign(gr))
        return y
    return tap


@functools.lru_cache(maxsize=None)
def pyramid_reference(key, device="cpu"):
    """-> (ref, A) of pyramid_inputs(key) through batch statistics (pyramid_reference_for)."""
    return pyramid_reference_for(pyramid_inputs(key, device), device)


def pyramid_reference_for(c, device="cpu", batch_stats=True):
    """-> (ref, A) over the 24 gradients, "memory", "res2" .. "res5", "p1" and the 16 running statistics after one forward (unchanged
    with batch_stats=False: the stored statistics normalise), for inputs in pyramid_inputs' form.  `device`: where the float64
    restatement and its draws are evaluated (the production-size case takes 20 s on a CPU); results on the CPU."""
    x = _pyramid_x(c)
    ref, S = pyramid_run(c, x, F64, mags=True, device=device, batch_stats=batch_stats)
    g = torch.Generator(device=device).manual_seed(81)
    tap = sign_tap(g, device)
    jig = lambda t: tap(t.to(device=device, dtype=F64))
    C = {k: torch.zeros_like(ref[k]) for k in ref}
    for _ in range(DRAWS):
        got = pyramid_run(c, {k: jig(v) for k, v in x.items()}, F64, tap=tap, device=device, batch_stats=batch_stats)
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return {k: v.cpu() for k, v in ref.items()}, {k: (EPS24 * S[k] + C[k]).cpu() for k in ref}


# ===================================================================================================================== references
INPUTS = {"stats": bn_inputs, "running": bn_inputs, "apply": bn_inputs, "backward": bn_inputs, "adjoint": adjoint_inputs}


def family_keys(family):
    if family in ("stats", "running"):
        return [k for k in BN_CASES if k[-1] != "frozen"]
    return {"apply": list(BN_CASES), "backward": list(BN_CASES), "adjoint": list(ADJ_CASES), "pyramid": list(PYR_CASES)}[family]


@functools.lru_cache(maxsize=None)
def _reference(group, key):
    c = (bn_inputs if group == "bn" else adjoint_inputs)(key)
    run, mags = (bn_run, bn_mags) if group == "bn" else (adjoint_run, adjoint_mags)
    x = {k: c[k] for k in (BN_FLOATS if group == "bn" else ("du",)) if c[k] is not None}
    ref, S = run(c, x, F64), mags(c, x)
    g = _g(83)
    jig = lambda t: t.double() * (1 + EPS23 * (2.0 * torch.randint(0, 2, t.shape, generator=g).double() - 1))
    C = {k: torch.zeros_like(S[k]) for k in S}
    for _ in range(DRAWS):
        got = run(c, {k: jig(v) for k, v in x.items()}, F64, **({"tap": jiggle_tap(g)} if group == "bn" else {}))
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return ref, {k: EPS24 * S[k] + C[k] for k in S}


def reference(family, key, device="cpu"):
    """-> (ref, A): the float64 result and the allowance 2^-24 S + C per element, over the family's outputs."""
    if family == "pyramid":
        return pyramid_reference(key, device)
    ref, A = _reference("adjoint" if family == "adjoint" else "bn", key)
    return {k: ref[k] for k in OUTPUTS[family]}, {k: A[k] for k in OUTPUTS[family]}


def worst_ratio(family, key, got, device="cpu"):
    """{output: (worst error / A, flat index)} of `got` over the family's outputs (pyramid: over the keys `got` holds)."""
    ref, A = reference(family, key, device)
    out = {}
    for k in (got if family == "pyramid" else ref):
        assert tuple(got[k].shape) == tuple(ref[k].shape), (k, got[k].shape, ref[k].shape)
        q = ratios(got[k].cpu(), ref[k], A[k]).reshape(-1)
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        out[k] = (float(q.max()), int(q.argmax())) if q.numel() else (0.0, -1)
    return out


def fixture_view(full):
    """The fixture's keys and subsamplings (scripts/gen_plane_pyramid_golden.py) of a full result dict with pyramid_run's keys."""
    out = {"p1_sub": full["p1"][:, ::4, ::4], "d_memory": full["memory"], "d_res5_sub": full["res5"][..., ::32]}
    for k, t in full.items():
        if k.startswith(PREFIX):
            if k.split(".")[-1] in ("running_mean", "running_var"):
                out[k] = t
            else:
                out["d." + k] = t[::16] if t.dim() == 4 else t
    return out


def fixture_worst(key, view, device="cpu"):
    """{fixture key: worst error / A} of results in the fixture's form (the fixture itself, or fixture_view of a run)."""
    ref, A = reference("pyramid", key, device)
    rv, av = fixture_view(ref), fixture_view(A)
    assert len(rv) == 3 + 16 + 24
    out = {}
    for k in rv:
        t = view[k] if torch.is_tensor(view[k]) else torch.from_numpy(view[k])
        assert tuple(t.shape) == tuple(rv[k].shape), (k, t.shape, rv[k].shape)
        q = ratios(t.cpu(), rv[k], av[k])
        out[k] = float(torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).max())
    return out


@functools.lru_cache(maxsize=None)
def f32_restatement(family, key):
    if family == "pyramid":
        c = pyramid_inputs(key)
        return pyramid_run(c, _pyramid_x(c), F32)
    c = INPUTS[family](key)
    if family == "adjoint":
        return adjoint_run(c, {"du": c["du"]}, F32)
    got = bn_run(c, {k: c[k] for k in BN_FLOATS if c[k] is not None}, F32)
    return {k: got[k] for k in OUTPUTS[family]}


def f32_worst(family):
    return max(q for key in family_keys(family) for q, _ in worst_ratio(family, key, f32_restatement(family, key)).values())


def print_f32_worst():
    for family in F32_WORST:
        print('"%s": %.3g,' % (family, f32_worst(family)))
