"""The grouped training-mode BatchNorm kernels of the camera head's conv stacks (csrc/camera_bn_train.hip: statistics with the running
update, apply and backward over G groups of rows of one tensor) and CameraHeadTrainer(batch_stats=True) as data: seeded cases, each
operation restated in plain torch (F.batch_norm(training=True) per group, the groups in order; float64 is the reference, differentiated
with torch.autograd.grad; float32 is the restatement the limits are measured from), a per-element allowance A_k = 2^-24 S_k + C_k for
every element of every output - the construction, the S_k terms and the constants of tests/plane_pyramid_forms.py - and a float32
emulation of the kernels' formulas in which errors can be planted.  tests/test_camera_bn_forms_gpu.py and
tests/test_camera_bn_training_gpu.py hold the kernels and the trainer to it; tests/test_camera_bn_forms_cpu.py proves case lists, margins,
references, constants and the sharpness of the bound.  Imports without a GPU.

  S_k    the sum of the magnitudes of the terms that make element k, in float64, per group g: mean: sum |c| / n; var: the variance
         itself; rstd: itself; a running statistic: r <- (1 - m) |r| + m |stat_g| through the groups and calls; y: a (|gamma xhat| +
         |beta|), a = |act'(z)| (1, or the slope 0.01 where a LeakyReLU is closed, 0 where a ReLU is); dgamma: sum_g sum |dz xhat|;
         dbeta: sum_g sum |dz|; dc: |gamma| rstd_g (|dz| + S1_g / n + |xhat| S2_g / n) with S1_g, S2_g the group's own magnitude sums
  C_k    conditioning: the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input by 1 +- 2^-23
  limit  LIMIT_FACTOR x max(F32_WORST[family], 1): the worst error / A of the float32 torch restatement over the cases of the family
         (measured on the CPU, never from a kernel; a CPU test re-measures it)

Activation decisions: no pre-activation z of a RELU or LEAKY case lies within its margin of 0 in float64 (MARGIN of tests/fused_forms.py,
times 1 + |mean_g| rstd_g per channel and group, as in the pyramid's forms).  Marginal elements get their input moved and the case is
evaluated again, statistics included, until none is left.

In every G = 2 case the second group's rows are drawn with another mean and another scale per channel than the first's: kernels that
pool the groups cannot pass.

The trainer: TRAINER_F32 holds, per parameter tensor, the error of a float32 torch run of the oracle's training-mode camera head under
batch statistics against the float64 run (both with the float32 run's LeakyReLU sides and max-pool winners), in the measure of
tests/test_pose_net_training_gpu.py: max |error| / max(|ref|_max, 1e-4 of the largest gradient).  The trainer's bound per tensor is
max(3e-3, LIMIT_FACTOR x that figure)."""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g
from tests.fused_forms import LEAK, MARGIN
from tests.refine_bwd_forms import DRAWS, EPS23, EPS24, F32, F64, LIMIT_FACTOR, _cot, ratios

RPS = 256                                    # rows of a group per partial block (include/nopesac_hip.h NPS_BN_GROUPED_RPS; a CPU test compares)
SEGMENTS = 16                                # runs of consecutive blocks in the finishing kernels (NPS_BN_GROUPED_SEGMENTS): one block more
                                             # than runs makes a run of two
EPS, MOMENTUM = 1e-3, 0.01                   # nn.BatchNorm2d(eps=0.001, momentum=0.01), camera_modules.py:45
OFFSET = 1e3                                 # |mean| / std of the "offset" case
ACTS = {"none": 0, "relu": 1, "leaky": 2}    # NPS_ACT_* (a CPU test compares)

# worst error / A of the float32 torch restatement over every case of the family.  Printed by
#   python -c "from tests import camera_bn_forms as P; P.print_f32_worst()"
# and re-measured by tests/test_camera_bn_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"stats": 4.9, "running": 2.91, "apply": 10.3, "backward": 6.03}


def limit(family):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


# ===================================================================================================================== cases
ROWS = (2, 6, RPS - 1, RPS, RPS + 1, 2 * RPS + 1, SEGMENTS * RPS + 1)       # per group
GROUPS = (1, 2)
CHANNELS = (4, 128, 256)
TAGS = ("leaky", "relu", "none", "offset", "gamma0", "neggamma")
TAG_SHAPE = (RPS + 1, 2, 128)
# (rows per group, G, C, tag).  leaky: LeakyReLU(0.01), signs of gamma mixed; relu / none: the other activations; offset: |mean| / std = 1e3
# in every channel and group (LeakyReLU); gamma0: gamma = 0 in every third channel; neggamma: every gamma negative
CASES = tuple((n, G, C, "leaky") for n in ROWS for G in GROUPS for C in CHANNELS) + tuple(TAG_SHAPE + (t,) for t in TAGS[1:])
RUNNING_CALLS = (1, 3)


def _act(z, act):
    if act == "none":
        return z
    return torch.where(z > 0, z, (LEAK if act == "leaky" else 0.0) * z)


def _slope(z, act):
    """|act'(z)| per element"""
    if act == "none":
        return torch.ones_like(z)
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LEAK if act == "leaky" else 0.0))


def bn_z(c, src, dtype=F64):
    """(z [G, n, C], margin [G, 1, C]) of a case in `dtype`: the pre-activations of its BatchNorm, per group."""
    v = src.to(dtype).view(c["G"], c["n"], c["C"])
    mean, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (v - mean) * rstd * c["gamma"].to(dtype) + c["beta"].to(dtype), MARGIN * (1 + mean.abs() * rstd)


@functools.lru_cache(maxsize=None)
def bn_inputs(key):
    """One case: src [G n, C] (group g = rows [g n, (g + 1) n), every group with its own mean and scale per channel), gamma, beta, the
    cotangent g at y, the running buffers' start.  Settled: an element whose z lies within twice the margin of 0 is moved by a quarter of
    its channel's standard deviation, until none is left."""
    n, G, C, tag = key
    g = _g(71000 + 13 * n + 1009 * G + C + 100003 * TAGS.index(tag))
    scale = 0.5 + torch.rand(1, 1, C, generator=g)
    shift = torch.randn(1, 1, C, generator=g) * 2.0
    if G == 2:                                                         # group 1: the scale 1.5 to 2 times larger or smaller, the mean at
        factor = 1.5 + 0.5 * torch.rand(1, 1, C, generator=g)          # least the sum of both scales away
        scale = torch.cat([scale, torch.where(torch.rand(1, 1, C, generator=g) < 0.5, scale * factor, scale / factor)])
        away = (2.0 * torch.randint(0, 2, (1, 1, C), generator=g).float() - 1) * (1 + torch.rand(1, 1, C, generator=g))
        shift = torch.cat([shift, shift + away * scale.sum(0, keepdim=True)])
    if tag == "offset":
        shift = OFFSET * scale * (2.0 * torch.randint(0, 2, (G, 1, C), generator=g).float() - 1)
    src = (torch.randn(G, n, C, generator=g) * scale + shift).view(G * n, C)
    gamma = (0.5 + torch.rand(C, generator=g)) * (2.0 * torch.randint(0, 2, (C,), generator=g).float() - 1)
    if tag == "gamma0":
        gamma[::3] = 0.0
    if tag == "neggamma":
        gamma = -gamma.abs()
    beta = 0.3 * torch.randn(C, generator=g)
    beta = torch.where(beta < 0, beta - 0.01, beta + 0.01)             # (where gamma = 0, z = beta: it keeps its distance from 0 too)
    act = tag if tag in ("relu", "none") else "leaky"
    c = dict(key=key, n=n, G=G, C=C, tag=tag, act=act, src=src, gamma=gamma, beta=beta, g=_cot(g, G * n, C),
             run_mean=(shift[0, 0] + 0.1 * scale[0, 0] * torch.randn(C, generator=g)).clone(),
             run_var=((scale[0, 0] * (0.8 + 0.4 * torch.rand(C, generator=g))) ** 2).clone())
    for _ in range(64):
        z, margin = bn_z(c, src)
        bad = ((z.abs() <= 2 * margin) & (gamma != 0)).view(G * n, C)
        if act == "none" or not bad.any():
            break
        src[bad] += (0.25 * scale).expand(G, n, C).reshape(G * n, C)[bad]
    else:
        raise AssertionError("bn_inputs%r: the activation margins did not settle" % (key,))
    return c


BN_FLOATS = ("src", "gamma", "beta", "g", "run_mean", "run_var")
STATS_OUT = ("mean", "var", "rstd")
RUNNING_OUT = tuple("%s%d" % (n, k) for k in RUNNING_CALLS for n in ("run_mean", "run_var"))
OUTPUTS = {"stats": STATS_OUT, "running": RUNNING_OUT, "apply": ("y",), "backward": ("dc", "dgamma", "dbeta")}
FAMILIES = tuple(OUTPUTS)


def bn_run(c, x, dtype):
    """Every output of a case from plain torch in `dtype`: F.batch_norm in training mode on every group in group order - the statistics
    [G, C], the running buffers after RUNNING_CALLS calls of all groups, y, and the VJP of sum(y g) at src, gamma and beta."""
    G, n, C = c["G"], c["n"], c["C"]
    src, gamma, beta = (x[k].to(dtype).clone().requires_grad_(True) for k in ("src", "gamma", "beta"))
    v = src.view(G, n, C)
    rm, rv = x["run_mean"].to(dtype).clone(), x["run_var"].to(dtype).clone()
    out = {}
    with torch.no_grad():
        for k in range(1, max(RUNNING_CALLS) + 1):
            for grp in range(G):
                F.batch_norm(v[grp], rm, rv, gamma, beta, True, MOMENTUM, EPS)
            if k in RUNNING_CALLS:
                out["run_mean%d" % k], out["run_var%d" % k] = rm.clone(), rv.clone()
        out["mean"], out["var"] = v.mean(1), v.var(1, unbiased=False)
        out["rstd"] = 1.0 / torch.sqrt(out["var"] + EPS)
    z = torch.cat([F.batch_norm(v[grp], None, None, gamma, beta, True, MOMENTUM, EPS) for grp in range(G)])
    y = _act(z, c["act"])
    out["y"] = y.detach()
    grads = torch.autograd.grad((y * x["g"].to(dtype)).sum(), [src, gamma, beta])
    out["dc"], out["dgamma"], out["dbeta"] = (t.detach() for t in grads)
    return out


def bn_mags(c, x):
    """S of every output of bn_run (float64)."""
    G, n, C = c["G"], c["n"], c["C"]
    src, gamma, beta, g = (x[k].double() for k in ("src", "gamma", "beta", "g"))
    v = src.view(G, n, C)
    mean, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    S = {"mean": v.abs().mean(1), "var": var[:, 0], "rstd": rstd[:, 0]}
    sm, sv = x["run_mean"].double().abs(), x["run_var"].double().abs()
    for k in range(1, max(RUNNING_CALLS) + 1):
        for grp in range(G):
            sm = (1 - MOMENTUM) * sm + MOMENTUM * S["mean"][grp]
            sv = (1 - MOMENTUM) * sv + MOMENTUM * S["var"][grp] * n / (n - 1)
        if k in RUNNING_CALLS:
            S["run_mean%d" % k], S["run_var%d" % k] = sm, sv
    xh = (v - mean) * rstd
    z = xh * gamma + beta
    a = _slope(z, c["act"])
    S["y"] = (a * ((gamma * xh).abs() + beta.abs())).view(G * n, C)
    dz = (g.view(G, n, C) * a).abs()
    s2, s1 = (dz * xh.abs()).sum(1, keepdim=True), dz.sum(1, keepdim=True)
    S["dgamma"], S["dbeta"] = s2.sum(0)[0], s1.sum(0)[0]
    S["dc"] = (gamma.abs() * rstd * (dz + s1 / n + xh.abs() * s2 / n)).view(G * n, C)
    return S


# ===================================================================================================================== the kernels' formulas
PLANTS = ("one_pass_variance", "dgamma_term_omitted", "unbiased_variance", "pooled_groups", "running_order_reversed", "leaky_as_relu")


def emulate(key, plant=None):
    """The kernels' formulas in f32: two-pass statistics per group, z = gamma ((c - mean_g) rstd_g) + beta, dz = g act'(z), per group
    S2 = sum dz xhat and S1 = sum dz, dc = gamma rstd_g ((dz - S1 / n) - xhat S2 / n), dgamma / dbeta the groups' sums in group order,
    the running statistics through the groups in group order - without the blocks (a change of summation order only)."""
    c = bn_inputs(key)
    G, n, C = c["G"], c["n"], c["C"]
    v = c["src"].view(G, n, C)
    if plant == "pooled_groups":
        mean = c["src"].mean(0).expand(G, 1, C)
        var = ((c["src"] - mean[0]) ** 2).mean(0).expand(G, 1, C)
    else:
        mean = v.mean(1, keepdim=True)
        var = ((v * v).mean(1, keepdim=True) - mean * mean) if plant == "one_pass_variance" else ((v - mean) ** 2).mean(1, keepdim=True)
    out = {"mean": mean[:, 0], "var": var[:, 0]}
    rm, rv = c["run_mean"].clone(), c["run_var"].clone()
    m = torch.tensor(MOMENTUM, dtype=F32)
    order = range(G - 1, -1, -1) if plant == "running_order_reversed" else range(G)
    for k in range(1, max(RUNNING_CALLS) + 1):
        for grp in order:
            rm = (1 - m) * rm + m * mean[grp, 0]
            rv = (1 - m) * rv + m * (var[grp, 0] * (n / (n - 1)))
        if k in RUNNING_CALLS:
            out["run_mean%d" % k], out["run_var%d" % k] = rm, rv
    norm_var = var * n / (n - 1) if plant == "unbiased_variance" else var
    rstd = 1.0 / torch.sqrt(norm_var + torch.tensor(EPS, dtype=F32))
    out["rstd"] = rstd[:, 0]
    xh = (v - mean) * rstd
    z = c["gamma"] * xh + c["beta"]
    act = "relu" if plant == "leaky_as_relu" else c["act"]
    out["y"] = _act(z, act).view(G * n, C)
    dz = c["g"].view(G, n, C) * _slope(z, act)
    s2, s1 = (dz * xh).sum(1, keepdim=True), dz.sum(1, keepdim=True)
    out["dgamma"], out["dbeta"] = s2.sum(0)[0], s1.sum(0)[0]
    inv = 1.0 / n
    out["dc"] = ((c["gamma"] * rstd) * ((dz - s1 * inv) - (0.0 if plant == "dgamma_term_omitted" else xh * (s2 * inv)))).view(G * n, C)
    return out


# ===================================================================================================================== references
def family_keys(family):
    assert family in OUTPUTS
    return list(CASES)


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = bn_inputs(key)
    x = {k: c[k] for k in BN_FLOATS}
    ref, S = bn_run(c, x, F64), bn_mags(c, x)
    g = _g(87)
    jig = lambda t: t.double() * (1 + EPS23 * (2.0 * torch.randint(0, 2, t.shape, generator=g).double() - 1))
    C = {k: torch.zeros_like(S[k]) for k in S}
    for _ in range(DRAWS):
        got = bn_run(c, {k: jig(v) for k, v in x.items()}, F64)
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return ref, {k: EPS24 * S[k] + C[k] for k in S}


def reference(family, key):
    """-> (ref, A): the float64 result and the allowance 2^-24 S + C per element, over the family's outputs."""
    ref, A = _reference(key)
    return {k: ref[k] for k in OUTPUTS[family]}, {k: A[k] for k in OUTPUTS[family]}


def worst_ratio(family, key, got):
    """{output: (worst error / A, flat index)} of `got` over the family's outputs."""
    ref, A = reference(family, key)
    out = {}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape), (k, got[k].shape, ref[k].shape)
        q = ratios(got[k].cpu(), ref[k], A[k]).reshape(-1)
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        out[k] = (float(q.max()), int(q.argmax())) if q.numel() else (0.0, -1)
    return out


@functools.lru_cache(maxsize=None)
def f32_restatement(key):
    c = bn_inputs(key)
    return bn_run(c, {k: c[k] for k in BN_FLOATS}, F32)


def f32_worst(family):
    return max(q for key in family_keys(family) for q, _ in worst_ratio(family, key, {k: f32_restatement(key)[k] for k in OUTPUTS[family]}).values())


def print_f32_worst():
    for family in F32_WORST:
        print('"%s": %.3g,' % (family, f32_worst(family)))


# ===================================================================================================================== the trainer
CAM = "camera_head_list.0"
TRAIN_CASE = (50, (7, 2), 80)                # tests/golden_inputs.camera_train_case: nq, planes per pair (B = 2), seed; res5 at 15 x 20
TIE = 1e-5                                   # a float64 run cannot decide within this share of a tensor's largest magnitude: the float32
                                             # forward's side of a LeakyReLU, its winner of a max-pool window, is taken there
TOWER = tuple("convs_backbone.%d" % i for i in (0, 1, 3, 4, 6, 7))
BRANCHES = tuple("%s.%d" % (b, i) for b in ("convs_trans", "convs_rots") for i in range(6))
GRAD_FLOOR = 3e-3                            # the stored-statistics trainer's bound (tests/test_pose_net_training_gpu.py)

# per parameter tensor: max |error| / max(|ref|_max, 1e-4 of the largest gradient) of the float32 torch run of camera_head_run against
# the float64 run that takes the float32 run's LeakyReLU sides and max-pool winners - the tensors whose figure times LIMIT_FACTOR
# exceeds GRAD_FLOOR (every other tensor stays below GRAD_FLOOR / LIMIT_FACTOR and keeps the floor).  Printed by
#   python -c "from tests import camera_bn_forms as P; P.print_trainer_f32()"
# and re-measured by tests/test_camera_bn_forms_cpu.py (a figure off by more than 2x fails).
TRAINER_F32 = {CAM + "." + k: v for k, v in {
    "decoder_rot.layers.0.bias": 0.00455, "decoder_rot.layers.0.weight": 0.00332, "decoder_rot.layers.1.bias": 0.00552,
    "decoder_rot.layers.1.weight": 0.00383, "decoder_rot.layers.2.bias": 0.00461, "decoder_rot.layers.2.weight": 0.00313,
    "decoder_rot.layers.3.bias": 0.00432, "decoder_rot.layers.3.weight": 0.00301, "decoder_rot.layers.4.bias": 0.00321,
    "decoder_rot.layers.4.weight": 0.00238, "decoder_rot.layers.5.bias": 0.00339, "decoder_rot.layers.5.weight": 0.00243,
    "decoder_tran.layers.0.bias": 0.00368, "decoder_tran.layers.0.weight": 0.00272, "decoder_tran.layers.1.bias": 0.00316,
    "decoder_tran.layers.1.weight": 0.00227, "decoder_tran.layers.2.bias": 0.00276, "decoder_tran.layers.2.weight": 0.00179,
    "decoder_tran.layers.3.bias": 0.0204, "decoder_tran.layers.3.weight": 0.015, "geo_encoder.layers.0.bias": 0.00489,
    "geo_encoder.layers.0.weight": 0.00291, "geo_encoder.layers.1.bias": 0.0048, "geo_encoder.layers.1.weight": 0.00308,
    "geo_encoder.layers.2.bias": 0.00425, "geo_encoder.layers.2.weight": 0.0028, "geo_encoder.layers.3.bias": 0.00397,
    "geo_encoder.layers.3.weight": 0.003, "geo_encoder.layers.4.bias": 0.00318, "geo_encoder.layers.4.weight": 0.00216,
    "geo_encoder.layers.5.bias": 0.00314, "geo_encoder.layers.5.weight": 0.00217, "geo_proj_s1.layers.0.bias": 0.00509,
    "geo_proj_s1.layers.0.weight": 0.00359, "geo_proj_s1.layers.1.bias": 0.00404, "geo_proj_s1.layers.1.weight": 0.00315,
    "geo_proj_s1.layers.2.bias": 0.00331, "geo_proj_s1.layers.2.weight": 0.00251, "geo_proj_s2.layers.0.bias": 0.00304,
    "geo_proj_s2.layers.0.weight": 0.00237, "geo_proj_s2.layers.1.bias": 0.00274, "geo_proj_s2.layers.1.weight": 0.00175,
    "geo_proj_s2.layers.2.bias": 0.00284, "geo_proj_s2.layers.2.weight": 0.00184,
}.items()}


def grad_bound(key):
    return max(GRAD_FLOOR, LIMIT_FACTOR * TRAINER_F32.get(key, 0.0))


def loss_weights():
    """The three loss weights of the training forward as the test model's camera head holds them (configs/inference_mp3d.yaml)."""
    import os
    from types import SimpleNamespace

    from nopesac_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "inference_mp3d.yaml"))
    C = cfg.MODEL.CAMERA_HEAD
    return SimpleNamespace(initial_cam_weight=float(getattr(C, "INITIAL_CAM_WEIGHT", 1.0)), plane_cam_weight=float(getattr(C, "PLANE_CAM_WEIGHT", 1.0)),
                           plane_cam_weight_predplane=float(getattr(C, "PLANE_CAM_WEIGHT_PREDPLANE", 0.1)))


class BatchStatBlock:
    """Stands in for the oracle's _conv_bn_lrelu: conv3x3 (no bias) + F.batch_norm(training=True, momentum 0.01, eps 1e-3) - the running
    buffers of the state dict it is handed are updated in place, as nn.BatchNorm2d does - + LeakyReLU(0.01).  The oracle calls its tower
    once per view, so the per-view statistics and the update order are the reference's by construction.  With `rec` ({layer: the
    float32 forward's outputs, NCHW, the 2B images of the tower view 1 first}) a pre-activation within TIE of the kink takes the side
    the float32 forward took.  Keeps every call's output (`seen`), per-channel statistics (`stats`: mean, unbiased variance, mean
    magnitude of the conv output) and the state dict (`sd`); `tap` is applied to every conv output."""

    def __init__(self, rec=None, B=2, tap=None):
        self.rec, self.B, self.tap = rec, B, tap
        self.calls, self.seen, self.stats, self.sd = {}, {}, {}, None

    def __call__(self, x, sd, p, stride=1):
        self.sd = sd
        name = p[len(CAM) + 1:]
        cv = F.conv2d(x, sd[p + ".0.weight"], None, stride, 1)
        if self.tap is not None:
            cv = self.tap(cv)
        with torch.no_grad():
            self.stats.setdefault(name, []).append((cv.mean((0, 2, 3)), cv.var((0, 2, 3), unbiased=True), cv.abs().mean((0, 2, 3))))
        z = F.batch_norm(cv, sd[p + ".1.running_mean"], sd[p + ".1.running_var"], sd[p + ".1.weight"], sd[p + ".1.bias"], True, MOMENTUM, EPS)
        pos = z.detach() > 0
        if self.rec is not None:
            ref = self.rec[name]
            if ref.shape[0] != z.shape[0]:                    # the siamese tower: view 1's images first, then view 2's
                i = self.calls.get(name, 0)
                self.calls[name] = i + 1
                ref = ref[i * self.B:(i + 1) * self.B]
            near = z.detach().abs() <= TIE * z.detach().abs().max()
            pos = torch.where(near, ref.to(z.device) > 0, pos)
        y = torch.where(pos, z, LEAK * z)
        self.seen.setdefault(name, []).append(y.detach())
        return y

    def recorded(self):
        """{layer: this run's outputs as float64, the tower's views concatenated}: the `rec` of a run that follows this one's decisions"""
        return {k: torch.cat(v).double() for k, v in self.seen.items()}


class ConsistentPool:
    """Stands in for F.max_pool2d inside the oracle's pixel pose net (2 x 2, stride 2, behind convs_backbone.1 and .4 of each view): where
    the window's value at the float32 forward's winner lies within TIE of the float64 maximum, the float32 winner is taken."""

    def __init__(self, rec, B=2):
        self.rec, self.B, self.calls, self.orig = rec, B, 0, F.max_pool2d

    def __call__(self, x, *args, **kw):
        if tuple(args) != (2, 2) or kw:
            return self.orig(x, *args, **kw)
        view, layer = divmod(self.calls, 2)
        self.calls += 1
        ref = self.rec["convs_backbone.%d" % (1, 4)[layer]][view * self.B:(view + 1) * self.B].to(x.device)
        _, i32 = self.orig(ref, 2, 2, return_indices=True)
        m64, i64 = self.orig(x.detach(), 2, 2, return_indices=True)
        flat = x.flatten(2)
        at32 = flat.detach().gather(2, i32.flatten(2)).view_as(m64)
        idx = torch.where(m64 - at32 <= TIE * x.detach().abs().max(), i32, i64)
        return flat.gather(2, idx.flatten(2)).view_as(m64)


class patched_oracle:
    """with patched_oracle(block, pool): the oracle's conv + BN + LeakyReLU block and (pool not None) its 2 x 2 max-pool replaced"""

    def __init__(self, block, pool=None):
        self.block, self.pool = block, pool

    def __enter__(self):
        from oracle import nopesac_oracle as O
        self.O, self.old = O, (O._conv_bn_lrelu, O.F.max_pool2d)
        O._conv_bn_lrelu = self.block
        if self.pool is not None:
            O.F.max_pool2d = self.pool
        return self

    def __exit__(self, *exc):
        self.O._conv_bn_lrelu, self.O.F.max_pool2d = self.old


def camera_head_run(sd, c, nq, weights, names, dtype):
    """The oracle's training-mode camera head with the reference's detach points (tests/test_training_gpu.py
    _oracle_camera_head_train_like_the_reference, in `dtype`) -> (the 34 losses, {name: gradient of their sum}).  Call it inside
    patched_oracle; the default dtype is `dtype` while it runs."""
    from oracle import nopesac_oracle as O
    cfg = O.OracleConfig(num_queries=nq)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        sdg = {k: (v.clone().to(dtype).requires_grad_(True) if k in names else v.to(dtype).clone()) for k, v in sd.items()
               if torch.is_tensor(v) and v.is_floating_point()}
        dd = lambda t: t.to(dtype)
        f1, f2, gt = {k: dd(v) for k, v in c["feats1"].items()}, {k: dd(v) for k, v in c["feats2"].items()}, dd(c["gt_pose"])
        losses = {}
        trans0, rot0, tf0, rf0, _ = O.pixel_pose_net(sdg, f1, f2, CAM)
        l_t, l_r = O.camera_pose_loss(torch.cat((trans0, rot0), -1), gt)
        losses["loss_tran_pixelReg"], losses["loss_rot_pixelReg"] = l_t * weights.initial_cam_weight, l_r * weights.initial_cam_weight

        def rec(trans_in, rot_in, suffix):
            trans_in, rot_in = trans_in.detach(), rot_in.detach()
            sig = ((rot_in[:, 0:1] >= 0.0).to(dtype) - 0.5) * 2.0
            rec_t, rec_r, rec_tf, rec_rf = O.aim_reembed(sdg, trans_in, rot_in, CAM)
            losses["loss_rot" + suffix] = (F.normalize(rot_in * sig, dim=1) - rec_r).norm(dim=1).mean()
            losses["loss_trans" + suffix] = ((trans_in + 1e-10) - rec_t).norm(dim=1).mean()
            return rec_t, rec_r, rec_tf, rec_rf

        rec_t, rec_r, rec_tf, rec_rf = rec(trans0, rot0, "_initCamRec")
        B = gt.shape[0]
        for sfx, pl1, pl2, AA, w in (("", c["gt_planes1"], c["gt_planes2"], c["gt_A"], weights.plane_cam_weight),
                                     ("_Aux", c["planes1"], c["planes2"], c["A"], weights.plane_cam_weight_predplane)):
            for name, it, ir, itf, irf in (("initCamRef", trans0, rot0, tf0, rf0), ("initRecCamRef", rec_t, rec_r, rec_tf, rec_rf)):
                gl, gg, sg, ms = [], [], [], []
                for b in range(B):
                    l, m = O.geo_sequence(dd(pl1[b]), dd(pl2[b]), dd(AA[b]), nq)
                    g_, _ = O.geo_sequence(dd(pl1[b]), dd(pl2[b]), dd(AA[b]), nq, ir[b].detach(), it[b].detach())
                    a_, _ = O.geo_sequence(dd(pl1[b]), dd(pl2[b]), dd(AA[b]), nq, ir[b].detach(), torch.zeros(3, dtype=dtype))
                    gl.append(l); gg.append(g_); ms.append(m)
                    sg.append((((g_[:, 0:1] * a_[:, 0:1]) >= 0).to(dtype) - 0.5) * 2.0)
                ls, _ = O.ransac_refine_train(sdg, itf, irf, torch.stack(gg), torch.stack(gl), torch.stack(sg), ms, it, ir, gt, cfg, suffix=name + sfx,
                                              weight=w, p=CAM)
                losses.update(ls)
        rec(dd(c["rand_trans"]), dd(c["rand_rot"]), "_randCamRecLBS_N1")
        sum(losses.values()).backward()
        return {k: v.detach() for k, v in losses.items()}, {k: sdg[k].grad for k in names}
    finally:
        torch.set_default_dtype(old)


def float64_like(sd, c, nq, weights, names, rec):
    """The float64 run that takes the decisions of the float32 forward whose block outputs are `rec` -> (losses, gradients, its block)."""
    B = c["gt_pose"].shape[0]
    block = BatchStatBlock(rec, B)
    with patched_oracle(block, ConsistentPool(rec, B)):
        losses, grads = camera_head_run(sd, c, nq, weights, names, F64)
    return losses, grads, block


def grad_errors(grads, ref, names):
    """{name: max |error| / max(|ref|_max, 1e-4 of the largest reference gradient)} - the measure of tests/test_pose_net_training_gpu.py"""
    gmax = max(float(ref[k].abs().max()) for k in names)
    return {k: float((grads[k].detach().cpu().double() - ref[k].double()).abs().max()) / max(float(ref[k].abs().max()), 1e-4 * gmax) for k in names}


@functools.lru_cache(maxsize=None)
def trainer_case():
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.training import CameraHeadTrainer
    from tests import golden_inputs as GI
    nq = TRAIN_CASE[0]
    sd = synth_state_dict(nq)
    return nq, GI.camera_train_case(*TRAIN_CASE), sd, CameraHeadTrainer.parameter_names(sd.keys(), True)


@functools.lru_cache(maxsize=None)
def trainer_f32_figures():
    """{parameter: the float32 torch run's error against the float64 run with the float32 run's decisions} (CPU)"""
    nq, c, sd, names = trainer_case()
    w = loss_weights()
    block = BatchStatBlock()
    with patched_oracle(block):
        _, g32 = camera_head_run(sd, c, nq, w, names, F32)
    _, g64, _ = float64_like(sd, c, nq, w, names, block.recorded())
    return grad_errors(g32, g64, names)


def print_trainer_f32():
    fig = trainer_f32_figures()
    keep = {k: v for k, v in fig.items() if v * LIMIT_FACTOR > GRAD_FLOOR}
    print("TRAINER_F32 = {%s}" % ", ".join('"%s": %.3g' % kv for kv in sorted(keep.items())))
    print("largest of the rest: %.3g" % max(v for k, v in fig.items() if k not in keep))


def running_progress(start, stats, calls=RUNNING_CALLS):
    """{calls: (running_mean, running_var)} from `start` = (mean, var) through `stats` = [(mean, unbiased variance, ...) per call of
    the module within one iteration], repeated for every iteration: r <- (1 - m) r + m stat"""
    rm, rv = start
    out = {}
    for k in range(1, max(calls) + 1):
        for st in stats:
            rm, rv = (1 - MOMENTUM) * rm + MOMENTUM * st[0], (1 - MOMENTUM) * rv + MOMENTUM * st[1]
        if k in calls:
            out[k] = (rm, rv)
    return out


def running_reference(sd, c, rec, device="cpu", calls=RUNNING_CALLS):
    """-> (ref, A): {(buffer key, calls): tensor} of the 36 running buffers after `calls` training iterations on the case, the float64
    progression through the per-view batch statistics of the float64 pixel pose net (the forward does not depend on the buffers, so
    every iteration contributes the same statistics), and its allowance 2^-24 S + C: S the progression of the magnitudes, C the largest
    change over DRAWS draws that multiply every parameter, buffer, input map and conv output by 1 +- 2^-23.  `device`: where the
    float64 forwards run."""
    from oracle import nopesac_oracle as O
    B = c["gt_pose"].shape[0]
    g = torch.Generator(device=device).manual_seed(89)
    sign = lambda t: torch.where(torch.randint(0, 2, t.shape, generator=g, device=device, dtype=torch.int8) > 0, 1 + EPS23, 1 - EPS23).to(t.dtype)
    jig = lambda t: t * sign(t)

    def forward(j, tap):
        sdd = {k: j(v.to(device=device, dtype=F64)) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point() and k.startswith(CAM)}
        start = {k: v.clone() for k, v in sdd.items() if k.endswith(("running_mean", "running_var"))}
        f1, f2 = ({k: j(v.to(device=device, dtype=F64)) for k, v in c[f].items()} for f in ("feats1", "feats2"))
        block = BatchStatBlock(rec, B, tap)
        old = torch.get_default_dtype()
        torch.set_default_dtype(F64)
        try:
            with torch.no_grad(), patched_oracle(block, ConsistentPool(rec, B)):
                O.pixel_pose_net(sdd, f1, f2, CAM)
        finally:
            torch.set_default_dtype(old)
        return sdd, start, block

    def progressions(start, block, mags=False):
        out = {}
        for name, stats in block.stats.items():
            q = "%s.%s.1." % (CAM, name)
            s0 = (start[q + "running_mean"], start[q + "running_var"])
            if mags:
                s0, stats = (s0[0].abs(), s0[1].abs()), [(st[2], st[1]) for st in stats]
            for k, (rm, rv) in running_progress(s0, stats, calls).items():
                out[(q + "running_mean", k)], out[(q + "running_var", k)] = rm, rv
        return out

    sdd, start, block = forward(lambda t: t, None)
    ref, S = progressions(start, block), progressions(start, block, mags=True)
    assert all(len(block.stats[n]) == 2 for n in TOWER) and all(len(block.stats[n]) == 1 for n in BRANCHES) and len(block.stats) == 18
    for (k, n), v in ref.items():                               # the closed form is F.batch_norm's own in-place update
        if n == 1:
            assert float((sdd[k] - v).abs().max()) <= 1e-12 * (1 + float(v.abs().max())), k
    C = {k: torch.zeros_like(v) for k, v in ref.items()}
    for _ in range(DRAWS):
        _, st, bl = forward(jig, jig)
        for k, v in progressions(st, bl).items():
            C[k] = torch.maximum(C[k], (v - ref[k]).abs())
    return {k: v.cpu() for k, v in ref.items()}, {k: (EPS24 * S[k] + C[k]).cpu() for k in ref}
