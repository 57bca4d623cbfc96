"""The Linear backward that reads its operands in place (csrc/linear_bwd.hip: linear_dgrad_kernel, linear_wgrad_kernel,
linear_bwd_reduce_kernel) and PlaneEncoderTrainer as data, in the construction of tests/plane_decoder_forms.py (from which the keep mask,
the attention restatement, the tap and the constants are imported): seeded inputs, each forward restated in plain torch with
MATERIALISED masks (float64 is the reference, float32 the restatement the limits are measured from), a per-element allowance
A_k = 2^-24 S_k + C_k for every element of every output, and planted errors.  tests/test_plane_encoder_forms_gpu.py and
tests/test_plane_encoder_training_gpu.py hold the kernels and the trainer to it; tests/test_plane_encoder_forms_cpu.py proves case
lists, streams, names, references, constants and the sharpness of the bound.  Imports without a GPU.

  S_k    the sum of the magnitudes of the terms that make element k, in float64.  linear_bwd: |g'| |W| for dx, |g'|^T |x| for dW,
         the column sums of |g'| for db.  Whole encoder: the last accumulation of every gradient from the float64 restatement's own
         intermediates, as plane_decoder_forms.decoder_run (|dY|^T |X| for a Linear's weight, sum |dY| for a bias, sum |dY xhat| /
         sum |dY| for a LayerNorm's affine pair), |dY| |W| of input_proj for res5, |xhat gamma| + |beta| of the final norm for memory
  C_k    conditioning: the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input by
         1 +- 2^-23; for the whole encoder (a pipeline of some 150 operations) also every intermediate tensor and the gradient arriving
         at it (plane_decoder_forms.jiggle_tap)
  limit  LIMIT_FACTOR x max(F32_WORST[family], 1): the worst error / A of the float32 torch restatement over the cases of the family
         (measured on the CPU, never from a kernel; a CPU test re-measures it)
"""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g
from tests.plane_decoder_forms import (FFN, HD, NHEADS, PREFIX, RELU_BUMP, RELU_MARGIN, SEED, _mha, jiggle_tap, keep_mask)
from tests.refine_bwd_forms import DRAWS, EPS23, EPS24, F32, F64, LIMIT_FACTOR, _cot, ratios

TILE, STAGE = 128, 16                        # the kernels' tile edge and rows per LDS stage (include/nopesac_hip.h NPS_LINEAR_BWD_TILE / _STAGE; a CPU test compares)

# worst error / A of the float32 torch restatement over every case of the family.  Printed by
#   python -c "from tests import plane_encoder_forms as E; E.print_f32_worst()"
# and re-measured by tests/test_plane_encoder_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"linear_bwd": 3.99, "encoder": 9.9}


def limit(family):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


def encoder_dropout_stream(step: int, layer: int, site: int) -> int:
    return -(step * 32 + layer * 4 + site) - 1


# ===================================================================================================================== linear backward
LIN_MS = (1, 5, TILE - 1, TILE + 1, 24, 600)
LIN_KN = ((256, 512), (256, 256), (256, 1024), (1024, 256), (2048, 256), (4, 4), (132, 260))
LIN_GATES = (("none", 0.0), ("relu", 0.0), ("drop", 0.1), ("drop", 0.5), ("both", 0.1))        # (gate, p)
LIN_CASES = tuple((M, K, N, gate, p) for M in LIN_MS for K, N in LIN_KN for gate, p in LIN_GATES)
LIN_STREAM = encoder_dropout_stream(5, 3, 2)          # step 5, layer 3, the FFN's inner site


def lin_splits(M: int):
    """The split counts of a case: 1, and one whose ranges (ceil(M / S) rounded up to STAGE rows) leave the last one short or empty."""
    return (1, 9 if M == 600 else 3)


def split_ranges(M: int, S: int):
    chunk = -(-(-(-M // S)) // STAGE) * STAGE
    return [(min(z * chunk, M), min((z + 1) * chunk, M)) for z in range(S)]


@functools.lru_cache(maxsize=None)
def lin_inputs(key):
    """x [M, K], w [N, K], the gradient g [M, N] (with exact zeros), the saved output y of a ReLU (exact zeros and negative zeros among
    its entries) where the gate asks for it, the keep mask [M, N]."""
    M, K, N, gate, p = key
    g = _g(61000 + 7 * M + 3 * K + N + 11 * len(gate) + int(1000 * p))
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    gr = _cot(g, M, N)
    y = None
    if gate in ("relu", "both"):
        y = torch.randn(M, N, generator=g).clamp_min(0.0)
        y[torch.rand(M, N, generator=g) < 0.125] = -0.0
        y.view(-1)[0] = 0.0
        y.view(-1)[-1] = -0.0
    return dict(key=key, M=M, K=K, N=N, p=p, x=x, w=w, g=gr, y=y, mask=keep_mask((M, N), p, SEED, LIN_STREAM))


def _lin_gated(c, x, dtype):
    gp = x["g"].to(dtype)
    if c["y"] is not None:
        gp = gp * (c["y"] > 0).to(dtype)
    return gp * c["mask"].to(dtype) / (1.0 - c["p"])


def lin_run(c, x, dtype):
    gp = _lin_gated(c, x, dtype)
    return {"dx": gp @ x["w"].to(dtype), "dw": gp.t() @ x["x"].to(dtype), "db": gp.sum(0)}


def lin_mags(c, x):
    gp = _lin_gated(c, x, F64).abs()
    return {"dx": gp @ x["w"].double().abs(), "dw": gp.t() @ x["x"].double().abs(), "db": gp.sum(0)}


LIN_PLANTS = ("dw_without_dropout_gate", "mask_index_transposed")


def emulate_linear_backward(key, plant=None):
    """The kernels' formulas in f32 without the tiling: g' = y > 0 ? g : 0, then keep ? g' inv_keep : 0; dx = g' W, dW = g'^T x,
    db = column sums."""
    c = lin_inputs(key)
    inv = torch.tensor(1.0 / (1.0 - c["p"]), dtype=F32)
    gp = c["g"] if c["y"] is None else torch.where(c["y"] > 0, c["g"], torch.zeros_like(c["g"]))
    mask = c["mask"]
    if plant == "mask_index_transposed":
        mask = keep_mask((c["N"], c["M"]), c["p"], SEED, LIN_STREAM).t()
    gd = torch.where(mask.bool(), gp * inv, torch.zeros_like(gp))
    return {"dx": gd @ c["w"], "dw": (gp if plant == "dw_without_dropout_gate" else gd).t() @ c["x"], "db": gd.sum(0)}


# ===================================================================================================================== the whole encoder
ENC = PREFIX + "context_SA"
IPROJ = PREFIX + "input_proj"
LAYERS, CIN = 6, 2048
# (B, h, w, p): the issue's cases
ENC_CASES = ((2, 3, 4, 0.0), (2, 3, 4, 0.1), (3, 3, 4, 0.1), (2, 15, 20, 0.0), (2, 15, 20, 0.1))
ENC_STEP = 3
ENC_PLANTS = ("pos_added_to_value",)


def encoder_parameter_names(keys):
    return sorted(k for k in keys if k.startswith(ENC + ".") or k.startswith(IPROJ + "."))


def encoder_masks(B, L, p, seed=SEED, step=ENC_STEP):
    """{(layer, site): uint8 keep mask} over the four sites of every layer, in the kernels' logical shapes (rows in (b, token) order)."""
    shapes = {0: (B, NHEADS, L, L), 1: (B * L, 256), 2: (B * L, FFN), 3: (B * L, 256)}
    return {(i, s): keep_mask(shapes[s], p, seed, encoder_dropout_stream(step, i, s)) for i in range(LAYERS) for s in range(4)}


def encoder_forward(sd, res5, pos, B, masks=None, p=0.0, rec=None, tap=None, plant=None):
    """input_proj + the post-norm encoder (planeTR_head.py:77-82, 125-132; transformer.py:183-199, normalize_before=False) in batch-major
    layout, extended with the keep masks of the four dropout sites -> memory [B, L, 256].  sd: the 76 tensors by state-dict key, res5
    [B, h, w, 2048], pos [L, 256].  `rec` / `tap` as plane_decoder_forms.decoder_forward."""
    tap = tap or (lambda t: t)
    rec0 = rec or (lambda name, x, y, w: y)
    rec = lambda name, x, y, w: tap(rec0(name, x, y, w))
    inv = 1.0 / (1.0 - p)
    drop = (lambda t, i, s: t) if masks is None else (lambda t, i, s: tap(t * masks[(i, s)].to(t.dtype).view(t.shape) * inv))
    att_keep = (lambda i: None) if masks is None else (lambda i: masks[(i, 0)])

    def ln(x, n):
        xc = tap(x - tap(x.mean(-1, keepdim=True)))
        xhat = tap(xc * tap(torch.rsqrt(tap((xc * xc).mean(-1, keepdim=True)) + 1e-5)))
        return rec(n, x, xhat * sd[n + ".weight"] + sd[n + ".bias"], None)
    x = res5.reshape(B, -1, CIN)
    wip = sd[IPROJ + ".weight"].view(256, CIN)
    src = rec(IPROJ, x, F.linear(x, wip, sd[IPROJ + ".bias"]), wip)
    for i in range(LAYERS):
        lp = f"{ENC}.layers.{i}"
        g = lambda n: sd[lp + n]
        q = tap(src + pos)
        a = _mha(q, q, q if plant == "pos_added_to_value" else src, g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias"),
                 g(".self_attn.out_proj.weight"), g(".self_attn.out_proj.bias"), att_keep(i), inv, rec, tap, lp + ".self_attn")
        src = ln(tap(src + drop(a, i, 1)), lp + ".norm1")
        hdn = drop(tap(F.relu(rec(lp + ".linear1", src, F.linear(src, g(".linear1.weight"), g(".linear1.bias")), g(".linear1.weight")))), i, 2)
        src = ln(tap(src + drop(rec(lp + ".linear2", hdn, F.linear(hdn, g(".linear2.weight"), g(".linear2.bias")), g(".linear2.weight")), i, 3)),
                 lp + ".norm2")
    return ln(src, ENC + ".norm")


def ffn_inputs(sd, res5, pos, B, masks, p):
    """{layer: (x, S)} of the float64 forward: the inputs x [rows, FFN] of every layer's ReLU and their term magnitudes
    S = |W| |src| + |b|."""
    out = {}

    def rec(name, xin, y, w):
        if name.endswith(".linear1"):
            b = sd[name + ".bias"].double()
            S = xin.detach().abs() @ w.detach().abs().t() + b.abs()
            out[int(name.split(".")[-2])] = (y.detach().reshape(-1, y.shape[-1]), S.reshape(-1, y.shape[-1]))
        return y
    with torch.no_grad():
        encoder_forward({k: v.double() for k, v in sd.items()}, res5.double(), pos.double(), B, masks, p, rec=rec)
    return out


def relu_margins(sd, res5, pos, B, masks, p):
    """{layer: per unit, the smallest |x| / (|W| |src| + |b|) over the rows} of the float64 forward's FFN inputs."""
    return {i: (x.abs() / S).min(0).values for i, (x, S) in ffn_inputs(sd, res5, pos, B, masks, p).items()}


SETTLE_ROUNDS, SETTLE_STEPS = 32, 64


def settle_relu_margins(sd, res5, pos, B, masks, p):
    """Move linear1.bias entries (in place) until no input of an FFN's ReLU lies within RELU_MARGIN of 0 on any row; raises if that
    cannot be reached.  First plane_decoder_forms.decoder_inputs' rule: every unit that is marginal on some row moves by RELU_BUMP, all
    layers at once, up to SETTLE_ROUNDS times.  With hundreds of rows per unit (15 x 20) that walk does not end: a step that frees one
    row catches another, and a step in one layer moves every later layer's inputs.  What is left is then settled layer by layer, first
    to last (a layer's inputs depend on the earlier layers only): a marginal unit moves by the smallest multiple k <= SETTLE_STEPS of
    RELU_BUMP that puts all its rows at least 2 RELU_MARGIN from 0, relative to S + k RELU_BUMP >= the S after the move."""
    def marginal_units():
        return {i: m < RELU_MARGIN for i, m in relu_margins(sd, res5, pos, B, masks, p).items()}
    for _ in range(SETTLE_ROUNDS):
        marginal = marginal_units()
        if not any(bool(m.any()) for m in marginal.values()):
            return
        for i, m in marginal.items():
            sd[f"{ENC}.layers.{i}.linear1.bias"][m] += RELU_BUMP
    for i in range(LAYERS):
        x, S = ffn_inputs(sd, res5, pos, B, masks, p)[i]
        units = ((x.abs() / S).min(0).values < RELU_MARGIN).nonzero().flatten()
        if not units.numel():
            continue
        x, S = x[:, units], S[:, units]
        steps = torch.zeros(units.numel(), dtype=torch.int64)
        for k in range(SETTLE_STEPS, 0, -1):                        # (downwards: the smallest k that serves is written last)
            d = k * RELU_BUMP
            steps[((x + d).abs() / (S + d)).min(0).values >= 2 * RELU_MARGIN] = k
        if bool((steps == 0).any()):
            raise RuntimeError("settle_relu_margins: layer %d, units %s: no bias step up to %d x RELU_BUMP frees every row"
                               % (i, units[steps == 0].tolist(), SETTLE_STEPS))
        sd[f"{ENC}.layers.{i}.linear1.bias"][units] += steps.float() * RELU_BUMP
    left = {i: int(m.sum()) for i, m in marginal_units().items() if bool(m.any())}
    if left:
        raise RuntimeError("settle_relu_margins: marginal ReLU inputs remain, units per layer %s" % left)


@functools.lru_cache(maxsize=None)
def encoder_inputs(key):
    """(sd: the 76 f32 tensors of the name-seeded synthetic checkpoint, res5 [B, h, w, 2048] (behind a ReLU, as the backbone's), pos: the
    head's sine embedding, d_memory [B L, 256], masks).  The linear1 biases of units whose ReLU input is marginal on some row are moved
    until no input is within RELU_MARGIN of 0 (settle_relu_margins, which raises if it cannot): a float32 run that takes such a decision
    the other way differs from float64 by a whole term, not by rounding."""
    from nopesac_amd.modeling.plane_head import sine_position_embedding
    from nopesac_amd.synth import synth_state_dict
    B, h, w, p = key
    L = h * w
    full = synth_state_dict(7)
    sd = {k: full[k].float().clone() for k in encoder_parameter_names(full.keys())}
    g = _g(71000 + 100 * B + L)
    res5 = torch.randn(B, h, w, CIN, generator=g).clamp_min(0.0)
    pos = sine_position_embedding(h, w).float()
    d_memory = _cot(g, B * L, 256) / 16.0
    d_memory[1] = 0.0
    masks = encoder_masks(B, L, p) if p else None
    settle_relu_margins(sd, res5, pos, B, masks, p)
    return dict(key=key, B=B, h=h, w=w, L=L, p=p, sd=sd, res5=res5, pos=pos, d_memory=d_memory, masks=masks)


def encoder_run(c, x, dtype, mags=False, tap=None, plant=None):
    """memory and the VJP of sum(memory d_memory) at the 76 tensors and res5.  x: {"res5", "pos", "d_memory", parameter keys}."""
    sd = {k: x[k].to(dtype).clone().requires_grad_(True) for k in c["sd"]}
    res5 = x["res5"].to(dtype).clone().requires_grad_(True)
    recs = []

    def rec(name, xin, y, w):
        if mags:
            y.retain_grad()
            recs.append((name, xin, y, w))
        return y
    memory = encoder_forward(sd, res5, x["pos"].to(dtype), c["B"], c["masks"], c["p"], rec=rec, tap=tap, plant=plant).reshape(-1, 256)
    (memory * x["d_memory"].to(dtype)).sum().backward()
    out = {k: sd[k].grad.detach() for k in sorted(sd)}
    out["res5"] = res5.grad.detach()
    out["memory"] = memory.detach()
    if not mags:
        return out
    S = {k: torch.zeros_like(out[k]) for k in out if k != "memory"}
    flat = lambda t: t.reshape(-1, t.shape[-1])
    for name, xin, y, w in recs:
        if y.grad is None:
            continue
        gy = flat(y.grad.abs())
        if w is None:                                                        # a LayerNorm: y = xhat gamma + beta
            xf = flat(xin.detach())
            xhat = (xf - xf.mean(1, keepdim=True)) / torch.sqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
            S[name + ".weight"] += (gy * xhat.abs()).sum(0)
            S[name + ".bias"] += gy.sum(0)
            continue
        term = gy.t() @ flat(xin.detach()).abs()
        base, part = name.rsplit(".", 1)
        if name == IPROJ:
            S[IPROJ + ".weight"] += term.view_as(S[IPROJ + ".weight"])
            S[IPROJ + ".bias"] += gy.sum(0)
            S["res5"] += (gy @ w.detach().abs()).view_as(S["res5"])
        elif part in ("q", "k", "v"):
            rows = {"q": slice(0, 256), "k": slice(256, 512), "v": slice(512, 768)}[part]
            S[base + ".in_proj_weight"][rows] += term
            S[base + ".in_proj_bias"][rows] += gy.sum(0)
        else:
            key = base + ".out_proj" if part == "o" else name
            S[key + ".weight"] += term
            S[key + ".bias"] += gy.sum(0)
    return out, S


def _encoder_x(c):
    return dict(c["sd"], res5=c["res5"], pos=c["pos"], d_memory=c["d_memory"])


@functools.lru_cache(maxsize=None)
def encoder_reference(key):
    """-> (ref, A) over the 76 gradients, "res5" and "memory"."""
    c = encoder_inputs(key)
    x = _encoder_x(c)
    ref, S = encoder_run(c, x, F64, mags=True)
    beta = c["sd"][ENC + ".norm.bias"].double()
    S["memory"] = (ref["memory"] - beta).abs() + beta.abs()
    g = _g(83)
    jig = lambda t: t.double() * (1 + EPS23 * (2.0 * torch.randint(0, 2, t.shape, generator=g).double() - 1))
    C = {k: torch.zeros_like(ref[k]) for k in ref}
    for _ in range(DRAWS):
        got = encoder_run(c, {k: jig(v) for k, v in x.items()}, F64, tap=jiggle_tap(g))
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return ref, {k: EPS24 * S[k] + C[k] for k in ref}


# ===================================================================================================================== the fixture
GOLDEN = "L_plane_encoder_%dx%d.npz"         # tests/golden/: the reference's input_proj + context_SA (scripts/gen_plane_encoder_golden.py)
GOLDEN_CASES = {"eval": (2, 3, 4, 0.0), "train": (2, 3, 4, 0.1)}       # the reference in eval mode / in train mode under the materialised masks
GOLDEN_ROWS = 64                             # matrices are stored at rows [::GOLDEN_ROWS], d res5 at channels [::GOLDEN_ROWS]


def golden(h, w):
    import os

    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN % (h, w)))


def fixture_view(full):
    """The fixture's keys and subsamplings of a full result dict with encoder_run's keys."""
    out = {"memory": full["memory"], "d_res5_sub": full["res5"][..., ::GOLDEN_ROWS]}
    for k, t in full.items():
        if k.startswith(PREFIX):
            out["d." + k] = t[::GOLDEN_ROWS] if t.dim() >= 2 else t
    return out


# ===================================================================================================================== references
def family_keys(family):
    return {"linear_bwd": list(LIN_CASES), "encoder": list(ENC_CASES)}[family]


@functools.lru_cache(maxsize=None)
def _lin_reference(key):
    c = lin_inputs(key)
    x = {k: c[k] for k in ("x", "w", "g")}
    ref = lin_run(c, x, F64)
    S = lin_mags(c, x)
    g = _g(81)
    jig = lambda t: t.double() * (1 + EPS23 * (2.0 * torch.randint(0, 2, t.shape, generator=g).double() - 1))
    C = {k: torch.zeros_like(S[k]) for k in S}
    for _ in range(DRAWS):
        got = lin_run(c, {k: jig(v) for k, v in x.items()}, F64)
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return ref, {k: EPS24 * S[k] + C[k] for k in S}


def reference(family, key):
    """-> (ref, A): the float64 result and the allowance 2^-24 S + C per element, over the family's outputs."""
    return encoder_reference(key) if family == "encoder" else _lin_reference(key)


def worst_ratio(family, key, got):
    """{output: (worst error / A, flat index)} of `got` over the keys it holds."""
    ref, A = reference(family, key)
    out = {}
    for k in got:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        q = ratios(got[k], ref[k], A[k]).reshape(-1)
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        out[k] = (float(q.max()), int(q.argmax())) if q.numel() else (0.0, -1)
    return out


@functools.lru_cache(maxsize=None)
def f32_restatement(family, key):
    if family == "encoder":
        c = encoder_inputs(key)
        return encoder_run(c, _encoder_x(c), F32)
    c = lin_inputs(key)
    return lin_run(c, {k: c[k] for k in ("x", "w", "g")}, F32)


def f32_worst(family):
    return max(q for key in family_keys(family) for q, _ in worst_ratio(family, key, f32_restatement(family, key)).values())


def print_f32_worst():
    for family in F32_WORST:
        print('"%s": %.3g,' % (family, f32_worst(family)))
