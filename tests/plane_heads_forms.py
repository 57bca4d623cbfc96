"""The backward of the plane head's folded mask product (csrc/plane_head_bwd.hip: mask_wgrad_kernel + mask_wgrad_reduce_kernel,
mask_dgrad_kernel) as data: seeded inputs, the forward restated in plain torch (float64 is the reference, differentiated with
torch.autograd.grad; the closed-form vector-Jacobian products beside it), a per-element allowance A_k = 2^-24 S_k + C_k for every element
of every gradient, the float32 restatement the limits are measured from, and a float32 emulation of the kernels' formulas in which errors
can be planted.  tests/test_plane_heads_forms_gpu.py holds the kernels to it, tests/test_plane_heads_forms_cpu.py proves cases,
references, constants and the sharpness of the bound.  Imports without a GPU.

  forward    M[l,b,q,p] = sum_k F[l,b,q,k] p1[b,p,k] + beta[l,b,q],   Z[b,c,p] = sum_k Wc[c,k] p1[b,p,k] + bc[c]   (c = 0, 1)
  cotangents dM [L,B,nq,h*w] (about one entry in ten exactly zero; whole rows zero where a case says so), dZ [B,2,h*w]
  S_k        the float64 sum of the magnitudes of the terms that make element k (the same products on absolute values)
  C_k        conditioning: the largest change of the float64 VJP at k over DRAWS seeded draws that multiply every f32 input (cotangents
             included) by 1 + d, d = +- 2^-23 with random signs
  limit      LIMIT_FACTOR x max(F32_WORST[family], 1): F32_WORST = the worst error / A of the float32 restatement over the cases,
             measured on the CPU, never from a kernel.  The restatement of a long sum accumulates blocks of 16 terms in order, a plain
             loop of small f32 products into an f32 tensor, as a single-pass kernel does: a library matmul's blocked summation is more
             accurate than any one fmaf chain per accumulator can be and would set a limit no correct kernel meets - for the same
             reason the limit is not taken below LIMIT_FACTOR x 1.
"""
from __future__ import annotations

import functools

import torch

from tests.refine_bwd_forms import DRAWS, EPS23, EPS24, LIMIT_FACTOR

F32, F64 = torch.float32, torch.float64
C = 256
BLOCK = 16
FAMILIES = {"wgrad": ("d_fold", "d_beta", "d_wc", "d_bc"), "dgrad": ("d_p1",)}

# worst error / A of the float32 restatement over every case of the family.  Printed by
#   python -c "from tests import plane_heads_forms as H; H.print_f32_worst()"
# and re-measured by tests/test_plane_heads_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"wgrad": 1.08, "dgrad": 1.8}

# name: L, B, nq, h, w, centre rows, forced split count (None: the wrapper's choice), flags, seed
CASES = {
    "q7_5x7": (1, 1, 7, 5, 7, False, None, (), 201),
    "q21_6x8_b3": (3, 3, 7, 6, 8, True, None, (), 202),
    "q50_5x7_b3": (1, 3, 50, 5, 7, False, None, (), 203),
    "q150_30x40": (3, 1, 50, 30, 40, True, None, (), 204),                  # two row tiles, ten pixel tiles
    "q384_6x8": (3, 1, 128, 6, 8, True, None, (), 205),                     # 384 + 2 rows: a fourth row tile of two rows
    "q21_30x40_b3_short_split": (3, 3, 7, 30, 40, True, 3, (), 206),        # ranges of 416 pixels: the last holds 368
    "q7_6x8_empty_splits": (1, 1, 7, 6, 8, True, 4, (), 207),               # 48 pixels: ranges 32, 16, none, none
    "q50_30x40_many_splits": (1, 1, 50, 30, 40, False, 7, (), 208),         # more ranges than 256-pixel blocks (4)
    "q21_6x8_zero_rows": (3, 1, 7, 6, 8, True, None, ("zero_rows",), 209),
    "q7_5x7_b3_slice": (1, 3, 7, 5, 7, True, None, ("slice",), 210),        # p1 = channels 8 .. 263 of a 272-channel buffer
    "q50_120x160": (1, 1, 50, 120, 160, True, None, (), 211),
}
SLICE_WIDTH, SLICE_OFFSET = 272, 8


def limit(family):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's float32 inputs on the CPU: F, beta, p1, wc, bc and the cotangents dM, dZ (dZ / wc / bc None without centre rows)."""
    L, B, nq, h, w, centre, _, flags, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    hw = h * w
    rn = lambda *s: torch.randn(*s, generator=g)
    scale = lambda: 0.3 + 2.7 * torch.rand(1, generator=g).item()
    x = {"F": 0.5 * rn(L, B, nq, C), "beta": rn(L, B, nq), "p1": torch.relu(rn(B, hw, C))}
    x["dM"] = scale() * rn(L, B, nq, hw) * (torch.rand(L, B, nq, hw, generator=g) >= 0.1).float()
    if "zero_rows" in flags:                                      # the criterion's unmatched queries: exact zeros
        x["dM"][:, :, 1::2] = 0.0
    x["wc"] = 0.1 * rn(2, C) if centre else None
    x["bc"] = rn(2) if centre else None
    x["dZ"] = scale() * rn(B, 2, hw) if centre else None
    return x


def forward(x):
    """(M, Z) in the dtype of x"""
    M = torch.einsum("lbqk,bpk->lbqp", x["F"], x["p1"]) + x["beta"][..., None]
    Z = None if x["wc"] is None else torch.einsum("ck,bpk->bcp", x["wc"], x["p1"]) + x["bc"][None, :, None]
    return M, Z


def cast(x, dtype):
    return {k: (None if v is None else v.to(dtype)) for k, v in x.items()}


def vjp_closed(x):
    """The closed-form VJPs in the dtype of x: d_fold, d_beta, d_p1 (+ d_wc, d_bc)."""
    out = {"d_fold": torch.einsum("lbqp,bpk->lbqk", x["dM"], x["p1"]), "d_beta": x["dM"].sum(-1),
           "d_p1": torch.einsum("lbqp,lbqk->bpk", x["dM"], x["F"])}
    if x["dZ"] is not None:
        out["d_p1"] = out["d_p1"] + torch.einsum("bcp,ck->bpk", x["dZ"], x["wc"])
        out["d_wc"] = torch.einsum("bcp,bpk->ck", x["dZ"], x["p1"])
        out["d_bc"] = x["dZ"].sum((0, 2))
    return out


def vjp_autograd(x):
    """The same through torch.autograd.grad of sum(M dM) + sum(Z dZ)."""
    leaves = {k: x[k].clone().requires_grad_(True) for k in ("F", "beta", "p1", "wc", "bc") if x[k] is not None}
    M, Z = forward(dict(x, **leaves))
    total = (M * x["dM"]).sum() + (0 if Z is None else (Z * x["dZ"]).sum())
    g = dict(zip(leaves, torch.autograd.grad(total, list(leaves.values()))))
    out = {"d_fold": g["F"], "d_beta": g["beta"], "d_p1": g["p1"]}
    if "wc" in g:
        out["d_wc"], out["d_bc"] = g["wc"], g["bc"]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64: the gradients (autograd), S (magnitude sums), C (conditioning) and the allowance A per output."""
    x = cast(inputs(name), F64)
    ref = vjp_autograd(x)
    S = vjp_closed({k: (None if v is None else v.abs()) for k, v in x.items()})
    g = torch.Generator().manual_seed(CASES[name][-1] + 1000)
    Cc = {k: torch.zeros_like(v) for k, v in ref.items()}
    base = vjp_closed(x)
    for _ in range(DRAWS):
        xd = {k: (None if v is None else v * (1.0 + EPS23 * (2.0 * torch.randint(0, 2, v.shape, generator=g).double() - 1.0))) for k, v in x.items()}
        for k, v in vjp_closed(xd).items():
            Cc[k] = torch.maximum(Cc[k], (v - base[k]).abs())
    return {"g": ref, "S": S, "C": Cc, "A": {k: EPS24 * S[k] + Cc[k] for k in ref}}


def _blocked(n, step=BLOCK):
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def f32_restatement(name, plant=None):
    """The float32 restatement / emulation of the kernels' formulas: every long sum accumulates blocks of 16 terms in order (pixels in
    the wgrad, stacked rows (l, q) then the centre rows in the dgrad).  plant: None, or an error to plant - "drop_block" (one pixel
    block / row block left out), "swap_layer" (layers 0 and 1 of dM read for each other), "no_dbeta" (d_beta = the first block only)."""
    x = inputs(name)
    L, B, nq, h, w, centre = CASES[name][:6]
    hw = h * w
    dM = x["dM"]
    if plant == "swap_layer":
        assert L > 1
        dM = dM[[1, 0] + list(range(2, L))]
    out = {"d_fold": torch.zeros(L, B, nq, C), "d_beta": torch.zeros(L, B, nq), "d_p1": torch.zeros(B, hw, C)}
    if centre:
        out["d_wc"], out["d_bc"] = torch.zeros(2, C), torch.zeros(2)
    pix = _blocked(hw)
    for i, (a, b) in enumerate(pix):
        if plant == "drop_block" and i == len(pix) // 2:
            continue
        out["d_fold"] += torch.einsum("lbqp,bpk->lbqk", dM[..., a:b], x["p1"][:, a:b])
        if plant != "no_dbeta" or i == 0:
            out["d_beta"] += dM[..., a:b].sum(-1)
        if centre:
            for bi in range(B):                                   # the shared rows: images in order
                out["d_wc"] += torch.einsum("cp,pk->ck", x["dZ"][bi, :, a:b], x["p1"][bi, a:b])
                out["d_bc"] += x["dZ"][bi, :, a:b].sum(-1)
    rows = dM.permute(1, 0, 2, 3).reshape(B, L * nq, hw)          # [B, (l, q), p]
    Fr = x["F"].permute(1, 0, 2, 3).reshape(B, L * nq, C)
    if centre:
        rows = torch.cat([rows, x["dZ"]], 1)
        Fr = torch.cat([Fr, x["wc"][None].expand(B, 2, C)], 1)
    blocks = _blocked(rows.shape[1])
    for i, (a, b) in enumerate(blocks):
        if plant == "drop_block" and i == len(blocks) // 2:
            continue
        out["d_p1"] += torch.einsum("brp,brk->bpk", rows[:, a:b], Fr[:, a:b])
    return out


def ratios(got, name):
    """max over the elements of |got - f64| / A, per output"""
    ref = reference(name)
    out = {}
    for k, v in got.items():
        A = ref["A"][k]
        err = (v.double().reshape(A.shape) - ref["g"][k]).abs()
        out[k] = float((err / A.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    return out


def measure_f32_worst(names=None):
    worst = {f: 0.0 for f in FAMILIES}
    for name in (names or CASES):
        r = ratios(f32_restatement(name), name)
        for f, keys in FAMILIES.items():
            worst[f] = max([worst[f]] + [r[k] for k in keys if k in r])
    return worst


def print_f32_worst():
    print({k: float("%.3g" % v) for k, v in measure_f32_worst().items()})
