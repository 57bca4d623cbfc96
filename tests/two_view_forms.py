"""The plane gradients of the camera head's refinement stage (csrc/two_view_train.hip: refine_score_maps_bwd_geo_kernel,
geo_sequence_bwd_kernel) as data, under the rule of tests/refine_bwd_forms.py: seeded inputs and cotangents whose decisions are not
marginal, the two forwards restated in plain dtype-generic torch (float64 differentiated with torch.autograd.grad is the yardstick - the
oracle's geo_sequence builds f32 buffers and cannot run in float64; float32 is the restatement the limits are measured from), a
per-element allowance A_k = 2^-24 S_k + C_k, and a float32 emulation of geo_sequence_bwd_kernel's formulas in which errors can be planted.
tests/test_two_view_forms_gpu.py holds the kernels to it, tests/test_two_view_forms_cpu.py proves inputs, constants and the sharpness of
the bound.  Also the numpy restatement of match_compact / corr_compact.  Imports without a GPU.

  score_maps_geo   leaves: geo_local [B,nq,6]; forward: refine_bwd_forms.score_maps_fwd (its geo_local is already an input); key = nq
  geo_sequence     leaves: planes1, planes2 [B,nq,3]; forward: geo_sequence_fwd below; key = (nq, warp_in_ref)
"""
from __future__ import annotations

import functools

import numpy as np
import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g, quat_to_rotmat, rand_planes, rand_unit_quat
from oracle import nopesac_oracle as O           # (here, not under a switched default dtype: it makes constants as it is imported)
from tests import refine_bwd_forms as R

F32, F64 = torch.float32, torch.float64
NQS = (1, 2, 50, 64, 128)
WARPS = (True, False)
EPS24, EPS23 = R.EPS24, R.EPS23
DRAWS = R.DRAWS
LIMIT_FACTOR = R.LIMIT_FACTOR                  # the project's factor 8: a kernel may order its sums differently from autograd

# worst error / A of the float32 autograd restatement over every case of the family.  Printed by
#   python -c "from tests import two_view_forms as T; T.print_f32_worst()"
# and re-measured by tests/test_two_view_forms_cpu.py (a figure off by more than 2x fails).  Never measured from a kernel.
F32_WORST = {"score_maps_geo": 2.03, "geo_sequence": 5.62}

SIG_MARGIN = 1e-3            # |w1[0] wa[0]| / (|w1| |wa|) of every sequence position under warp_in_ref: the sign of the product is not marginal
DIST_MARGIN = R.DIST_MARGIN  # dn, dl2 over the live hypotheses x matched planes: exactly 0 or above this
NORM_MARGIN = 1e-2           # every live plane norm (and that of its warp) is above this
SEED_STEP = {}               # (nq,) -> seed step where the first seed breaks an input condition


def limit(family):
    return LIMIT_FACTOR * F32_WORST[family]


# ===================================================================================================================== inputs
def pair_kinds(nq):
    """The pairs of one launch: m = 1, 2, nq // 2, nq (clipped to [1, nq], deduplicated), an empty pair, and where nq allows them a fan
    pair (one row matched to three columns, one column matched to three rows), a ragged pair (n1, n2 below nq, ones in the assignment
    beyond them) and, at nq = 2, the overflow pair (the assignment all ones: four matches cut to m = 2)."""
    out = []
    for v in (1, 2, nq // 2, nq):
        v = min(max(v, 1), nq)
        if ("plain", v) not in out:
            out.append(("plain", v))
    out.append(("empty", 0))
    if nq >= 8:
        out += [("fan", nq // 2), ("ragged", nq // 2)]
    if nq == 2:
        out.append(("overflow", 2))
    return out


def pair_margins(a1, a2, q, t):
    """(sig, norm) of one pair over EVERY plane of both views (the fan and the overflow pair match planes the pose does not relate): the
    sig product's distance from 0 relative to its factors, and the smallest norm among the planes and the warps of view 1."""
    _, _, (w1, wa) = _encode(a1.double(), a2.double(), q.double(), t.double(), True)
    sig = ((w1[:, 0] * wa[:, 0]).abs() / (w1.norm(dim=-1) * wa.norm(dim=-1))).min()
    norm = torch.cat([a1.double().norm(dim=-1), a2.double().norm(dim=-1), w1.norm(dim=-1), wa.norm(dim=-1)]).min()
    return float(sig), float(norm)


def draw_pair(nq, mm, g):
    """synth.consistent_planes with the input conditions built in: two sets of nq planes related by a pose on mm (permuted) planes, and the
    initial pose next to that pose.  A view-1 plane (with its partner, if it has one) is drawn again from the same generator until its
    own conditions hold with a factor 2 to spare (pair_margins) - with some hundred matched planes per launch a seed step of the whole
    launch would never end - and the number of rejected draws is recorded.  -> planes1, planes2, perm (-1: none), init_rot, init_trans,
    rejected."""
    q, t = rand_unit_quat(g), 0.4 * torch.randn(3, generator=g)
    Rgt = quat_to_rotmat(q)
    r0q = F.normalize(q + 0.05 * torch.randn(4, generator=g), dim=0)
    r0q, t0 = (-r0q if r0q[0] < 0 else r0q), t + 0.1 * torch.randn(3, generator=g)
    flip = torch.tensor([1.0, -1.0, -1.0])
    planes1, planes2 = torch.zeros(nq, 3), rand_planes(nq, g)
    cols, rows = torch.randperm(nq, generator=g)[:mm].tolist(), torch.randperm(nq, generator=g)[:mm].tolist()
    perm = torch.full((nq,), -1, dtype=torch.long)
    perm[rows] = torch.tensor(cols, dtype=torch.long)
    rejected = 0
    for i in range(nq):
        while True:
            p, noise = rand_planes(1, g)[0], 0.05 * torch.randn(3, generator=g)
            other = planes2[i]                                   # (any plane of norm >= 0.5 when plane i has no partner)
            if perm[i] >= 0:
                f = p * flip
                nrm = Rgt @ (f / f.norm())
                other = (nrm * (f.norm() + (t * nrm).sum()) + noise) * flip
            sig, norm = pair_margins(p[None], other[None], r0q, t0)
            if sig >= 2 * SIG_MARGIN and norm >= 2 * NORM_MARGIN:
                break
            rejected += 1
        planes1[i] = p
        if perm[i] >= 0:
            planes2[perm[i]] = other
    return planes1, planes2, perm, r0q, t0, rejected


@functools.lru_cache(maxsize=None)
def inputs(nq):
    """One launch at nq (f32 CPU tensors): planes of both views consistent with a pose on the matched pairs, the assignment, the initial
    pose next to the true one, raw hypotheses, and the cotangents of both kernels."""
    g = _g(21000 + nq + 1000 * SEED_STEP.get((nq,), 0))
    kinds = pair_kinds(nq)
    B, NH = len(kinds), nq + 1
    p1, p2, A = torch.zeros(B, nq, 3), torch.zeros(B, nq, 3), torch.zeros(B, nq, nq)
    n1, n2 = torch.full((B,), nq, dtype=torch.int32), torch.full((B,), nq, dtype=torch.int32)
    rots, trs, redraws = [], [], []
    for b, (kind, mm) in enumerate(kinds):
        a1, a2, perm, r0q, t0, rejected = draw_pair(nq, mm, g)
        redraws.append(rejected)
        p1[b], p2[b] = a1, a2
        for i in torch.nonzero(perm >= 0)[:, 0].tolist():
            A[b, i, perm[i]] = 1.0
        if kind == "fan":
            rows = torch.nonzero(perm >= 0)[:, 0].tolist()
            r0, r1 = rows[0], rows[1]
            free_c = [c for c in range(nq) if A[b, :, c].sum() == 0][:2]
            free_r = [r for r in range(nq) if A[b, r].sum() == 0][:2]
            A[b, r0, free_c] = 1.0                               # row r0: three columns
            A[b, free_r, perm[r1]] = 1.0                         # column perm[r1]: three rows
        if kind == "ragged":
            n1[b], n2[b] = nq - 2, nq - 1
            A[b, nq - 1, :] = 1.0                                # ones beyond n1 / n2: never read
            A[b, :, nq - 1] = 1.0
        if kind == "overflow":
            A[b] = 1.0
        rots.append(r0q)
        trs.append(t0)
    rot_raw = torch.randn(B, nq, 4, generator=g) * (0.2 + 2.0 * torch.rand(B, nq, 1, generator=g))
    c = {"nq": nq, "kinds": kinds, "redraws": redraws, "planes1": p1, "planes2": p2, "A": A, "n1": n1, "n2": n2, "init_rot": torch.stack(rots),
         "init_trans": torch.stack(trs), "rot_raw": rot_raw, "trans_raw": 0.5 * torch.randn(B, nq, 3, generator=g)}
    for k in ("g_normal_score", "g_param_score", "g_l2_dist"):
        c[k] = R._cot(g, B, NH, nq)
    c["g_geo_local"], c["g_geo_enc"] = R._cot(g, B, nq, 6), R._cot(g, B, nq, 8)
    c["seq"] = sequence_index(A, n1, n2)
    c["m"] = torch.tensor([len(r) for r, _ in c["seq"]], dtype=torch.int32)
    with torch.no_grad():                                        # what the score-maps kernels read: the f32 sequence
        c["geo_local"] = geo_sequence_fwd(p1, p2, A, c["init_trans"], c["init_rot"], True, n1, n2)[0]
    return c


# ===================================================================================================================== the forward
def sequence_index(A, n1, n2):
    """Per pair (rows, cols) of the matched pairs in row-major order of A[:n1, :n2], cut at nq pairs (geo_sequence_kernel)."""
    nq = A.shape[1]
    out = []
    for b in range(A.shape[0]):
        idx = torch.nonzero(A[b, :int(n1[b]), :int(n2[b])] != 0)[:nq]
        out.append((idx[:, 0], idx[:, 1]))
    return out


def _encode(p1, p2, q, t, warp_in_ref):
    """geo_local [k,6] and geo_enc [k,8] of k matched pairs of one pair of views; also the two factors of the sig product."""
    flip = R._flip(p1)
    Rm = R.quat_to_rot(q)[None, None]
    f = (p1 * flip)[None, None]
    w1 = R.warp(f, Rm, t[None, None])[0, 0]
    wa = R.warp(f, Rm, torch.zeros_like(t)[None, None])[0, 0]
    sg = torch.where(w1[:, 0] * wa[:, 0] >= 0, 1.0, -1.0).to(p1.dtype).detach()[:, None]
    s0, s1 = (w1, p2 * flip) if warp_in_ref else (p1, p2)
    o0, o1 = s0.norm(dim=-1, keepdim=True), s1.norm(dim=-1, keepdim=True)
    first = torch.cat([s0 / (o0 + 1e-10), o0], -1)
    if warp_in_ref:
        first = first * sg
    return torch.cat([p1, p2], -1), torch.cat([first, s1 / (o1 + 1e-10), o1], -1), (w1.detach(), wa.detach())


def geo_sequence_fwd(planes1, planes2, A, init_trans, init_rot, warp_in_ref, n1=None, n2=None):
    """geo_sequence_kernel's two differentiable outputs in the dtype of the planes -> (geo_local [B,nq,6], geo_enc [B,nq,8], m [B]).
    The pose is a constant; sig is piecewise constant."""
    B, nq = A.shape[:2]
    full = torch.full((B,), nq)
    seq = sequence_index(A, full if n1 is None else n1, full if n2 is None else n2)
    local, enc = [], []
    for b, (rows, cols) in enumerate(seq):
        l, e, _ = _encode(planes1[b, rows], planes2[b, cols], init_rot[b].to(planes1.dtype), init_trans[b].to(planes1.dtype), warp_in_ref)
        pad = nq - len(rows)
        local.append(torch.cat([l, l.new_zeros(pad, 6)]))
        enc.append(torch.cat([e, e.new_zeros(pad, 8)]))
    return torch.stack(local), torch.stack(enc), torch.tensor([len(r) for r, _ in seq])


# ===================================================================================================================== families
FAMILIES = {"score_maps_geo": dict(leaves=("geo_local",), consts=("rot_raw", "trans_raw", "init_rot", "init_trans"),
                                   cots=("g_normal_score", "g_param_score", "g_l2_dist"), out=("g_geo_local",)),
            "geo_sequence": dict(leaves=("planes1", "planes2"), consts=("init_trans", "init_rot"), cots=("g_geo_local", "g_geo_enc"),
                                 out=("g_planes1", "g_planes2"))}


def family_keys(family):
    return list(NQS) if family == "score_maps_geo" else [(nq, w) for nq in NQS for w in WARPS]


def problem(family, key):
    """(x: every float input, f32; aux; cotangents f32) of one case."""
    fam = FAMILIES[family]
    c = inputs(key if family == "score_maps_geo" else key[0])
    x = {k: c[k] for k in fam["leaves"] + fam["consts"]}
    aux = {"m": c["m"].long()} if family == "score_maps_geo" else {"A": c["A"], "n1": c["n1"], "n2": c["n2"], "warp_in_ref": key[1]}
    return x, aux, [c[k] for k in fam["cots"]]


def forward(family, xs, aux):
    if family == "score_maps_geo":
        return R.score_maps_fwd(xs, aux)
    return list(geo_sequence_fwd(xs["planes1"], xs["planes2"], aux["A"], xs["init_trans"], xs["init_rot"], aux["warp_in_ref"], aux["n1"],
                                 aux["n2"])[:2])


def vjp(family, x, aux, cots, dtype):
    """J^T g with torch.autograd in `dtype` -> {leaf: gradient} (zeros where nothing arrives)."""
    fam = FAMILIES[family]
    xs = {k: v.to(dtype).clone().requires_grad_(k in fam["leaves"]) for k, v in x.items()}
    outs = forward(family, xs, dict(aux))
    total = sum((o * g.to(dtype)).sum() for o, g in zip(outs, cots))
    grads = torch.autograd.grad(total, [xs[k] for k in fam["leaves"]], allow_unused=True)
    return {k: (torch.zeros_like(xs[k]) if g is None else g).detach() for k, g in zip(fam["leaves"], grads)}


def term_magnitudes(family, x, aux, cots):
    """S_k = sum_i |g_i| |J_ik| in float64.  score_maps_geo: output (h, j) reads plane row j alone, so one backward pass per (output,
    hypothesis) serves every row.  geo_sequence: the planes are made one leaf per SEQUENCE POSITION, which makes the Jacobian block
    diagonal over positions - one pass per output component - and the magnitudes of a plane's positions are added afterwards."""
    if family == "score_maps_geo":
        xs = {k: v.double().clone().requires_grad_(k == "geo_local") for k, v in x.items()}
        S = torch.zeros_like(xs["geo_local"])
        for o, g in zip(R.score_maps_fwd(xs, dict(aux)), cots):
            for h in range(o.shape[1]):
                (gr,) = torch.autograd.grad((o[:, h] * g[:, h].double().abs()).sum(), [xs["geo_local"]], retain_graph=True, allow_unused=True)
                if gr is not None:
                    S += gr.abs()
        return {"geo_local": S.detach()}
    p1, p2 = x["planes1"].double(), x["planes2"].double()
    S1, S2 = torch.zeros_like(p1), torch.zeros_like(p2)
    for b, (rows, cols) in enumerate(sequence_index(aux["A"], aux["n1"], aux["n2"])):
        if not len(rows):
            continue
        a, c = p1[b, rows].clone().requires_grad_(True), p2[b, cols].clone().requires_grad_(True)
        l, e, _ = _encode(a, c, x["init_rot"][b].double(), x["init_trans"][b].double(), aux["warp_in_ref"])
        for o, g in zip((l, e), cots):
            for d in range(o.shape[1]):
                ga, gc = torch.autograd.grad((o[:, d] * g[b, :len(rows), d].double().abs()).sum(), [a, c], retain_graph=True, allow_unused=True)
                if ga is not None:
                    S1[b].index_add_(0, rows, ga.abs())
                if gc is not None:
                    S2[b].index_add_(0, cols, gc.abs())
    return {"planes1": S1, "planes2": S2}


def conditioning(family, x, aux, cots, ref):
    """C_k: the largest change of the float64 VJP over DRAWS draws that multiply every f32 input by 1 + d, |d| <= 2^-23."""
    g = _g(78)
    C = {k: torch.zeros_like(v) for k, v in ref.items()}
    for _ in range(DRAWS):
        got = vjp(family, {k: R.jiggle(v, g) for k, v in x.items()}, aux, [R.jiggle(t, g) for t in cots], F64)
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return C


@functools.lru_cache(maxsize=None)
def reference(family, key):
    """-> (ref, A): the float64 VJP and the allowance 2^-24 S + C per element, keyed by the kernel's output names."""
    x, aux, cots = problem(family, key)
    ref = vjp(family, x, aux, cots, F64)
    S = term_magnitudes(family, x, aux, cots)
    C = conditioning(family, x, aux, cots, ref)
    names = dict(zip(FAMILIES[family]["leaves"], FAMILIES[family]["out"]))
    return {names[k]: v for k, v in ref.items()}, {names[k]: EPS24 * S[k] + C[k] for k in ref}


def worst_ratio(family, key, got):
    """{output: (worst error / A, flat index)} of `got` (a dict over the kernel's output names)."""
    ref, A = reference(family, key)
    out = {}
    for k in ref:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        q = R.ratios(got[k], ref[k], A[k]).reshape(-1)
        out[k] = (float(q.max()), int(q.argmax()))
    return out


def f32_restatement(family, key):
    x, aux, cots = problem(family, key)
    got = vjp(family, x, aux, cots, F32)
    return dict(zip(FAMILIES[family]["out"], (got[k] for k in FAMILIES[family]["leaves"])))


def f32_worst(family):
    return max(q for key in family_keys(family) for q, _ in worst_ratio(family, key, f32_restatement(family, key)).values())


def print_f32_worst():
    for family in FAMILIES:
        print('"%s": %.3g,' % (family, f32_worst(family)))


def expected_zero(nq):
    """Where the contract says exact zero: (rows of g_geo_local at or beyond m, planes of view 1 / view 2 that no sequence position names)
    as bool masks [B,nq]."""
    c = inputs(nq)
    B = len(c["kinds"])
    z0 = torch.arange(nq)[None] >= c["m"][:, None]
    z1, z2 = torch.ones(B, nq, dtype=torch.bool), torch.ones(B, nq, dtype=torch.bool)
    for b, (rows, cols) in enumerate(c["seq"]):
        z1[b, rows] = False
        z2[b, cols] = False
    return z0, z1, z2


# ===================================================================================================================== margins
def margins(nq):
    """The input conditions of one launch as measured figures: the sig product's relative distance from 0, the smallest non-zero dn / dl2
    over live hypotheses x matched planes, the smallest live plane norm (the planes and their warps)."""
    c = inputs(nq)
    sig, norm = float("inf"), float("inf")
    for b, (rows, cols) in enumerate(c["seq"]):
        if not len(rows):
            continue
        a, d = c["planes1"][b, rows].double(), c["planes2"][b, cols].double()
        _, _, (w1, wa) = _encode(a, d, c["init_rot"][b].double(), c["init_trans"][b].double(), True)
        sig = min(sig, float(((w1[:, 0] * wa[:, 0]).abs() / (w1.norm(dim=-1) * wa.norm(dim=-1))).min()))
        norm = min(norm, float(torch.cat([a.norm(dim=-1), d.norm(dim=-1), w1.norm(dim=-1), wa.norm(dim=-1)]).min()))
    xs = {k: c[k].double() for k in ("geo_local", "rot_raw", "trans_raw", "init_rot", "init_trans")}
    aux = {"m": c["m"].long()}
    m = aux["m"]
    dl2 = R.score_maps_fwd(xs, aux)[2]
    live = (torch.arange(nq + 1)[None, :, None] <= m[:, None, None]) & (torch.arange(nq)[None, None, :] < m[:, None, None])
    dl2, dn = dl2[live], aux["dn"][live]
    nz = lambda d: float(d[d != 0].min()) if (d != 0).any() else float("inf")
    return {"sig": sig, "norm": norm, "dist": min(nz(dl2), nz(dn))}


# ===================================================================================================================== f32 emulation
PLANTS = ("missing_flip", "fan_summed_once", "cut_ignored")


def _enc_half_bwd(s, g4, sg):
    o = s.norm(dim=-1, keepdim=True)
    den = o + 1e-10
    dot = (g4[:, :3] * s).sum(-1, keepdim=True)
    go = sg * (g4[:, 3:4] - dot / (den * den))
    return sg * g4[:, :3] / den + torch.where(o > 0, go * s / torch.where(o > 0, o, torch.ones_like(o)), torch.zeros_like(s))


def _warp_bwd_plane(p, Rm, t, g):
    flip = R._flip(p)
    u = (p * flip) @ Rm.T
    nu = u.norm(dim=-1, keepdim=True)
    gu, _ = R._warp_bwd(u, nu, t.expand_as(u), g, None)
    return (gu @ Rm) * flip


def emulate_geo_sequence(key, plant=None):
    """geo_sequence_bwd_kernel's formulas in float32, position by position in sequence order; `plant` puts one error in:
    missing_flip (the view-2 gradient of the warped form is not flipped back), fan_summed_once (a plane keeps the gradient of its first
    position only), cut_ignored (a row starts at its uncut position, wrapped into the buffer)."""
    nq, wir = key
    c = inputs(nq)
    B = len(c["kinds"])
    g1, g2 = torch.zeros(B, nq, 3), torch.zeros(B, nq, 3)
    flip = torch.tensor([1.0, -1.0, -1.0])
    for b in range(B):
        n1, n2 = int(c["n1"][b]), int(c["n2"][b])
        idx = torch.nonzero(c["A"][b, :n1, :n2] != 0)
        if plant != "cut_ignored":
            idx = idx[:nq]
        if not len(idx):
            continue
        rows, cols = idx[:, 0], idx[:, 1]
        pos = torch.arange(len(idx)) % nq
        p1, p2 = c["planes1"][b, rows], c["planes2"][b, cols]
        Rm, t = R.quat_to_rot(c["init_rot"][b]), c["init_trans"][b][None]
        gl, ge = c["g_geo_local"][b, pos], c["g_geo_enc"][b, pos]
        a, d = gl[:, :3].clone(), gl[:, 3:].clone()
        if wir:
            _, _, (w1, wa) = _encode(p1, p2, c["init_rot"][b], c["init_trans"][b], True)
            sg = torch.where(w1[:, 0] * wa[:, 0] >= 0, 1.0, -1.0)[:, None]
            a = a + _warp_bwd_plane(p1, Rm, t, _enc_half_bwd(w1, ge[:, :4], sg))
            gs1 = _enc_half_bwd(p2 * flip, ge[:, 4:], torch.ones_like(sg))
            d = d + (gs1 if plant == "missing_flip" else gs1 * flip)
        else:
            one = torch.ones(len(idx), 1)
            a, d = a + _enc_half_bwd(p1, ge[:, :4], one), d + _enc_half_bwd(p2, ge[:, 4:], one)
        seen1, seen2 = set(), set()
        for k in range(len(idx)):                                # sequence order
            r, cc = int(rows[k]), int(cols[k])
            if not (plant == "fan_summed_once" and r in seen1):
                g1[b, r] += a[k]
            if not (plant == "fan_summed_once" and cc in seen2):
                g2[b, cc] += d[k]
            seen1.add(r); seen2.add(cc)
    return {"g_planes1": g1, "g_planes2": g2}


# ===================================================================================================================== trainer level
# The refinement pass with the PLANES as leaves: the sequence restated above in front of the oracle's ransac_refine_train (which is
# dtype-generic; only the oracle's geo_sequence builds f32 buffers).  tests/test_two_view_forms_cpu.py pins the f32 form of this to
# oracle._refine_train_from_assignment, which is pinned to the reference.
AUX_CASE = dict(nq=50, ms=(7, 2, 32, 50, 1), seeds=(67, 62, 92, 110, 61), weight=0.1)          # the five pairs of tests/test_training_gpu.py
TRAIN_CASE = dict(nq=50, ms=(7, 19), seed=80)                                                     # tests/test_two_view_training_gpu.py (B = 2)
# error of the float32 restatement against float64 over the tensor's own scale (max |error| / max |reference|) on TRAIN_CASE, measured on
# the CPU by  python -c "from tests import two_view_forms as T; print(T.trainer_f32_error())"  and re-measured by the CPU tests (2x);
# the GPU test's bound is LIMIT_FACTOR times this.
TRAINER_F32_ERR = {"planes1": 1.55e-6, "planes2": 1.87e-6}


def refine_restated(sd, planes1, planes2, A, n1, n2, init_trans, init_rot, trans_feat, rot_feat, gt_pose, nq, suffix, weight, dtype,
                    warp_in_ref=True):
    """forawrd_refineLoop + __forward_PlaneCamRefHead for padded planes [B,nq,3] that may require grad -> the seven losses.  The geometry
    sequence is built from the DETACHED initial pose (camera_head.py:353-368)."""
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=dtype)
    gl, gg, sg, ms = [], [], [], []
    for b, (rows, cols) in enumerate(sequence_index(A, n1, n2)):
        a, d = planes1[b, rows], planes2[b, cols]
        q, t = init_rot[b].detach().to(dtype), init_trans[b].detach().to(dtype)
        Rm, f = R.quat_to_rot(q)[None, None], (a * flip)[None, None]
        w1, wa = R.warp(f, Rm, t[None, None])[0, 0], R.warp(f, Rm, torch.zeros_like(t)[None, None])[0, 0]
        pad = a.new_zeros(nq - len(rows), 6)
        gl.append(torch.cat([torch.cat([a, d], -1), pad]))
        gg.append(torch.cat([torch.cat([w1, d * flip], -1), pad]))
        sg.append(torch.cat([torch.where(w1[:, 0:1] * wa[:, 0:1] >= 0, 1.0, -1.0).to(dtype).detach(), a.new_ones(nq - len(rows), 1)]))
        ms.append(len(rows))
    sdd = {k: v.to(dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    cfg = O.OracleConfig(num_queries=nq, out_cam_type="soft", warp_plane_in_cam_ref=warp_in_ref)
    losses, _ = O.ransac_refine_train(sdd, trans_feat, rot_feat, torch.stack(gg), torch.stack(gl), torch.stack(sg), ms, init_trans, init_rot,
                                      gt_pose.to(dtype), cfg, suffix=suffix, weight=weight)
    return losses


class _default_dtype:
    """(the oracle creates a few constants in the default dtype)"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


@functools.lru_cache(maxsize=None)
def aux_case():
    """The five pairs of AUX_CASE as one padded batch (f32)."""
    from tests import golden_inputs as GI
    nq = AUX_CASE["nq"]
    cases = [GI.refine_case(nq, m, s) for m, s in zip(AUX_CASE["ms"], AUX_CASE["seeds"])]
    B = len(cases)
    A = torch.zeros(B, nq, nq)
    pad = lambda t: torch.cat([t, torch.zeros(nq - t.shape[0], 3)], 0)
    for b, c in enumerate(cases):
        A[b, :c["A"].shape[0], :c["A"].shape[1]] = c["A"]
    st = lambda k: torch.stack([c[k] for c in cases])
    return {"A": A, "planes1": torch.stack([pad(c["planes1"]) for c in cases]), "planes2": torch.stack([pad(c["planes2"]) for c in cases]),
            "n1": torch.tensor([c["planes1"].shape[0] for c in cases], dtype=torch.int32),
            "n2": torch.tensor([c["planes2"].shape[0] for c in cases], dtype=torch.int32), "init_trans": st("init_trans"),
            "init_rot": st("init_rot"), "trans_feat": st("trans_feat"), "rot_feat": st("rot_feat"),
            "gt_pose": GI.gt_pose_case(B, AUX_CASE["seeds"][0])}


def aux_restated(dtype, suffix="initCamRef_Aux"):
    """The _Aux pass on aux_case() in `dtype` -> (losses, g_planes1, g_planes2) of the sum of the seven losses."""
    from nopesac_amd.synth import synth_state_dict
    c, sd = aux_case(), synth_state_dict(AUX_CASE["nq"])         # (drawn in the default dtype: outside the switch)
    with _default_dtype(dtype):
        p1, p2 = c["planes1"].to(dtype).requires_grad_(True), c["planes2"].to(dtype).requires_grad_(True)
        cv = lambda k: c[k].to(dtype)
        losses = refine_restated(sd, p1, p2, c["A"], c["n1"], c["n2"], cv("init_trans"), cv("init_rot"),
                                 cv("trans_feat"), cv("rot_feat"), c["gt_pose"], AUX_CASE["nq"], suffix, AUX_CASE["weight"], dtype)
        g1, g2 = torch.autograd.grad(sum(losses.values()), [p1, p2])
    return {k: v.detach() for k, v in losses.items()}, g1, g2


@functools.lru_cache(maxsize=None)
def train_case():
    from tests import golden_inputs as GI
    return GI.camera_train_case(TRAIN_CASE["nq"], TRAIN_CASE["ms"], TRAIN_CASE["seed"])


def camera_aux_restated(sd, c, nq, weight, dtype, conv_feats=None, fc_feats=None):
    """The two _Aux passes of the training-mode camera head (initCamRef_Aux, initRecCamRef_Aux: 14 losses - the only ones the predicted
    planes reach) in `dtype` with the planes as leaves -> (losses, g_planes1, g_planes2).  conv_feats: the conv stacks' outputs (yt, yr)
    [B,768] as the trainer hands them to its Linear layers; fc_feats: the outputs (tf0, rf0) [B,256] of fc_trans / fc_rots instead; neither:
    the oracle's own conv stacks."""
    p = "camera_head_list.0"
    with _default_dtype(dtype):
        sdd = {k: v.to(dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
        lin = lambda x, n: F.linear(x, sdd[f"{p}.{n}.weight"], sdd[f"{p}.{n}.bias"])
        if fc_feats is not None:
            tf0, rf0 = fc_feats[0].to(dtype), fc_feats[1].to(dtype)
            trans0, rot0 = lin(tf0, "trans"), F.normalize(lin(rf0, "rots"), p=2, dim=1)
        elif conv_feats is None:
            trans0, rot0, tf0, rf0, _ = O.pixel_pose_net(sdd, {k: v.to(dtype) for k, v in c["feats1"].items()},
                                                         {k: v.to(dtype) for k, v in c["feats2"].items()}, p)
        else:
            tf0, rf0 = torch.relu(lin(conv_feats[0].to(dtype), "fc_trans")), torch.relu(lin(conv_feats[1].to(dtype), "fc_rots"))
            trans0, rot0 = lin(tf0, "trans"), F.normalize(lin(rf0, "rots"), p=2, dim=1)
        rec_t, rec_r, rec_tf, rec_rf = O.aim_reembed(sdd, trans0.detach(), rot0.detach(), p)
        p1, p2 = c["planes1"].to(dtype).requires_grad_(True), c["planes2"].to(dtype).requires_grad_(True)
        losses = {}
        for name, it, ir, itf, irf in (("initCamRef", trans0, rot0, tf0, rf0), ("initRecCamRef", rec_t, rec_r, rec_tf, rec_rf)):
            losses.update(refine_restated(sd, p1, p2, c["A"], c["n1"], c["n2"], it, ir, itf, irf, c["gt_pose"], nq, name + "_Aux", weight, dtype))
        g1, g2 = torch.autograd.grad(sum(losses.values()), [p1, p2])
    return {k: v.detach() for k, v in losses.items()}, g1, g2


def scale_error(got, ref):
    """max |error| over the tensor's own scale (the trainer-level form of tests/test_training_gpu.py)."""
    return float((got.double() - ref.double()).abs().max()) / float(ref.double().abs().max())


def trainer_f32_error(weight=0.1):
    from nopesac_amd.synth import synth_state_dict
    sd, c, nq = synth_state_dict(TRAIN_CASE["nq"]), train_case(), TRAIN_CASE["nq"]
    with torch.no_grad():                                        # the conv stacks once (f32): both precisions start from the same features
        fc = O.pixel_pose_net(sd, c["feats1"], c["feats2"])[2:4]
    _, a1, a2 = camera_aux_restated(sd, c, nq, weight, F64, fc_feats=fc)
    _, b1, b2 = camera_aux_restated(sd, c, nq, weight, F32, fc_feats=fc)
    return {"planes1": scale_error(b1, a1), "planes2": scale_error(b2, a2)}


# ===================================================================================================================== match_compact / corr_compact
COMPACT_NQS = (2, 50, 128)


def compact_case(nq, nmax, orders=("sorted", "reversed", "random"), seed=0):
    """N images: for every n in (0, 1, nmax) and every order of match_q one image; match_q rows are padded with -1 behind n."""
    rng = np.random.default_rng(31000 + 7 * nq + nmax + seed)
    ns = [n for n in dict.fromkeys((0, 1, nmax))]
    imgs = [(n, o) for n in ns for o in orders]
    N = len(imgs)
    mq = np.full((N, nmax), -1, np.int32)
    for i, (n, o) in enumerate(imgs):
        q = np.sort(rng.choice(nq, size=n, replace=False)).astype(np.int32)
        mq[i, :n] = q if o == "sorted" else q[::-1] if o == "reversed" else rng.permutation(q)
    return {"x": rng.standard_normal((N, nq, 256)).astype(np.float32), "params": rng.standard_normal((N, nq, 3)).astype(np.float32),
            "match_q": mq, "n": np.array([n for n, _ in imgs], np.int32)}


def match_compact_np(x, params, match_q, n):
    """numpy restatement of nopesac_match_compact -> (x_c, params_c, order, rank, bad)."""
    N, nq, _ = x.shape
    nmax = match_q.shape[1]
    x_c, p_c = np.zeros_like(x), np.zeros_like(params)
    order, rank = np.full((N, nq), -1, np.int32), np.full((N, nq), -1, np.int32)
    bad = np.zeros(N, np.int32)
    for i in range(N):
        ni = int(n[i])
        q = match_q[i, :max(min(ni, nmax), 0)]
        if ni < 0 or ni > min(nq, nmax) or (q < 0).any() or (q >= nq).any() or len(set(q.tolist())) != len(q):
            bad[i] = 1
            continue
        s = np.sort(q)
        order[i, :ni], rank[i, s] = s, np.arange(ni)
        x_c[i, :ni], p_c[i, :ni] = x[i, s], params[i, s]
    return x_c, p_c, order, rank, bad


def corr_compact_np(gt_corr, order1, order2, n1, n2):
    B, S, _ = gt_corr.shape
    nq = S - 1
    out = np.zeros_like(gt_corr)
    for b in range(B):
        a = [int(q) if (r < n1[b] and 0 <= q < nq) else -1 for r, q in enumerate(order1[b])] + [nq]
        c = [int(q) if (r < n2[b] and 0 <= q < nq) else -1 for r, q in enumerate(order2[b])] + [nq]
        for r in range(S):
            for k in range(S):
                if a[r] >= 0 and c[k] >= 0:
                    out[b, r, k] = gt_corr[b, a[r], c[k]]
    return out
