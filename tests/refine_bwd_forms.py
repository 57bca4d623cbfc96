"""The geometry half of the camera head's backward pass (csrc/refine_bwd.hip: refine_score_maps_bwd_kernel, refine_vote_bwd_kernel,
refine_losses_bwd_kernel, camera_pose_loss_bwd_kernel) as data: seeded inputs and cotangents whose decisions are not marginal, each of
the four forwards restated in plain torch (dtype-generic: float64 is the reference, differentiated with torch.autograd.grad; float32 is
the restatement the limits are measured from), a per-element allowance A_k = 2^-24 S_k + C_k for every element of every gradient, and a
hand-written float32 emulation of the kernels' own backward formulas in which errors can be planted.  tests/test_refine_bwd_forms_gpu.py
holds the kernels to it, tests/test_refine_bwd_forms_cpu.py proves inputs, constants, references and the sharpness of the bound.
Imports without a GPU.

  S_k = sum_i |g_i| |J_ik|   the magnitudes of the terms that make element k, in float64: one backward pass per cotangent column
                             (the Jacobians are block diagonal over pairs / hypotheses, so one pass serves every block at once)
  C_k                        conditioning: the largest change of the float64 VJP at k over DRAWS seeded draws that multiply every
                             f32 input (cotangents included) by 1 + d, d = +- 2^-23 with random signs (the largest step allowed, so
                             that C_k is not small by the luck of a small draw)
  limit                      8 x the worst error / A of the float32 autograd restatement over the cases of the family (F32_WORST,
                             measured on the CPU; never measured from a kernel)
"""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g, consistent_planes, rand_planes, rand_unit_quat

F32, F64 = torch.float32, torch.float64
NQS = (1, 2, 50, 64, 100, 128)
LOSS_BS = (1, 64, 65)                         # the two loss kernels: one thread per pair in blocks of 64
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23
DRAWS = 8
LIMIT_FACTOR = 8.0
LOSS_WEIGHT, POSE_WEIGHT = 0.75, 0.5
TRANS_EPS = (0.0, 1e-3)

# worst error / A of the float32 autograd restatement over every case of the family.  Printed by
#   python -c "from tests import refine_bwd_forms as R; R.print_f32_worst()"
# and re-measured by tests/test_refine_bwd_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"score_maps": 16.0, "vote": 4.35, "losses": 2.32, "pose_loss": 0.894}

# decision margins (checked for every case by the CPU tests; a seed that breaks one is stepped in SEED_STEP)
CLAMP_MARGIN = 1e-5          # relative distance of every softmax probability from 0.01 and 0.9
ARGMIN_MARGIN = 1e-4         # relative top-two gap of the index losses' argmin over the live hypotheses
SCORE_MARGIN = 1e-3          # |1 - score| at the picked hypothesis: 0 or at least this
DIST_MARGIN = 1e-3           # dn, dl2: exactly 0 or above this
SEED_STEP = {("geometry", 1): 1, ("losses", (50, 65)): 1, ("losses", (128, 64)): 1}           # (family, key) -> seed step where the first seed breaks an input condition (a cotangent of nq = 1 that is zero where it must not be; the argmin gap)


def limit(family):
    return LIMIT_FACTOR * F32_WORST[family]


def case_ms(nq):
    """Matched-plane counts of one launch: 1, 2, nq // 2, nq - 1, nq (clipped to [1, nq], deduplicated), then one empty pair."""
    out = []
    for v in (1, 2, nq // 2, nq - 1, nq):
        v = min(max(v, 1), nq)
        if v not in out:
            out.append(v)
    return out + [0]


def _cot(g, *shape):
    """A cotangent: N(0, 1) times a per-tensor scale in [0.3, 3), about one entry in ten exactly zero."""
    scale = 0.3 + 2.7 * torch.rand(1, generator=g).item()
    return scale * torch.randn(*shape, generator=g) * (torch.rand(*shape, generator=g) >= 0.1).float()


# ===================================================================================================================== float64 / float32 forwards
def _flip(x):
    return torch.tensor([1.0, -1.0, -1.0], dtype=x.dtype)


def quat_to_rot(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                        2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], dim=-1).reshape(*q.shape[:-1], 3, 3)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def warp(f, R, t):
    """common.h warp_plane on flipped planes f [B,1,n,3], R [B,NH,3,3], t [B,NH,3]: b = R f, out = ((b + t) . b) / (|b| + 1e-5)^2 b."""
    b = torch.einsum("bhik,bjk->bhji", R, f[:, 0])
    end = b + t.unsqueeze(-2)
    return ((end * b).sum(-1) / (b.norm(dim=-1) + 1e-5) ** 2).unsqueeze(-1) * b


def score_maps_fwd(x, aux, jsel=None):
    """ransac_score_maps_kernel's three differentiable outputs, batched over pairs: (normal_score, param_score, l2_dist) [B,NH,nq]
    (or the plane columns `jsel` of them)."""
    gl, rr = x["geo_local"], x["rot_raw"]
    m = aux["m"]
    B, nq = rr.shape[:2]
    if jsel is not None:
        gl = gl[:, jsel]
    rots = torch.cat([x["init_rot"][:, None], rr / rr.norm(dim=-1, keepdim=True).clamp_min(1e-12)], 1)
    trans = torch.cat([x["init_trans"][:, None], x["trans_raw"]], 1)
    R = quat_to_rot(rots)
    f0, p1 = (gl[..., :3] * _flip(gl))[:, None], (gl[..., 3:] * _flip(gl))[:, None]
    w_r, w_rt = warp(f0, R, torch.zeros_like(trans)), warp(f0, R, trans)
    dn = (unit(w_r) - unit(p1)).norm(dim=-1)
    dl2 = (w_rt - p1).norm(dim=-1)
    js = torch.arange(nq) if jsel is None else torch.as_tensor(jsel)
    mask = ((torch.arange(nq + 1)[None, :, None] <= m[:, None, None]) & (js[None, None, :] < m[:, None, None])).to(gl.dtype)
    aux["dn"] = (dn * mask).detach()                             # (for margins(): where dn reaches a gradient)
    return [torch.exp(-dn * mask) * mask, torch.exp(-dl2 * mask) * mask, dl2]


def _head(W, b, f):
    return (W * f[:, None, :]).sum(-1) + b


def vote_fwd(x, aux):
    """ransac_soft_vote_kernel in mode 16 (the training-side twin), batched over pairs with m >= 1, every parameter one leaf per pair:
    (pred_rot, pred_trans, avg_rot, avg_trans, score_rot, score_trans).  Also returns the softmax probabilities under "p" of aux."""
    m = aux["m"]
    nq = x["fused_rot"].shape[1]
    live = torch.arange(nq + 1)[None] <= m[:, None]
    pm = (torch.arange(nq)[None] < m[:, None]).to(x["fused_rot"].dtype)[:, :, None]
    mf = m.to(x["fused_rot"].dtype)[:, None]

    def scores(sf, w, b):
        raw = (sf * w[:, None, :]).sum(-1) + b
        p = torch.softmax(raw.masked_fill(~live, float("-inf")), 1)
        s = p.clamp(0.01, 0.9) * live.to(p.dtype)
        return s / (s.sum(1, keepdim=True) + 1e-10), p
    s_r, p_r = scores(x["sf_rot"], x["reg_rot_w"], x["reg_rot_b"])
    s_t, p_t = scores(x["sf_trans"], x["reg_trans_w"], x["reg_trans_b"])
    aux["p"] = (p_r.detach(), p_t.detach())
    fr_soft = x["init_rot_feat"] * s_r[:, 0:1] + (x["fused_rot"] * s_r[:, 1:, None]).sum(1)
    ft_soft = x["init_trans_feat"] * s_t[:, 0:1] + (x["fused_trans"] * s_t[:, 1:, None]).sum(1)
    fr_avg, ft_avg = (x["fused_rot"] * pm).sum(1) / mf, (x["fused_trans"] * pm).sum(1) / mf
    return [unit(_head(x["rots_w"], x["rots_b"], fr_soft)), _head(x["trans_w"], x["trans_b"], ft_soft),
            unit(_head(x["rots_w"], x["rots_b"], fr_avg)), _head(x["trans_w"], x["trans_b"], ft_avg), s_r, s_t]


def losses_fwd(x, aux):
    """plane_cam_ref_losses_kernel over the pairs with m >= 1 of a launch of aux["B"] pairs; the hypotheses the two index losses pick
    (aux["hr"], aux["ht"]) are constants.  -> [losses f[7]]."""
    gt = x["gt_pose"]
    dq = lambda q: (unit(gt[:, 3:]) - unit(q)).norm(dim=-1)
    dt = lambda t: (gt[:, :3] - t).norm(dim=-1)
    diag = torch.diagonal(x["l2_dist"][:, 1:, :], dim1=1, dim2=2).sum(-1) / aux["m"].to(gt.dtype)
    per = torch.stack([dt(x["avg_trans"]), dq(x["avg_rot"]), dt(x["pred_trans"]), dq(x["pred_rot"]),
                       (1 - x["score_rot"].gather(1, aux["hr"][:, None])[:, 0]).abs() * 0.01,
                       (1 - x["score_trans"].gather(1, aux["ht"][:, None])[:, 0]).abs() * 0.02, diag * 0.1])
    return [per.sum(1) * (aux["weight"] / aux["B"])]


def pose_loss_fwd(x, aux):
    """camera_pose_loss_kernel: [w mean |gt_t + eps - est_t|, w mean |n(gt_q) - n(est_q)|]."""
    lx = (x["gt_trans"] + aux["eps"] - x["est_trans"]).norm(dim=-1)
    lq = (unit(x["gt_rot"]) - unit(x["est_rot"])).norm(dim=-1)
    return [torch.stack([lx.sum(), lq.sum()]) * (aux["weight"] / aux["B"])]


def index_picks(rots_all, trans_all, gt_pose, m):
    """First minimum of the error against the ground truth over the live hypotheses (f64 from the f32 values) and the relative top-two
    gap of either choice.  Pairs with m >= 1."""
    er = (unit(gt_pose[:, None, 3:].double()) - unit(rots_all.double())).norm(dim=-1)
    et = (gt_pose[:, None, :3].double() - trans_all.double()).norm(dim=-1)
    dead = torch.arange(er.shape[1])[None] > m[:, None]
    er, et = er.masked_fill(dead, 1e10), et.masked_fill(dead, 1e10)
    gaps = []
    for e in (er, et):
        two = (-e).topk(2, dim=1).values.neg()
        gaps.append((two[:, 1] - two[:, 0]) / two[:, 1])
    return er.argmin(1), et.argmin(1), torch.minimum(*gaps)


# ===================================================================================================================== families
# family -> (forward, leaves in the order of OUTPUTS, every float input, names of the cotangents, names of the gradients the kernel writes)
VOTE_LEAVES = ("sf_rot", "sf_trans", "init_rot_feat", "init_trans_feat", "fused_rot", "fused_trans", "rots_w", "rots_b", "trans_w", "trans_b",
               "reg_rot_w", "reg_rot_b", "reg_trans_w", "reg_trans_b")
VOTE_OUT = ("g_sf_rot", "g_sf_trans", "g_init_rot_feat", "g_init_trans_feat", "g_fused_rot", "g_fused_trans", "pb_rots_w", "pb_rots_b",
            "pb_trans_w", "pb_trans_b", "pb_reg_rot_w", "pb_reg_rot_b", "pb_reg_trans_w", "pb_reg_trans_b")
# The gradient of a score regressor's bias is identically zero in exact arithmetic (the softmax does not see a shift), J_ik = 0 for every i,
# so S_k as defined above is 0 while the kernel adds nq + 1 terms gr[h] that cancel.  The bias is therefore one leaf per (pair, HYPOTHESIS):
# the reference and the allowance of pb_reg_*_b are the sums over h of those of the per-hypothesis leaves - S_k is then the sum of the
# magnitudes of the terms the kernel adds, which is what S_k stands for.
VOTE_BIAS_PER_HYPOTHESIS = ("reg_rot_b", "reg_trans_b")
VOTE_PARAMS = ("rots_w", "rots_b", "trans_w", "trans_b", "reg_rot_w", "reg_rot_b", "reg_trans_w", "reg_trans_b")
FAMILIES = {
    "score_maps": dict(fwd=score_maps_fwd, leaves=("rot_raw", "trans_raw", "init_rot", "init_trans"), consts=("geo_local",),
                       cots=("g_normal_score", "g_param_score", "g_l2_dist"), out=("g_rot_raw", "g_trans_raw", "g_init_rot", "g_init_trans")),
    "vote": dict(fwd=vote_fwd, leaves=VOTE_LEAVES, consts=(), out=VOTE_OUT,
                 cots=("g_pred_rot", "g_pred_trans", "g_avg_rot", "g_avg_trans", "g_score_rot", "g_score_trans")),
    "losses": dict(fwd=losses_fwd, leaves=("pred_rot", "pred_trans", "avg_rot", "avg_trans", "score_rot", "score_trans", "l2_dist"),
                   consts=("gt_pose",), cots=("g_loss",),
                   out=("g_pred_rot", "g_pred_trans", "g_avg_rot", "g_avg_trans", "g_score_rot", "g_score_trans", "g_l2_dist")),
    "pose_loss": dict(fwd=pose_loss_fwd, leaves=("est_trans", "est_rot", "gt_trans", "gt_rot"), consts=(), cots=("g_out",),
                      out=("g_est_trans", "g_est_rot", "g_gt_trans", "g_gt_rot")),
}


def family_keys(family):
    if family == "losses":
        return [(nq, B) for nq in NQS for B in LOSS_BS]
    if family == "pose_loss":
        return [(B, eps) for B in LOSS_BS for eps in TRANS_EPS]
    return list(NQS)


# ===================================================================================================================== inputs
@functools.lru_cache(maxsize=None)
def geometry_inputs(nq):
    """One launch of the score-maps and the vote kernel at nq (f32 CPU tensors), one pair per m of case_ms(nq), the empty pair last.
    Geometry as stage_forms.ransac_inputs: matched planes consistent with a pose, the initial pose next to it, raw hypothesis quaternions
    of every scale with two of norm < 1e-12 (the g / 1e-12 branch; one at nq = 1).  geo_local rows >= m are zero on even pairs (what geo_sequence
    writes) and random planes on odd ones (l2_dist is not masked: its gradient must reach them).  The m = 1 pair's rotation scores are all
    clamped (0.9975 / 0.0025), its translation scores are not (0.73 / 0.27).  Two hypotheses per launch receive no cotangent at all."""
    g = _g(11000 + nq + 1000 * SEED_STEP.get(("geometry", nq), 0))
    ms = case_ms(nq)
    B, NH = len(ms), nq + 1
    gl = torch.zeros(B, nq, 6)
    rots, trs = [], []
    for b, m in enumerate(ms):
        if m:
            a1, a2, perm, (t, q) = consistent_planes(m, m, m, g, noise=0.05)
            gl[b, :m] = torch.cat([a1, a2[perm]], -1)
        else:
            t, q = 0.4 * torch.randn(3, generator=g), rand_unit_quat(g)
        if b % 2 and m < nq:
            gl[b, m:] = torch.cat([rand_planes(nq - m, g), rand_planes(nq - m, g)], -1)
        r0 = F.normalize(q + 0.05 * torch.randn(4, generator=g), dim=0)
        rots.append(-r0 if r0[0] < 0 else r0)
        trs.append(t + 0.1 * torch.randn(3, generator=g))
    rot_raw = torch.randn(B, nq, 4, generator=g) * (0.2 + 2.0 * torch.rand(B, nq, 1, generator=g))
    rot_raw[0, 0] = 1e-20 * torch.randn(4, generator=g)
    if nq > 1:                                                 # (at nq = 1 the other hypothesis keeps the ordinary branch)
        rot_raw[B - 1, nq - 1] = 1e-20 * torch.randn(4, generator=g)
    r = lambda *s: torch.randn(*s, generator=g)
    c = {"nq": nq, "ms": ms, "m": torch.tensor(ms, dtype=torch.int32), "geo_local": gl, "init_rot": torch.stack(rots), "init_trans": torch.stack(trs),
         "rot_raw": rot_raw, "trans_raw": 0.5 * r(B, nq, 3),
         "sf_rot": r(B, NH, 64), "sf_trans": r(B, NH, 64), "reg_rot_w": r(64) / 4, "reg_rot_b": r(1), "reg_trans_w": r(64) / 4,
         "reg_trans_b": r(1), "init_rot_feat": F.relu(r(B, 256)), "init_trans_feat": F.relu(r(B, 256)), "fused_rot": F.relu(r(B, nq, 256)),
         "fused_trans": F.relu(r(B, nq, 256)), "rots_w": r(4, 256) / 16, "rots_b": r(4) / 4, "trans_w": r(3, 256) / 16, "trans_b": r(3) / 4}
    b1 = ms.index(1)
    for k, w, delta in (("sf_rot", "reg_rot_w", 6.0), ("sf_trans", "reg_trans_w", 1.0)):
        c[k][b1, 1] += (delta - ((c[k][b1, 1] - c[k][b1, 0]) * c[w]).sum()) * c[w] / (c[w] * c[w]).sum()       # raw score 1 = raw score 0 + delta
    for k in ("g_normal_score", "g_param_score", "g_l2_dist"):
        c[k] = _cot(g, B, NH, nq)
    c["no_cotangent"] = [(0, min(1, nq)), (B - 1, max(nq - 1, 0))] if nq > 1 else [(B - 1, 0)]      # (pair, hypothesis)
    for b, h in c["no_cotangent"]:
        for k in ("g_normal_score", "g_param_score", "g_l2_dist"):
            c[k][b, h] = 0.0
    for k, s in (("g_pred_rot", (B, 4)), ("g_pred_trans", (B, 3)), ("g_avg_rot", (B, 4)), ("g_avg_trans", (B, 3)), ("g_score_rot", (B, NH)),
                 ("g_score_trans", (B, NH))):
        c[k] = _cot(g, *s)
    return c


def _even_quat(g):
    """The target of the antipodal pair: four components of one magnitude, random signs.  At an antipodal estimate the gradient is zero by
    symmetry and all of the allowance is C_k; with components of one magnitude every draw of C_k turns the quaternion by about the same
    angle about every axis, so no element's allowance is small by the luck of eight draws."""
    return (0.5 + torch.rand(1, generator=g)) * torch.where(torch.rand(4, generator=g) < 0.5, -0.5, 0.5)


@functools.lru_cache(maxsize=None)
def loss_inputs(nq, B):
    """One launch of refine_losses_bwd_kernel: B pairs, m cycling through case_ms(nq); pair 1 is the empty one (B > 1), pair 2 has every
    estimate equal to its target (all-zero pose gradients), pair 3 an antipodal soft rotation; quaternions of norm != 1 on both sides;
    the score at the picked hypothesis is 1 / above 1 / below 1 in turn.  One entry of g_loss is exactly zero."""
    g = _g(13000 + 7 * nq + B + 1000 * SEED_STEP.get(("losses", (nq, B)), 0))
    NH = nq + 1
    live = [m for m in case_ms(nq) if m]
    m = torch.tensor([live[b % len(live)] for b in range(B)], dtype=torch.int32)
    if B > 1:
        m[1] = 0
    r = lambda *s: torch.randn(*s, generator=g)
    sc = lambda *s: 0.5 + 1.5 * torch.rand(*s, generator=g)
    gt = torch.cat([0.4 * r(B, 3), F.normalize(r(B, 4), dim=-1) * sc(B, 1)], -1)
    if B > 3:
        gt[3, 3:] = _even_quat(g)
    c = {"nq": nq, "B": B, "m": m, "gt_pose": gt, "weight": LOSS_WEIGHT}
    for k in ("pred", "avg"):
        c[k + "_trans"] = gt[:, :3] + 0.3 * r(B, 3)
        c[k + "_rot"] = F.normalize(F.normalize(gt[:, 3:], dim=-1) + 0.2 * r(B, 4), dim=-1) * (0.8 + 0.45 * torch.rand(B, 1, generator=g))
    if B > 2:
        for k in ("pred", "avg"):
            c[k + "_trans"][2], c[k + "_rot"][2] = gt[2, :3], gt[2, 3:]
    if B > 3:
        c["pred_rot"][3] = -1.1 * gt[3, 3:]
    c["rots_all"] = F.normalize(F.normalize(gt[:, None, 3:], dim=-1) + 0.5 * r(B, NH, 4), dim=-1)
    c["trans_all"] = gt[:, None, :3] + 0.5 * r(B, NH, 3)
    c["score_rot"], c["score_trans"] = 0.9 * torch.rand(B, NH, generator=g), 0.9 * torch.rand(B, NH, generator=g)
    c["l2_dist"] = 3.0 * torch.rand(B, NH, nq, generator=g)                    # (read by the forward only: the gradient does not depend on it)
    idx = torch.nonzero(m > 0)[:, 0]
    hr, ht, gap = index_picks(c["rots_all"][idx], c["trans_all"][idx], gt[idx], m[idx])
    for i, b in enumerate(idx.tolist()):
        c["score_rot"][b, hr[i]] = (1.0, 1.5, c["score_rot"][b, hr[i]])[b % 3]
        c["score_trans"][b, ht[i]] = (1.25, 1.0, c["score_trans"][b, ht[i]])[b % 3]
    c.update(live=idx, hr=hr, ht=ht, argmin_gap=gap)
    gl = (0.5 + 1.5 * torch.rand(7, generator=g)) * torch.tensor([(-1.0) ** (i + nq + B) for i in range(7)])            # signs alternate
    gl[(nq + B) % 7] = 0.0
    c["g_loss"] = gl
    return c


@functools.lru_cache(maxsize=None)
def pose_inputs(B, eps):
    """One launch of camera_pose_loss_bwd_kernel: the ground truth as the columns of one [B,7] tensor (`pose`: the test passes views of it, or
    dense copies); pair 2 has the estimate equal to the target, pair 3 an antipodal quaternion."""
    g = _g(15000 + B + (500 if eps else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    pose = torch.cat([0.4 * r(B, 3), F.normalize(r(B, 4), dim=-1) * (0.5 + 1.5 * torch.rand(B, 1, generator=g))], -1)
    if B > 3:
        pose[3, 3:] = _even_quat(g)
    c = {"B": B, "eps": eps, "weight": POSE_WEIGHT, "pose": pose, "gt_trans": pose[:, :3], "gt_rot": pose[:, 3:],
         "est_trans": pose[:, :3] + 0.3 * r(B, 3),
         "est_rot": F.normalize(F.normalize(pose[:, 3:], dim=-1) + 0.2 * r(B, 4), dim=-1) * (0.8 + 0.45 * torch.rand(B, 1, generator=g))}
    if B > 2:
        c["est_trans"][2], c["est_rot"][2] = pose[2, :3], pose[2, 3:]
    if B > 3:
        c["est_rot"][3] = -0.9 * pose[3, 3:]
    c["g_out"] = torch.tensor([-1.7, 0.6]) * (0.5 + torch.rand(2, generator=g))
    return c


def problem(family, key):
    """(x: every float input the reference reads, f32; aux; cotangents f32) of one case, restricted to the pairs the reference is defined
    for (m >= 1 for the vote and the loss kernels)."""
    fam = FAMILIES[family]
    if family == "score_maps":
        c = geometry_inputs(key)
        x, aux = {k: c[k] for k in fam["leaves"] + fam["consts"]}, {"m": c["m"].long()}
    elif family == "vote":
        c = geometry_inputs(key)
        n = len(c["ms"]) - 1                                   # the empty pair is the last one
        x = {k: (c[k][None].expand(n, *c[k].shape).contiguous() if k in VOTE_PARAMS else c[k][:n]) for k in fam["leaves"]}
        for k in VOTE_BIAS_PER_HYPOTHESIS:
            x[k] = x[k].expand(n, key + 1).contiguous()
        c = {k: (v[:n] if k in fam["cots"] else v) for k, v in c.items()}
        aux = {"m": c["m"][:n].long()}
    elif family == "losses":
        c = loss_inputs(*key)
        i = c["live"]
        x = {k: c[k][i] for k in fam["leaves"] + fam["consts"]}
        aux = {"m": c["m"][i].long(), "hr": c["hr"], "ht": c["ht"], "B": c["B"], "weight": c["weight"]}
    else:
        c = pose_inputs(*key)
        x = {k: c[k] for k in fam["leaves"]}
        aux = {"B": c["B"], "weight": c["weight"], "eps": float(torch.tensor(c["eps"], dtype=F32))}
    return x, aux, [c[k] for k in fam["cots"]]


# ===================================================================================================================== VJP, S, C, A
def vjp(family, x, aux, cots, dtype):
    """J^T g of the family's forward with torch.autograd in `dtype` -> {leaf: gradient} (zeros where nothing arrives)."""
    fam = FAMILIES[family]
    xs = {k: v.to(dtype).clone().requires_grad_(k in fam["leaves"]) for k, v in x.items()}
    outs = fam["fwd"](xs, aux)
    total = sum((o * g.to(dtype)).sum() for o, g in zip(outs, cots))
    grads = torch.autograd.grad(total, [xs[k] for k in fam["leaves"]], allow_unused=True)
    return {k: (torch.zeros_like(xs[k]) if g is None else g).detach() for k, g in zip(fam["leaves"], grads)}


def _accumulate(S, selected, weights, leaves):
    grads = torch.autograd.grad((selected * weights).sum(), leaves, retain_graph=True, allow_unused=True)
    for s, g in zip(S, grads):
        if g is not None:
            s += g.abs()


def term_magnitudes(family, x, aux, cots):
    """S_k = sum_i |g_i| |J_ik| in float64.  Every Jacobian here is block diagonal (a block: one pair; one hypothesis of one pair for the
    score maps), so one backward pass with |g| on output column i of EVERY block gives |g_i| J_ik of every block at once."""
    fam = FAMILIES[family]
    xs = {k: v.double().clone().requires_grad_(k in fam["leaves"]) for k, v in x.items()}
    leaves = [xs[k] for k in fam["leaves"]]
    S = [torch.zeros_like(v) for v in leaves]
    if family == "score_maps":                                  # column = (output, plane j): the forward of plane j alone, [B,NH,1]
        for j in range(x["rot_raw"].shape[1]):
            for o, g in zip(fam["fwd"](xs, aux, jsel=[j]), cots):
                _accumulate(S, o[..., 0], g[..., j].double().abs(), leaves)
    else:
        for o, g in zip(fam["fwd"](xs, aux), cots):
            g = g.double().abs()
            if o.dim() == 1:                                    # the losses: a sum over the pairs, one column per loss
                for i in range(o.shape[0]):
                    _accumulate(S, o[i], g[i], leaves)
            else:
                for i in range(o.shape[1]):
                    _accumulate(S, o[:, i], g[:, i], leaves)
    return dict(zip(fam["leaves"], (s.detach() for s in S)))


def jiggle(t, g):
    """t in float64 with every element multiplied by 1 + d, d = +- 2^-23 with signs drawn from the generator g."""
    return t.double() * (1 + EPS23 * (2.0 * torch.randint(0, 2, t.shape, generator=g).double() - 1))


def conditioning(family, x, aux, cots, ref):
    """C_k: the largest change of the float64 VJP over DRAWS draws that multiply every f32 input by 1 + d, |d| <= 2^-23."""
    g = _g(77)
    C = {k: torch.zeros_like(v) for k, v in ref.items()}
    jig = lambda t: jiggle(t, g)
    for _ in range(DRAWS):
        got = vjp(family, {k: jig(v) for k, v in x.items()}, dict(aux), [jig(t) for t in cots], F64)
        for k in C:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
    return C


@functools.lru_cache(maxsize=None)
def reference(family, key):
    """-> (ref, A): the float64 VJP and the allowance 2^-24 S + C per element, keyed by the kernel's output names.  The vote and the loss
    families cover the pairs with m >= 1, in launch order."""
    x, aux, cots = problem(family, key)
    ref = vjp(family, x, dict(aux), cots, F64)
    S = term_magnitudes(family, x, dict(aux), cots)
    C = conditioning(family, x, aux, cots, ref)
    fam = FAMILIES[family]
    names = dict(zip(fam["leaves"], fam["out"]))
    A = {k: EPS24 * S[k] + C[k] for k in ref}
    if family == "vote":
        for k in VOTE_BIAS_PER_HYPOTHESIS:
            ref[k], A[k] = ref[k].sum(1, keepdim=True), A[k].sum(1, keepdim=True)
    return {names[k]: v for k, v in ref.items()}, {names[k]: v for k, v in A.items()}


def ratios(got, ref, A):
    """error / A per element (0 where both are 0, inf where an error meets no allowance)."""
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / A)


def worst_ratio(family, key, got):
    """{output: (worst error / A, flat index)} of `got` (a dict over the kernel's output names, rows as reference(family, key))."""
    ref, A = reference(family, key)
    out = {}
    for k in ref:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        q = ratios(got[k], ref[k], A[k]).reshape(-1)
        out[k] = (float(q.max()), int(q.argmax())) if q.numel() else (0.0, -1)
    return out


def f32_restatement(family, key):
    fam = FAMILIES[family]
    x, aux, cots = problem(family, key)
    got = vjp(family, x, dict(aux), cots, F32)
    if family == "vote":
        for k in VOTE_BIAS_PER_HYPOTHESIS:
            got[k] = got[k].sum(1, keepdim=True)
    return dict(zip(fam["out"], (got[k] for k in fam["leaves"])))


def f32_worst(family):
    return max(q for key in family_keys(family) for q, _ in worst_ratio(family, key, f32_restatement(family, key)).values())


def print_f32_worst():
    for family in FAMILIES:
        print('"%s": %.3g,' % (family, f32_worst(family)))


# ===================================================================================================================== margins
def margins(family, key):
    """The decision margins of one case (see the constants above) as a dict of measured figures."""
    x, aux, _ = problem(family, key)
    xs = {k: v.double() for k, v in x.items()}
    if family == "score_maps":
        dl2 = score_maps_fwd(xs, aux)[2]
        nz = lambda d: float(d[d != 0].min()) if (d != 0).any() else float("inf")
        return {"dist": min(nz(dl2), nz(aux["dn"])), "zero_dl2": int((dl2 == 0).sum())}
    if family == "vote":
        vote_fwd(xs, aux)
        out = {"clamp": float("inf"), "all_clamped": 0, "none_clamped": 0, "above_0.9": 0}
        live = torch.arange(xs["sf_rot"].shape[1])[None] <= aux["m"][:, None]
        for p in aux["p"]:
            for b in range(p.shape[0]):
                pb = p[b][live[b]]
                out["clamp"] = min(out["clamp"], float(torch.minimum((pb - 0.01).abs() / 0.01, (pb - 0.9).abs() / 0.9).min()))
                inside = (pb >= 0.01) & (pb <= 0.9)
                out["all_clamped"] += int(not inside.any())
                out["none_clamped"] += int(inside.all())
                out["above_0.9"] += int((pb > 0.9).any())
        return out
    if family == "losses":
        c = loss_inputs(*key)
        i = torch.arange(len(c["live"]))
        d = torch.cat([(1 - c["score_rot"][c["live"]][i, c["hr"]]).abs(), (1 - c["score_trans"][c["live"]][i, c["ht"]]).abs()]).double()
        sr, st = c["score_rot"][c["live"]][i, c["hr"]], c["score_trans"][c["live"]][i, c["ht"]]
        return {"argmin": float(c["argmin_gap"].min()), "score": float(d[d != 0].min()) if (d != 0).any() else float("inf"),
                "sides": {int(torch.sign(v - 1)) for v in torch.cat([sr, st])}}
    return {}


# ===================================================================================================================== f32 emulation
PLANTS = {"score_maps": ("quat_factor_2", "dcdu_second_term", "l2_masked", "normalize_projection"),
          "vote": ("wavg_m_plus_1", "clamp_passes_outside", "renorm_dot", "normalize_projection"),
          "losses": ("index_sign", "diag_j_below_m", "inv_b_64", "normalize_projection"),
          "pose_loss": ("gt_sign", "eps_ignored")}


def _safe_div(a, b):
    return torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), torch.zeros_like(a))


def normalize_bwd(x, g, plant=None):
    """refine_bwd.hip normalize_bwd on the last dimension."""
    n = x.norm(dim=-1, keepdim=True)
    small = n < 1e-12
    ns = torch.where(small, torch.ones_like(n), n)
    dot = (g * x / ns).sum(-1, keepdim=True)
    if plant == "normalize_projection":
        dot = torch.zeros_like(dot)
    return torch.where(small, g / 1e-12, (g - dot * x / ns) / ns)


def _warp_bwd(u, nu, t, g, plant):
    nb = nu + 1e-5
    dot = ((u + t) * u).sum(-1, keepdim=True)
    c = dot / (nb * nb)
    gu_dot = (g * u).sum(-1, keepdim=True)
    dc = (2.0 * u + t) / (nb * nb)
    if plant != "dcdu_second_term":
        dc = dc - 2.0 * dot * u / (nb * nb * nb * torch.where(nu > 0, nu, torch.ones_like(nu)))
    ok = nu > 0
    return torch.where(ok, c * g + gu_dot * dc, torch.zeros_like(g)), torch.where(ok, gu_dot * u / (nb * nb), torch.zeros_like(g))


def emulate_score_maps(key, plant=None):
    c = geometry_inputs(key)
    gl, rr, m = c["geo_local"], c["rot_raw"], c["m"].long()
    B, nq = rr.shape[:2]
    q = torch.cat([c["init_rot"][:, None], rr / rr.norm(dim=-1, keepdim=True).clamp_min(1e-12)], 1)
    t = torch.cat([c["init_trans"][:, None], c["trans_raw"]], 1)[:, :, None, :]
    R = quat_to_rot(q)
    f, p1 = gl[..., :3] * _flip(gl), (gl[..., 3:] * _flip(gl))[:, None]
    u = torch.einsum("bhik,bjk->bhji", R, f)
    nu = u.norm(dim=-1, keepdim=True)
    nb = nu + 1e-5
    fwd = lambda tt: ((u + tt) * u).sum(-1, keepdim=True) / (nb * nb) * u
    z = torch.zeros_like(t)
    w_r, w_rt = fwd(z), fwd(t)
    mask = ((torch.arange(nq + 1)[None, :, None] <= m[:, None, None]) & (torch.arange(nq)[None, None, :] < m[:, None, None])).float()[..., None]
    g_ns, g_ps, g_l2 = c["g_normal_score"][..., None] * mask, c["g_param_score"][..., None] * mask, c["g_l2_dist"][..., None]
    if plant == "l2_masked":
        g_l2 = g_l2 * mask
    nw = w_r.norm(dim=-1, keepdim=True)
    n0, n1v = w_r / nw.clamp_min(1e-12), p1 / p1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    d = n0 - n1v
    dn = d.norm(dim=-1, keepdim=True)
    gn0 = _safe_div(-torch.exp(-dn) * g_ns * d, dn.expand_as(d))
    dt = (gn0 * n0).sum(-1, keepdim=True)
    gw = torch.where(nw >= 1e-12, (gn0 - dt * n0) / nw.clamp_min(1e-12), torch.zeros_like(gn0))
    gu1, _ = _warp_bwd(u, nu, z, gw, plant)
    e = w_rt - p1
    dl2 = e.norm(dim=-1, keepdim=True)
    gw2 = _safe_div((-torch.exp(-dl2) * g_ps + g_l2) * e, dl2.expand_as(e))
    gu2, gt2 = _warp_bwd(u, nu, t, gw2, plant)
    G = torch.einsum("bhji,bjk->bhik", gu1 + gu2, f).reshape(B, nq + 1, 9).unbind(-1)
    gt_ = gt2.sum(2)
    w, x, y, zz = q.unbind(-1)
    k4 = 1.0 if plant == "quat_factor_2" else 2.0
    gq = torch.stack([2.0 * (-zz * G[1] + y * G[2] + zz * G[3] - x * G[5] - y * G[6] + x * G[7]),
                      2.0 * (y * G[1] + zz * G[2] + y * G[3] - k4 * x * G[4] - w * G[5] + zz * G[6] + w * G[7] - 2.0 * x * G[8]),
                      2.0 * (-2.0 * y * G[0] + x * G[1] + w * G[2] + x * G[3] + zz * G[5] - w * G[6] + zz * G[7] - 2.0 * y * G[8]),
                      2.0 * (-2.0 * zz * G[0] - w * G[1] + x * G[2] + w * G[3] - 2.0 * zz * G[4] + y * G[5] + x * G[6] + y * G[7])], -1)
    return {"g_rot_raw": normalize_bwd(rr, gq[:, 1:], plant), "g_trans_raw": gt_[:, 1:], "g_init_rot": gq[:, 0], "g_init_trans": gt_[:, 0]}


def emulate_vote(key, plant=None):
    c = geometry_inputs(key)
    n, nq = len(c["ms"]) - 1, c["nq"]
    m = c["m"][:n].long()
    live = torch.arange(nq + 1)[None] <= m[:, None]
    lf = live.float()
    pm = (torch.arange(nq)[None] < m[:, None]).float()[:, :, None]
    wavg = (1.0 / (m.float() + (1.0 if plant == "wavg_m_plus_1" else 0.0)))[:, None]
    out = {}
    for kind, head_w, head_b, gp_k, ga_k in (("rot", "rots_w", "rots_b", "g_pred_rot", "g_avg_rot"), ("trans", "trans_w", "trans_b", "g_pred_trans", "g_avg_trans")):
        sf, w, bias = c["sf_" + kind][:n], c["reg_%s_w" % kind], c["reg_%s_b" % kind]
        f0, FF, W, bb = c["init_%s_feat" % kind][:n], c["fused_" + kind][:n], c[head_w], c[head_b]
        p = torch.softmax((sf @ w + bias).masked_fill(~live, float("-inf")), 1)
        s0 = p.clamp(0.01, 0.9) * lf
        cs = s0.sum(1, keepdim=True)
        s = s0 / (cs + 1e-10)
        f_soft = f0 * s[:, 0:1] + (FF * s[:, 1:, None]).sum(1)
        f_avg = (FF * pm).sum(1) * wavg
        gh_a, gh_s = c[ga_k][:n], c[gp_k][:n]
        if kind == "rot":
            gh_a, gh_s = normalize_bwd(f_avg @ W.T + bb, gh_a, plant), normalize_bwd(f_soft @ W.T + bb, gh_s, plant)
        out["pb_%s_b" % head_w[:-2]] = gh_a + gh_s
        out["pb_" + head_w] = gh_a[:, :, None] * f_avg[:, None, :] + gh_s[:, :, None] * f_soft[:, None, :]
        g_avg, g_soft = gh_a @ W, gh_s @ W
        out["g_init_%s_feat" % kind] = s[:, 0:1] * g_soft
        out["g_fused_" + kind] = (s[:, 1:, None] * g_soft[:, None, :] + wavg[:, :, None] * g_avg[:, None, :]) * pm
        gs = ((torch.cat([f0[:, None], FF], 1) * g_soft[:, None, :]).sum(-1) + c["g_score_" + kind][:n]) * lf
        dot = torch.zeros_like(cs) if plant == "renorm_dot" else (gs * s).sum(1, keepdim=True)
        gc = (gs - dot) / (cs + 1e-10)
        inside = ((p >= 0.01) & (p <= 0.9)) | (plant == "clamp_passes_outside")
        gp = torch.where(inside & live, gc, torch.zeros_like(gc))
        gr = p * (gp - (gp * p).sum(1, keepdim=True)) * lf
        out["pb_reg_%s_b" % kind] = gr.sum(1, keepdim=True)
        out["g_sf_" + kind] = gr[:, :, None] * w
        out["pb_reg_%s_w" % kind] = (gr[:, :, None] * sf).sum(1)
    return out


def _pose_terms(t, q, gt_t, gt_q, gl_t, gl_q, k, plant):
    """d (gl_t k |t - gt_t| + gl_q k |n(gt_q) - n(q)|) / d (t, q, and the n(q)-side gradient before the normalisation)."""
    e = t - gt_t
    g_t = _safe_div(gl_t * k * e, e.norm(dim=-1, keepdim=True).expand_as(e))
    d = unit(q) - unit(gt_q)
    gy = _safe_div(gl_q * k * d, d.norm(dim=-1, keepdim=True).expand_as(d))
    return g_t, normalize_bwd(q, gy, plant), gy


def emulate_losses(key, plant=None):
    c = loss_inputs(*key)
    i, nq, B = c["live"], c["nq"], c["B"]
    m, gt, gl = c["m"][i].long(), c["gt_pose"][i], c["g_loss"]
    k = torch.tensor(c["weight"], dtype=F32) * (1.0 / (64.0 if plant == "inv_b_64" else float(B)))
    out = {}
    out["g_avg_trans"], out["g_avg_rot"], _ = _pose_terms(c["avg_trans"][i], c["avg_rot"][i], gt[:, :3], gt[:, 3:], gl[0], gl[1], k, plant)
    out["g_pred_trans"], out["g_pred_rot"], _ = _pose_terms(c["pred_trans"][i], c["pred_rot"][i], gt[:, :3], gt[:, 3:], gl[2], gl[3], k, plant)
    rows = torch.arange(len(i))
    sign = 1.0 if plant == "index_sign" else -1.0
    for kind, pick, gli, scale in (("rot", c["hr"], 4, 0.01), ("trans", c["ht"], 5, 0.02)):
        gs = torch.zeros(len(i), nq + 1)
        gs[rows, pick] = gl[gli] * scale * k * sign * torch.sign(1.0 - c["score_" + kind][i][rows, pick])
        out["g_score_" + kind] = gs
    g_l2 = torch.zeros(len(i), nq + 1, nq)
    gd = (gl[6] * 0.1 * k / m.float())[:, None].expand(-1, nq)
    if plant == "diag_j_below_m":
        gd = gd * (torch.arange(nq)[None] < m[:, None]).float()
    g_l2[:, torch.arange(1, nq + 1), torch.arange(nq)] = gd
    out["g_l2_dist"] = g_l2
    return out


def emulate_pose_loss(key, plant=None):
    c = pose_inputs(*key)
    eps = torch.tensor(0.0 if plant == "eps_ignored" else c["eps"], dtype=F32)
    k = torch.tensor(c["weight"], dtype=F32) / float(c["B"])
    g_t, g_q, gy = _pose_terms(c["est_trans"], c["est_rot"], c["gt_trans"] + eps, c["gt_rot"], c["g_out"][0], c["g_out"][1], k, None)
    side = 1.0 if plant == "gt_sign" else -1.0
    return {"g_est_trans": g_t, "g_est_rot": g_q, "g_gt_trans": side * g_t, "g_gt_rot": normalize_bwd(c["gt_rot"], side * gy)}


EMULATE = {"score_maps": emulate_score_maps, "vote": emulate_vote, "losses": emulate_losses, "pose_loss": emulate_pose_loss}
