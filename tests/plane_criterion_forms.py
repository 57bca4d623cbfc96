"""The plane head's set criterion (csrc/plane_criterion.hip) as data: seeded cases that reach every chunk / band / wave path of its
kernels, inputs whose decisions are not marginal, the float64 restatement tests/plane_criterion_ref.py evaluated on the f32 values the
kernels read with the test's own match, a per-element allowance A_k = 2^-24 S_k + C_k for every element of every output, the float32
restatement the limits are measured from, a numpy emulation of the assignment, and a float32 emulation of the kernels' documented
order of operations in which errors can be planted.  tests/test_plane_criterion_forms_gpu.py holds the kernels to
it, tests/test_plane_criterion_forms_cpu.py proves inputs, constants, references and the sharpness of the bound.  Imports without a GPU.

  S_k     the float64 magnitudes of the terms that make element k (see magnitudes(), and docs/kernels.md for the three rules it adds)
  C_k     conditioning: the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input (cotangents
          included) by 1 +- 2^-23
  limit   LIMIT_FACTOR x the worst error / A of the float32 restatement over the cases, per output family (F32_WORST, measured on the
          CPU; never measured from a kernel)
"""
from __future__ import annotations

import collections
import functools
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from tests import plane_criterion_ref as R
from tests.refine_bwd_forms import DRAWS, EPS24, LIMIT_FACTOR, jiggle, ratios

F32, F64 = torch.float32, torch.float64
WTS = dict(R.DEFAULT_WEIGHTS)
EOS_F32 = float(torch.tensor(WTS["eos_coef"], dtype=torch.float32))           # the weight as the kernels and the restatement hold it
CHUNK, COST_BLOCKS, BAND, QCHUNKS = 64, 16, 8, 16          # PC_CHUNK, PC_COST_BLOCKS, PC_BAND, PC_QCHUNKS of the kernels
TINY = 2.0 ** -126                                          # float32's least normal number: below it no float32 program keeps a relative error (p^3 at a logit of -30)
GUARD = 64                                                  # elements behind every output that must stay untouched

# decision margins (asserted for every case in float64 and in float32 by the CPU half; a seed that breaks one is stepped in SEED_STEP)
GD_MARGIN = 1e-4             # |gd - 0.2| of every covered pixel (the threshold of q_valid)
RES_MARGIN = 1e-5            # |p' . X - 1| on a valid pixel of a matched plane
DIFF_MARGIN = 1e-4           # |p[e] - t[e]| of a matched pair: exactly 0 or at least this
NORM_MARGIN = 0.1            # |p|, |t|
DIST_MARGIN = 1e-3           # centre distances: exactly 0 or above this
# case name -> seed step where the first seeds break an input condition (mostly a gd within 1e-4 of 0.2 among thousands of pixels)
SEED_STEP = {"cost_8x8_s4": 1, "cost_25x41_s2": 1, "mask_2x2_s8": 1, "mask_2x5_s8": 1, "mask_7x2_s4": 1, "mask_7x13_s4": 1,
             "mask_7x13_s8": 2, "mask_8x8_s4": 1, "mask_8x8_s8": 3, "mask_8x13_s3": 1, "mask_8x13_s8": 1, "mask_9x13_s2": 1,
             "mask_9x13_s8": 4, "mask_16x8_s3": 1, "mask_16x8_s4": 2, "mask_16x8_s8": 1, "mask_16x13_s1": 1, "mask_16x13_s5": 1,
             "mask_16x13_s8": 4, "mask_17x5_s5": 1, "mask_17x5_s8": 1, "mask_17x8_s8": 2, "mask_17x13_s5": 4, "mask_17x13_s8": 11,
             "mask_9x160_s4": 2}

OUT_FLOAT = ("cost", "losses", "mask_stats", "q_stats")
GRADS = ("d_logits", "d_mask_logits", "d_centers", "d_params", "d_pixel_centers")

# worst error / A of the float32 restatement over every case of the lists below, per output family.  Printed by
#   python -c "from tests import plane_criterion_forms as P; P.print_f32_worst()"
# and re-measured by tests/test_plane_criterion_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"cost": 7.25, "losses": 5.15, "mask_stats": 4.1, "q_stats": 1.29, "d_logits": 1.99, "d_mask_logits": 7.81, "d_centers": 0.681,
             "d_params": 2.44, "d_pixel_centers": 4.46}


def limit(family):
    return LIMIT_FACTOR * F32_WORST[family]


# ===================================================================================================================== cases
Case = collections.namedtuple("Case", "name L B nq h w s n nmax match pixel num_masks no_valid seed")


def _c(name, L, B, nq, h, w, s, n, nmax, match, pixel=True, num_masks=0.0, no_valid=(), seed=0):
    return Case(name, L, B, nq, h, w, s, tuple(n), nmax, match, pixel, num_masks, tuple(no_valid), seed)


def _cost_cases():
    """The cost kernel's h x w table at s = 1, 2 (4 on the first three), with every nq, n, nmax and (L, B) of the issue spread over it."""
    rows = [  # h, w, s, L, B, nq, n, nmax, match, num_masks, no_valid
        (6, 8, 1, 1, 1, 1, [1], 1, "identity", 0.0, []),
        (6, 8, 2, 3, 2, 2, [2, 1], 3, "reversed", 2.5, [1]),
        (6, 8, 4, 2, 3, 3, [1, 3, 2], 3, "perlayer", 0.0, [2]),
        (8, 8, 1, 8, 1, 4, [4], 50, "identity", 0.0, []),
        (8, 8, 2, 1, 1, 5, [5], 5, "reversed", 2.5, []),
        (8, 8, 4, 3, 2, 63, [50, 1], 50, "perlayer", 0.0, [0]),
        (5, 13, 1, 2, 3, 64, [1, 50, 7], 50, "reversed", 0.0, []),
        (5, 13, 2, 1, 1, 65, [50], 50, "high", 0.0, []),
        (5, 13, 4, 3, 2, 100, [50, 3], 50, "high", 2.5, []),
        (32, 32, 1, 2, 3, 128, [1, 50, 20], 50, "high", 0.0, [1]),
        (32, 32, 2, 1, 1, 100, [12], 13, "perlayer", 0.0, []),
        (25, 41, 1, 3, 2, 5, [5, 2], 6, "identity", 0.0, []),
        (25, 41, 2, 1, 1, 128, [50], 50, "reversed", 0.0, []),
        (46, 46, 1, 2, 3, 3, [3, 1, 2], 3, "perlayer", 2.5, []),
        (46, 46, 2, 1, 1, 64, [7], 8, "perlayer", 0.0, []),
    ]
    out = []
    for k, (h, w, s, L, B, nq, n, nmax, match, nm, nv) in enumerate(rows):
        out.append(_c("cost_%dx%d_s%d" % (h, w, s), L, B, nq, h, w, s, n, nmax, match, pixel=k % 3 != 2, num_masks=nm, no_valid=nv, seed=100 + k))
    return out


MASK_HS, MASK_WS, MASK_SS = (1, 2, 7, 8, 9, 16, 17), (1, 2, 5, 8, 13), (1, 2, 3, 4, 5, 8)
MATCHES = ("identity", "reversed", "perlayer", "high")


def _mask_cases():
    """The band kernels' sweep: every h x w x s, two layers of two images, six planes (the whole image, a stripe across every band seam, a
    one-pixel plane on each corner) and two; with and without the centre map, the default num_masks and the override, every match."""
    out, k = [], 0
    for hi, h in enumerate(MASK_HS):
        for wi, w in enumerate(MASK_WS):
            for si, s in enumerate(MASK_SS):                                    # every flag from its own mix of the three indices, so that none follows s, h or w
                m = hi * len(MASK_WS) + wi
                out.append(_c("mask_%dx%d_s%d" % (h, w, s), 2, 2, 8, h, w, s, [6, 2], 7 if (m + si) % 2 else 6, MATCHES[(m + si) % 4],
                              pixel=(hi + wi + si) % 3 != 1, num_masks=2.5 if (m + 2 * si) % 5 == 2 else 0.0,
                              no_valid=[1] if (m + 3 * si) % 7 == 3 else [], seed=1000 + k))
                k += 1
    out.append(_c("mask_9x160_s4", 1, 3, 8, 9, 160, 4, [6, 1, 3], 6, "perlayer", no_valid=[2], seed=2000))          # H W = 36 x 640
    return out


def _q_cases():
    """The Q loss by H W: 48 is cost_6x8_s1, 36 x 640 is mask_9x160_s4; 4096 = one pass per chunk group, 4097 = one pixel into a second."""
    return [_c("q_4096", 1, 3, 4, 16, 16, 4, [3, 1, 2], 3, "reversed", no_valid=[2], seed=3000),
            _c("q_4097", 2, 3, 4, 17, 241, 1, [3, 1, 2], 4, "identity", no_valid=[2], seed=3001)]


COST_CASES, MASK_CASES, Q_CASES = _cost_cases(), _mask_cases(), _q_cases()
CASES = {c.name: c for c in COST_CASES + MASK_CASES + Q_CASES}
PADDED = ("cost_6x8_s4", "mask_9x13_s3")                      # the cases that also run with the query / channel stride padded by 3
CHAIN = ("cost_6x8_s2", "cost_5x13_s4", "cost_32x32_s1", "mask_17x13_s3")      # costs -> assign -> losses -> backward on the kernel's own match


def chunk_walk(case):
    """chunks per workgroup of pc_cost_partial_kernel, live lanes of the last chunk"""
    hw = case.h * case.w
    nchunks = -(-hw // CHUNK)
    nblk = min(nchunks, COST_BLOCKS)
    return [len(range(b, nchunks, nblk)) for b in range(nblk)], hw - (nchunks - 1) * CHUNK


def bands(case):
    """(bands of the mask / centre-map kernels, rows of the last one)"""
    nb = -(-case.h // BAND)
    return nb, case.h - (nb - 1) * BAND


# ===================================================================================================================== inputs
def _plane_mask(j, H, W, g):
    m = torch.zeros(H, W, dtype=torch.uint8)
    if j == 0:
        m[:] = 1                                                                # the whole image
    elif j == 1:
        x0 = W // 3
        m[:, x0:max(x0 + 1, (2 * W) // 3)] = 1                                  # a stripe across every band seam
    elif j <= 5:
        y, x = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))[j - 2]          # one pixel on a corner; odd coordinates at s >= 2
        m[y, x] = 1
    else:
        y0, x0 = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        y1, x1 = int(torch.randint(y0 + 1, H + 1, (1,), generator=g)), int(torch.randint(x0 + 1, W + 1, (1,), generator=g))
        m[y0:y1, x0:x1] = 1
    return m


def make_match(case, g):
    """An injective match of every target, chosen by the test (not the optimum): match_q [L B, nmax] and its inverse match_gt [L B, nq]"""
    LB = case.L * case.B
    mq = torch.full((LB, case.nmax), -1, dtype=torch.int32)
    for i in range(LB):
        n = case.n[i % case.B]
        j = torch.arange(n)
        kind = case.match if case.match != "perlayer" else ("perm", "identity", "reversed", "high")[(i // case.B) % 4] if case.L > 1 else "perm"
        if kind == "identity":
            q = j
        elif kind == "reversed":
            q = case.nq - 1 - j                                                 # includes the last query
        elif kind == "high":
            q = case.nq - n + j                                                 # the top n queries: lane column 1 where nq - n >= 64
        else:
            q = torch.randperm(case.nq, generator=g)[:n]
        mq[i, :n] = q.to(torch.int32)
    return mq, invert_match(mq, case)


def invert_match(mq, case):
    mg = torch.full((mq.shape[0], case.nq), -1, dtype=torch.int32)
    for i in range(mq.shape[0]):
        n = case.n[i % case.B]
        mg[i, mq[i, :n].long()] = torch.arange(n, dtype=torch.int32)
    return mg


def cotangents(case, g):
    """g_losses of the backward launches: one random (a negative entry, a zero entry), then single entries so that each gradient path is
    judged alone: (ce, mask, center_ins, param_l1, center_pixel), (dice, param_cos), (q)"""
    L, n = case.L, 6 * case.L + 2
    g0 = (0.3 + 2.7 * torch.rand(1, generator=g)) * torch.randn(n, generator=g)
    g0[0], g0[3] = -g0[0].abs() - 0.1, 0.0
    one = lambda: float(0.5 + torch.rand(1, generator=g)) * (1.0 if float(torch.rand(1, generator=g)) < 0.5 else -1.0)
    gs = [g0] + [torch.zeros(n) for _ in range(3)]
    for k, (launch, fam) in enumerate(((1, 0), (1, 1), (1, 3), (1, 4), (2, 2), (2, 5))):
        gs[launch][6 * (k % L) + fam] = one()
    gs[1][6 * L] = one()
    gs[3][6 * L + 1] = one()
    return [t.to(F32) for t in gs]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Every tensor the kernels read, as float32 / uint8 / int32 on the CPU, pixel-minor."""
    case = CASES[name]
    g = torch.Generator().manual_seed(case.seed + 100000 * SEED_STEP.get(name, 0))
    L, B, nq, h, w, s, nmax = case.L, case.B, case.nq, case.h, case.w, case.s, case.nmax
    H, W, LB = s * h, s * w, L * B
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=F64)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    z = torch.tensor([0.0, 0.0, 1.0], dtype=F64)
    x = {"logits": rn(LB, nq, 2), "mlog": 2.0 * rn(LB, nq, h, w), "centers": r(LB, nq, 2),
         "params": F.normalize(rn(LB, nq, 3) * 0.4 + z, dim=-1) * (1.0 + 2.0 * r(LB, nq, 1)), "pixc": r(B, 2, h, w)}
    sat = r(LB, nq, h, w)
    x["mlog"] = torch.where(sat < 0.03, torch.full_like(sat, 30.0), torch.where(sat > 0.97, torch.full_like(sat, -30.0), x["mlog"]))
    masks = torch.zeros(B, nmax, H, W, dtype=torch.uint8)
    tparams = torch.zeros(B, nmax, 3, dtype=F64)
    depth = torch.ones(B, H, W, dtype=F64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    kinv = torch.stack([xs / W - 0.5, ys / H - 0.5, torch.ones_like(xs)])[None].repeat(B, 1, 1, 1)
    for b in range(B):
        for j in range(case.n[b]):
            masks[b, j] = _plane_mask(j, H, W, g)
        nrm = F.normalize(torch.cat([0.3 * rn(case.n[b], 2), torch.ones(case.n[b], 1, dtype=F64)], 1), dim=-1)
        off = 1.0 + 2.0 * r(case.n[b], 1)
        tparams[b, :case.n[b]] = nrm * off
        inv = ((nrm[0] / off[0])[:, None, None] * kinv[b]).sum(0)                # g' . k_inv_dot_xy1 of plane 0, the whole image
        assert float(inv.min()) > 0
        mag, far = 0.001 + 0.149 * r(H, W), r(H, W) < (0.3 if case.n[b] > 1 else 0.0)       # within +-15 %, or beyond +-25 % (not where n = 1: all valid)
        noise = torch.where(far, 0.25 + 0.15 * r(H, W) + 0.01, mag) * torch.where(r(H, W) < 0.5, -1.0, 1.0)
        depth[b] = (1.0 / inv) * (1.0 + noise) * (3.0 if b in case.no_valid else 1.0)
    tcenters, tpixel = R.prepare_targets(masks, list(case.n), F64)
    x.update(tparams=tparams, tcenters=tcenters, tpixel=tpixel, depth=depth, kinv=kinv)
    x = {k: v.to(F32) for k, v in x.items()}
    mq, mg = make_match(case, g)
    tied = {"params": [], "centers": []}                                         # (image, query, batch element, target) set equal on purpose
    for i in sorted({0, LB - 1}):                                                # the first image of the last layer and the last image
        b, n = i % B, case.n[i % B]
        q = mq[i].long()
        x["params"][i, q[0]] = x["tparams"][b, 0]                                # a prediction that equals its target
        tied["params"].append((i, int(q[0]), b, 0))
        if n >= 3:
            tied["centers"].append((i, int(q[2]), b, 2))
        if n >= 2:
            x["params"][i, q[1]] = 2.0 * x["tparams"][b, 1]                      # parallel: |cos| clamped at 0.999999 in the cost
        if n >= 3:
            x["centers"][i, q[2]] = x["tcenters"][b, 2]                          # distance exactly 0
        if n >= 4:
            x["centers"][i, q[3]] = x["tcenters"][b, 3] + 1.5e-3                 # a predicted centre next to its target
    x["pixc"][0, :, :2, :2] = 0.5                                                # the four taps of high-resolution pixel (0, 0) equal its
    x["tpixel"][0, :, 0, 0] = 0.5                                                # target: a distance of exactly 0 in the centre-map loss
    x.update(masks=masks, match_q=mq, match_gt=mg, gs=cotangents(case, g), tied=tied)
    return x


# ===================================================================================================================== restatement
LEAVES = ("logits", "mlog", "centers", "params", "pixc")
FLOAT_INPUTS = LEAVES + ("tparams", "tcenters", "tpixel", "depth", "kinv")
LEAF_GRAD = dict(zip(LEAVES, GRADS))


def _indices(mq, case):
    return [[(mq[l * case.B + b, :case.n[b]].long(), torch.arange(case.n[b])) for b in range(case.B)] for l in range(case.L)]


def loss_vector(losses, L, dtype):
    """The restatement's dict in the kernel's order [6 L + 2]"""
    zero = torch.zeros((), dtype=dtype)
    v = [losses[k + ("" if l == 0 else "_%d" % (l - 1))] for l in range(L) for k in R.LOSS_NAMES]
    return torch.stack(v + [losses.get("loss_center_pixel", zero), losses["loss_q"]])


def _focal_terms(sm, tm):
    p = sm.sigmoid()
    ce = F.binary_cross_entropy_with_logits(sm, tm, reduction="none")
    pt = p * tm + (1 - p) * (1 - tm)
    return p, (0.25 * tm + 0.75 * (1 - tm)) * ce * (1 - pt) ** 2


def stats(t, case, mq):
    """What the loss entry keeps for its backward: mask_stats [L B, nmax, 4] = (focal sum, sum sigmoid t, sum sigmoid, sum t) of each
    matched mask, q_valid [B, H, W], q_stats [B, 2] = (sum, count); and sum |X| over the valid pixels of each mask [B, nmax, 3]"""
    dtype = t["mlog"].dtype
    L, B, nmax = case.L, case.B, case.nmax
    H, W = t["masks"].shape[-2:]
    ms = torch.zeros(L * B, nmax, 4, dtype=dtype)
    for i in range(L * B):
        b, n = i % B, case.n[i % B]
        sm = F.interpolate(t["mlog"][i, mq[i, :n].long()][:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].flatten(1)
        tm = t["masks"][b, :n].to(dtype).flatten(1)
        p, fo = _focal_terms(sm, tm)
        ms[i, :n] = torch.stack([fo.sum(1), (p * tm).sum(1), p.sum(1), tm.sum(1)], 1)
    valid = torch.zeros(B, H, W, dtype=torch.uint8)
    qs = torch.zeros(B, 2, dtype=dtype)
    absx = torch.zeros(B, nmax, 3, dtype=dtype)
    gds, res, flips = [], [], 0
    for b in range(B):
        n = case.n[b]
        pts = (t["kinv"][b] * t["depth"][b][None]).reshape(3, -1)
        gm = (t["masks"][b, :n] > 0).to(dtype).flatten(1)
        gp = t["tparams"][b, :n]
        go = gp.norm(dim=-1, keepdim=True)
        gd = (torch.abs((gp / go / go) @ pts - 1.0) * gm).sum(0)
        ok = (gd < 0.2) & (gm.sum(0) > 0)
        pp = t["params"][b][mq[b, :n].long()]
        po = pp.norm(dim=-1, keepdim=True)
        rs = (pp / po / po) @ pts - 1.0
        d = (torch.abs(rs) * gm).sum(0)
        valid[b] = ok.reshape(H, W).to(torch.uint8)
        qs[b, 0], qs[b, 1] = d[ok].sum(), ok.sum()
        absx[b, :n] = (gm * ok.to(dtype)[None]) @ pts.abs().T
        gds.append(gd[gm.sum(0) > 0])
        flips += int((((d < 0.2) & (gm.sum(0) > 0)) != ok).sum())
        res.append(rs[(gm > 0) & ok[None]])
    return dict(mask_stats=ms, q_valid=valid, q_stats=qs, absx=absx, gd=torch.cat(gds), res=torch.cat(res), flips=flips)


def evaluate(x, case, dtype, gs=None):
    """The restatement in `dtype` on the values of x with x's match -> every output of the cost, loss and gradient entries (gradients: one
    dict per cotangent vector of gs)."""
    L, B, nq, nmax = case.L, case.B, case.nq, case.nmax
    t = {k: x[k].to(dtype) for k in FLOAT_INPUTS}
    leaves = {k: t[k].clone().requires_grad_(True) for k in LEAVES}

    def layer(l):
        o = {"pred_logits": leaves["logits"][l * B:(l + 1) * B], "pred_mask_logits": leaves["mlog"][l * B:(l + 1) * B],
             "pred_centers": leaves["centers"][l * B:(l + 1) * B], "pred_params": leaves["params"][l * B:(l + 1) * B]}
        if l == 0 and case.pixel:
            o["pixel_centers"] = leaves["pixc"]
        return o
    outputs = layer(0)
    if L > 1:
        outputs["aux_outputs"] = [layer(l) for l in range(1, L)]
    targets = {"masks": x["masks"], "n": list(case.n), "plane_params": t["tparams"], "depth": t["depth"], "k_inv_dot_xy1": t["kinv"]}
    losses, _, costs = R.criterion(outputs, targets, WTS, indices=_indices(x["match_q"], case), num_masks=case.num_masks or None,
                                   prepared=(t["tcenters"], t["tpixel"]))
    vec = loss_vector(losses, L, dtype)
    cost = torch.zeros(L * B, nq, nmax, dtype=dtype)
    for l in range(L):
        for b in range(B):
            cost[l * B + b, :, :case.n[b]] = costs[l][b].detach()
    out = dict(cost=cost, losses=vec.detach())
    with torch.no_grad():
        t["masks"] = x["masks"]
        st = stats(t, case, x["match_q"])
    out.update(mask_stats=st["mask_stats"], q_stats=st["q_stats"], q_valid=st["q_valid"], gd=st["gd"], res=st["res"], absx=st["absx"])
    out["grads"] = []
    for g in ([] if gs is None else gs):
        gr = torch.autograd.grad((vec * g.to(dtype)).sum(), [leaves[k] for k in LEAVES], retain_graph=True, allow_unused=True)
        out["grads"].append({LEAF_GRAD[k]: (torch.zeros_like(leaves[k]) if v is None else v.detach()) for k, v in zip(LEAVES, gr)})
    return out


def _one_minus_magnitude(v, p):
    """The magnitude of the terms of 1 - sigmoid(v) as float32 code forms it: at v >= 0 it is the difference of 1 and a rounded p >= 1/2
    (absolute error 2^-24 however small the result: terms 1 and p), below 0 it is accurate to its own size."""
    return torch.where(v >= 0, 1 + p, 1 - p)


def _focal_magnitudes(sm, tm):
    """per pixel: sigmoid, the focal summand and the focal derivative with every 1 - sigmoid taken at _one_minus_magnitude"""
    p = sm.sigmoid()
    qm, sp0, sp1 = _one_minus_magnitude(sm, p), F.softplus(sm), F.softplus(-sm)
    fo = torch.where(tm > 0, 0.25 * qm ** 2 * sp1, 0.75 * p ** 2 * sp0)
    # the derivative: the modulating factor 1 - pt is formed by subtraction from a rounded pt on either side (the restatement forms
    # pt = p t + (1 - p) (1 - t) and then 1 - pt): its terms are 1 and pt
    mt, mf = 1 + p, 2 - p
    dfo = torch.where(tm > 0, 0.25 * (2 * mt * p * qm * sp1 + mt ** 2 * qm), 0.75 * (2 * mf * p * qm * sp0 + mf ** 2 * p))
    return p, fo, dfo


def _tap_tables(lo, hi, s):
    """Of one axis, [lo, hi] each: the float64 tap weights of F.interpolate(bilinear, align_corners=False); the indicator of the
    high-resolution indices whose source coordinate lies within 1 of the low-resolution index (the taps a rounded coordinate can
    reach) times the rounding of that coordinate in float32 - (dst + 0.5) * fl(1 / s) - 0.5 is exact where s is a power of two,
    elsewhere it is off by up to 2^-23 (src + 1)"""
    src = ((torch.arange(hi, dtype=F64) + 0.5) / s - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=lo - 1)
    i1 = (i0 + 1).clamp(max=lo - 1)
    wt = torch.zeros(lo, hi, dtype=F64)
    r = torch.arange(hi)
    wt[i0, r] += 1 - (src - i0)
    wt[i1, r] += src - i0
    near = ((src[None] - torch.arange(lo, dtype=F64)[:, None]).abs() <= 1).double()
    return wt, near * (torch.zeros_like(src) if s & (s - 1) == 0 else 2.0 ** -23 * (src + 1))[None]


def _tap_rounding(cot, case):
    """What the rounding of the bilinear source coordinate can move into a low-resolution pixel: the error of the tap weight along one
    axis times the true weight along the other, e_y w_x + w_y e_x, applied to |cotangent| [n, H, W].  Zero at s = 1, 2, 4, 8.  At s = 3, 5
    a coordinate that is an integer in exact arithmetic lands 1e-7 beside it, and a tap of weight exactly 0 gets 1e-7: against the
    gradient of a pixel whose own dependants are saturated that is its whole value."""
    wy, ey = _tap_tables(case.h, cot.shape[-2], case.s)
    wx, ex = _tap_tables(case.w, cot.shape[-1], case.s)
    return torch.einsum("yY,nYX,xX->nyx", ey, cot, wx) + torch.einsum("yY,nYX,xX->nyx", wy, cot, ex)


def magnitudes(x, case, ev):
    """S_k in float64 (ev = evaluate(x, case, F64)): the cost's seven weighted terms (dice as 1 + (2 B + 1) / den, focal as the two sums);
    a loss as the sum of its non-negative summands (dice: 1 + ratio per mask); the sums kept for the backward as themselves; per
    cotangent vector d_logits |k| (p + 1), d_centers |g| / matched, d_params the L1, the two cosine and (layer 0) the two Q terms with
    sum |X| over the valid pixels of the mask, d_mask_logits / d_pixel_centers one more backward pass of F.interpolate with the absolute
    cotangent of every high-resolution pixel.  One rule is added to the plain magnitudes: a focal or dice term that holds 1 - sigmoid
    takes it at _one_minus_magnitude, and the dice derivative's 2 D1 t - N1 counts both terms; without it a logit of +30 (the sweep
    has them) asks float32 for the relative accuracy of a 1e-13 that it can only form as 1 - 1."""
    L, B, nq, nmax, s = case.L, case.B, case.nq, case.nmax, case.s
    t = {k: x[k].double() for k in FLOAT_INPUTS}
    mq, mg = x["match_q"], x["match_gt"]
    H, W = x["masks"].shape[-2:]
    matched = float(sum(case.n))
    nm = case.num_masks if case.num_masks > 0 else max(matched, 1.0)
    S = {"cost": torch.zeros(L * B, nq, nmax, dtype=F64)}
    Tf, Td = torch.zeros_like(t["mlog"]), torch.zeros_like(t["mlog"])           # transposed |d focal|, |d dice| per low-resolution pixel
    dice_s, focal_l, focal_s = torch.zeros(L, dtype=F64), torch.zeros(L, dtype=F64), torch.zeros(L * B, nmax, dtype=F64)
    for i in range(L * B):
        b, n = i % B, case.n[i % B]
        # cost
        xl = t["mlog"][i].flatten(1)
        tm = F.interpolate(x["masks"][b, :n].double()[:, None], size=(case.h, case.w), mode="nearest")[:, 0].flatten(1)
        p = xl.sigmoid()
        fpos = 0.25 * _one_minus_magnitude(xl, p) ** 2 * F.softplus(-xl)
        fneg = 0.75 * p ** 2 * F.softplus(xl)
        pr, tp = t["params"][i], t["tparams"][b, :n]
        cos = torch.clamp(F.normalize(pr, dim=-1) @ F.normalize(tp, dim=-1).T, min=-0.999999, max=0.999999)
        S["cost"][i, :, :n] = (WTS["cost_mask"] * (fpos @ tm.T + fneg @ (1 - tm).T) / xl.shape[1]
                               + WTS["cost_class"] * t["logits"][i].softmax(-1)[:, :1]
                               + WTS["cost_dice"] * (1 + (2 * (p @ tm.T) + 1) / (p.sum(-1)[:, None] + tm.sum(-1)[None] + 1))
                               + WTS["cost_center"] * torch.cdist(t["centers"][i], t["tcenters"][b, :n])
                               + WTS["cost_param"] * torch.cdist(pr, tp, p=1)
                               + WTS["cost_offset"] * (pr.norm(dim=-1)[:, None] - tp.norm(dim=-1)[None]).abs()
                               + WTS["cost_angle"] * torch.acos(cos) * 180.0 / np.pi)
        # the matched masks at the high resolution
        qs = mq[i, :n].long()
        lo = t["mlog"][i, qs].clone().requires_grad_(True)
        sm = F.interpolate(lo[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        tmh = x["masks"][b, :n].double()
        ph, fo, dfo = _focal_magnitudes(sm.detach(), tmh)
        D1 = (ph.flatten(1).sum(1) + tmh.flatten(1).sum(1) + 1)[:, None, None]
        N1 = (2 * (ph * tmh).flatten(1).sum(1) + 1)[:, None, None]
        ddi = (2 * D1 * tmh + N1) / D1 ** 2 * ph * _one_minus_magnitude(sm.detach(), ph)
        Tf[i, qs], = torch.autograd.grad((sm * dfo).sum(), lo, retain_graph=True)
        Td[i, qs], = torch.autograd.grad((sm * ddi).sum(), lo)
        Tf[i, qs] += _tap_rounding(dfo, case) / EPS24
        Td[i, qs] += _tap_rounding(ddi, case) / EPS24
        dice_s[i // B] += (1 + N1 / D1).sum()
        focal_s[i, :n] = fo.flatten(1).sum(1)
        focal_l[i // B] += fo.flatten(1).mean(1).sum()
    S["losses"] = ev["losses"].abs().clone()
    for l in range(L):
        S["losses"][6 * l + 1], S["losses"][6 * l + 2] = focal_l[l] / nm, dice_s[l] / nm
    S["mask_stats"], S["q_stats"] = ev["mask_stats"].abs().clone(), ev["q_stats"].abs().clone()
    S["mask_stats"][..., 0] = focal_s
    lo = t["pixc"].clone().requires_grad_(True)
    Tp, = torch.autograd.grad(F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).sum(), lo)
    prob = t["logits"].softmax(-1)
    wsum = sum(n + EOS_F32 * (nq - n) for n in case.n)
    on = (mg >= 0)
    per = []
    for g in x["gs"]:
        g = g.double().abs()
        Sg = {}
        layer_of = torch.arange(L * B) // B
        k = g[6 * layer_of][:, None] * torch.where(on, 1.0, EOS_F32) / wsum
        Sg["d_logits"] = k[..., None] * (prob + 1)
        Sg["d_mask_logits"] = (g[6 * layer_of + 1] / (nm * H * W))[:, None, None, None] * Tf + (g[6 * layer_of + 2] / nm)[:, None, None, None] * Td
        Sg["d_centers"] = (g[6 * layer_of + 3] / matched)[:, None, None] * on[..., None].double().expand(-1, -1, 2)
        Sg["d_pixel_centers"] = g[6 * L] / (B * H * W) * Tp
        dp = torch.zeros_like(t["params"])
        for i in range(L * B):
            b, n = i % B, case.n[i % B]
            qs = mq[i, :n].long()
            p, tt = t["params"][i, qs], t["tparams"][b, :n]
            np_, nt = p.norm(dim=-1, keepdim=True), tt.norm(dim=-1, keepdim=True)
            cosv = (p * tt).sum(-1, keepdim=True) / (np_ * nt)
            v = g[6 * (i // B) + 4] / matched * (p != tt).double() + g[6 * (i // B) + 5] / matched * (tt.abs() / (np_ * nt) + (cosv * p).abs() / np_ ** 2)
            cnt = float(ev["q_stats"][b, 1])
            if i < B and cnt > 0:
                ax = ev["absx"][b, :n]
                v = v + g[6 * L + 1] / (B * cnt) * (ax / np_ ** 2 + 2 * p.abs() * (ax * p.abs()).sum(-1, keepdim=True) / np_ ** 4)
            dp[i, qs] = v
        Sg["d_params"] = dp
        per.append(Sg)
    S["grads"] = per
    return S




def conditioning(x, case, ref):
    """C_k over DRAWS draws that multiply every f32 input and cotangent by 1 +- 2^-23"""
    g = torch.Generator().manual_seed(77)
    C = {k: torch.zeros_like(ref[k]) for k in OUT_FLOAT}
    C["grads"] = [{k: torch.zeros_like(v) for k, v in gr.items()} for gr in ref["grads"]]
    for _ in range(DRAWS):
        xj = dict(x)
        for k in FLOAT_INPUTS:
            xj[k] = jiggle(x[k], g)
        for key, tkey in (("params", "tparams"), ("centers", "tcenters")):      # what is equal on purpose gets the same factor: there the
            for i, q, b, j in x["tied"][key]:                                    # kernels promise the subgradient 0, and a C_k from independent
                xj[key][i, q] = xj[tkey][b, j]                                   # draws would be as large as the gradient and accept anything
        xj["pixc"][0, :, :2, :2] = xj["tpixel"][0, :, 0, 0][:, None, None]
        got = evaluate(xj, case, F64, [jiggle(t, g) for t in x["gs"]])
        for k in OUT_FLOAT:
            C[k] = torch.maximum(C[k], (got[k] - ref[k]).abs())
        for a, b, c in zip(C["grads"], got["grads"], ref["grads"]):
            for k in a:
                a[k] = torch.maximum(a[k], (b[k] - c[k]).abs())
    return C


def build_reference(x, case):
    """-> (ref, A): the float64 outputs and the allowance 2^-24 S + C per element.  The integer-valued outputs get no allowance."""
    ref = evaluate(x, case, F64, x["gs"])
    S, C = magnitudes(x, case, ref), conditioning(x, case, ref)
    A = {k: EPS24 * S[k] + C[k] + TINY for k in OUT_FLOAT}
    A["mask_stats"][..., 3] = 0.0
    A["q_stats"][..., 1] = 0.0
    A["grads"] = [{k: EPS24 * s[k] + c[k] + TINY for k in s} for s, c in zip(S["grads"], C["grads"])]
    return ref, A


@functools.lru_cache(maxsize=None)
def reference(name):
    return build_reference(inputs(name), CASES[name])


def worst(got, ref, A, case):
    """{family: worst error / A over every element} of one set of outputs (the restatement's names; grads = one dict per cotangent)"""
    out = {}
    for k in OUT_FLOAT:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        out[k] = float(ratios(got[k], ref[k], A[k]).max())
    for gg, gr, ga in zip(got["grads"], ref["grads"], A["grads"]):
        for k in GRADS:
            if k == "d_pixel_centers" and not case.pixel:
                continue
            assert gg[k].shape == gr[k].shape, (k, gg[k].shape, gr[k].shape)
            out[k] = max(out.get(k, 0.0), float(ratios(gg[k], gr[k], ga[k]).max()))
    return out


def f32_ratios(name):
    x, case = inputs(name), CASES[name]
    ref, A = reference(name)
    return worst(evaluate(x, case, F32, x["gs"]), ref, A, case)


def f32_worst(names=None):
    out = {}
    for name in (CASES if names is None else names):
        for k, v in f32_ratios(name).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def print_f32_worst():
    print(", ".join('"%s": %.3g' % kv for kv in f32_worst().items()))


def conditions_hold(name):
    """Every input condition of the issue, in float64 and in float32"""
    for dtype in (F64, F32):
        m = margins(name, dtype)
        if not (m["gd"] >= GD_MARGIN and m["res"] >= RES_MARGIN and m["diff"] >= DIFF_MARGIN and m["norm"] >= NORM_MARGIN and m["dist"] > DIST_MARGIN):
            return False
    return True


def margins(name, dtype):
    """The measured decision margins of one case in `dtype` (see the constants above)"""
    x, case = inputs(name), CASES[name]
    t = {k: x[k].to(dtype) for k in FLOAT_INPUTS}
    t["masks"] = x["masks"]
    st = stats(t, case, x["match_q"])
    nz = lambda d: float(d[d != 0].min()) if (d != 0).any() else float("inf")
    diffs, dists, norms = [], [], [t["tparams"][b, :n].norm(dim=-1) for b, n in enumerate(case.n)] + [t["params"].norm(dim=-1).flatten()]
    for i in range(case.L * case.B):
        b, n = i % case.B, case.n[i % case.B]
        qs = x["match_q"][i, :n].long()
        diffs.append((t["params"][i, qs] - t["tparams"][b, :n]).abs().flatten())
        dists.append((t["centers"][i, qs] - t["tcenters"][b, :n]).norm(dim=-1))
    if case.pixel:
        up = F.interpolate(t["pixc"], size=t["tpixel"].shape[-2:], mode="bilinear", align_corners=False)
        dists.append((up - t["tpixel"]).norm(dim=1).flatten())
    return {"gd": float((st["gd"] - 0.2).abs().min()), "res": float(st["res"].abs().min()) if st["res"].numel() else float("inf"),
            "diff": nz(torch.cat(diffs)), "zero_diff": int((torch.cat(diffs) == 0).sum()), "norm": float(torch.cat(norms).min()),
            "dist": nz(torch.cat(dists)), "zero_dist": int((torch.cat(dists) == 0).sum()),
            "valid": [int(v) for v in st["q_stats"][:, 1]], "flips": st["flips"], "covered_twice": int((x["masks"].sum(1) > 1).sum())}


# ===================================================================================================================== targets
TARGET_CASES = {"1x1": (1, 1, [1, 1], 1, 0), "3x5": (3, 5, [3, 1], 4, 1), "24x32": (24, 32, [7, 50], 50, 2), "36x640": (36, 640, [6, 2], 6, 3)}


@functools.lru_cache(maxsize=None)
def target_inputs(name, empty=False):
    """masks uint8 [B, nmax, H, W] of non-empty planes (with `empty`, plane 1 of image 0 is blank), n"""
    H, W, n, nmax, seed = TARGET_CASES[name]
    g = torch.Generator().manual_seed(4000 + seed)
    masks = torch.zeros(len(n), nmax, H, W, dtype=torch.uint8)
    for b in range(len(n)):
        for j in range(n[b]):
            masks[b, j] = _plane_mask(j if j < 6 else 6, H, W, g)
    if empty:
        masks[0, 1] = 0
    return masks, list(n)


def exact_centroids(masks, n):
    """[B, nmax, 2] of Fractions (None beyond n[b] and for an empty mask): sum x / (W count), sum y / (H count)"""
    B, nmax, H, W = masks.shape
    out = [[None] * nmax for _ in range(B)]
    for b in range(B):
        for j in range(n[b]):
            ys, xs = np.nonzero(masks[b, j].numpy())
            if len(xs):
                out[b][j] = (Fraction(int(xs.sum()), W * len(xs)), Fraction(int(ys.sum()), H * len(xs)))
    return out


def centre_map_f32(masks, n, centers):
    """The centre map as the kernel documents it: per pixel the float32 sum of centre * mask in plane order"""
    B, nmax, H, W = masks.shape
    out = torch.zeros(B, 2, H, W, dtype=F32)
    for b in range(B):
        for j in range(n[b]):
            on = masks[b, j] != 0
            for c in range(2):
                out[b, c] = out[b, c] + torch.where(on, centers[b, j, c], torch.zeros((), dtype=F32))
    return out


# ===================================================================================================================== assignment
INF = 1e300


def assign_emulate(C, plant=None):
    """pc_assign_kernel in numpy on one image's float32 cost [nq, n]: rows = targets, columns = queries, shortest augmenting paths with f64
    duals, the column of least path cost taken with the lanes' tie rule (an unassigned column first, then the lowest index); non-finite
    costs leave the remaining targets unmatched.  -> (match_q [n], match_gt [nq], failed).  plant "row_duals": the dual update of the
    scanned rows dropped."""
    nq, n = C.shape
    nr = min(n, nq)
    cs = np.ascontiguousarray(C.T).astype(np.float32)
    u, v = np.zeros(n), np.zeros(nq)
    r4c, col4row = -np.ones(nq, dtype=np.int64), -np.ones(n, dtype=np.int64)
    failed = False
    for cur in range(nr):
        spc, path, sc = np.full(nq, INF), -np.ones(nq, dtype=np.int64), np.zeros(nq, dtype=bool)
        minval, ii, sink = 0.0, cur, -1
        for _ in range(nq + 1):                                                  # the kernel's bound: every step scans one more column
            if sink >= 0:
                break
            with np.errstate(invalid="ignore"):
                r = minval + cs[ii].astype(np.float64) - u[ii] - v
                upd = ~sc & (r < spc)
            spc[upd], path[upd] = r[upd], ii
            cand = np.nonzero(~sc)[0]
            if len(cand) == 0:
                failed = True
                break
            best = spc[cand].min()
            if not best < INF:
                failed = True
                break
            tie = cand[spc[cand] == best]
            free = tie[r4c[tie] < 0]
            j = int(free[0] if len(free) else tie[0])
            minval = best
            sc[j] = True
            if r4c[j] < 0:
                sink = j
            else:
                ii = int(r4c[j])
        if failed or sink < 0:
            failed = True
            break
        d = minval - spc
        for c in np.nonzero(sc)[0]:
            if r4c[c] >= 0 and plant != "row_duals":
                u[r4c[c]] += d[c]
            v[c] -= d[c]
        u[cur] += minval
        j = sink
        for _ in range(nr + 1):
            pi = int(path[j])
            r4c[j] = pi
            j, col4row[pi] = int(col4row[pi]), j
            if pi == cur:
                break
    return col4row, r4c, failed


def _perm_costs(g, nq, n, cols):
    """uniform costs in [0, 1) with a permutation of cost -1 planted onto `cols`"""
    C = torch.rand(nq, n, generator=g)
    C[torch.as_tensor(cols)[torch.randperm(n, generator=g)], torch.arange(n)] = -1.0
    return C


def assign_launches():
    """name -> (nq, nmax, [(kind, cost [nq, n] float32), ...]): hand-made costs, one launch per (nq, nmax), a different n per image"""
    g = torch.Generator().manual_seed(5000)
    rnd = lambda nq, n: torch.randn(nq, n, generator=g)
    ints = lambda nq, n, hi=4: torch.randint(0, hi, (nq, n), generator=g).float()
    twin = rnd(128, 10)
    twin[5] = twin[90]                                                           # two identical query columns
    big = (2.0 ** 20 + ints(128, 20, 8))
    order = rnd(100, 30) * 1e-3 + 4096.0                                         # steps of 2^-11 on 4096: only duals wider than f32 keep the order
    out = {
        "q128": (128, 50, [("continuous", rnd(128, 50)), ("continuous", rnd(128, 1)), ("ties", ints(128, 7)), ("ties", ints(128, 50)),
                           ("ties", torch.full((128, 50), 0.25)), ("planted", _perm_costs(g, 128, 50, range(64, 114))),
                           ("planted", _perm_costs(g, 128, 50, range(78, 128))), ("planted", _perm_costs(g, 128, 13, range(115, 128))),
                           ("ties", big), ("continuous", rnd(128, 33) * torch.where(torch.rand(128, 33, generator=g) < 0.5, -50.0, 0.02)),
                           ("ties", twin), ("ties", torch.full((128, 1), -3.0))]),
        "q100": (100, 30, [("ties", order), ("ties", 2.0 ** 20 - ints(100, 30, 3)), ("continuous", rnd(100, 2))]),
        "square50": (50, 50, [("continuous", rnd(50, 50)), ("ties", ints(50, 50)), ("ties", torch.zeros(50, 50)), ("continuous", rnd(50, 1)),
                              ("planted", _perm_costs(g, 50, 50, range(50))), ("ties", 2.0 ** 20 + ints(50, 50, 8)),
                              ("ties", torch.outer(torch.arange(1.0, 51.0), torch.arange(1.0, 51.0))), ("ties", ints(50, 50, 100))]),
        "q1": (1, 3, [("continuous", rnd(1, 1)), ("ties", torch.zeros(1, 1))]),
        "q65": (65, 20, [("continuous", rnd(65, 20)), ("planted", _perm_costs(g, 65, 1, [64])), ("ties", ints(65, 9, 2)),
                         ("planted", _perm_costs(g, 65, 20, range(45, 65)))]),
    }
    return out


def refusal_launch():
    """(nq, nmax, images): a sound image, a column of +inf (feasible: the optimum avoids it), a target row of +inf, a NaN row, a sound
    image.  kind = (name, first failing target or None)"""
    g = torch.Generator().manual_seed(5001)
    nq, n = 16, 10
    mk = lambda: torch.randn(nq, n, generator=g)
    col, row, nan = mk(), mk(), mk()
    col[3, :] = float("inf")
    row[:, 4] = float("inf")
    nan[:, 6] = float("nan")
    return nq, n, [(("sound", None), mk()), (("inf_column", None), col), (("inf_row", 4), row), (("nan_row", 6), nan), (("sound", None), mk())]


def pack_costs(nq, nmax, images):
    """-> cost [B, nq, nmax] (NaN beyond n[b]: never read), n"""
    cost = torch.full((len(images), nq, nmax), float("nan"))
    for b, (_, C) in enumerate(images):
        cost[b, :, :C.shape[1]] = C
    return cost, [C.shape[1] for _, C in images]


def scipy_assign(C):
    from scipy.optimize import linear_sum_assignment
    q, j = linear_sum_assignment(np.asarray(C, dtype=np.float64))
    return q, j


def check_match(mq, mg, C, upto=None):
    """match_q / match_gt of one image are a valid injection of the targets [0, upto) and each other's inverse; -> the total cost"""
    nq, n = C.shape
    upto = n if upto is None else upto
    mq, mg = np.asarray(mq), np.asarray(mg)
    assert (mq[upto:] == -1).all(), mq
    q = mq[:upto]
    assert ((q >= 0) & (q < nq)).all() and len(set(q.tolist())) == upto, mq
    want = -np.ones(nq, dtype=np.int64)
    want[q] = np.arange(upto)
    assert (mg == want).all(), (mq, mg)
    return float(np.asarray(C, dtype=np.float64)[q, np.arange(upto)].sum())


def optimum_gap(C):
    """The least increase of the optimum when one of its pairs is forbidden (> 0: the optimum is unique)"""
    C = np.asarray(C, dtype=np.float64)
    q, j = scipy_assign(C)
    best, gap = C[q, j].sum(), float("inf")
    if C.shape[0] == 1:
        return gap
    for a, b in zip(q, j):
        D = C.copy()
        D[a, b] = 1e9
        q2, j2 = scipy_assign(D)
        gap = min(gap, D[q2, j2].sum() - best)
    return gap


# ===================================================================================================================== correspondence matrix
def corr_cases():
    """name -> (nq, nmax, n1, n2, corrs per pair): K = 1, K above 256, nq 1 and 128, nmax < 50 with gt indices in [nmax, 50), duplicates,
    rows of padding only"""
    g = torch.Generator().manual_seed(6000)
    pairs = lambda k, hi: [(int(a), int(b)) for a, b in torch.randint(0, hi, (k, 2), generator=g)]
    return {
        "k1": (8, 6, [4, 6], [5, 3], [[(1, 2)], [(5, 0)]]),
        "k300": (128, 50, [50, 20, 1], [50, 7, 50], [pairs(300, 50), pairs(280, 50) + [(51, 2), (3, 60)], []]),
        "nq1": (1, 1, [1, 1, 1], [1, 1, 1], [[(0, 0)], [], [(0, 0), (0, 0)]]),
        "small_nmax": (64, 12, [12, 5], [9, 12], [pairs(40, 12) + [(12, 3), (49, 49), (20, 1), (2, 30)], pairs(10, 50) + [(4, 4), (4, 4)]]),
        "padding": (50, 50, [3, 4], [4, 3], [[], []]),
    }


def corr_inputs(name):
    """-> corrs, gt_corrs int32 [B, K, 2] padded with -1, match1 / match2 int32 [B, nmax], the restatement's index pairs"""
    nq, nmax, n1, n2, corrs = corr_cases()[name]
    g = torch.Generator().manual_seed(6001)
    K = max(1, max(len(c) for c in corrs))
    pad = torch.full((len(corrs), K, 2), -1, dtype=torch.int32)
    for b, c in enumerate(corrs):
        if c:
            pad[b, :len(c)] = torch.tensor(c, dtype=torch.int32)

    def match(n):
        mq = torch.full((len(n), nmax), -1, dtype=torch.int32)
        for b, nb in enumerate(n):
            mq[b, :nb] = torch.randperm(nq, generator=g)[:nb].to(torch.int32)
        return mq
    m1, m2 = match(n1), match(n2)
    as_ref = lambda mq, n: [(mq[b, :nb].long(), torch.arange(nb)) for b, nb in enumerate(n)]
    return corrs, pad, m1, m2, as_ref(m1, n1), as_ref(m2, n2)


# ===================================================================================================================== f32 emulation
# The kernels' own formulas in float32 with their documented order of partial sums: the 64-pixel chunks of a workgroup added in chunk
# order and the block partials by index (cost), the band partials in band order (masks, centre map), the transposed bilinear weights
# over each low-resolution pixel's dependants (gradients), the 16 Q chunks.  The sums inside one workgroup are torch's.  `plant` names
# one error; PLANTS maps it to the output families it must push over the limit and to the cases that reach the faulty term.
PLANTS = {
    "no_half_pixel": ("losses", "d_mask_logits"), "border_tap_not_folded": ("d_mask_logits",), "dependants_one_short": ("d_mask_logits",),
    "halo_from_first_row": ("losses", "d_mask_logits"), "alpha_swapped": ("cost", "losses", "d_mask_logits"), "dice_no_smoothing": ("cost", "losses"),
    "dice_grad_no_2d1": ("d_mask_logits",), "override_ignored": ("d_mask_logits",), "nearest_at_centre": ("cost",), "dead_lanes_counted": ("cost",),
    "first_block_only": ("cost",), "eos_on_matched": ("losses",), "weight_sum_nq_b": ("d_logits",), "targets_at_i_div_l": ("cost",),
    "valid_on_prediction": ("q_stats",), "p_over_norm": ("q_stats", "d_params"), "q_grad_no_projection": ("d_params",),
    "cos_grad_no_projection": ("d_params",), "centre_map_scale_hw": ("d_pixel_centers",), "row_duals": ("assignment",),
}


def plant_reaches(plant, case):
    """Does the case reach the term the plant breaks?"""
    s, L, B = case.s, case.L, case.B
    chunks, live = chunk_walk(case)
    some_valid = plant in ("valid_on_prediction", "p_over_norm", "q_grad_no_projection") and any(v > 0 for v in margins(case.name, F64)["valid"])
    free = any(n < case.nq for n in case.n)                                     # an unmatched query
    return {"no_half_pixel": s >= 2 and case.h * case.w > 1, "border_tap_not_folded": s >= 2, "dependants_one_short": s >= 2,
            "halo_from_first_row": case.h > BAND and s >= 2, "override_ignored": case.num_masks > 0, "nearest_at_centre": s >= 2,
            "dead_lanes_counted": live < CHUNK, "first_block_only": len(chunks) > 1, "targets_at_i_div_l": L > 1 and B > 1 and L != B,
            "centre_map_scale_hw": case.pixel and s >= 2, "eos_on_matched": free, "weight_sum_nq_b": free,
            "valid_on_prediction": plant == "valid_on_prediction" and margins(case.name, F64)["flips"] > 0, "p_over_norm": some_valid, "q_grad_no_projection": some_valid,
            "row_duals": False}.get(plant, True)


def plant_shows(name, plant):
    """Does the emulation with the plant leave the limit (or a decision) on one of the plant's families?"""
    case = CASES[name]
    ref, A = reference(name)
    got = emulate(name, plant)
    w = worst(got, ref, A, case)
    return (not torch.equal(got["q_valid"], ref["q_valid"])) or any(not w.get(fam, 0.0) <= limit(fam) for fam in PLANTS[plant])


def _taps(hi, lo, plant):
    inv = torch.tensor(lo, dtype=F32) / torch.tensor(hi, dtype=F32)
    dst = torch.arange(hi, dtype=F32)
    src = torch.clamp(dst * inv if plant == "no_half_pixel" else (dst + 0.5) * inv - 0.5, min=0.0)
    i0 = torch.clamp(src.long(), max=lo - 1)
    i1 = torch.clamp(i0 + 1, max=lo - 1)
    return i0, i1, src - i0.to(F32)


def _weights(hi, lo, s, plant):
    """[hi, lo] transposed-gather weights: pc_tap_weight restricted to pc_dependants"""
    i0, i1, l1 = _taps(hi, lo, plant)
    Wm = torch.zeros(hi, lo, dtype=F32)
    r = torch.arange(hi)
    if plant == "border_tap_not_folded":
        Wm[r, i1] = l1
        Wm[r, i0] = 1 - l1
    else:
        Wm[r, i0] += 1 - l1
        Wm[r, i1] += l1
    k = torch.arange(lo)
    a = 2 * s * k - s - 1
    first = torch.clamp(torch.div(a, 2, rounding_mode="floor") + 1, min=0)
    last = torch.clamp((2 * s * k + 3 * s) // 2 - 1, max=hi - 1) - (1 if plant == "dependants_one_short" else 0)
    return Wm * ((r[:, None] >= first[None]) & (r[:, None] <= last[None])).to(F32)


def _upsample(lo, H, W, plant):
    """the forward interpolation of the band kernels, band by band: [n, h, w] -> [n, H, W]"""
    n, h, w = lo.shape
    iy0, iy1, ly = _taps(H, h, plant)
    ix0, ix1, lx = _taps(W, w, plant)
    if plant == "halo_from_first_row":                                          # the top halo row of every band but the first
        y0 = (torch.arange(H) // (H // h) // BAND) * BAND
        iy0 = torch.where((iy0 < y0), y0, iy0)
    r0, r1 = lo[:, iy0], lo[:, iy1]
    top = (1 - lx) * r0[:, :, ix0] + lx * r0[:, :, ix1]
    bot = (1 - lx) * r1[:, :, ix0] + lx * r1[:, :, ix1]
    return (1 - ly)[None, :, None] * top + ly[None, :, None] * bot


def _sig(v):
    e = torch.exp(-v.abs())
    l = torch.log1p(e)
    return torch.where(v >= 0, 1 / (1 + e), e / (1 + e)), torch.clamp(v, min=0) + l, torch.clamp(-v, min=0) + l


def _in_order(parts):
    """float32 sum of a list of tensors, added by index"""
    acc = torch.zeros_like(parts[0])
    for p in parts:
        acc = acc + p
    return acc


def emulate(name, plant=None):
    x, case = inputs(name), CASES[name]
    L, B, nq, nmax, h, w, s = case.L, case.B, case.nq, case.nmax, case.h, case.w, case.s
    H, W, LB, hw = s * h, s * w, L * B, h * w
    f = lambda v: torch.tensor(v, dtype=F32)
    al = 0.75 if plant == "alpha_swapped" else 0.25
    eos, mq, mg = f(WTS["eos_coef"]), x["match_q"], x["match_gt"]
    matched = f(float(sum(case.n)))
    nm = f(case.num_masks) if case.num_masks > 0 else torch.clamp(matched, min=1.0)
    nm_bwd = torch.clamp(matched, min=1.0) if plant == "override_ignored" else nm
    sm1 = 0.0 if plant == "dice_no_smoothing" else 1.0
    out = {"cost": torch.zeros(LB, nq, nmax), "mask_stats": torch.zeros(LB, nmax, 4), "q_stats": torch.zeros(B, 2)}
    img = torch.zeros(LB, 7)
    # ---- costs
    chunks, live = chunk_walk(case)
    nblk, off = len(chunks), (s // 2 if plant == "nearest_at_centre" else 0)
    for i in range(LB):
        b = i // L if plant == "targets_at_i_div_l" else i % B
        n = case.n[i % B]
        xl = x["mlog"][i].flatten(1)
        p, sp0, sp1 = _sig(xl)
        fp, fn = al * ((1 - p) * (1 - p)) * sp1, (1 - al) * (p * p) * sp0
        tm = x["masks"][i % B, :n, off::s, off::s][:, :h, :w].to(F32).flatten(1)
        if tm.shape[1] != hw:
            tm = torch.nn.functional.pad(tm, (0, hw - tm.shape[1]))
        blocks = []
        for blk in range(1 if plant == "first_block_only" else nblk):
            parts = []
            for c in range(blk, len(range(0, hw, CHUNK)), nblk):
                sl = slice(c * CHUNK, min((c + 1) * CHUNK, hw))
                D, S_, t_ = (fp - fn)[:, sl], p[:, sl], tm[:, sl]
                part = [D @ t_.T, S_ @ t_.T, fn[:, sl].sum(1), S_.sum(1), t_.sum(1)]
                if plant == "dead_lanes_counted" and sl.stop - sl.start < CHUNK:
                    k = CHUNK - (sl.stop - sl.start)
                    part = [part[0] + k * (fp - fn)[:, :1] * tm[:, 0][None], part[1] + k * p[:, :1] * tm[:, 0][None], part[2] + k * fn[:, 0],
                            part[3] + k * p[:, 0], part[4] + k * tm[:, 0]]
                parts.append(part)
            blocks.append([_in_order([q[k] for q in parts]) for k in range(5)])
        A_, Bq, fns, sg, tj = (_in_order([q[k] for q in blocks]) for k in range(5))
        focal = (fns[:, None] + A_) / hw
        dice = 1 - (2 * Bq + sm1) / (sg[:, None] + tj[None] + sm1)
        z = x["logits"][i]
        e = torch.exp(z - z.max(-1, keepdim=True).values)
        cls = -(e[:, 0] / e.sum(-1))
        pr, tp = x["params"][i], x["tparams"][b, :n]
        cen = (x["centers"][i][:, None] - x["tcenters"][b, :n][None]).pow(2).sum(-1).sqrt()
        l1 = (pr[:, None] - tp[None]).abs().sum(-1)
        np_, nt = pr.pow(2).sum(-1).sqrt(), tp.pow(2).sum(-1).sqrt()
        cosv = torch.clamp(((pr / np_[:, None])[:, None] * (tp / nt[:, None])[None]).sum(-1), -0.999999, 0.999999)
        out["cost"][i, :, :n] = (WTS["cost_mask"] * focal + WTS["cost_class"] * cls[:, None] + WTS["cost_dice"] * dice + WTS["cost_center"] * cen
                                 + WTS["cost_param"] * l1 + WTS["cost_offset"] * (np_[:, None] - nt[None]).abs()
                                 + WTS["cost_angle"] * torch.acos(cosv) * f(180.0 / np.pi))
    # ---- losses
    wy, wx = _weights(H, h, s, plant), _weights(W, w, s, plant)
    grads = [{"d_logits": torch.zeros(LB, nq, 2), "d_mask_logits": torch.zeros(LB, nq, h, w), "d_centers": torch.zeros(LB, nq, 2),
              "d_params": torch.zeros(LB, nq, 3), "d_pixel_centers": torch.zeros(B, 2, h, w)} for _ in x["gs"]]
    wsum = _in_order([f(float(n)) + eos * f(float(nq - n)) for n in case.n])
    if plant == "weight_sum_nq_b":
        wsum = f(float(nq * B))
    nbands = -(-h // BAND)
    # Q loss of the last layer
    valid, G, qpart = torch.zeros(B, H * W, dtype=torch.bool), torch.zeros(B, nmax, 3), torch.zeros(B)
    chunk_of = (torch.arange(H * W) // 256) % QCHUNKS
    for b in range(B):
        n = case.n[b]
        X = (x["kinv"][b] * x["depth"][b][None]).reshape(3, -1)
        inv = lambda pp: pp / pp.pow(2).sum(-1, keepdim=True).sqrt() if plant == "p_over_norm" else pp / pp.pow(2).sum(-1, keepdim=True)
        gp, pp = x["tparams"][b, :n] / x["tparams"][b, :n].pow(2).sum(-1, keepdim=True), inv(x["params"][b][mq[b, :n].long()])
        gm = (x["masks"][b, :n] != 0).flatten(1).to(F32)
        ge, res = ((gp @ X - 1).abs() * gm).sum(0), pp @ X - 1
        pe = (res.abs() * gm).sum(0)
        ok = ((pe if plant == "valid_on_prediction" else ge) < 0.2) & (gm.sum(0) > 0)
        valid[b] = ok
        parts = [(torch.where(ok & (chunk_of == c), pe, torch.zeros(())).sum(), (ok & (chunk_of == c)).sum().to(F32)) for c in range(QCHUNKS)]
        out["q_stats"][b, 0], out["q_stats"][b, 1] = _in_order([q[0] for q in parts]), _in_order([q[1] for q in parts])
        sgn = torch.sign(res) * gm * ok.to(F32)[None]
        G[b, :n] = _in_order([(sgn * (chunk_of == c).to(F32)[None]) @ X.T for c in range(QCHUNKS)])
        qpart[b] = out["q_stats"][b, 0] / out["q_stats"][b, 1] if out["q_stats"][b, 1] > 0 else 0.0
    out["q_valid"] = valid.reshape(B, H, W).to(torch.uint8)
    for i in range(LB):
        b, layer, n = i % B, i // B, case.n[i % B]
        qs = mq[i, :n].long()
        on = mg[i] >= 0
        z = x["logits"][i]
        zm = z.max(-1).values
        lse = zm + torch.log(torch.exp(z[:, 0] - zm) + torch.exp(z[:, 1] - zm))
        wt = torch.where(on, torch.ones(()), eos) if plant != "eos_on_matched" else eos.expand(nq)
        img[i, 0], img[i, 1] = (wt * (lse - torch.where(on, z[:, 0], z[:, 1]))).sum(), wt.sum()
        c, tc, p, t = x["centers"][i, qs], x["tcenters"][b, :n], x["params"][i, qs], x["tparams"][b, :n]
        dist = (tc - c).pow(2).sum(-1).sqrt()
        np_, nt = p.pow(2).sum(-1, keepdim=True).sqrt(), t.pow(2).sum(-1, keepdim=True).sqrt()
        cosv = (p * t).sum(-1, keepdim=True) / (np_ * nt)
        img[i, 2], img[i, 3], img[i, 4] = dist.sum(), (t - p).abs().sum(), (1 - cosv).sum()
        v = _upsample(x["mlog"][i, qs], H, W, plant)
        tmh = x["masks"][b, :n] != 0
        ps, sp0, sp1 = _sig(v)
        fo = torch.where(tmh, al * ((1 - ps) * (1 - ps)) * sp1, (1 - al) * (ps * ps) * sp0)
        band = lambda q: _in_order([q[:, s * k * BAND:s * (k + 1) * BAND].flatten(1).sum(1) for k in range(nbands)])
        st = torch.stack([band(fo), band(torch.where(tmh, ps, torch.zeros(()))), band(ps), band(tmh.to(F32))], 1)
        out["mask_stats"][i, :n] = st
        img[i, 5] = _in_order(list(st[:, 0] / (H * W)))
        img[i, 6] = _in_order(list(1 - (2 * st[:, 1] + sm1) / (st[:, 2] + st[:, 3] + sm1)))
        D1, N1 = (st[:, 2] + st[:, 3] + 1)[:, None, None], (2 * st[:, 1] + 1)[:, None, None]
        dfo = torch.where(tmh, -al * ((1 - ps) * (1 - ps)) * (2 * ps * sp1 + (1 - ps)), (1 - al) * (ps * ps) * (2 * (1 - ps) * sp0 + ps))
        ddi = -((0.0 if plant == "dice_grad_no_2d1" else 2 * D1 * tmh.to(F32)) - N1) / (D1 * D1) * (ps * (1 - ps))
        for gr, g in zip(grads, x["gs"]):
            k = g[6 * layer] * torch.where(on, torch.ones(()), eos) / wsum
            e = torch.exp(z - zm[:, None])
            pz = e / e.sum(-1, keepdim=True)
            gr["d_logits"][i] = k[:, None] * (pz - torch.stack([on.to(F32), 1 - on.to(F32)], 1))
            gmk, gdk = g[6 * layer + 1] / (nm_bwd * H * W), g[6 * layer + 2] / nm_bwd
            gr["d_mask_logits"][i, qs] = torch.einsum("Yy,nYX,Xx->nyx", wy, gmk * dfo + gdk * ddi, wx)
            d = c - tc
            gr["d_centers"][i, qs] = torch.where(dist[:, None] > 0, g[6 * layer + 3] / matched * d / dist[:, None], torch.zeros(()))
            dp = g[6 * layer + 4] / matched * torch.sign(p - t)
            proj = 0.0 if plant == "cos_grad_no_projection" else cosv * p / (np_ * np_)
            dp = dp + g[6 * layer + 5] / matched * -(t / (np_ * nt) - proj)
            if layer == 0 and out["q_stats"][b, 1] > 0:
                r2, gpd = np_ * np_, (G[b, :n] * p).sum(-1, keepdim=True)
                kq = g[6 * L + 1] / (B * out["q_stats"][b, 1])
                dp = dp + kq * (G[b, :n] / r2 - (0.0 if plant == "q_grad_no_projection" else 2 * p * gpd / (r2 * r2)))
            gr["d_params"][i, qs] = dp
    losses = torch.zeros(6 * L + 2)
    for l in range(L):
        s7 = _in_order([img[l * B + b] for b in range(B)])
        losses[6 * l:6 * l + 6] = torch.stack([s7[0] / s7[1], s7[5] / nm, s7[6] / nm, s7[2] / matched, s7[3] / matched, s7[4] / matched])
    if case.pixel:
        up = _upsample(x["pixc"].flatten(0, 1), H, W, plant).view(B, 2, H, W)
        d = up - x["tpixel"]
        dist = d.pow(2).sum(1).sqrt()
        losses[6 * L] = _in_order([dist[b, s * k * BAND:s * (k + 1) * BAND].sum() for b in range(B) for k in range(nbands)]) / (f(float(B)) * (H * W))
        kk = torch.where(dist > 0, 1 / dist, torch.zeros(()))[:, None] * d
        for gr, g in zip(grads, x["gs"]):
            scale = g[6 * L] / (B * (h * w if plant == "centre_map_scale_hw" else H * W))
            gr["d_pixel_centers"] = scale * torch.einsum("Yy,bcYX,Xx->bcyx", wy, kk, wx)
    losses[6 * L + 1] = _in_order(list(qpart)) / B
    out.update(losses=losses, grads=grads)
    return out

