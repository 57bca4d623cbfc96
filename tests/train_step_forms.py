"""View groups of the plane head's training path as data: the cases of the grouped criterion (csrc/plane_criterion.hip, `groups`) and of
the grouped pyramid BatchNorm (csrc/pyramid_train.hip, the bn_train_groups entries), the slicing of a batch into its groups, and the
numpy restatement of the criterion's group normalisers.  tests/test_plane_groups_forms_gpu.py holds the kernels to it: a group's
results must have the BITS of an ungrouped call on the group's images alone, and that ungrouped call is existing code, held to float64
by tests/test_plane_criterion_forms_gpu.py and tests/test_plane_pyramid_forms_gpu.py.  tests/test_plane_groups_forms_cpu.py proves the
restatement against the float64 criterion of tests/plane_criterion_ref.py run per group.  Imports without a GPU."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import plane_criterion_forms as P
from tests import plane_criterion_ref as R

F32, F64 = torch.float32, torch.float64

# ===================================================================================================================== criterion cases
# nq = 20, nmax = 8, mask logits 6 x 8 against 24 x 32 targets (s = 4: one band of 6 rows, 48 low-resolution pixels = one chunk).  n per
# image: a group of one-plane images, a group at the maximum (nmax = 8), a mixed one; no_valid: every image of ONE group has no valid
# pixel of loss_q (that group's loss_q is 0 and its d_params carry no Q term), the other groups do.
NQ, NMAX, H_LO, W_LO, SCALE = 20, 8, 6, 8, 4


def _case(name, L, B, n, no_valid, match, seed):
    return P._c(name, L, B, NQ, H_LO, W_LO, SCALE, n, NMAX, match, pixel=True, num_masks=0.0, no_valid=no_valid, seed=seed)


#                       name        L  B  n                   no_valid  match        seed    groups
CRITERION_CASES = {c.name: (c, G) for c, G in (
    (_case("g2_L1", 1, 4, [1, 1, 8, 8], [2, 3], "perlayer", 7001), 2),
    (_case("g2_L3", 3, 4, [8, 8, 1, 1], [0, 1], "perlayer", 7002), 2),
    (_case("g3_L1", 1, 6, [1, 1, 8, 8, 3, 5], [4, 5], "reversed", 7003), 3),
    (_case("g3_L3", 3, 6, [3, 5, 1, 1, 8, 8], [2, 3], "perlayer", 7004), 3),
)}
NUM_MASKS = ("default", "scalar", "per_group")          # the group's sum of n; one override for every group; one override per group


def num_masks_of(kind, G):
    """(what the grouped call takes, what the ungrouped call on group g takes)"""
    if kind == "default":
        return 0.0, [0.0] * G
    if kind == "scalar":
        return 2.5, [2.5] * G
    per = [1.5 + 2.25 * g for g in range(G)]
    return per, per


@functools.lru_cache(maxsize=None)
def criterion_inputs(name):
    """Every tensor the loss and gradient entries read, f32 / uint8 / int32 on the CPU, pixel-minor, [L][B] stacking - the generator of
    tests/plane_criterion_forms.py::inputs without its planted ties (nothing here is judged against a tolerance)."""
    case, G = CRITERION_CASES[name]
    g = torch.Generator().manual_seed(case.seed)
    L, B, nq, h, w, s, nmax = case.L, case.B, case.nq, case.h, case.w, case.s, case.nmax
    H, W, LB = s * h, s * w, L * B
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=F64)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    z = torch.tensor([0.0, 0.0, 1.0], dtype=F64)
    x = {"logits": rn(LB, nq, 2), "mlog": 2.0 * rn(LB, nq, h, w), "centers": r(LB, nq, 2),
         "params": F.normalize(rn(LB, nq, 3) * 0.4 + z, dim=-1) * (1.0 + 2.0 * r(LB, nq, 1)), "pixc": r(B, 2, h, w)}
    masks = torch.zeros(B, nmax, H, W, dtype=torch.uint8)
    tparams = torch.zeros(B, nmax, 3, dtype=F64)
    depth = torch.ones(B, H, W, dtype=F64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    kinv = torch.stack([xs / W - 0.5, ys / H - 0.5, torch.ones_like(xs)])[None].repeat(B, 1, 1, 1)
    for b in range(B):
        for j in range(case.n[b]):
            masks[b, j] = P._plane_mask(j, H, W, g)
        nrm = F.normalize(torch.cat([0.3 * rn(case.n[b], 2), torch.ones(case.n[b], 1, dtype=F64)], 1), dim=-1)
        off = 1.0 + 2.0 * r(case.n[b], 1)
        tparams[b, :case.n[b]] = nrm * off
        inv = ((nrm[0] / off[0])[:, None, None] * kinv[b]).sum(0)
        noise = torch.where(r(H, W) < 0.3, 0.4 * torch.ones(H, W, dtype=F64), 0.001 + 0.149 * r(H, W)) * torch.where(r(H, W) < 0.5, -1.0, 1.0)
        depth[b] = (1.0 / inv) * (1.0 + noise) * (3.0 if b in case.no_valid else 1.0)
    tcenters, tpixel = R.prepare_targets(masks, list(case.n), F64)
    x.update(tparams=tparams, tcenters=tcenters, tpixel=tpixel, depth=depth, kinv=kinv)
    x = {k: v.to(F32) for k, v in x.items()}
    mq, mg = P.make_match(case, g)
    x.update(masks=masks, match_q=mq, match_gt=mg, gs=P.cotangents(case, g))
    return x


def group_images(case, G, grp):
    """-> (batch elements of group grp, their rows in the [L][B] stacking, layer-major: the [L][B / G] stacking of the group alone)"""
    Bg = case.B // G
    bs = list(range(grp * Bg, (grp + 1) * Bg))
    return bs, [l * case.B + b for l in range(case.L) for b in bs]


PER_IMAGE = ("logits", "mlog", "centers", "params", "match_q", "match_gt")        # [L B, ...]
PER_BATCH = ("pixc", "masks", "tparams", "tcenters", "tpixel", "depth", "kinv")    # [B, ...]


def group_slice(x, case, G, grp):
    """The inputs of an ungrouped call on group grp alone, and its case."""
    bs, rows = group_images(case, G, grp)
    sub = {k: x[k][rows].contiguous() for k in PER_IMAGE}
    sub.update({k: x[k][bs].contiguous() for k in PER_BATCH})
    sub["gs"] = x["gs"]
    return sub, case._replace(B=len(bs), n=tuple(case.n[b] for b in bs), no_valid=tuple(b - bs[0] for b in case.no_valid if b in bs))


def group_cotangents(x, G, launch):
    """g_losses [G][6 L + 2] of backward launch `launch`: every group its own vector of the case's cotangents, so that a kernel reading
    another group's row shows"""
    return torch.stack([x["gs"][(launch + grp) % len(x["gs"])] for grp in range(G)])


# ===================================================================================================================== the float64 criterion per group
def reference_losses(x, case, dtype=F64, num_masks=None):
    """tests/plane_criterion_ref.py on the values of x with x's match -> the loss vector [6 L + 2] in the kernels' order"""
    L, B = case.L, case.B
    t = {k: x[k].to(dtype) for k in P.FLOAT_INPUTS}

    def layer(l):
        o = {"pred_logits": t["logits"][l * B:(l + 1) * B], "pred_mask_logits": t["mlog"][l * B:(l + 1) * B],
             "pred_centers": t["centers"][l * B:(l + 1) * B], "pred_params": t["params"][l * B:(l + 1) * B]}
        if l == 0 and case.pixel:
            o["pixel_centers"] = t["pixc"]
        return o
    outputs = layer(0)
    if L > 1:
        outputs["aux_outputs"] = [layer(l) for l in range(1, L)]
    targets = {"masks": x["masks"], "n": list(case.n), "plane_params": t["tparams"], "depth": t["depth"], "k_inv_dot_xy1": t["kinv"]}
    losses, _, _ = R.criterion(outputs, targets, P.WTS, indices=P._indices(x["match_q"], case), num_masks=num_masks or None,
                               prepared=(t["tcenters"], t["tpixel"]))
    return P.loss_vector(losses, L, dtype).numpy()


# ===================================================================================================================== the group normalisers, in numpy
def image_sums(x, case):
    """What the loss entry keeps per image before any batch-wide normaliser is applied (pc_image_kernel's row, the centre-map partials,
    the Q partials), from the float64 criterion run on ONE image at a time: with B = 1 and num_masks = 1 every normaliser of the
    criterion is that image's own, so multiplying it back out leaves the image's sum.
    -> per layer and batch element (ce numerator, ce weight sum, focal, dice, centre distance, param L1, 1 - cos) [L, B, 7], and per
    batch element (centre-map mean, loss_q term) [B, 2]"""
    L, B, nq = case.L, case.B, case.nq
    eos = float(torch.tensor(P.WTS["eos_coef"], dtype=F32))          # the reference's empty_weight buffer is made in float32
    img, last = np.zeros((L, B, 7)), np.zeros((B, 2))
    for b in range(B):
        sub, one = group_slice(x, case, B, b)
        v = reference_losses(sub, one, F64, num_masks=1.0)
        n = case.n[b]
        den = n + eos * (nq - n)
        for l in range(L):
            ce, mask, dice, cins, l1, cos = v[6 * l:6 * l + 6]
            img[l, b] = (ce * den, den, mask, dice, cins * n, l1 * n, cos * n)
        last[b] = v[6 * L], v[6 * L + 1]
    return img, last


def group_losses(img, last, n, G, num_masks=None):
    """The group normalisers as the kernels apply them (csrc/plane_criterion.hip, pc_final_kernel): per group g of B / G consecutive
    images  num_masks_g = the override, else max(sum of the group's n, 1);  matched_g = the group's sum of n;  loss_ce = the group's
    numerators over the group's weight sums;  loss_mask, loss_dice over num_masks_g;  loss_center_ins, loss_param_l1, loss_param_cos
    over matched_g;  loss_center_pixel and loss_q = the mean of the group's images over B / G.  -> [G][6 L + 2]"""
    L, B = img.shape[:2]
    Bg = B // G
    out = np.zeros((G, 6 * L + 2))
    for g in range(G):
        sl = slice(g * Bg, (g + 1) * Bg)
        matched = float(sum(n[sl]))
        nm = float(num_masks[g]) if num_masks is not None and num_masks[g] > 0 else max(matched, 1.0)
        for l in range(L):
            s = img[l, sl].sum(0)
            out[g, 6 * l:6 * l + 6] = (s[0] / s[1], s[2] / nm, s[3] / nm, s[4] / matched, s[5] / matched, s[6] / matched)
        out[g, 6 * L] = last[sl, 0].sum() / Bg
        out[g, 6 * L + 1] = last[sl, 1].sum() / Bg
    return out


# ===================================================================================================================== pyramid BatchNorm cases
# C at a partial channel block, one full wave of quads and the pyramid's width; rows per group around the kernels' block of
# NPS_BN_TRAIN_RPS = 256 rows (2: the least a BatchNorm takes; 255 / 256 / 257: one block short, full, one row into a second) and the
# images of an NHWC map; G = 2, 3.  Plain (matrix / NHWC) and upsampled sources, ReLU and none, with and without the addend.
RPS = 256
BN_CHANNELS = (4, 64, 256)
BN_GROUPS = (2, 3)
BN_ROWS = (2, 255, 256, 257)
BN_IMAGES = (2, 3, 4)                                  # an NHWC group of 2 images of 3 x 4: up2 gives 2 x 6 x 8 = 96 rows per group
EPS, MOMENTUM = 1e-5, 0.1


def bn_cases():
    """(form, G, rows per group or None, C, relu, addend, tag): every C x rows x G of the plain matrix form, flags alternating; the NHWC
    geometry in the plain and the upsampled form for every C x G, with every flag pair on C = 64.  tag "slice": the source is a channel
    slice of a buffer 8 channels wider (channel stride C + 8, the first channel 16 bytes into a row), as the existing pyramid sweep has it"""
    out, k = [], 0
    for C in BN_CHANNELS:
        for G in BN_GROUPS:
            for rows in BN_ROWS:
                out.append(("plain", G, rows, C, k % 2 == 0, k % 3 == 0, "slice" if k % 4 == 1 else "base"))
                k += 1
            for form in ("nhwc", "up"):
                flags = ((True, True), (True, False), (False, True), (False, False)) if C == 64 else (((k % 2 == 0), (k % 3 != 0)),)
                for relu, addend in flags:
                    out.append((form, G, None, C, relu, addend, "slice" if k % 2 == 0 else "base"))
                    k += 1
    return out


def bn_id(key):
    form, G, rows, C, relu, addend, tag = key
    return "%s-G%d-%s-C%d-%s-%s-%s" % (form, G, "img" if rows is None else rows, C, "relu" if relu else "lin", "add" if addend else "noadd", tag)


@functools.lru_cache(maxsize=None)
def bn_inputs(key):
    """src (matrix [G rows, C] or NHWC [G 2, 3, 4, C]), cotangent g and addend in the output's shape, gamma, beta, running buffers; a
    different offset and spread per group, so that statistics taken over the wrong rows show"""
    form, G, rows, C, relu, addend, tag = key
    gen = torch.Generator().manual_seed(9000 + 100000 * ("plain", "nhwc", "up").index(form) + 10000 * G + 10 * (rows or 0) + 7 * C)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    if form == "plain":
        shape, out_shape = (G * rows, C), (G * rows, C)
    else:
        B, H, W = G * BN_IMAGES[0], BN_IMAGES[1], BN_IMAGES[2]
        shape = (B, H, W, C)
        out_shape = (B, 2 * H, 2 * W, C) if form == "up" else shape
    src = rn(*shape)
    per = shape[0] // G
    for grp in range(G):
        src[grp * per:(grp + 1) * per] = src[grp * per:(grp + 1) * per] * (1.0 + 0.5 * grp) + (0.75 * grp - 0.5)
    buf = rn(*shape[:-1], C + 8)
    buf[..., 4:4 + C] = src
    return {"src": src, "buf": buf, "tag": tag, "g": rn(*out_shape), "addend": rn(*out_shape) if addend else None, "gamma": 1.0 + 0.3 * rn(C), "beta": 0.2 * rn(C),
            "run_mean": 0.1 * rn(C), "run_var": 1.0 + 0.2 * torch.rand(C, generator=gen), "up": form == "up", "relu": relu, "G": G, "C": C,
            "out_shape": out_shape}


# ===================================================================================================================== dataset pairs for the step
def pair_entries(pairs, H, W, image_dir, seed=0):
    """`pairs` dataset dicts in the form TargetMapper.pair_targets and PairMapper.map_batch take, with PNG files written to image_dir:
    per view a label map partitioned into 4 .. 7 planes (tests/train_targets_forms.partition), a depth map, plane annotations; a few
    correspondences and a relative pose per pair.  Seeded; scripts/train_step_bench.py and scripts/training_digest.py use it."""
    import os

    from PIL import Image

    from tests import train_targets_forms as TF
    rng = np.random.default_rng(seed)
    out = []
    for b in range(pairs):
        e = {}
        counts = (4 + b % 4, 4 + (b + 2) % 4)
        for v, k in zip("01", counts):
            planes = rng.standard_normal((k, 3))
            planes = planes / np.linalg.norm(planes, axis=1, keepdims=True) * (1.0 + 2.0 * rng.random((k, 1)))
            coarse = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
            name = os.path.join(image_dir, "pair%d_%s.png" % (b, v))
            Image.fromarray((coarse.astype(np.int32) + rng.integers(-20, 21, (H, W, 3))).clip(0, 255).astype(np.uint8)).save(name)
            e[v] = {"image_id": "p%d_%s" % (b, v), "file_name": name, "semantic_map": TF.partition(H, W, list(range(2, 2 + k)), seed + 2 * b + int(v)),
                    "depth": np.full((H, W), 2.0, np.float32) + rng.random((H, W)).astype(np.float32),
                    "annotations": [{"plane": planes[j].tolist(), "category_id": 0} for j in range(k)]}
        e["gt_corrs"] = [(j, (j + 1) % counts[1]) for j in range(min(counts) - 1)]
        q = rng.standard_normal(4)
        q[0] = abs(q[0]) + 1.0
        e["rel_pose"] = {"position": (0.3 * rng.standard_normal(3)).tolist(), "rotation": (q / np.linalg.norm(q)).tolist()}
        out.append(e)
    return out
