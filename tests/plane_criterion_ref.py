"""Plain-torch restatement of the plane head's set criterion (reference: modeling/matcher.py HungarianMatcher, modeling/criterion.py
SetCriterion, siamese_planeTR.py prepare_targets / process_plane_corr_matrix), dtype-generic and autograd-able: the float64 yardstick of
tests/test_plane_criterion_gpu.py and, pinned to the reference itself by tests/golden/H_plane_criterion_*.npz, of
tests/test_plane_criterion_cpu.py.  Tensors, not lists of dicts: outputs = {"pred_logits" [B, nq, 2], "pred_mask_logits" [B, nq, h, w],
"pred_centers" [B, nq, 2], "pred_params" [B, nq, 3], "pixel_centers" [B, 2, h, w], "aux_outputs": [the first four, ...]}; targets =
{"masks" uint8 [B, nmax, H, W], "n" list, "plane_params" [B, nmax, 3], "depth" [B, H, W], "k_inv_dot_xy1" [B, 3, H, W]}."""
import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_WEIGHTS = dict(cost_class=1.0, cost_mask=20.0, cost_dice=1.0, cost_center=0.5, cost_param=0.5, cost_offset=0.01, cost_angle=0.0028,
                       eos_coef=0.1)
LOSS_NAMES = ("loss_ce", "loss_mask", "loss_dice", "loss_center_ins", "loss_param_l1", "loss_param_cos")


def prepare_targets(masks, n, dtype):
    """plane_centers [B, nmax, 2] (0 beyond n[b]) and pixel_centers [B, 2, H, W]"""
    B, nmax, H, W = masks.shape
    xy = torch.stack([(torch.arange(W, dtype=dtype) / W).view(1, W).expand(H, W), (torch.arange(H, dtype=dtype) / H).view(H, 1).expand(H, W)])
    centers = torch.zeros(B, nmax, 2, dtype=dtype)
    pixel = torch.zeros(B, 2, H, W, dtype=dtype)
    for b in range(B):
        m = masks[b, :n[b]].to(dtype)
        c = (xy[None] * m[:, None]).flatten(2).sum(-1) / m[:, None].flatten(2).sum(-1)
        centers[b, :n[b]] = c
        pixel[b] = (c[:, :, None, None] * m[:, None]).sum(0)
    return centers, pixel


def cost_matrix(logits, mask_logits, centers, params, tgt_masks, tgt_centers, tgt_params, wts):
    """One image: [nq, n] (matcher.py:98-163; every target is of class 0)"""
    prob = logits.softmax(-1)
    cost_class = -prob[:, :1].expand(-1, tgt_masks.shape[0])
    tm = F.interpolate(tgt_masks.to(mask_logits.dtype)[:, None], size=mask_logits.shape[-2:], mode="nearest")[:, 0].flatten(1)
    x = mask_logits.flatten(1)
    hw = x.shape[1]
    p = x.sigmoid()
    fpos = 0.25 * (1 - p) ** 2 * F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    fneg = 0.75 * p ** 2 * F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    cost_mask = (fpos @ tm.T + fneg @ (1 - tm).T) / hw
    cost_dice = 1 - (2 * (p @ tm.T) + 1) / (p.sum(-1)[:, None] + tm.sum(-1)[None] + 1)
    cost_center = torch.cdist(centers, tgt_centers, p=2)
    cost_param = torch.cdist(params, tgt_params, p=1)
    cos = torch.clamp(F.normalize(params, dim=-1) @ F.normalize(tgt_params, dim=-1).T, min=-0.999999, max=0.999999)
    angle = torch.acos(cos) * 180.0 / np.pi
    offset = torch.cdist(params.norm(dim=-1, keepdim=True), tgt_params.norm(dim=-1, keepdim=True), p=1)
    return (wts["cost_mask"] * cost_mask + wts["cost_class"] * cost_class + wts["cost_dice"] * cost_dice + wts["cost_center"] * cost_center
            + wts["cost_param"] * cost_param + wts["cost_offset"] * offset + wts["cost_angle"] * angle)


def layer_costs(out, targets, tgt_centers, wts):
    n = targets["n"]
    return [cost_matrix(out["pred_logits"][b], out["pred_mask_logits"][b], out["pred_centers"][b], out["pred_params"][b],
                        targets["masks"][b, :n[b]], tgt_centers[b, :n[b]], targets["plane_params"][b, :n[b]].to(out["pred_logits"].dtype), wts)
            for b in range(len(n))]


def hungarian(costs):
    from scipy.optimize import linear_sum_assignment
    out = []
    for C in costs:
        i, j = linear_sum_assignment(C.detach().cpu().numpy())
        out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
    return out


def _layer_losses(out, targets, tgt_centers, tgt_pixel, indices, wts, num_masks, aux):
    dtype = out["pred_logits"].dtype
    n, masks = targets["n"], targets["masks"]
    B, nq = out["pred_logits"].shape[:2]
    bi = torch.cat([torch.full_like(s, b) for b, (s, _) in enumerate(indices)])
    si = torch.cat([s for s, _ in indices])
    losses = {}
    tc = torch.full((B, nq), 1, dtype=torch.int64)
    tc[bi, si] = 0
    empty_weight = torch.tensor([1.0, wts["eos_coef"]], dtype=torch.float32).to(dtype)       # the reference's buffer is made in float32
    losses["loss_ce"] = F.cross_entropy(out["pred_logits"].transpose(1, 2), tc, empty_weight)
    tm = torch.cat([masks[b, j] for b, (_, j) in enumerate(indices)]).to(dtype)
    sm = F.interpolate(out["pred_mask_logits"][bi, si][:, None], size=tm.shape[-2:], mode="bilinear", align_corners=False)[:, 0].flatten(1)
    tm = tm.flatten(1)
    p = sm.sigmoid()
    ce = F.binary_cross_entropy_with_logits(sm, tm, reduction="none")
    pt = p * tm + (1 - p) * (1 - tm)
    losses["loss_mask"] = ((0.25 * tm + 0.75 * (1 - tm)) * ce * (1 - pt) ** 2).mean(1).sum() / num_masks
    losses["loss_dice"] = (1 - (2 * (p * tm).sum(-1) + 1) / (p.sum(-1) + tm.sum(-1) + 1)).sum() / num_masks
    tcen = torch.cat([tgt_centers[b, j] for b, (_, j) in enumerate(indices)])
    losses["loss_center_ins"] = torch.norm(torch.abs(tcen - out["pred_centers"][bi, si]), dim=-1).mean()
    if not aux and "pixel_centers" in out:
        up = F.interpolate(out["pixel_centers"], size=tgt_pixel.shape[-2:], mode="bilinear", align_corners=False)
        losses["loss_center_pixel"] = torch.norm(torch.abs(tgt_pixel - up), dim=1, keepdim=True).mean()
    tp = torch.cat([targets["plane_params"][b, j] for b, (_, j) in enumerate(indices)]).to(dtype)
    sp = out["pred_params"][bi, si]
    losses["loss_param_l1"] = torch.abs(tp - sp).sum(1).mean()
    losses["loss_param_cos"] = (1 - F.cosine_similarity(sp, tp, dim=1)).mean()
    if aux:
        return losses
    loss_q = 0.0
    for b in range(B):
        s, j = indices[b]
        pts = (targets["k_inv_dot_xy1"][b].to(dtype) * targets["depth"][b].to(dtype)[None]).reshape(3, -1)
        gm = (masks[b, j] > 0).to(dtype)
        H, W = gm.shape[-2:]
        gp = targets["plane_params"][b, j].to(dtype)
        go = gp.norm(dim=-1, keepdim=True)
        gd = (torch.abs((gp / go / go) @ pts - 1.0).reshape(-1, H, W) * gm).sum(0)
        valid = (gd < 0.2) & (gm.sum(0) > 0)
        if valid.sum() == 0:
            continue
        pp = out["pred_params"][b][s]
        po = pp.norm(dim=-1, keepdim=True)
        d = (torch.abs((pp / po / po) @ pts - 1.0).reshape(-1, H, W) * gm).sum(0)
        loss_q = loss_q + d[valid].mean()
    losses["loss_q"] = loss_q / B if torch.is_tensor(loss_q) else torch.zeros((), dtype=dtype)
    return losses


def criterion(outputs, targets, wts=DEFAULT_WEIGHTS, indices=None, num_masks=None, prepared=None):
    """-> (losses: the reference's names with _0, _1 for the auxiliary layers, unweighted; indices of every layer, last layer first;
    float cost matrices of every layer).  `indices` (per layer) replaces the Hungarian match, `prepared` = (plane_centers, pixel_centers)
    replaces prepare_targets (the values a kernel was handed)."""
    dtype = outputs["pred_logits"].dtype
    tgt_centers, tgt_pixel = prepare_targets(targets["masks"], targets["n"], dtype) if prepared is None else prepared
    layers = [outputs] + list(outputs.get("aux_outputs", []))
    costs = [layer_costs(o, targets, tgt_centers, wts) for o in layers]
    if indices is None:
        with torch.no_grad():
            indices = [hungarian(c) for c in costs]
    nm = float(max(sum(targets["n"]), 1)) if num_masks is None else float(num_masks)
    losses = {}
    for l, o in enumerate(layers):
        ll = _layer_losses(o, targets, tgt_centers, tgt_pixel, indices[l], wts, nm, aux=l > 0)
        losses.update({k + ("" if l == 0 else "_%d" % (l - 1)): v for k, v in ll.items()})
    return losses, indices, costs


def plane_corr_matrix(gt_corrs, idx1, idx2, nq):
    """process_plane_corr_matrix (siamese_planeTR.py:566-623): gt_corrs = per pair a list of (gt plane in view 1, in view 2); idx1 / idx2 =
    the (src, tgt) index pairs of the two views -> bool [B, nq+1, nq+1]"""
    B = len(gt_corrs)
    out = torch.zeros(B, nq + 1, nq + 1)
    g2p = []
    for idx in (idx1, idx2):
        t = torch.full((B, nq), nq, dtype=torch.int64)
        for b, (s, j) in enumerate(idx):
            t[b, j] = s
        g2p.append(t)
    for b in range(B):
        for a, c in gt_corrs[b]:
            if a < 50 and c < 50:
                out[b, g2p[0][b, a], g2p[1][b, c]] = 1
    row = 1 - out[:, :-1, :].sum(1, keepdim=True)
    col = 1 - out[:, :, :-1].sum(2, keepdim=True)
    out[:, -1:, :] = row
    out[:, :, -1:] = col
    out[:, -1, -1] = 0
    return out > 0
