"""Seeded inputs of the plane criterion tests (float64 on the CPU; the tests cast).  Targets: n planes that tile most of the image (a
nearest-seed partition with a background band), gt parameters facing the camera, a depth map that satisfies the gt planes where a plane
lies - so the Q loss has a valid region - except in the images listed in `no_valid`, whose depth is doubled (no valid pixel)."""
import torch

# name: (L, B, nq, h, w, s, n per batch element, images without a valid Q region, seed)
CASES = {
    "border_s4": (3, 2, 7, 6, 8, 4, [3, 5], [1], 11),
    "s1": (1, 2, 7, 6, 8, 1, [4, 2], [], 12),
    "s2": (2, 2, 7, 6, 8, 2, [4, 6], [0], 13),
    "square50": (1, 1, 50, 6, 8, 4, [50], [], 14),
    "q128": (1, 1, 128, 6, 8, 4, [50], [], 15),
    "ragged": (3, 3, 7, 6, 8, 4, [1, 3, 5], [2], 16),
    "real": (1, 1, 50, 120, 160, 4, [12], [], 17),
}
GOLDEN_CASES = ("border_s4", "s1", "s2", "ragged")          # the small ones: pinned to the reference in tests/golden/


def make(name):
    L, B, nq, h, w, s, n, no_valid, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    H, W, nmax = s * h, s * w, max(n)
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=f64)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=f64)

    def layer(with_pixel):
        o = {"pred_logits": rn(B, nq, 2), "pred_mask_logits": 2.0 * rn(B, nq, h, w), "pred_centers": r(B, nq, 2),
             "pred_params": torch.nn.functional.normalize(rn(B, nq, 3) * 0.4 + torch.tensor([0.0, 0.0, 1.0], dtype=f64), dim=-1) * (1.0 + 2.0 * r(B, nq, 1))}
        if with_pixel:
            o["pixel_centers"] = r(B, 2, h, w)
        return o
    outputs = layer(True)
    if L > 1:
        outputs["aux_outputs"] = [layer(False) for _ in range(L - 1)]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=f64), torch.arange(W, dtype=f64), indexing="ij")
    masks = torch.zeros(B, nmax, H, W, dtype=torch.uint8)
    params = torch.zeros(B, nmax, 3, dtype=f64)
    depth = torch.ones(B, H, W, dtype=f64)
    kinv = torch.stack([xs / W - 0.5, ys / H - 0.5, torch.ones_like(xs)])[None].repeat(B, 1, 1, 1)
    for b in range(B):
        seeds = torch.stack([r(n[b]) * H, r(n[b]) * W], 1)
        d2 = (ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2
        own = d2.argmin(0)
        own[:, : max(W // 8, 1)] = -1                                            # a band that belongs to no plane
        for j in range(n[b]):
            masks[b, j] = (own == j).to(torch.uint8)
            if masks[b, j].sum() == 0:                                           # every plane owns at least one pixel
                masks[b, j, int(seeds[j, 0]) % H, W - 1 - j % (W // 2)] = 1
        nrm = torch.nn.functional.normalize(torch.cat([0.3 * rn(n[b], 2), torch.ones(n[b], 1, dtype=f64)], 1), dim=-1)
        off = 1.0 + 2.0 * r(n[b], 1)
        params[b, : n[b]] = nrm * off
        for j in range(n[b]):
            inv = ((nrm[j] / off[j])[:, None, None] * kinv[b]).sum(0)            # g' . k_inv_dot_xy1 > 0
            on = masks[b, j] > 0
            depth[b][on] = (1.0 / inv)[on] * (1.0 + 0.4 * (r(H, W)[on] - 0.5) * (r(H, W)[on] < 0.3))
        if b in no_valid:
            depth[b] *= 2.0
    targets = {"masks": masks, "n": list(n), "plane_params": params, "depth": depth, "k_inv_dot_xy1": kinv}
    return outputs, targets


def cast(outputs, targets, dtype, device="cpu"):
    f = lambda t: t.to(device=device, dtype=dtype) if torch.is_tensor(t) and t.is_floating_point() else (t.to(device) if torch.is_tensor(t) else t)
    o = {k: f(v) for k, v in outputs.items() if k != "aux_outputs"}
    if "aux_outputs" in outputs:
        o["aux_outputs"] = [{k: f(v) for k, v in a.items()} for a in outputs["aux_outputs"]]
    return o, {k: f(v) for k, v in targets.items()}
