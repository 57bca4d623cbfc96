"""Times the training-target kernels (csrc/train_targets.hip, nopesac_amd/targets.py) on 64 views of 480 x 640 with 20 and with 50 planes
per view and writes profiles/train_targets.txt:

    python scripts/train_targets_bench.py [--out profiles/train_targets.txt] [--views 64]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tt -- python scripts/train_targets_bench.py --launches-only
    python scripts/train_targets_bench.py --stats DIR/.../tt_kernel_stats.csv      # adds each launch's own time

Every figure is the time of ONE call between two device events, the median of 11 after 3 warm-up calls.  label_targets is three
launches (partial sums, centres, masks); its bytes are the label map read twice (4 bytes per pixel each), nmax mask bytes and 8
centre-map bytes per pixel written, and the share is those bytes over the call's time against the 6.3 TB/s float4-copy rate of an
MI355X (the figure of scripts/augment_bench.py).  With --stats the mask launch's own time from the profiler's kernel trace (a run of
its own: --launches-only makes the calls at 50 planes and times nothing) gives the mask launch's bytes - one read of the labels, the masks, the
centre map - over ITS time.  Last, the whole TargetMapper.view_targets from host records (upload, ids, the host sync, masks, depth,
coordinate map) against a torch restatement of the reference's prepare_targets on the same device from the same host arrays (per
view: upload, torch.unique, ids == map, the f32 centre sums, the coordinate map by matmul).  A run without a GPU fails: nothing here
is a CPU measurement."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12                     # bytes / s, float4 copy on an MI355X (profiles/model_optimizer.txt)
H, W = 480, 640
REPS, WARM = 11, 3


def label_map(planes: int, seed: int) -> np.ndarray:
    """a nearest-seed partition into `planes` regions with the labels 1 .. planes and a band of 0 at the left"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    sy, sx = rng.integers(0, H, planes), rng.integers(W // 8, W, planes)
    own = ((ys[None] - sy[:, None, None]) ** 2 + (xs[None] - sx[:, None, None]) ** 2).argmin(0) + 1
    own[:, :W // 8] = 0
    for j in range(1, planes + 1):                                     # every label owns a pixel
        if not (own == j).any():
            own[sy[j - 1], sx[j - 1]] = j
    return own.astype(np.int32)


def torch_prepare_targets(records, device, xy_map, default_k):
    """the reference's prepare_targets (siamese_planeTR.py:475-532) restated in torch, per view as it runs there"""
    import torch
    out = []
    for r in records:
        sem = torch.from_numpy(r["semantic_map"]).to(device)
        ids = torch.unique(sem)
        if ids[0] == 0:
            ids = ids[1:]
        n = min(len(ids), 50)
        assert len(ids) == len(r["annotations"])
        masks = ids[:n].reshape(-1, 1, 1) == sem.unsqueeze(0)
        xy = xy_map.unsqueeze(0) * masks.unsqueeze(1).to(torch.float32)
        centers = xy.flatten(2, 3).sum(-1) / masks.unsqueeze(1).flatten(2, 3).sum(-1)
        pixel = (centers.unsqueeze(-1).unsqueeze(-1) * masks.unsqueeze(1).to(torch.float32)).sum(0)
        out.append({"masks": masks, "plane_centers": centers, "pixel_centers": pixel, "depth": torch.from_numpy(r["depth"]).to(device),
                    "plane_params": torch.tensor([a["plane"] for a in r["annotations"][:n]], device=device), "k_inv_dot_xy1": default_k})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_targets.txt"))
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv of a --launches-only run")
    ap.add_argument("--launches-only", action="store_true", help="make the label_targets calls (for a kernel trace) and time nothing")
    a = ap.parse_args()
    import torch
    from nopesac_amd import ops
    from nopesac_amd.targets import TargetMapper
    if not torch.cuda.is_available():
        raise SystemExit("train_targets_bench: no GPU - nothing is timed without one")
    dev = torch.device("cuda:0")
    B = a.views
    maps = {p: np.stack([label_map(p, 1000 * p + k) for k in range(4)])[np.arange(B) % 4] for p in (20, 50)}
    labels = {p: torch.from_numpy(np.ascontiguousarray(m)).to(dev) for p, m in maps.items()}
    found = {p: ops.label_ids(labels[p], 50) for p in labels}
    if a.launches_only:
        for _ in range(WARM + REPS):
            ops.label_targets(labels[50], found[50][0], found[50][2], 50)
        torch.cuda.synchronize()
        return

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[REPS // 2], ts[0], ts[-1]

    HW = H * W
    lines = ["training targets, %d views of %d x %d, %s" % (B, H, W, torch.cuda.get_device_name(0)),
             "one call between two device events, median (min .. max) of %d after %d warm-up calls; share = bytes over time against the %.1f TB/s float4-copy rate"
             % (REPS, WARM, COPY_RATE / 1e12), ""]

    def row(name, t, nbytes=None):
        s = "  %-44s %8.4f (%7.4f .. %7.4f) ms" % (name, t[0], t[1], t[2])
        if nbytes:
            s += "   %8.2f MB   %5.1f %% of the copy rate" % (nbytes / 1e6, 100.0 * nbytes / (t[0] * 1e-3) / COPY_RATE)
        lines.append(s)

    mask_bytes = {}
    for p in (20, 50):
        assert found[p][2].cpu().tolist() == [p] * B and not bool(found[p][3].any())
        row("label_ids, %d planes (1 launch)" % p, timed(lambda: ops.label_ids(labels[p], 50)), B * HW * 4)
        outs = tuple(torch.empty(s, device=dev, dtype=d) for s, d in (((B, p, H, W), torch.uint8), ((B, p, 2), torch.float32), ((B, 2, H, W), torch.float32)))
        row("label_targets, %d planes (3 launches)" % p, timed(lambda: ops.label_targets(labels[p], found[p][0], found[p][2], p, out=outs)), B * HW * (8 + p + 8))
        mask_bytes[p] = B * HW * (4 + p + 8)
    # the polygon / RLE route: 50 masks per view
    masks50 = ops.label_targets(labels[50], found[50][0], found[50][2], 50)[0]
    n_host = torch.full((B,), 50, dtype=torch.int32)
    n_dev = n_host.to(dev)
    words = (HW + 31) // 32
    packed = torch.randint(-2**31, 2**31 - 1, (B * 50, words), device=dev, dtype=torch.int32)
    offsets = torch.arange(0, B * 50 + 1, 50, device=dev, dtype=torch.int64)
    out_m = torch.empty(B, 50, H, W, device=dev, dtype=torch.uint8)
    row("bits_to_masks, 50 masks per view", timed(lambda: ops.bits_to_masks(packed, offsets, 50, H, W, out=out_m)), B * 50 * (words * 4 + HW))
    row("plane_targets, 50 byte masks per view (2 launches)", timed(lambda: ops.plane_targets(masks50, n_host, n_dev)), B * HW * (2 * 50 + 8))
    d16 = torch.from_numpy(np.random.default_rng(1).integers(0, 65536, (B, H, W)).astype(np.uint16)).to(dev)
    out_d = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    row("depth_from_u16", timed(lambda: ops.depth_from_u16(d16, out=out_d)), B * HW * 6)
    kinv = torch.eye(3, device=dev).reshape(1, 9).repeat(B, 1).contiguous()
    out_k = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    row("coordinate_map", timed(lambda: ops.coordinate_map(kinv, H, W, out=out_k)), B * HW * 12)
    if a.stats:
        lines += ["", "the launches of label_targets at 50 planes by themselves (rocprofv3 --kernel-trace --stats, a run of its own, %d calls;" % (WARM + REPS),
                  "the mask launch's bytes: one read of the labels, the masks, the centre map = %.1f MB):" % (mask_bytes[50] / 1e6)]
        with open(a.stats) as f:
            for r in csv.DictReader(f):
                if "tt_label_" in r["Name"]:
                    avg = float(r["AverageNs"])
                    s = "  %-34s %4d calls   average %9.1f us (min %.1f, max %.1f)" % (r["Name"].split("(")[0].replace("nps::", ""), int(r["Calls"]), avg / 1e3,
                                                                                       float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
                    if "tt_label_masks" in r["Name"]:
                        s += "   %5.1f %% of the copy rate" % (100.0 * mask_bytes[50] / (avg * 1e-9) / COPY_RATE)
                    lines.append(s)
    # the whole mapper from host records against the reference's route in torch
    lines += ["", "whole route from host records (uploads and the host sync included), %d views:" % B]
    tm = TargetMapper(dev)
    depth = np.full((H, W), 2.0, np.float32)
    xy = np.stack(np.meshgrid(np.arange(W) / W, np.arange(H) / H)).astype(np.float32)
    xy_map = torch.from_numpy(xy).to(dev)
    kinv_d = torch.tensor([[517.97, 0, 320], [0, 517.97, 240], [0, 0, 1]]).inverse().to(dev)
    x = (torch.arange(W, dtype=torch.float32) / W * 640).to(dev).repeat(H, 1)
    y = (torch.arange(H, dtype=torch.float32).view(H, 1) / H * 480).to(dev).repeat(1, W)
    default_k = torch.matmul(kinv_d, torch.stack((x, y, torch.ones_like(x))).view(3, -1)).reshape(3, H, W)
    for p in (20, 50):
        recs = [{"semantic_map": maps[p][b], "depth": depth, "annotations": [{"plane": [0.0, 1.0, 2.0], "category_id": 0}] * p} for b in range(B)]
        mine = tm.view_targets(recs)
        theirs = torch_prepare_targets(recs, dev, xy_map, default_k)
        same = all(torch.equal(mine["masks"][b].bool(), theirs[b]["masks"]) for b in range(B))
        gap = max(float((mine["plane_centers"][b] - theirs[b]["plane_centers"]).abs().max()) for b in range(B))
        row("TargetMapper.view_targets, %d planes" % p, timed(lambda: tm.view_targets(recs)))
        row("torch restatement of prepare_targets, %d planes" % p, timed(lambda: torch_prepare_targets(recs, dev, xy_map, default_k)))
        lines.append("      masks equal: %s; largest centre difference %.3g (the restatement sums in f32)" % (same, gap))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
