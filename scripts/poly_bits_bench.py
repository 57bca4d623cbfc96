"""GT masks to bits, polygons against RLE strings (nopesac_poly_to_bits against nopesac_rle_string_runs + nopesac_rle_runs_to_bits, csrc/plane_eval.hip): 64 views x 20 masks at 480 x 640,
every mask one seeded outline of 40 to 400 vertices.  Timed: rle.polygon_bits on the polygons, and rle.decode_bits on the compressed
COCO strings of the very same masks (what the evaluators did for GT before polygons were taken).  Both calls hold their upload, their
launches and their one host sync; each is timed between two events after warm-up, median of `--reps`.  The same batch then goes through
evaluation.plane_rows (predictions = the masks' strings, GT = the polygons) for the rasteriser's share of an evaluator step.  Prints one
JSON line and writes profiles/poly_bits.txt with the numbers and the engine clock read on the device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import evaluation, ops, rle  # noqa: E402

H, W = 480, 640


def outline(rng):
    k = int(rng.integers(40, 401))
    cx, cy = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.1, 0.45, k) * H * rng.uniform(0.3, 1.0)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1).tolist()


def timed(fn, reps, warmup=3):
    """median, min, max (ms) of `reps` single runs, each between two events, after `warmup` runs"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def strings_of(bits: torch.Tensor):
    """Compressed COCO strings of bit-packed masks (host: flip positions -> the library's encoder)."""
    out = []
    for row in bits.cpu().numpy().view(np.uint32):
        flat = np.unpackbits(row.view(np.uint8), bitorder="little")[:H * W]
        flips = np.flatnonzero(np.diff(np.concatenate([[0], flat]).astype(np.int8))).astype(np.uint32)
        out.append({"size": [H, W], "counts": rle.compress(flips, H, W)[0]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--masks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_bits.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = a.views * a.masks
    segs = [[outline(rng)] for _ in range(n)]
    verts = [len(s[0]) // 2 for s in segs]
    bits, area = rle.polygon_bits(segs, H, W, dev)
    rles = strings_of(bits)
    back, back_area = rle.decode_bits(rles, dev)
    assert torch.equal(back, bits) and torch.equal(back_area, area), "the two paths disagree"
    poly = timed(lambda: rle.polygon_bits(segs, H, W, dev), a.reps)
    dec = timed(lambda: rle.decode_bits(rles, dev), a.reps)
    d_xy = torch.from_numpy(np.concatenate([np.asarray(s[0]) for s in segs])).to(dev)
    d_po = torch.from_numpy(np.concatenate([[0], np.cumsum(verts)]).astype(np.int64)).to(dev)
    d_mo = torch.arange(n + 1, dtype=torch.int64, device=dev)
    kern = timed(lambda: ops.poly_to_bits(d_xy, d_po, d_mo, H, W, bits=bits), a.reps)      # the launch alone (and three allocations)
    views = [{"instances": [{"segmentation": r, "score": 0.9 - 0.01 * j, "category_id": 0} for j, r in enumerate(rles[v * a.masks:(v + 1) * a.masks])],
              "pred_plane": np.ones((a.masks, 3), np.float32),
              "annotations": [{"segmentation": s, "plane": [0.0, 0.0, 1.0], "category_id": 1} for s in segs[v * a.masks:(v + 1) * a.masks]]}
             for v in range(a.views)]
    for _ in range(2):
        evaluation.plane_rows(views, dev, gt_polygons=True)
    steps = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluation.plane_rows(views, dev, gt_polygons=True)              # (ends in a copy to the host)
        steps.append(1e3 * (time.perf_counter() - t0))
    step = sorted(steps)[len(steps) // 2]
    probe = ops.clock_probe()
    torch.cuda.synchronize()
    cyc, ticks = probe.tolist()
    mhz = 100.0 * cyc / max(ticks, 1)
    res = {"device": torch.cuda.get_device_name(0), "engine_clock_mhz": round(mhz, 1), "views": a.views, "masks_per_view": a.masks, "size": [H, W],
           "vertices": [min(verts), int(np.median(verts)), max(verts)], "mean_area_px": float(area.float().mean()),
           "polygon_bits_ms": poly, "decode_bits_ms": dec, "poly_to_bits_launch_ms": kern, "plane_rows_step_ms": step,
           "polygon_bits_share_of_step": poly[0] / step, "reps": a.reps}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("GT masks to bits: polygons (nopesac_poly_to_bits) against compressed RLE strings (nopesac_rle_string_runs + nopesac_rle_runs_to_bits), scripts/poly_bits_bench.py\n")
        f.write("%s, engine clock read on the device %.0f MHz; %d views x %d masks at %d x %d, one outline of %d .. %d vertices (median %d)\n"
                % (res["device"], mhz, a.views, a.masks, H, W, min(verts), max(verts), int(np.median(verts))))
        f.write("per call (upload + launches + one host sync), between two events, after warm-up; median (min .. max) of %d, ms\n\n" % a.reps)
        f.write("rle.polygon_bits  (%d polygons)        %8.3f  (%.3f .. %.3f)\n" % ((n,) + poly))
        f.write("rle.decode_bits   (%d strings)         %8.3f  (%.3f .. %.3f)\n" % ((n,) + dec))
        f.write("ops.poly_to_bits  (the launch alone)     %8.3f  (%.3f .. %.3f)\n" % kern)
        f.write("evaluation.plane_rows, same batch, %d predictions per view, polygon GT (host clock, ends in a copy back)  %8.3f\n" % (a.masks, step))
        f.write("rle.polygon_bits' share of that step     %8.1f %%\n" % (100.0 * poly[0] / step))


if __name__ == "__main__":
    main()
