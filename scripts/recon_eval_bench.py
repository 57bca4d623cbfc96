"""The reconstruction AP evaluator at production shapes (csrc/recon_eval.hip through evaluation.recon_rows): a batch of `--batch`
synthetic pairs at 480x640 with nq = 50 and nq = 128 predictions per view (a partition of the image, as the model's winner map is)
and 20 GT planes per view, masks as uncompressed run lists.  Timed: recon_rows end to end on the GPU (host preparation, upload,
RLE decode, mask IoU, the per-pair kernel, download; wall clock around a synchronised call, median of `--reps`), the per-pair
kernel alone (events around ops.recon_ap_assign), and the float64 host restatement tests/recon_eval_ref.py on the same inputs with
the IoU from nopesac_amd.rle.iou (run lengths on the host) over the first `--host-pairs` pairs.  Checks that both give the same
flags.  Prints the figures and one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import evaluation as E  # noqa: E402
from nopesac_amd import ops, rle  # noqa: E402
from tests import recon_eval_inputs as RI  # noqa: E402
from tests import recon_eval_ref as REF  # noqa: E402


def run_lengths(mask):
    flat = np.asarray(mask, bool).reshape(-1, order="F")
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], edges, [flat.size]]))
    return {"size": list(mask.shape), "counts": ([0] if flat[0] else []) + counts.tolist()}


def partition(rng, h, w, n, cell=8):
    yy, xx = np.mgrid[0:h // cell, 0:w // cell]
    cx, cy = rng.uniform(0, w // cell, n), rng.uniform(0, h // cell, n)
    lab = np.argmin((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2, 0)
    return np.kron(lab, np.ones((cell, cell), np.int64))


def synthetic_pair(rng, nq, n_gt=20, h=480, w=640):
    cam = RI._camera(rng)
    glob = [RI._unit(rng.normal(size=3)) * rng.uniform(1.5, 4.0) for _ in range(2 * n_gt)]
    gt_planes = [np.asarray([RI._local_in_view0(g, cam)[0] for g in glob[:n_gt]], np.float32), np.asarray([g * RI.FLIP for g in glob[n_gt:]], np.float32)]
    gt_planes[1][:n_gt // 2] = np.asarray([g * RI.FLIP for g in glob[:n_gt // 2]], np.float32)      # half of the planes are seen in both views
    views = []
    for v in range(2):
        gt_lab, dt_lab = partition(rng, h, w, n_gt), partition(rng, h, w, nq)
        src = [int(np.bincount(gt_lab[dt_lab == k], minlength=n_gt).argmax()) if (dt_lab == k).any() else 0 for k in range(nq)]
        planes = np.asarray([RI._perturbed(rng, gt_planes[v][s].astype(np.float64)) for s in src], np.float32)
        views.append({"instances": [{"segmentation": run_lengths(dt_lab == k), "score": float(s)} for k, s in enumerate(rng.uniform(0.15, 1.0, nq).astype(np.float32))],
                      "pred_plane": planes, "annotations": [{"segmentation": run_lengths(gt_lab == k), "plane": [float(x) for x in gt_planes[v][k]]} for k in range(n_gt)]})
    k = nq // 3
    corr = np.stack([np.sort(rng.permutation(nq)[:k]), rng.permutation(nq)[:k]], 1).astype(np.int32)
    return {"views": tuple(views), "pred_camera": {"position": cam["position"] + rng.normal(size=3) * 0.05, "rotation": cam["rotation"]},
            "gt_camera": cam, "pred_corrs": corr, "gt_corrs": [[i, i] for i in range(n_gt // 2)]}


def host_rows(pair):
    v0, v1 = pair["views"]
    iou = [rle.iou([i["segmentation"] for i in v["instances"]], [a["segmentation"] for a in v["annotations"]]) for v in (v0, v1)]
    return REF.pair_rows(iou[0], iou[1], [i["score"] for i in v0["instances"]], [i["score"] for i in v1["instances"]], v0["pred_plane"], v1["pred_plane"],
                         [a["plane"] for a in v0["annotations"]], [a["plane"] for a in v1["annotations"]], pair["pred_camera"], pair["gt_camera"],
                         pair["pred_corrs"], pair["gt_corrs"])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-pairs", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kernel_ms = []
    inner = ops.recon_ap_assign

    def timed_kernel(*args, **kw):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = inner(*args, **kw)
        ev[1].record()
        torch.cuda.synchronize()
        kernel_ms.append(ev[0].elapsed_time(ev[1]))
        return out
    ops.recon_ap_assign = timed_kernel
    result = {"batch": a.batch, "device": torch.cuda.get_device_name(0)}
    for nq in (50, 128):
        rng = np.random.default_rng(nq)
        pairs = [synthetic_pair(rng, nq) for _ in range(a.batch)]
        rows = E.recon_rows(pairs, dev)[0]                                  # warm-up, and the rows to compare
        del kernel_ms[:]
        wall = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.recon_rows(pairs, dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host = [host_rows(p) for p in pairs[:a.host_pairs]]
        host_ms = (time.perf_counter() - t0) * 1e3 / max(a.host_pairs, 1)
        n_host = sum(len(h) for h in host)
        same = bool(np.array_equal(np.concatenate(host)[:, :6], rows[:n_host, :6])) if host else None
        result[f"nq{nq}"] = {"recon_rows_ms_per_batch": float(np.median(wall)), "kernel_ms_per_batch": float(np.median(kernel_ms)),
                             "host_restatement_ms_per_pair": host_ms, "host_restatement_ms_per_batch_extrapolated": host_ms * a.batch,
                             "entries": int(len(rows)), "flags_equal_on_host_pairs": same}
        print(f"nq {nq:3d}: recon_rows {np.median(wall):8.2f} ms / batch of {a.batch} (kernel alone {np.median(kernel_ms):.3f} ms), "
              f"host restatement {host_ms:8.1f} ms / pair ({host_ms * a.batch:.0f} ms / batch, from {a.host_pairs} pairs), flags equal: {same}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
