"""The reconstruction meshes (csrc/recon_mesh.hip, nopesac_amd/mesh.py) on the export workload: `--pairs` pairs at 480 x 640 with
`--instances` instances per view - a seeded partition of the image into blobs, planes and camera from synth.consistent_planes, the
planes both views share matched - at strides 1 and 4.  Timed between two events after warm-up, median of `--reps`: the decode
(rle.decode_bits: upload, two launches, one host sync), the merge, count and fill launches each alone, and pair_meshes as a whole;
from the fill: the bytes it writes (12 per vertex position, 8 per texture coordinate, 12 per face) and the fraction of the HBM write
bandwidth that is; on the host clock: write_obj of the first pair.  Prints one JSON line and writes profiles/recon_mesh_bench.txt."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import mesh, ops, rle, synth  # noqa: E402

H, W = 480, 640
HBM_PEAK = 8.0e12        # bytes / s, the MI355X specification


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


def blob_strings(rng, n):
    """A partition of the image into n blobs as compressed COCO strings."""
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    lab = np.argmin((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2, 0)
    out = []
    for k in range(n):
        flat = (lab == k).reshape(-1, order="F")
        flips = np.flatnonzero(np.diff(np.concatenate([[0], flat]).astype(np.int8))).astype(np.uint32)
        out.append({"size": [H, W], "counts": rle.compress(flips, H, W)[0]})
    return out


def workload(n_pairs, n_inst):
    pairs = []
    for i in range(n_pairs):
        rng = np.random.default_rng(i)
        p1, p2, perm, (t, q) = synth.consistent_planes(n_inst, n_inst, n_inst // 2, torch.Generator().manual_seed(i))
        corrs = [[a, int(b)] for a, b in enumerate(perm.tolist()) if b >= 0]
        views = tuple({"instances": [{"segmentation": s} for s in blob_strings(rng, n_inst)], "pred_plane": p.numpy()} for p in (p1, p2))
        pairs.append({"views": views, "camera": {"position": t.numpy(), "rotation": q.numpy()}, "corrs": np.asarray(corrs, np.int64).reshape(-1, 2),
                      "K": None})
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--instances", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_mesh_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pairs = workload(a.pairs, a.instances)
    P, n = a.pairs, 2 * a.pairs * a.instances
    segs = [ins["segmentation"] for p in pairs for v in p["views"] for ins in v["instances"]]
    decode = timed(lambda: rle.decode_bits(segs, dev), a.reps)
    bits, _ = rle.decode_bits(segs, dev)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    planes = to(np.concatenate([np.asarray(v["pred_plane"], np.float32) for p in pairs for v in p["views"]]))
    view_off = to(np.arange(2 * P + 1, dtype=np.int64) * a.instances)
    corr = to(np.concatenate([p["corrs"] for p in pairs]).astype(np.int32).reshape(-1))
    corr_off = to(np.concatenate([[0], np.cumsum([len(p["corrs"]) for p in pairs])]).astype(np.int64))
    cam = np.stack([np.concatenate([p["camera"]["position"], p["camera"]["rotation"]]).astype(np.float64) for p in pairs])
    view_cam = to(np.stack([c for row in cam for c in (row, np.array([0, 0, 0, 1.0, 0, 0, 0]))]))
    kinv = to(np.tile(np.linalg.inv(mesh.default_K(H, W)).reshape(1, 9), (2 * P, 1)))
    inst_view = to(np.repeat(np.arange(2 * P, dtype=np.int32), a.instances))
    d_cam = to(cam)
    merge = timed(lambda: ops.recon_mesh_merge(planes, view_off, d_cam, corr, corr_off, a.instances), a.reps)
    merged, bad = ops.recon_mesh_merge(planes, view_off, d_cam, corr, corr_off, a.instances)
    assert not bad.any().item()
    res = {"device": torch.cuda.get_device_name(0), "pairs": P, "instances_per_view": a.instances, "size": [H, W], "reps": a.reps,
           "decode_bits_ms": decode, "merge_ms": merge, "strides": {}}
    for stride in (1, 4):
        count = timed(lambda: ops.recon_mesh_count(bits, H, W, stride), a.reps)
        nv, nf = ops.recon_mesh_count(bits, H, W, stride)
        zero = torch.zeros(1, device=dev, dtype=torch.int64)
        vert_off, face_off = (torch.cat([zero, torch.cumsum(c.to(torch.int64), 0)]) for c in (nv, nf))
        V, F = int(vert_off[-1].item()), int(face_off[-1].item())
        call = lambda: ops.recon_mesh_fill(bits, H, W, stride, merged, inst_view, kinv, view_cam, vert_off, face_off, V, F)      # noqa: E731
        fill = timed(call, a.reps)
        assert not call()[3].any().item()
        whole = timed(lambda: mesh.pair_meshes(pairs, dev, stride=stride), a.reps)
        first = mesh.pair_meshes(pairs[:1], dev, stride=stride)[0]
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            obj, _ = mesh.write_obj(d, "pair", first, ["view0.png", "view1.png"])
            obj_s, obj_bytes = time.perf_counter() - t0, os.path.getsize(obj)
        nbytes = 20 * V + 12 * F
        res["strides"][stride] = {"vertices": V, "faces": F, "count_ms": count, "fill_ms": fill, "fill_bytes": nbytes,
                                  "fill_fraction_of_hbm_peak": nbytes / (fill[0] * 1e-3) / HBM_PEAK, "pair_meshes_ms": whole,
                                  "write_obj_first_pair_s": obj_s, "obj_bytes_first_pair": obj_bytes}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("Reconstruction meshes (csrc/recon_mesh.hip), scripts/recon_mesh_bench.py\n")
        f.write("%s; %d pairs x 2 views x %d instances at %d x %d (%d masks); between two events, after warm-up; median (min .. max) of %d, ms\n\n"
                % (res["device"], P, a.instances, H, W, n, a.reps))
        f.write("rle.decode_bits (upload, two launches, one host sync)   %9.3f  (%.3f .. %.3f)\n" % decode)
        f.write("ops.recon_mesh_merge                                   %9.3f  (%.3f .. %.3f)\n" % merge)
        for stride, r in res["strides"].items():
            f.write("\nstride %d: %d vertices, %d faces\n" % (stride, r["vertices"], r["faces"]))
            f.write("ops.recon_mesh_count                                   %9.3f  (%.3f .. %.3f)\n" % r["count_ms"])
            f.write("ops.recon_mesh_fill                                    %9.3f  (%.3f .. %.3f)\n" % r["fill_ms"])
            f.write("  writes %.1f MB: %.2f TB/s, %.1f %% of the 8 TB/s HBM peak\n"
                    % (r["fill_bytes"] / 1e6, r["fill_bytes"] / (r["fill_ms"][0] * 1e-3) / 1e12, 100.0 * r["fill_fraction_of_hbm_peak"]))
            f.write("mesh.pair_meshes (decode, three launches, one more sync) %9.3f  (%.3f .. %.3f)\n" % r["pair_meshes_ms"])
            f.write("mesh.write_obj, first pair, host clock: %.2f s for %.1f MB of text\n" % (r["write_obj_first_pair_s"], r["obj_bytes_first_pair"] / 1e6))


if __name__ == "__main__":
    main()
