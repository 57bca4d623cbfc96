"""The two-view planar reconstruction as textured meshes: the counterpart of the reference's third entry point, `vis_NopeSAC.py`
(`save_pair_objects`: `merge_plane_params_from_local_params`, `get_single_image_mesh*`, `transform_meshes`, `save_obj`).  It reads what
`--dump-dir` writes (or a batch of model outputs, or a dataset pair's annotations), merges the parameters of matched planes, lifts
every mask onto its plane, puts both views into view 1's frame through the camera and writes an `.obj` / `.mtl` pair.

The geometry is the reference's DENSE route, `get_single_image_mesh(..., reduce_size=False)`: one vertex per mask pixel in row-major
order, two triangles per 2 x 2 block, the view's own image as the texture of all its planes (uv = (x / W, 1 - y / H)).  `stride`
s >= 1 is this port's addition: the same algorithm on m[::s, ::s] with the pixel coordinates multiplied back by s; s = 1 is the
reference exactly.  Everything per pixel runs on the device (csrc/recon_mesh.hip: nopesac_recon_mesh_merge / _count / _fill, masks
from rle.segmentation_bits); the host scans the per-instance counts and writes the text.

Merged plane parameters (merge=True, `merge_plane_params_from_local_params`): both views' planes go to the common frame
(`get_plane_params_in_global`), a correspondence (a, b) replaces both planes by the merged normal (csrc/two_view.h states the rule
and its sign) times the mean offset, and every plane - matched or not - comes back through `get_plane_params_in_local`; a pair
without correspondences keeps its planes untouched, as in the reference.

Out of scope: the contour / earcut meshes of `get_single_image_mesh_plane` and their per-plane rectified texture maps, camera frusta
(`get_camera_meshes`), `rotate_mesh_for_webview`, the matching figure and blended segmentations, depth-map meshes.
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .evaluation import assignment_corrs, camera7, checked_planes, corr_pairs
from .rle import exclusive_offsets

DEFAULT_FOCAL = 517.97              # the reference's intrinsics when a pair has no K: this focal length, principal point (W / 2, H / 2)
_IDENTITY7 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


@dataclass
class PairMesh:
    """One pair's meshes, on the device.  Instances are view 0's in their order, then view 1's; instance k owns vertices
    vert_off[k] : vert_off[k + 1] and faces face_off[k] : face_off[k + 1], and its faces hold vertex ids local to it, from 0."""
    verts: torch.Tensor               # f32 [V, 3], common frame (view 1's, after the y / z flip)
    uvs: torch.Tensor                 # f32 [V, 2]
    faces: torch.Tensor               # int32 [F, 3]
    vert_off: torch.Tensor            # int64 [n + 1]
    face_off: torch.Tensor            # int64 [n + 1]
    view_of_instance: torch.Tensor    # int32 [n], 0 or 1
    planes: torch.Tensor              # float64 [n, 3], the (merged) parameters in each instance's own view frame
    bad: torch.Tensor                 # int32 [n], the fill kernel's flags (all zero; write_obj checks them)
    size: tuple                       # (H, W)
    stride: int


def default_K(H: int, W: int) -> np.ndarray:
    return np.array([[DEFAULT_FOCAL, 0.0, W / 2], [0.0, DEFAULT_FOCAL, H / 2], [0.0, 0.0, 1.0]], np.float64)


def _empty_mesh(device, n: int, view_of, planes, size, stride: int) -> PairMesh:
    z = lambda *s, dtype: torch.zeros(s, device=device, dtype=dtype)      # noqa: E731
    return PairMesh(z(0, 3, dtype=torch.float32), z(0, 2, dtype=torch.float32), z(0, 3, dtype=torch.int32), z(n + 1, dtype=torch.int64),
                    z(n + 1, dtype=torch.int64), view_of, planes, z(n, dtype=torch.int32), size, stride)


def pair_meshes(pairs: List[dict], device, stride: int = 1, merge: bool = True, size=None) -> List[PairMesh]:
    """The meshes of a list of pairs in ONE decode and one launch of each kernel.  pairs: [{"views": (view0, view1), "camera":
    {"position" | "tran", "rotation" | "rot" wxyz}, "corrs": int [k, 2], "K": 3 x 3 or None}] with view = {"instances":
    [{"segmentation"}], "pred_plane": [n, 3]} - the shape evaluation.recon_rows takes, minus the GT.  Segmentations are RLE dicts or
    polygon lists (rle.segmentation_bits; all of one image size, `size` = (H, W) when the call holds polygons only); K = None is the
    reference's default (focal 517.97, principal point (W / 2, H / 2)).  merge=False leaves every plane as it is.  At most
    ops.PLANE_MAX_QUERIES instances per view, and a mask must fit the LDS bound of the header (NPS_MESH_LDS_WORDS) at `stride`.
    One host sync besides the decode's: the scanned counts, which size the outputs.
    ValueError: a view whose `instances` and `pred_plane` differ in length (before any device work), stride < 1, and a correspondence
    that names a plane its view does not have or names a plane twice."""
    from . import ops, rle
    device = torch.device(device)
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"pair_meshes: stride >= 1 (got {stride})")
    P = len(pairs)
    if P == 0:
        return []
    views = [v for p in pairs for v in p["views"]]
    if len(views) != 2 * P:
        raise ValueError("pair_meshes: a pair has two views")
    n_inst = [len(v.get("instances") or []) for v in views]
    planes = checked_planes(views, n_inst, lambda k, n, rows: f"pair_meshes: view {k % 2} of pair {k // 2} has {n} instances but {rows} "
                                                              "pred_plane rows")
    if max(n_inst) > ops.PLANE_MAX_QUERIES:
        raise ValueError(f"pair_meshes: at most {ops.PLANE_MAX_QUERIES} instances per view (got {max(n_inst)})")
    total = int(sum(n_inst))
    view_off = exclusive_offsets(n_inst)
    corrs = [corr_pairs(p.get("corrs", ())) if merge else np.zeros((0, 2), np.int32) for p in pairs]
    corr_off = exclusive_offsets([len(c) for c in corrs])
    pair_cam = np.stack([camera7(p["camera"], "pair_meshes") for p in pairs])
    view_of = np.concatenate([np.full(n, k % 2, np.int32) for k, n in enumerate(n_inst)]) if total else np.zeros(0, np.int32)
    inst_view = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(n_inst)]) if total else np.zeros(0, np.int32)
    d_view_of = torch.from_numpy(view_of).to(device)
    if total == 0:
        e = torch.zeros((0, 3), device=device, dtype=torch.float64)
        return [_empty_mesh(device, 0, d_view_of, e, tuple(size) if size is not None else (0, 0), stride) for _ in pairs]
    segs = [ins["segmentation"] for v in views for ins in v["instances"]]
    bits, _ = rle.segmentation_bits(segs, device, size=size)
    sizes = {tuple(int(x) for x in s["size"]) for s in segs if isinstance(s, dict)}
    H, W = next(iter(sizes)) if sizes else (int(size[0]), int(size[1]))
    kinv = np.stack([np.linalg.inv(default_K(H, W) if p.get("K") is None else np.asarray(p["K"], np.float64).reshape(3, 3)).reshape(9)
                     for p in pairs for _ in range(2)])
    view_cam = np.stack([c for cam in pair_cam for c in (cam, _IDENTITY7)])
    d_f64 = torch.from_numpy(np.concatenate([pair_cam.reshape(-1), view_cam.reshape(-1), kinv.reshape(-1)])).to(device)
    d_i64 = torch.from_numpy(np.concatenate([view_off, corr_off])).to(device)
    d_i32 = torch.from_numpy(np.concatenate([np.concatenate(corrs).reshape(-1).astype(np.int32), inst_view])).to(device)
    d_planes = torch.from_numpy(np.concatenate(planes)).to(device)
    d_pair_cam, d_view_cam, d_kinv = d_f64[:7 * P], d_f64[7 * P:21 * P], d_f64[21 * P:]
    n_c = 2 * int(corr_off[-1])
    merged, mbad = ops.recon_mesh_merge(d_planes, d_i64[:2 * P + 1], d_pair_cam, d_i32[:n_c], d_i64[2 * P + 1:], max(n_inst))
    n_vert, n_face = ops.recon_mesh_count(bits, H, W, stride)
    zero = torch.zeros(1, device=device, dtype=torch.int64)
    vert_off = torch.cat([zero, torch.cumsum(n_vert.to(torch.int64), 0)])
    face_off = torch.cat([zero, torch.cumsum(n_face.to(torch.int64), 0)])
    host = torch.cat([vert_off, face_off, mbad.to(torch.int64)]).cpu().numpy()          # the host sync: offsets (and the merge's flags)
    h_vert, h_face, h_bad = host[:total + 1], host[total + 1:2 * total + 2], host[2 * total + 2:]
    if h_bad.any():
        raise ValueError(f"pair_meshes: pair(s) {np.flatnonzero(h_bad).tolist()} of the batch have a correspondence that names a plane "
                         "their view does not have, or name a plane twice")
    verts, uvs, faces, fbad = ops.recon_mesh_fill(bits, H, W, stride, merged, d_i32[n_c:], d_kinv, d_view_cam, vert_off, face_off,
                                                  int(h_vert[-1]), int(h_face[-1]))
    out = []
    for i in range(P):
        a, b = int(view_off[2 * i]), int(view_off[2 * i + 2])
        v0, v1, f0, f1 = int(h_vert[a]), int(h_vert[b]), int(h_face[a]), int(h_face[b])
        out.append(PairMesh(verts[v0:v1], uvs[v0:v1], faces[f0:f1], vert_off[a:b + 1] - v0, face_off[a:b + 1] - f0, d_view_of[a:b],
                            merged[a:b], fbad[a:b], (H, W), stride))
    return out


# ---- where pairs come from ---------------------------------------------------------------------------------------------------------
def _record_view(instances, planes) -> dict:
    """A view of a prediction record.  A record without instances contributes no mesh whatever its plane rows are (the records of
    run.py's --stub-model are of this kind)."""
    instances = instances or []
    return {"instances": instances, "pred_plane": planes if len(instances) else np.zeros((0, 3), np.float32)}


def pairs_from_dump(dump_dir: str, K=None) -> List[dict]:
    """The pairs of a `--dump-dir` (NopeSAC_instances_predictions.pth + continuous.pkl) as pair_meshes takes them - what
    vis_NopeSAC.py's vis(gt_on=False) uses: `best_camera`, `best_assignment` and `plane_param_override` of continuous.pkl, the
    instances of the predictions file.  Each pair also carries "ids" and "files" (image ids and file names of its two views)."""
    predictions = torch.load(os.path.join(dump_dir, "NopeSAC_instances_predictions.pth"), weights_only=False)
    with open(os.path.join(dump_dir, "continuous.pkl"), "rb") as f:
        optimized = pickle.load(f)
    pairs = []
    for idx, pred in enumerate(predictions):
        opt = optimized[idx]
        pairs.append({"views": tuple(_record_view(pred[v].get("instances"), opt["plane_param_override"][v]) for v in "01"),
                      "camera": opt["best_camera"], "corrs": assignment_corrs(opt["best_assignment"]), "K": K,
                      "ids": tuple(pred[v].get("image_id") for v in "01"), "files": tuple(pred[v].get("file_name") for v in "01")})
    return pairs


def meshes_from_dump(dump_dir: str, device, stride: int = 1, merge: bool = True, K=None, limit: int = 0) -> List[PairMesh]:
    """The meshes vis_NopeSAC.py's vis(gt_on=False) builds from a `--dump-dir`, on the dense route (pairs_from_dump + pair_meshes);
    limit > 0: the first `limit` pairs only."""
    pairs = pairs_from_dump(dump_dir, K)
    return pair_meshes(pairs[:limit] if limit > 0 else pairs, device, stride=stride, merge=merge)


def pair_from_gt(dataset_pair: dict) -> dict:
    """A dataset pair's ground truth as pair_meshes takes it (vis(gt_on=True)): the annotations' masks and planes, `gt_corrs`, `rel_pose`
    and `camera_K` when the pair has one."""
    views = tuple({"instances": [{"segmentation": a["segmentation"]} for a in dataset_pair[v]["annotations"]],
                   "pred_plane": np.asarray([a["plane"] for a in dataset_pair[v]["annotations"]], np.float32).reshape(-1, 3)} for v in "01")
    return {"views": views, "camera": dataset_pair["rel_pose"], "corrs": np.asarray(dataset_pair["gt_corrs"], np.int64).reshape(-1, 2),
            "K": dataset_pair.get("camera_K")}


def meshes_from_gt(dataset_pair: dict, device, stride: int = 1, merge: bool = True) -> PairMesh:
    """The mesh of a dataset pair's ground truth (vis(gt_on=True)).  Polygon annotations take the image size from the view's `height` /
    `width`."""
    v0 = dataset_pair["0"]
    size = (v0["height"], v0["width"]) if "height" in v0 and "width" in v0 else None
    return pair_meshes([pair_from_gt(dataset_pair)], device, stride=stride, merge=merge, size=size)[0]


# ---- the text ------------------------------------------------------------------------------------------------------------------------
def _material(prefix: str, view: int) -> str:
    return f"{prefix}_view{view}"


def _lines(head: str, columns: Sequence[np.ndarray]) -> np.ndarray:
    """'<head> c0 c1 ...' per row, from string columns."""
    out = np.char.add(head + " ", columns[0])
    for c in columns[1:]:
        out = np.char.add(np.char.add(out, " "), c)
    return out


def write_obj(folder: str, prefix: str, mesh: PairMesh, image_files: Sequence[str], double_sided: bool = True, decimal_places: int = 10):
    """`<folder>/<prefix>.obj` and `.mtl` in the layout of the reference's save_obj / _save: the `mtllib` line, then per instance
    `# mesh i`, its `v` lines, its `vt` lines, `usemtl`, and its faces as `f a/a b/b c/c` with 1-based indices into the whole file, each
    followed by its reverse when double_sided.  The .mtl has one material per view, `<prefix>_view<v>`, whose map_Kd names that view's
    image (image_files[v], written as given).  An instance without a pixel keeps its `# mesh i` and `usemtl` lines.  The numbers are
    formatted by numpy's string routines, a column at a time.  Returns the two paths."""
    if len(image_files) != 2:
        raise ValueError("write_obj: image_files names the images of view 0 and view 1")
    host = {k: getattr(mesh, k).detach().cpu().numpy() for k in ("verts", "uvs", "faces", "vert_off", "face_off", "view_of_instance", "bad")}
    if host["bad"].any():
        raise RuntimeError(f"write_obj: instance(s) {np.flatnonzero(host['bad']).tolist()} were not filled (counts and offsets disagree)")
    os.makedirs(folder, exist_ok=True)
    fmt = "%." + str(int(decimal_places)) + "f"
    num = lambda a: np.char.mod(fmt, a.astype(np.float64))      # noqa: E731
    v_lines = _lines("v", list(num(host["verts"]).T)) if len(host["verts"]) else np.zeros(0, "U1")
    t_lines = _lines("vt", list(num(host["uvs"]).T)) if len(host["uvs"]) else np.zeros(0, "U1")
    vert_off, face_off = host["vert_off"], host["face_off"]
    n = len(vert_off) - 1
    base = np.repeat(vert_off[:-1], np.diff(face_off)) + 1                    # 1-based, into the whole file
    ids = np.char.mod("%d", host["faces"].astype(np.int64) + base[:, None]) if len(host["faces"]) else np.zeros((0, 3), "U1")
    tok = np.char.add(np.char.add(ids, "/"), ids)
    f_lines = _lines("f", [tok[:, 0], tok[:, 1], tok[:, 2]]) if len(tok) else np.zeros(0, "U1")
    r_lines = _lines("f", [tok[:, 2], tok[:, 1], tok[:, 0]]) if len(tok) else np.zeros(0, "U1")
    parts = [f"mtllib {prefix}.mtl\n"]
    for k in range(n):
        parts.append(f"# mesh {k}")
        parts.extend(v_lines[vert_off[k]:vert_off[k + 1]].tolist())
        parts.extend(t_lines[vert_off[k]:vert_off[k + 1]].tolist())
        parts.append("usemtl " + _material(prefix, int(host["view_of_instance"][k])))
        a, b = face_off[k], face_off[k + 1]
        parts.extend((np.stack([f_lines[a:b], r_lines[a:b]], 1).reshape(-1) if double_sided else f_lines[a:b]).tolist())
    obj, mtl = os.path.join(folder, prefix + ".obj"), os.path.join(folder, prefix + ".mtl")
    with open(obj, "w") as f:
        f.write("\n".join(parts) + "\n")
    with open(mtl, "w") as f:
        for v in range(2):
            f.write(f"newmtl {_material(prefix, v)}\nmap_Kd {image_files[v]}\nKa 1.000 1.000 1.000\nKd 1.000 1.000 1.000\n"
                    "Ks 0.000 0.000 0.000\nNs 10.0\n")
    return obj, mtl


class MeshExporter:
    """DatasetEvaluator-style exporter for run.inference_on_dataset(..., also=...): process(inputs, outputs) writes
    `<out_dir>/<id0>__<id1>.obj` / `.mtl` (pairs without image ids: `pair<number>`) for the first `limit` pairs it sees (0 = all),
    one pair_meshes call per batch.  Camera: the output's "camera"; correspondences: its "pred_assignment"; K: the input's `camera_K`
    when it has one.  map_Kd names the input view's `file_name` (`view<v>.png` without one)."""

    def __init__(self, device, out_dir: str, stride: int = 4, limit: int = 16, merge: bool = True):
        self.device, self.out_dir, self.stride, self.limit, self.merge = torch.device(device), out_dir, int(stride), int(limit), bool(merge)
        if self.stride < 1:
            raise ValueError(f"MeshExporter: stride >= 1 (got {stride})")
        self.reset()

    def reset(self):
        self.written: List[str] = []
        self._seen = 0

    def process(self, inputs: List[dict], outputs: List[dict]):
        todo = []
        for inp, out in zip(inputs, outputs):
            number, self._seen = self._seen, self._seen + 1
            if self.limit and len(self.written) + len(todo) >= self.limit:
                continue
            ids = [inp[v].get("image_id") for v in "01"]
            prefix = f"pair{number:05d}" if any(i is None for i in ids) else f"{ids[0]}__{ids[1]}".replace(os.sep, "_")
            files = [inp[v].get("file_name") or f"view{v}.png" for v in "01"]
            cam = out["camera"]
            pair = {"views": tuple(_record_view((out[v] or {}).get("instances"), out[v]["pred_plane"]) for v in "01"),
                    "camera": cam.get("pred", cam), "corrs": assignment_corrs(out["pred_assignment"]), "K": inp.get("camera_K")}
            todo.append((prefix, files, pair))
        if not todo:
            return
        for (prefix, files, _), mesh in zip(todo, pair_meshes([t[2] for t in todo], self.device, stride=self.stride, merge=self.merge)):
            self.written.append(write_obj(self.out_dir, prefix, mesh, files)[0])

    def evaluate(self) -> dict:
        return {"exported": len(self.written), "stride": self.stride}
