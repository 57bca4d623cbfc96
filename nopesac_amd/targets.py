"""Ground truth for training: a dataset's per-view record -> the targets `training.PlaneCriterion` takes, and a pair's correspondences and
relative pose in the forms `training.plane_corr_matrix` and the camera losses take.

The reference builds these in two places: its mapper (data/planercnn_transforms.py:210-398) reads, per view, an mp3d observation pickle
(`semantic_sensor` int32 label map, `depth_sensor` f32) or a ScanNet annotation pickle (`plane_masks [n, H, W]`, `camera_K`) plus a 16-bit
depth PNG (`astype(float32) / 1000.`); its model (siamese_planeTR.py:475-532 prepare_targets, :549-562 process_camera, :566-576) turns
them into masks, plane centres, the per-pixel centre map, K^-1 . (x, y, 1), the pose vector and the filtered correspondences.  Here
the host part stays plain Python (the two readers below) and everything per pixel runs in csrc/train_targets.hip through the checked
wrappers of nopesac_amd.ops: label map -> distinct ids -> masks + centres in one pass over the labels, bit-packed polygon / RLE masks
-> byte masks, uint16 depth -> metres, K^-1 -> coordinate map.  There is no torch arithmetic on these routes, only uploads and copies.

Out of scope: the k-means pose classes of the mapper (`tran_cls` / `rot_cls`: no loss of this package reads them), `loss_depth_pixel`,
and a train CLI.  The follow-up that would remove the mask pass altogether - about nmax bytes written per pixel, 1 GB for 64 views of
480 x 640 with 50 planes - is to teach the criterion's kernels to read the label map and the id table instead of byte masks; it is
not done here, the criterion's interface is unchanged.
"""
from __future__ import annotations

import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops, rle

MAX_TARGETS = ops.PLANE_MAX_TARGETS                                   # the reference keeps at most 50 planes per view
DEFAULT_K = ((517.97, 0.0, 320.0), (0.0, 517.97, 240.0), (0.0, 0.0, 1.0))      # get_coordinate_map's intrinsics (siamese_planeTR.py:816-820)


def inverse_intrinsics(K) -> np.ndarray:
    """K^-1 as the f32 row [9] nopesac_coordinate_map takes: K is rounded to f32 first, as the reference does before it inverts, then
    inverted in float64 and rounded once (the reference inverts in f32)."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera_K of shape {K.shape}: a 3 x 3 matrix is expected")
    return np.linalg.inv(K.astype(np.float32).astype(np.float64)).astype(np.float32).reshape(9)


def read_mp3d_observation(path: str) -> Dict[str, np.ndarray]:
    """The mp3d observation pickle of one view -> {"semantic_map": int32 [H, W], "depth": f32 [H, W]} (planercnn_transforms.py:238-263)."""
    with open(path, "rb") as f:
        obs = pickle.load(f)
    return {"semantic_map": np.ascontiguousarray(np.asarray(obs["semantic_sensor"]).astype(np.int32)),
            "depth": np.ascontiguousarray(np.asarray(obs["depth_sensor"]).astype(np.float32))}


def read_scannet_view(ann_pkl: str, depth_png: str) -> Dict[str, np.ndarray]:
    """The ScanNet two-view annotation pickle and the 16-bit depth PNG of one view -> {"plane_masks": uint8 [n, H, W], "camera_K": [3, 3],
    "depth": uint16 [H, W]} (planercnn_transforms.py:337-355).  The depth stays in millimetres: it goes to the device unconverted and
    ops.depth_from_u16 divides there."""
    from PIL import Image
    with open(ann_pkl, "rb") as f:
        obs = pickle.load(f)
    with Image.open(depth_png) as im:
        depth = np.asarray(im)
    if depth.dtype != np.uint16 or depth.ndim != 2:
        raise ValueError(f"{depth_png}: a single-channel 16-bit PNG is expected, got {depth.dtype} {depth.shape}")
    return {"plane_masks": np.ascontiguousarray(np.asarray(obs["plane_masks"]).astype(np.uint8)), "camera_K": np.asarray(obs["camera_K"]),
            "depth": np.ascontiguousarray(depth)}


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _name(i: int, rec: dict) -> str:
    return f"view {i} ({rec['image_id']})" if "image_id" in rec else f"view {i}"


class TargetMapper:
    """view_targets(records) / pair_targets(entries) on `device`.  max_targets: the reference's cap of 50 planes per view;
    flip_negative_w: process_camera's sign rule (on unless cfg.MODEL.CAMERA_HEAD.CLASSIFICATION_ON)."""

    def __init__(self, device, max_targets: int = MAX_TARGETS, flip_negative_w: bool = True, depth_scale: float = 1000.0):
        if not 1 <= int(max_targets) <= MAX_TARGETS:
            raise ValueError(f"max_targets={max_targets} outside 1..{MAX_TARGETS}")
        self.device = torch.device(device)
        self.max_targets = int(max_targets)
        self.flip_negative_w = bool(flip_negative_w)
        self.depth_scale = float(depth_scale)
        self._default_kinv = inverse_intrinsics(DEFAULT_K)
        self._default_map = {}                                        # (H, W) -> [1, 3, H, W], computed once

    @classmethod
    def from_cfg(cls, cfg, device):
        return cls(device, flip_negative_w=not bool(cfg.MODEL.CAMERA_HEAD.CLASSIFICATION_ON))

    # ---- one batch of views ------------------------------------------------------------------------------------------------------------
    def view_targets(self, records: Sequence[dict]) -> dict:
        """records: per view a dict with exactly one of `semantic_map` (int32 [H, W] label map, 0 = no plane), `plane_masks` ([n, H, W])
        or segmentations in `annotations` (polygons or RLE), with `depth` (f32 metres, or uint16 millimetres) and `annotations` (each
        with `plane`, `category_id`; crowd annotations are skipped as the reference's mapper skips them), optionally `camera_K`.
        -> masks uint8 [B, nmax, H, W], n (device) / n_host int32 [B], plane_params f32 [B, nmax, 3], plane_centers f32 [B, nmax, 2],
        pixel_centers f32 [B, 2, H, W], depth f32 [B, H, W], k_inv_dot_xy1 f32 [B, 3, H, W], labels int64 [B, nmax] (-1 past n): the
        dict PlaneCriterion takes, nmax = the batch's largest n (at most 50).  One host sync on the label-map route (n and the
        refusal flags), none added on the others.  ValueError, naming the view: the planes found differ in number from the
        annotations (the reference's assert), a view without a plane, more distinct labels than the kernel's table holds."""
        records = list(records)
        if not records:
            raise ValueError("view_targets: no record")
        routes = [self._route(i, r) for i, r in enumerate(records)]
        if len(set(routes)) != 1:
            raise ValueError(f"view_targets: the views of one call must hold one kind of ground truth, got {sorted(set(routes))}")
        annos = [[a for a in r.get("annotations", []) if a.get("iscrowd", 0) == 0] for r in records]
        depth = self._depth(records)
        H, W = depth.shape[1:]
        masks, n_host, n_dev, centers, pixel = getattr(self, "_from_" + routes[0])(records, annos, H, W)
        B, nmax = masks.shape[:2]
        params = np.zeros((B, nmax, 3), np.float32)
        labels = np.full((B, nmax), -1, np.int64)
        for b, (rec, an) in enumerate(zip(records, annos)):
            k = int(n_host[b])
            if k:
                params[b, :k] = np.asarray([a["plane"] for a in an[:k]], dtype=np.float32).reshape(k, 3)
                labels[b, :k] = [int(a["category_id"]) for a in an[:k]]
        return {"masks": masks, "n": n_dev, "n_host": n_host, "plane_params": torch.from_numpy(params).to(self.device),
                "plane_centers": centers, "pixel_centers": pixel, "depth": depth, "k_inv_dot_xy1": self._coordinates(records, H, W),
                "labels": torch.from_numpy(labels).to(self.device)}

    @staticmethod
    def _route(i: int, rec: dict) -> str:
        segs = [a for a in rec.get("annotations", []) if "segmentation" in a]
        found = [k for k, have in (("semantic_map", "semantic_map" in rec), ("plane_masks", "plane_masks" in rec), ("segmentation", bool(segs))) if have]
        if len(found) != 1:
            raise ValueError(f"view_targets: {_name(i, rec)} holds {found or 'no ground-truth masks'}: exactly one of semantic_map, plane_masks "
                             "and annotation segmentations is expected")
        return found[0]

    def _check_counts(self, records, annos, counts) -> torch.Tensor:
        """The reference's assert (plane_num == len(instances)) and the empty view; -> n_host = min(count, max_targets)."""
        for i, (rec, an, c) in enumerate(zip(records, annos, counts)):
            if int(c) == 0:
                raise ValueError(f"view_targets: {_name(i, rec)} has no plane")
            if int(c) != len(an):
                raise ValueError(f"view_targets: {_name(i, rec)} has {int(c)} planes in its masks and {len(an)} annotations")
        return torch.tensor([min(int(c), self.max_targets) for c in counts], dtype=torch.int32)

    def _from_semantic_map(self, records, annos, H, W):
        maps = [_host(r["semantic_map"]) for r in records]
        for i, m in enumerate(maps):
            if m.shape != (H, W):
                raise ValueError(f"view_targets: {_name(i, records[i])}: semantic_map {m.shape}, depth {(H, W)}")
        labels = torch.from_numpy(np.stack([m.astype(np.int32, copy=False) for m in maps])).to(self.device)
        B = len(records)
        counts = torch.empty(3, B, device=self.device, dtype=torch.int32)            # n_all, n, bad: one download
        ids, _, n_dev, _ = ops.label_ids(labels, self.max_targets, out=(None, counts[0], counts[1], counts[2]))
        n_all, n, bad = counts.cpu().tolist()                                         # the call's host sync
        for i, rec in enumerate(records):
            if bad[i]:
                raise ValueError(f"view_targets: {_name(i, rec)} holds more than {ops.LABEL_MAX_IDS} distinct labels")
        n_host = self._check_counts(records, annos, n_all)
        assert n_host.tolist() == n
        masks, centers, pixel = ops.label_targets(labels, ids, n_dev, int(n_host.max()))
        return masks, n_host, n_dev, centers, pixel

    def _from_plane_masks(self, records, annos, H, W):
        stacks = [_host(r["plane_masks"]) for r in records]
        for i, m in enumerate(stacks):
            if m.ndim != 3 or m.shape[1:] != (H, W):
                raise ValueError(f"view_targets: {_name(i, records[i])}: plane_masks {m.shape}, depth {(H, W)}")
        n_host = self._check_counts(records, annos, [len(m) for m in stacks])
        nmax = int(n_host.max())
        kept = torch.from_numpy(np.concatenate([m[:k].astype(np.uint8, copy=False) for m, k in zip(stacks, n_host.tolist())])).to(self.device)
        masks = torch.zeros(len(records), nmax, H, W, device=self.device, dtype=torch.uint8)
        first = 0
        for b, k in enumerate(n_host.tolist()):
            masks[b, :k].copy_(kept[first:first + k])
            first += k
        n_dev = n_host.to(self.device)
        centers, pixel = ops.plane_targets(masks, n_host, n_dev)                      # stored masks may overlap: the general route
        return masks, n_host, n_dev, centers, pixel

    def _from_segmentation(self, records, annos, H, W):
        for i, (rec, an) in enumerate(zip(records, annos)):
            if any("segmentation" not in a for a in an):
                raise ValueError(f"view_targets: {_name(i, rec)}: an annotation without a segmentation")
        n_host = self._check_counts(records, annos, [len(an) for an in annos])
        bits, _ = rle.segmentation_bits([a["segmentation"] for an in annos for a in an], self.device, size=(H, W))
        if bits.shape[1] != (H * W + 31) // 32:
            raise ValueError(f"view_targets: the segmentations are not of the depth's size {(H, W)}")
        offsets = torch.from_numpy(rle.exclusive_offsets([len(an) for an in annos]).astype(np.int64)).to(self.device)
        masks = ops.bits_to_masks(bits, offsets, int(n_host.max()), H, W)
        n_dev = n_host.to(self.device)
        centers, pixel = ops.plane_targets(masks, n_host, n_dev)                      # polygons may overlap
        return masks, n_host, n_dev, centers, pixel

    def _depth(self, records) -> torch.Tensor:
        maps = []
        for i, r in enumerate(records):
            if "depth" not in r:
                raise ValueError(f"view_targets: {_name(i, r)} has no depth")
            maps.append(_host(r["depth"]))
        kinds = {m.dtype == np.uint16 for m in maps}
        if len(kinds) != 1 or len({m.shape for m in maps}) != 1 or maps[0].ndim != 2:
            raise ValueError("view_targets: the depth maps of one call must be [H, W], of one size, and all uint16 or all floating")
        if kinds == {True}:
            return ops.depth_from_u16(torch.from_numpy(np.stack(maps)).to(self.device), self.depth_scale)
        return torch.from_numpy(np.stack([m.astype(np.float32, copy=False) for m in maps])).to(self.device)

    def _coordinates(self, records, H: int, W: int) -> torch.Tensor:
        B = len(records)
        if not any("camera_K" in r for r in records):
            key = (H, W)
            if key not in self._default_map:
                self._default_map[key] = ops.coordinate_map(torch.from_numpy(self._default_kinv[None]).to(self.device), H, W)
            return self._default_map[key].expand(B, 3, H, W).contiguous()
        kinv = np.stack([inverse_intrinsics(_host(r["camera_K"])) if "camera_K" in r else self._default_kinv for r in records])
        return ops.coordinate_map(torch.from_numpy(kinv).to(self.device), H, W)

    # ---- one batch of pairs ------------------------------------------------------------------------------------------------------------
    def pair_targets(self, entries: Sequence[dict]) -> dict:
        """entries: B dataset dicts with the views "0" and "1", `gt_corrs` (rows of (plane of view 1, plane of view 2)) and `rel_pose`
        (`position` [3], `rotation` [4] = (w, x, y, z)).  -> {"targets": view_targets of the 2 B views, view-1 records first (the order the
        trainers stack them in), "gt_corrs": int32 [B, K, 2] on the device, rows with an index >= 50 dropped and the rest padded
        with -1 (the form training.plane_corr_matrix takes), "gt_pose": f32 [B, 7] = (t, q), q negated when q[0] < 0 unless the camera
        head classifies (process_camera, siamese_planeTR.py:549-562)}."""
        entries = list(entries)
        return {"targets": self.view_targets([e["0"] for e in entries] + [e["1"] for e in entries]),
                "gt_corrs": torch.from_numpy(pad_corrs([e["gt_corrs"] for e in entries])).to(self.device),
                "gt_pose": torch.from_numpy(pose_rows([e["rel_pose"] for e in entries], self.flip_negative_w)).to(self.device)}


def pad_corrs(corrs: List, limit: int = MAX_TARGETS) -> np.ndarray:
    """Per pair the rows (i, j) with i < limit and j < limit (siamese_planeTR.py:573-576), padded with -1 to the longest: int32 [B, K, 2], K >= 1."""
    kept = []
    for c in corrs:
        c = np.asarray(c, dtype=np.int64).reshape(-1, 2)
        kept.append(c[(c[:, 0] < limit) & (c[:, 1] < limit)])
    out = np.full((len(kept), max([len(c) for c in kept] + [1]), 2), -1, np.int32)
    for b, c in enumerate(kept):
        out[b, :len(c)] = c
    return out


def pose_rows(poses: List[dict], flip_negative_w: bool = True) -> np.ndarray:
    """(position, rotation) -> f32 [B, 7]; the quaternion is negated when its w < 0 and `flip_negative_w` (process_camera)."""
    out = np.zeros((len(poses), 7), np.float32)
    for b, p in enumerate(poses):
        q = np.asarray(p["rotation"], dtype=np.float64).astype(np.float32).reshape(4)
        if flip_negative_w and q[0] < 0:
            q = -q
        out[b, :3] = np.asarray(p["position"], dtype=np.float32).reshape(3)
        out[b, 3:] = q
    return out
