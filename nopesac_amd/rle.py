"""COCO RLE `instances` packaging from the post-selection winner map (replaces pycocotools.mask.encode / toBbox in
meta_arch/siamese_planeTR.py:685-720, 741-766).

Device: nopesac_rle_labels + nopesac_rle_transitions (csrc/rle.hip) produce, for every (view, kept plane), the
positions where the plane's mask flips along the column-major scan; no [n,H,W] mask tensor is ever built.
nopesac_rle_compress_device (a workgroup per mask) turns the flips into the compressed counts strings and the [x, y, w, h]
boxes, still on the device; the host receives finished byte strings.  Host syncs: two size reads (positions buffer, byte buffer).
nopesac_rle_compress_host / _batch_host (same library, plain C) are the host forms of the same encoder.

Reading side (evaluation): counts_of / decode / iou on the host; decode_bits / iou_device on the device (csrc/plane_eval.hip:
nopesac_rle_string_runs -> nopesac_rle_runs_to_bits -> nopesac_mask_iou_bits), bit-packed masks and IoU by popcount.  Polygon
annotations (what pycocotools.mask.frPyObjects + merge do for the evaluators) become the same bit-packed masks on the device:
polygon_bits (csrc/plane_eval.hip: nopesac_poly_to_bits); segmentation_bits takes RLE dicts and polygon lists mixed.
"""
from __future__ import annotations

import ctypes
from typing import List

import numpy as np
import torch

from . import _lib, ops
from .ops import _C


def exclusive_offsets(counts) -> np.ndarray:
    """Exclusive offsets of a list of counts: int64 [n + 1], the ragged layout every kernel of the evaluators takes."""
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def flip_positions(winner: torch.Tensor, kept_idx: torch.Tensor, n_kept: torch.Tensor, flags: torch.Tensor):
    """winner uint8 [V,H,W], kept_idx int32 [V,nq], n_kept int32 [V], flags int32 [V] (device) ->
    (counts int32 [V,nq] cpu, offsets int64 [V,nq] cpu, positions uint32 numpy [total])."""
    V, H, W = winner.shape
    nq = kept_idx.shape[1]
    labels = ops.rle_labels(winner, kept_idx, n_kept, flags)
    counts = ops.rle_transitions(labels, n_kept, nq)
    offsets = torch.cumsum(counts.view(-1).to(torch.int64), 0) - counts.view(-1).to(torch.int64)
    total = int(counts.sum().item())                                     # host sync (sizes the positions buffer)
    pos = torch.empty(max(total, 1), device=winner.device, dtype=torch.int32)
    if total:
        ops.rle_transitions(labels, n_kept, nq, offsets=offsets.view(V, nq), positions=pos)
    return counts.cpu(), offsets.view(V, nq).cpu(), pos[:total].cpu().numpy().view(np.uint32)


def compress(positions: np.ndarray, H: int, W: int):
    """One mask's ascending flip positions -> (counts bytes, bbox [x,y,w,h] list of float)."""
    positions = np.ascontiguousarray(positions, dtype=np.uint32)
    cap = 6 * (len(positions) + 1)
    buf = ctypes.create_string_buffer(cap)
    bbox = (ctypes.c_double * 4)()
    fn = _C.nopesac_rle_compress_host
    n = fn(positions.ctypes.data if len(positions) else None, len(positions), H, W, ctypes.cast(buf, ctypes.c_void_p), cap,
           ctypes.cast(bbox, ctypes.c_void_p))
    if n < 0:                                             # the result is a value: the string's length, or NPS_E_ARG
        _lib.check(n, fn.__name__)
    return buf.raw[:n], [float(b) for b in bbox]


def compress_batch(positions: np.ndarray, offsets: np.ndarray, counts: np.ndarray, H: int, W: int):
    """All masks of a batch in ONE library call: -> (list of counts bytes, bbox float64 [n,4])."""
    n = int(len(counts))
    positions = np.ascontiguousarray(positions, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    cap = 6 * (int(counts.sum()) + n) + 16
    buf = np.empty(cap, np.uint8)
    out_off = np.empty(n + 1, np.int64)
    bbox = np.empty((max(n, 1), 4), np.float64)
    fn = _C.nopesac_rle_compress_batch_host
    r = fn(positions.ctypes.data if positions.size else None, offsets.ctypes.data, counts.ctypes.data, n, H, W, buf.ctypes.data, cap,
           out_off.ctypes.data, bbox.ctypes.data)
    if r < 0:                                             # the result is a value: the total length, or NPS_E_ARG
        _lib.check(int(r), fn.__name__)
    raw = buf.tobytes()
    return [raw[out_off[i]:out_off[i + 1]] for i in range(n)], bbox[:n]


def encode_views(winner: torch.Tensor, kept_idx: torch.Tensor, n_kept: torch.Tensor, flags: torch.Tensor, n_kept_host=None) -> List[List[dict]]:
    """Per view, per kept plane (query order): {"segmentation": {"size": [H,W], "counts": bytes}, "bbox": [x,y,w,h]}.
    Flip positions AND the compressed strings are produced on the device (csrc/rle.hip); the host receives the finished byte
    strings (about 2 bytes per run instead of 4 per flip position) in one copy and only slices them.
    n_kept_host: n_kept as a Python list, when the caller has it already."""
    V, H, W = winner.shape
    nq = kept_idx.shape[1]
    labels = ops.rle_labels(winner, kept_idx, n_kept, flags)
    counts = ops.rle_transitions(labels, n_kept, nq)
    c64 = counts.view(-1).to(torch.int64)
    ends = torch.cumsum(c64, 0)
    offsets = (ends - c64).contiguous()
    total = int(ends[-1].item())                                         # host sync (sizes the positions buffer)
    pos = torch.empty(max(total, 1), device=winner.device, dtype=torch.int32)
    if total:
        ops.rle_transitions(labels, n_kept, nq, offsets=offsets.view(V, nq), positions=pos)
    data, out_off, lens, bbox = ops.rle_compress(pos, offsets, counts.view(-1).contiguous(), H, W)
    need = {"data": data, "out_off": out_off, "lens": lens, "bbox": bbox}
    if n_kept_host is None:
        need["n_kept"] = n_kept
    h = ops.gather_to_host(need)
    raw = h["data"].numpy().tobytes()
    out_off, lens, bbox = h["out_off"].tolist(), h["lens"].tolist(), h["bbox"].tolist()
    n_list = n_kept_host if n_kept_host is not None else h["n_kept"].tolist()
    out = []
    for v in range(V):
        row = []
        for p in range(n_list[v]):
            k = v * nq + p
            row.append({"segmentation": {"size": [H, W], "counts": raw[out_off[k]:out_off[k] + lens[k]]}, "bbox": bbox[k]})
        out.append(row)
    return out


class PendingRLE:
    """encode_views split in two so that a caller with several batches in flight never issues device work when it FETCHES results
    (a kernel enqueued behind other batches' launches waits for them; measured 6.8 ms per 32-pair step at the drop-in boundary):
    the constructor enqueues everything on the current stream - labels, flip positions (worst-case sized buffer: at most 2 flips
    per pixel and view), compressed strings into a byte buffer of fixed capacity, and the fetch of its filled part (at most `host_cap`
    bytes) plus the offset / length / box tables into pinned host memory; `finish()` (after the stream has passed the fetch) only slices.
    Totals beyond `host_cap` cost one more copy, beyond `cap` the synchronous encode_views."""

    def __init__(self, winner, kept_idx, n_kept, flags, cap: int = 64 << 20, host_cap: int = 6 << 20, host=None):
        V, H, W = winner.shape
        nq = kept_idx.shape[1]
        self.args, self.shape, self.cap, self.host_cap = (winner, kept_idx, n_kept, flags), (V, H, W, nq), int(cap), int(min(host_cap, cap))
        labels = ops.rle_labels(winner, kept_idx, n_kept, flags)
        counts = ops.rle_transitions(labels, n_kept, nq)
        c64 = counts.view(-1).to(torch.int64)
        ends = torch.cumsum(c64, 0)
        offsets = (ends - c64).contiguous()
        pos = torch.empty(V * 2 * H * W, device=winner.device, dtype=torch.int32)       # upper bound of the flips; only the used part is touched
        ops.rle_transitions(labels, n_kept, nq, offsets=offsets.view(V, nq), positions=pos)
        self.data, out_off, lens, bbox, total = ops.rle_compress_capped(pos, offsets, counts.view(-1).contiguous(), H, W, self.cap)
        # only the bytes the strings fill travel (one pair: ~20 KB of the 6 MB window - 0.11 ms of PCIe time per call before)
        # (finish() copies everything it hands out: the fetch may sit in a captured graph and be rewritten by the next replay)
        self.fetch = ops.HostFetch({"head": self.data[:self.host_cap], "out_off": out_off, "lens": lens, "bbox": bbox},
                                   dynamic={"head": total}, host=host)

    def finish(self, n_kept_host) -> List[List[dict]]:
        """Only after the stream the constructor ran on has passed the fetch (event / synchronize)."""
        V, H, W, nq = self.shape
        h = self.fetch.views()
        out_off, lens, bbox = h["out_off"].tolist(), h["lens"].tolist(), h["bbox"].tolist()
        if not out_off:                                        # no views / no plane slots: nothing was encoded
            return [[] for _ in range(V)]
        total = out_off[-1] + lens[-1]
        if total > self.cap:                                   # (never seen: 64 MB of run-length strings in one batch)
            return encode_views(*self.args, n_kept_host=n_kept_host)
        raw = h["head"].numpy()[:min(total, self.host_cap)].tobytes()
        if total > self.host_cap:
            raw += self.data[self.host_cap:total].cpu().numpy().tobytes()
        out = []
        for v in range(V):
            row = []
            for p in range(n_kept_host[v]):
                k = v * nq + p
                row.append({"segmentation": {"size": [H, W], "counts": raw[out_off[k]:out_off[k] + lens[k]]}, "bbox": bbox[k]})
            out.append(row)
        return out


# ---- reading side (evaluation): what pycocotools.mask.iou does for the matching evaluator (mp3d_evaluation.py:806-812)
def counts_of(rle: dict) -> np.ndarray:
    """Run lengths of a COCO RLE dict: `counts` is either the list of an uncompressed RLE or the compressed bytes / str
    (cocoapi rleFrString: 5 data bits per character + continuation bit, runs > 2 stored as differences)."""
    c = rle["counts"]
    if not isinstance(c, (bytes, str)):
        return np.asarray(c, dtype=np.int64)
    if isinstance(c, str):
        c = c.encode("ascii")
    out, p = [], 0
    while p < len(c):
        x, k, more = 0, 0, True
        while more:
            ch = c[p] - 48
            x |= (ch & 0x1F) << (5 * k)
            more = bool(ch & 0x20)
            p += 1
            k += 1
            if not more and (ch & 0x10):
                x |= -1 << (5 * k)
        if len(out) > 2:
            x += out[-2]
        out.append(x)
    return np.asarray(out, dtype=np.int64)


def decode(rle: dict) -> np.ndarray:
    """bool [H,W] mask of a COCO RLE (column-major runs, starting with zeros)."""
    h, w = rle["size"]
    counts = counts_of(rle)
    assert int(counts.sum()) == h * w, "RLE run lengths do not cover the image"
    vals = (np.arange(len(counts)) & 1).astype(np.uint8)
    return np.repeat(vals, counts).reshape((h, w), order="F").astype(bool)


def iou(dt: List[dict], gt: List[dict], iscrowd=None) -> np.ndarray:
    """[len(dt), len(gt)] float64 mask IoU (intersection / union; iscrowd[j] truthy: intersection / area(dt), as cocoapi rleIou)."""
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)), np.float64)
    D = np.stack([decode(r).reshape(-1) for r in dt]).astype(np.float64)
    G = np.stack([decode(r).reshape(-1) for r in gt]).astype(np.float64)
    inter = D @ G.T
    ad, ag = D.sum(1)[:, None], G.sum(1)[None, :]
    crowd = np.zeros(len(gt), bool) if iscrowd is None else np.asarray(iscrowd, bool)
    union = np.where(crowd[None, :], ad, ad + ag - inter)
    return np.where(union > 0, inter / np.maximum(union, 1e-300), 0.0)


# ---- the same on the device (csrc/plane_eval.hip): strings -> runs -> bit-packed masks -> IoU by popcount
def decode_bits(rles: List[dict], device):
    """COCO RLE dicts (all of one `size`) -> (bits int32 [n, ceil(H W / 32)], area int32 [n]) on `device`: bit p & 31 of word p >> 5
    is pixel p = x H + y of the column-major scan.  Compressed `counts` (bytes / str) are parsed by nopesac_rle_string_runs,
    uncompressed lists are uploaded as runs; one upload and one launch per kind, whatever the number of masks.  One host sync (the
    `bad` flags).  Raises ValueError when the masks differ in size or a mask's runs do not cover exactly H W pixels (what decode()
    asserts on the host)."""
    device = torch.device(device)
    n = len(rles)
    sizes = {tuple(int(s) for s in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"decode_bits: masks of different sizes in one call: {sorted(sizes)}")
    if n == 0:
        return torch.empty((0, 0), device=device, dtype=torch.int32), torch.empty(0, device=device, dtype=torch.int32)
    H, W = next(iter(sizes))
    kinds = {True: [], False: []}                                       # compressed?
    for i, r in enumerate(rles):
        kinds[isinstance(r["counts"], (bytes, str))].append(i)
    parts = []
    if kinds[True]:
        strs = [rles[i]["counts"] for i in kinds[True]]
        strs = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strs]
        off = exclusive_offsets([len(s) for s in strs])
        blob = b"".join(strs)
        host = torch.from_numpy(np.concatenate([np.frombuffer(blob + bytes(-len(blob) % 8), np.uint8), off.view(np.uint8)]))
        dev = host.to(device)                                           # one upload: the bytes (padded to 8) and their offsets
        nb = host.numel() - off.nbytes
        data, str_off = dev[:int(off[-1])], dev[nb:].view(torch.int64)
        runs, n_runs = ops.rle_string_runs(data, str_off)
        parts.append((kinds[True], ops.rle_runs_to_bits(runs, str_off, n_runs, H, W)))
    if kinds[False]:
        lists = [np.asarray(rles[i]["counts"], dtype=np.int64).reshape(-1) for i in kinds[False]]
        off = exclusive_offsets([len(c) for c in lists])
        allc = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        if allc.size and (allc.min() < -2**31 or allc.max() >= 2**31):
            raise ValueError("decode_bits: a run length does not fit 32 bits")
        lens = np.diff(off)
        tail = np.concatenate([allc, lens, np.zeros((allc.size + lens.size) % 2, np.int64)]).astype(np.int32)
        dev = torch.from_numpy(np.concatenate([off, tail.view(np.int64)])).to(device)      # one upload: offsets, runs, counts
        run_off, tail = dev[:off.size], dev[off.size:].view(torch.int32)
        runs, n_runs = tail[:allc.size], tail[allc.size:allc.size + lens.size]
        parts.append((kinds[False], ops.rle_runs_to_bits(runs, run_off, n_runs, H, W)))
    if len(parts) == 1:
        bits, area, bad = parts[0][1]
    else:
        words = (H * W + 31) // 32
        bits = torch.empty((n, words), device=device, dtype=torch.int32)
        area = torch.empty(n, device=device, dtype=torch.int32)
        bad = torch.empty(n, device=device, dtype=torch.int32)
        for idx, (b, a, d) in parts:
            where = torch.as_tensor(idx, device=device)
            bits[where], area[where], bad[where] = b, a, d
    if bool(bad.any().item()):                                          # host sync
        which = torch.nonzero(bad).view(-1).tolist()
        raise ValueError(f"decode_bits: RLE run lengths do not cover the image (masks {which[:8]} of {n})")
    return bits, area


def polygon_bits(segmentations, H: int, W: int, device):
    """COCO polygon annotations -> (bits int32 [n, ceil(H W / 32)], area int32 [n]) on `device`, the layout of decode_bits.
    segmentations: per mask a list of polygons, each a flat [x0, y0, x1, y1, ...]; a mask is the union of its polygons.  What
    pycocotools.mask.frPyObjects(polygons, H, W) + merge compute (cocoapi rleFrPoly), bit for bit, by nopesac_poly_to_bits: one upload
    (coordinates and both offset tables), one launch whatever the number of masks, one host sync (the `bad` flags).  Raises ValueError
    before anything is uploaded for a polygon of odd length or of fewer than 6 numbers, and after the launch, naming the masks, when
    a mask has no polygon, a coordinate that is not finite or too large, or more boundary points than the library's cap.
    Departure from cocoapi: frPyObjects reads a whole list whose first element has exactly 4 numbers as bounding boxes; here every
    element is a polygon (4 numbers: ValueError)."""
    device = torch.device(device)
    H, W = int(H), int(W)
    n, words = len(segmentations), (H * W + 31) // 32
    polys = []
    for i, seg in enumerate(segmentations):
        for poly in seg:
            xy = np.asarray(poly, dtype=np.float64).reshape(-1)
            if xy.size % 2 or xy.size < 6:
                raise ValueError(f"polygon_bits: a polygon of mask {i} has {xy.size} numbers (an even count of at least 6 is needed)")
            polys.append(xy)
    if n == 0:
        return torch.empty((0, words), device=device, dtype=torch.int32), torch.empty(0, device=device, dtype=torch.int32)
    poly_off, mask_off = exclusive_offsets([xy.size // 2 for xy in polys]), exclusive_offsets([len(seg) for seg in segmentations])
    off = np.concatenate([poly_off, mask_off])
    xy = np.concatenate(polys) if polys else np.zeros(0, np.float64)
    dev = torch.from_numpy(np.concatenate([xy.view(np.int64), off])).to(device)      # one upload: coordinates, polygon and mask offsets
    d_xy, d_off = dev[:xy.size].view(torch.float64), dev[xy.size:]
    bits, area, bad = ops.poly_to_bits(d_xy, d_off[:poly_off.size], d_off[poly_off.size:], H, W)
    if bool(bad.any().item()):                                          # host sync
        which = torch.nonzero(bad).view(-1).tolist()
        raise ValueError(f"polygon_bits: no polygon, a coordinate that is not finite or too large, or too many boundary points "
                         f"(masks {which[:8]} of {n})")
    return bits, area


def segmentation_bits(segs, device, size=None):
    """decode_bits for COCO `segmentation` entries of either kind: every seg is an RLE dict (compressed or not) or a list of polygons.
    RLE dicts go through decode_bits, polygon lists through polygon_bits, the results come back in input order.  The image size is the
    common size of the RLE dicts of the call, else `size` = (H, W); ValueError when polygons come with neither, or when both are there
    and differ."""
    device = torch.device(device)
    n = len(segs)
    is_rle = [isinstance(s, dict) for s in segs]
    for s, r in zip(segs, is_rle):
        if not r and not isinstance(s, (list, tuple)):
            raise TypeError(f"segmentation_bits: a segmentation is an RLE dict or a list of polygons, not {type(s).__name__}")
    rles = [s for s, r in zip(segs, is_rle) if r]
    if len(rles) == n:
        return decode_bits(rles, device)
    sizes = {tuple(int(x) for x in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"segmentation_bits: masks of different sizes in one call: {sorted(sizes)}")
    given = None if size is None else tuple(int(x) for x in size)
    if sizes and given is not None and given not in sizes:
        raise ValueError(f"segmentation_bits: size {given} but the RLE masks of the call are {sorted(sizes)[0]}")
    if not sizes and given is None:
        raise ValueError("segmentation_bits: polygons need an image size - the call holds no RLE dict and no `size`")
    H, W = next(iter(sizes)) if sizes else given
    p_bits, p_area = polygon_bits([s for s, r in zip(segs, is_rle) if not r], H, W, device)
    if not rles:
        return p_bits, p_area
    r_bits, r_area = decode_bits(rles, device)
    bits = torch.empty((n, (H * W + 31) // 32), device=device, dtype=torch.int32)
    area = torch.empty(n, device=device, dtype=torch.int32)
    for want, b, a in ((True, r_bits, r_area), (False, p_bits, p_area)):
        where = torch.as_tensor([i for i, r in enumerate(is_rle) if r == want], device=device)
        bits[where], area[where] = b, a
    return bits, area


def iou_views(dt_views, gt_views, device, crowd=None, polygons: bool = False, size=None, decode: bool = True):
    """Decode and IoU for V views in one set of launches: dt_views / gt_views are per view the lists of prediction and GT
    segmentations (all of one image size), crowd per view the GT iscrowd flags or None (crowd=None: no crowd anywhere).  All masks are
    decoded once (decode_bits, or with polygons=True segmentation_bits at `size`), the three rows of exclusive offsets - predictions,
    GT, IoU blocks - travel in one upload (the crowd flags with them), one nopesac_mask_iou_bits launch takes every block.  Returns
    (iou float64 [sum n_dt n_gt] on the device, the offsets int64 [3, V + 1] on the device, the same on the host, the bits with the
    predictions' rows first).  decode=False: only the offsets; iou is empty and bits None.  No host sync besides the decode's."""
    device = torch.device(device)
    n_dt, n_gt = [len(d) for d in dt_views], [len(g) for g in gt_views]
    offs = np.stack([exclusive_offsets(n_dt), exclusive_offsets(n_gt), exclusive_offsets(np.multiply(n_dt, n_gt))])
    flags = np.zeros(0, np.uint8) if crowd is None else np.concatenate([np.zeros(k, np.uint8) if c is None else np.asarray(c, bool).astype(np.uint8)
                                                                        for c, k in zip(crowd, n_gt)])
    packed = np.concatenate([offs.reshape(-1), np.concatenate([flags, np.zeros(-flags.size % 8, np.uint8)]).view(np.int64)])
    dev = torch.from_numpy(packed).to(device)                            # one upload: the three offset rows and the crowd flags
    d_off, d_crowd = dev[:offs.size].view(3, -1), None if crowd is None else dev[offs.size:].view(torch.uint8)[:flags.size]
    if not decode:
        return torch.zeros(0, device=device, dtype=torch.float64), d_off, offs, None
    segs = [s for d in dt_views for s in d] + [s for g in gt_views for s in g]
    bits, area = segmentation_bits(segs, device, size=size) if polygons else decode_bits(segs, device)
    nd = int(offs[0, -1])
    iou, _ = ops.mask_iou_bits(bits[:nd], area[:nd], d_off[0], bits[nd:], area[nd:], d_off[1], d_crowd, d_off[2], int(offs[2, -1]),
                               max(n_dt), max(n_gt))
    return iou, d_off, offs, bits


def iou_device_views(views, device) -> List[np.ndarray]:
    """rle.iou for many views at once: views = [(dt RLEs, gt RLEs, iscrowd or None)] -> [len(dt), len(gt)] float64 matrices, bit
    for bit those of iou().  All masks of one image size go through ONE upload per kind, one decode and one nopesac_mask_iou_bits
    launch, whatever the number of views (iou_views); one copy back.  A GT entry may also be a polygon list (segmentation_bits; the
    size is the predictions'); a view without predictions or without GT is never decoded."""
    out = [np.zeros((len(v[0]), len(v[1])), np.float64) for v in views]
    by_size = {}
    for k, (dt, gt, _) in enumerate(views):
        if len(dt) and len(gt):
            by_size.setdefault(tuple(int(s) for s in dt[0]["size"]), []).append(k)
    for ks in by_size.values():
        dts, gts, crowds = zip(*(views[k] for k in ks))
        m, _, offs, _ = iou_views(dts, gts, device, crowd=crowds, polygons=True)
        m = m.cpu().numpy()
        for j, k in enumerate(ks):
            out[k] = m[offs[2, j]:offs[2, j + 1]].reshape(len(views[k][0]), len(views[k][1]))
    return out


def iou_device(dt: List[dict], gt: List[dict], iscrowd=None, device="cuda") -> np.ndarray:
    """rle.iou on the device: the same [len(dt), len(gt)] float64 matrix, bit for bit (the counts are exact integers and the
    quotient is the float64 quotient of the same two integers)."""
    return iou_device_views([(dt, gt, iscrowd)], device)[0]
