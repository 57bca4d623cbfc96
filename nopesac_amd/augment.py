"""Training-time image augmentation (cfg.DATALOADER.AUGMENTATION): the reference mapper's per-view transform
(data/planercnn_transforms.py:183-191)

    RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.2), RandomGrayscale(p=0.2), RandomApply([GaussianBlur(sigma in [0.1, 2.0])], p=0.5)

on the GPU (csrc/augment.hip: Pillow's 8-bit arithmetic per pixel, one launch chain for a batch) with the parameters drawn on the host:

  * `AugmentParams`   the parameter table, one row per image
  * `sample_params`   rows with the reference's distribution, row i a function of (seed, step, first + i) alone
  * `augment`         the table applied to a batch of uint8 device images
  * `augment_pil`     one row applied by Pillow itself on the host: the CPU counterpart, and what the tests hold the kernels to

Importable without a GPU and without the built library (only `augment` needs them).
"""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

from . import _lib

_H = _lib.H
BRIGHTNESS, CONTRAST, SATURATION, HUE = _H.NPS_AUG_BRIGHTNESS, _H.NPS_AUG_CONTRAST, _H.NPS_AUG_SATURATION, _H.NPS_AUG_HUE
JITTER, GREY, BLUR = _H.NPS_AUG_JITTER, _H.NPS_AUG_GREY, _H.NPS_AUG_BLUR
MAX_SIGMA, APRON, TILE = _H.NPS_AUG_MAX_SIGMA, _H.NPS_AUG_APRON, _H.NPS_AUG_TILE
OPS = ("brightness", "contrast", "saturation", "hue")

# nopesac_aug_row of include/nopesac_hip.h
ROW_DTYPE = np.dtype([("flags", "<i4"), ("order", "<i4", (4,)), ("factor", "<f4", (4,)), ("sigma", "<f4")])
assert ROW_DTYPE.itemsize == 40

AugmentRow = namedtuple("AugmentRow", "jitter order factors grey blur sigma")   # order: operation ids; factors: indexed by operation id

P_JITTER, P_GREY, P_BLUR = 0.2, 0.2, 0.5
FACTOR_RANGE = ((0.2, 1.8), (0.2, 1.8), (0.2, 1.8), (-0.2, 0.2))       # ColorJitter(0.8, 0.8, 0.8, 0.2)
SIGMA_RANGE = (0.1, 2.0)
_ORDERS = np.array(list(itertools.permutations(range(4))), np.int32)  # the 24 orders torch.randperm(4) can give


class AugmentParams:
    """The parameter table: a host array of nopesac_aug_row (`rows`: flags, order, factor, sigma) and, after .to(device), its copy in
    device memory.  The launcher checks the host rows before any launch; the kernels read the device rows."""

    def __init__(self, rows: np.ndarray, device_rows=None):
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        if rows.ndim != 1:
            raise ValueError("AugmentParams: a one-dimensional array of rows expected")
        self.rows, self.device_rows = rows, device_rows

    @classmethod
    def from_rows(cls, rows) -> "AugmentParams":
        """From AugmentRow tuples."""
        t = np.zeros(len(rows), ROW_DTYPE)
        for i, r in enumerate(rows):
            t[i] = ((JITTER if r.jitter else 0) | (GREY if r.grey else 0) | (BLUR if r.blur else 0), tuple(r.order), tuple(r.factors), r.sigma)
        return cls(t)

    @classmethod
    def identity(cls, n: int) -> "AugmentParams":
        """n rows that change nothing (no flag set; order and factors as ColorJitter would leave an image alone)."""
        t = np.zeros(int(n), ROW_DTYPE)
        t["order"] = np.arange(4)
        t["factor"] = (1.0, 1.0, 1.0, 0.0)
        t["sigma"] = 1.0
        return cls(t)

    def __len__(self) -> int:
        return len(self.rows)

    def __getitem__(self, idx) -> "AugmentParams":
        """A slice of the table, or row idx as a table of one row (host rows only: .to(device) again)."""
        return AugmentParams(self.rows[idx] if isinstance(idx, slice) else self.rows[[idx]])

    def row(self, i: int) -> AugmentRow:
        r = self.rows[i]
        f = int(r["flags"])
        return AugmentRow(bool(f & JITTER), tuple(int(o) for o in r["order"]), tuple(np.float32(x) for x in r["factor"]), bool(f & GREY),
                          bool(f & BLUR), np.float32(r["sigma"]))

    def to(self, device) -> "AugmentParams":
        import torch
        dev = torch.from_numpy(self.rows.view(np.int32).reshape(len(self.rows), 10)).to(device)
        return AugmentParams(self.rows, dev)


def _mix(z: np.ndarray) -> np.ndarray:
    """splitmix64's finaliser on uint64 arrays (wrap-around arithmetic)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _uniforms(seed: int, step: int, index: np.ndarray, draws: int) -> np.ndarray:
    """[len(index), draws] doubles in [0, 1): draw k of image `index` is a hash of (seed, step, index, k) and of nothing else, so it
    does not depend on the batch an image came in, on the rank that drew it, on numpy's generators or on what was drawn before."""
    with np.errstate(over="ignore"):
        key = _mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + _GOLD)
        key = _mix(key ^ _mix(np.uint64(step & 0xFFFFFFFFFFFFFFFF) + _GOLD + _GOLD))
        key = _mix(key ^ _mix(index.astype(np.uint64) * _GOLD + np.uint64(1)))
        bits = _mix(key[:, None] + (np.arange(1, draws + 1, dtype=np.uint64) * _GOLD)[None, :])
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def sample_params(n: int, seed: int, step: int, first: int = 0) -> AugmentParams:
    """n rows with the reference's distribution (torchvision's RandomApply / ColorJitter.get_params / RandomGrayscale, the reference's
    GaussianBlur): jitter with probability 0.2 - a uniform random order of the four operations, brightness / contrast / saturation
    factors uniform on [0.2, 1.8], hue on [-0.2, 0.2]; grey with probability 0.2; blur with probability 0.5, sigma uniform on [0.1, 2].
    Row i is a function of (seed, step, first + i): every view is drawn on its own, as the reference draws it, and a batch that is
    split differently or spread over ranks, or a run that is resumed at `step`, draws the same transform for the same image."""
    u = _uniforms(int(seed), int(step), np.arange(first, first + n, dtype=np.int64), 9)
    t = np.zeros(n, ROW_DTYPE)
    t["flags"] = (np.where(u[:, 0] < P_JITTER, JITTER, 0) | np.where(u[:, 6] < P_GREY, GREY, 0) | np.where(u[:, 7] < P_BLUR, BLUR, 0))
    t["order"] = _ORDERS[np.minimum((u[:, 1] * 24).astype(np.int64), 23)]
    for k, (lo, hi) in enumerate(FACTOR_RANGE):
        t["factor"][:, k] = np.clip((lo + (hi - lo) * u[:, 2 + k]).astype(np.float32), np.float32(lo), np.float32(hi))
    t["sigma"] = np.clip((SIGMA_RANGE[0] + (SIGMA_RANGE[1] - SIGMA_RANGE[0]) * u[:, 8]).astype(np.float32), np.float32(SIGMA_RANGE[0]),
                         np.float32(SIGMA_RANGE[1]))
    return AugmentParams(t)


def augment(images_u8, params: AugmentParams, *, chw: bool = True, normalized: bool = False, mean=None, std=None):
    """images_u8: uint8 device images of one size - a tensor [n,H,W,3] or a list of [H,W,3] views lying evenly spaced in one buffer (the
    GPU JPEG decoder's output) - in cfg.INPUT.FORMAT order.  Returns the uint8 [n,3,H,W] images (chw; the mapper's layout, what
    ToTensor() * 255 holds), the normalised f32 [n,H,W,4] images BackboneTrainer.forward takes (normalized; mean, std: f32[3] device
    tensors), or both as a tuple."""
    import torch
    from . import ops
    imgs = list(images_u8) if not isinstance(images_u8, torch.Tensor) else images_u8
    first = imgs[0]
    n, (H, W) = len(imgs), first.shape[:2]
    if len(params) != n:
        raise ValueError("augment: %d images, %d parameter rows" % (n, len(params)))
    if params.device_rows is None or params.device_rows.device != first.device:
        params = params.to(first.device)
    chw_out = torch.empty((n, 3, H, W), device=first.device, dtype=torch.uint8) if chw else None
    nhwc_out = torch.empty((n, H, W, 4), device=first.device, dtype=torch.float32) if normalized else None
    ops.augment_images(imgs, params, chw_out=chw_out, nhwc_out=nhwc_out, mean=mean, std=std)
    return (chw_out, nhwc_out) if (chw and normalized) else (chw_out if chw else nhwc_out)


def augment_pil(image_hwc_u8: np.ndarray, row: AugmentRow) -> np.ndarray:
    """One row applied by Pillow on the host, as the reference mapper applies it: Image.fromarray of the array as it lies in memory
    (planercnn_transforms.py:219-221 hands it the BGR image, so channel 0 is Pillow's red), torchvision's functional_pil operations."""
    from PIL import Image, ImageEnhance, ImageFilter
    im = Image.fromarray(np.ascontiguousarray(image_hwc_u8, dtype=np.uint8))
    for op in (row.order if row.jitter else ()):
        if op != HUE:
            im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(float(row.factors[op]))
        else:
            h, s, v = im.convert("HSV").split()
            h = Image.fromarray((np.asarray(h).astype(np.int64) + int(float(row.factors[op]) * 255)).astype(np.uint8))
            im = Image.merge("HSV", (h, s, v)).convert("RGB")
    if row.grey:
        im = im.convert("L").convert("RGB")
    if row.blur:
        im = im.filter(ImageFilter.GaussianBlur(radius=float(row.sigma)))
    return np.asarray(im)
