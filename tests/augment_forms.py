"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py (not collected: no test_ prefix): the numpy restatement of the
augmentation arithmetic (torchvision's PIL path over Pillow's 8-bit operations, nopesac_amd/csrc/augment.hip's header comment), the
cases, and the loader of the Pillow fixtures under tests/golden/augment/ (written by scripts/gen_augment_golden.py).

The restatement is held to Pillow on the CPU (test_augment_cpu.py) and the kernels to the restatement on the GPU, bit for bit."""
from __future__ import annotations

import os

import numpy as np

from nopesac_amd.augment import BRIGHTNESS, CONTRAST, HUE, SATURATION, AugmentRow

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment")

BLEND_FACTORS = (0.2, 0.55, 1.0, 1.37, 1.8)
HUE_FACTORS = (-0.2, 0.2)
SIGMAS = (0.1, 0.3, 0.5, 1.0, 1.4142, 1.4143, 1.5, 2.0)        # 1.4142 / 1.4143: box radius 0 below sqrt 2, 1 above
# measured by test_augment_cpu.py against Pillow 12.2.0 (docs/kernels.md): share of differing values, H over all 2^24 colours, the blur
# per sigma over the noise and the ramp image.  The restatement is exact, so the conditions "at most 1" never come into play.
HSV_H_DIFFERING_SHARE = 0.0
BLUR_DIFFERING_SHARE = {s: 0.0 for s in SIGMAS}


def noise_image(h: int = 48, w: int = 64, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp_image(h: int = 48, w: int = 64) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 4) % 256, (yy * 5) % 256, ((xx + yy) * 3) % 256], -1).astype(np.uint8)


def all_colours() -> np.ndarray:
    """Every 8-bit colour once, as one 4096 x 4096 image."""
    v = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 4096, 3))


# ---------------------------------------------------------------------------------------------------------------- the restatement
def luma(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg: np.ndarray, im: np.ndarray, factor) -> np.ndarray:
    """Image.blend(deg, im, factor): f32, multiply and add rounded separately, clipped, truncated."""
    d = deg.astype(f32)
    t = d + f32(factor) * (im.astype(f32) - d)
    return np.clip(t, 0, 255).astype(np.int32).astype(np.uint8)


def contrast_mean(a: np.ndarray) -> int:
    """int(mean(L) + 0.5) in integers."""
    s, count = int(luma(a).astype(np.int64).sum()), a.shape[0] * a.shape[1]
    return (2 * s + count) // (2 * count)


def brightness(a, factor):
    return blend(np.zeros_like(a), a, factor)


def contrast(a, factor):
    return blend(np.full_like(a, contrast_mean(a)), a, factor)


def saturation(a, factor):
    return blend(np.repeat(luma(a)[..., None], 3, -1), a, factor)


def grey(a):
    return np.repeat(luma(a)[..., None], 3, -1)


def rgb2hsv(a: np.ndarray) -> np.ndarray:
    """Convert.c rgb2hsv_row: colorsys.rgb_to_hsv with float variables and double literals - the sums 2.0 + rc - bc and h / 6.0 + 1.0
    run in f64 and are stored to f32, the scalings by 255.0 run in f64."""
    r, g, b = (a[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f32)
    s = cr / np.where(flat, 1, maxc).astype(f32)
    rc, gc, bc = (maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr
    h = np.where(r == maxc, (bc - gc).astype(f64), np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64)))
    h = h.astype(f32)
    hq = h.astype(f64) / 6.0 + 1.0
    h = (hq - np.floor(hq)).astype(f32)
    uh = np.where(flat, 0, np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255))
    us = np.where(flat, 0, np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255))
    return np.stack([uh, us, maxc], -1).astype(np.uint8)


def _round_half_away(x: np.ndarray) -> np.ndarray:          # C round() of a non-negative double
    fl = np.floor(x)
    return fl + (x - fl >= 0.5)


def hsv2rgb(a: np.ndarray) -> np.ndarray:
    """Convert.c hsv2rgb: colorsys.hsv_to_rgb; f and fs are float variables, fs * f a float product, everything else f64."""
    h, s, v = (a[..., i].astype(f32) for i in range(3))
    h6 = h.astype(f64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int32)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    v64 = v.astype(f64)
    p = np.clip(_round_half_away(v64 * (1.0 - fs.astype(f64))), 0, 255)
    q = np.clip(_round_half_away(v64 * (1.0 - (fs * f).astype(f64))), 0, 255)
    t = np.clip(_round_half_away(v64 * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))), 0, 255)
    i = i % 6
    out = np.stack([np.choose(i, [v64, q, p, p, t, v64]), np.choose(i, [t, v64, v64, q, p, p]), np.choose(i, [p, p, t, v64, v64, q])], -1)
    return np.where((a[..., 1] == 0)[..., None], v64[..., None], out).astype(np.uint8)


def hue_shift(factor) -> int:
    """np.uint8(hue_factor * 255): the f64 product truncated towards zero, a negative value modulo 256."""
    return int(float(f32(factor)) * 255) % 256


def hue(a, factor):
    hsv = rgb2hsv(a)
    hsv[..., 0] += np.uint8(hue_shift(factor))
    return hsv2rgb(hsv)


def box_weights(sigma):
    """BoxBlur.c _gaussian_blur_radius and ImagingHorizontalBoxBlur's weights: (radius, ww, fw).  f32 but for sqrt and floor (f64)."""
    radius = f32(sigma)
    s2 = f32(f32(radius * radius) / f32(3))
    L = f32(np.sqrt(12.0 * f64(s2) + 1.0))
    l = f32(np.floor((f64(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def box_pass(x: np.ndarray, r: int, ww: int, fw: int, axis: int) -> np.ndarray:
    n = x.shape[axis]
    idx = np.arange(n)
    x = x.astype(np.int64)
    acc = sum(np.take(x, np.clip(idx + d, 0, n - 1), axis=axis) for d in range(-r, r + 1))
    far = np.take(x, np.clip(idx - r - 1, 0, n - 1), axis=axis) + np.take(x, np.clip(idx + r + 1, 0, n - 1), axis=axis)
    return ((acc * ww + far * fw + (1 << 23)) >> 24).astype(np.uint8)


def blur(a, sigma):
    r, ww, fw = box_weights(sigma)
    for axis in (1, 1, 1, 0, 0, 0):
        a = box_pass(a, r, ww, fw, axis)
    return a


def apply_row(a: np.ndarray, row: AugmentRow) -> np.ndarray:
    """The whole chain of one row on a uint8 [H,W,3] image."""
    for op in (row.order if row.jitter else ()):
        a = (brightness, contrast, saturation, hue)[op](a, row.factors[op])
    if row.grey:
        a = grey(a)
    if row.blur:
        a = blur(a, row.sigma)
    return np.ascontiguousarray(a)


def contrast_input_mean(a: np.ndarray, row: AugmentRow) -> int:
    """The integer the contrast pre-pass must arrive at: int(mean(L) + 0.5) of the image as it stands when contrast runs."""
    for op in row.order:
        if op == CONTRAST:
            return contrast_mean(a)
        a = (brightness, contrast, saturation, hue)[op](a, row.factors[op])
    raise ValueError("no contrast in the order")


# ------------------------------------------------------------------------------------------------------------------------ cases
def row_of(jitter=False, order=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0, 0.0), grey=False, blur=False, sigma=1.0) -> AugmentRow:
    return AugmentRow(bool(jitter), tuple(order), tuple(f32(x) for x in factors), bool(grey), bool(blur), f32(sigma))


IDENTITY = row_of()
B, C, S, Hh = BRIGHTNESS, CONTRAST, SATURATION, HUE
# every stage alone
STAGE_ROWS = {
    "identity": IDENTITY,
    "brightness": row_of(True, (B, C, S, Hh), (1.37, 1.0, 1.0, 0.0)),
    "contrast": row_of(True, (B, C, S, Hh), (1.0, 0.55, 1.0, 0.0)),
    "saturation": row_of(True, (B, C, S, Hh), (1.0, 1.0, 1.8, 0.0)),
    "hue": row_of(True, (B, C, S, Hh), (1.0, 1.0, 1.0, -0.2)),
    "grey": row_of(grey=True),
    "blur_r0": row_of(blur=True, sigma=1.0),
    "blur_r1": row_of(blur=True, sigma=2.0),
}
# everything on; the four orders put contrast first, last, after hue and before hue
CHAIN_ROWS = {
    "contrast_first": row_of(True, (C, B, Hh, S), (1.37, 0.55, 1.8, 0.2), True, True, 1.5),
    "contrast_last": row_of(True, (S, Hh, B, C), (0.55, 1.8, 0.2, -0.2), True, True, 0.5),
    "contrast_after_hue": row_of(True, (B, Hh, C, S), (1.8, 1.37, 0.55, 0.0137), True, True, 2.0),
    "contrast_before_hue": row_of(True, (S, C, Hh, B), (0.2, 0.2, 1.37, -0.11), True, True, 1.0),
}
# the same chains without grey, so that the colour of the jitter reaches the blur
COLOUR_CHAIN_ROWS = {k + "_colour": r._replace(grey=False) for k, r in CHAIN_ROWS.items()}
FULL_CHAIN = CHAIN_ROWS["contrast_after_hue"]._replace(grey=False)


def load_golden(name: str):
    """(input image, AugmentRow, Pillow's output) of fixture `name`."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        row = AugmentRow(bool(z["jitter"]), tuple(int(o) for o in z["order"]), tuple(f32(x) for x in z["factors"]), bool(z["grey"]), bool(z["blur"]),
                         f32(z["sigma"]))
        return z["image"], row, z["expected"]


GOLDEN_CASES = tuple(CHAIN_ROWS) + tuple(COLOUR_CHAIN_ROWS)
