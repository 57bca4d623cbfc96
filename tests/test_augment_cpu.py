"""Training-time augmentation without a GPU: the numpy restatement of tests/augment_forms.py (what the kernels of csrc/augment.hip are
held to bit for bit in test_augment_gpu.py) against Pillow itself, the sampler's distribution and keying, and the C surface's argument
stage.  Measured against Pillow 12.2.0: every stage, RGB -> HSV over all 2^24 colours and the blur at every sigma are bit-equal, so the
recorded differing shares (augment_forms.HSV_H_DIFFERING_SHARE, BLUR_DIFFERING_SHARE) are all 0."""
import ctypes
import itertools

import numpy as np
import pytest

from nopesac_amd import _lib, augment as AUG
from tests import augment_forms as A

H = _lib.H
IMAGES = {"noise": A.noise_image(), "ramp": A.ramp_image()}


def _pil():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageFilter
    return Image, ImageEnhance, ImageFilter


@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("factor", A.BLEND_FACTORS)
def test_blends_equal_pillow(image, factor):
    Image, ImageEnhance, _ = _pil()
    a = IMAGES[image]
    im = Image.fromarray(a)
    f = float(np.float32(factor))
    for enhance, mine in ((ImageEnhance.Brightness, A.brightness), (ImageEnhance.Contrast, A.contrast), (ImageEnhance.Color, A.saturation)):
        assert np.array_equal(np.asarray(enhance(im).enhance(f)), mine(a, factor)), enhance.__name__


@pytest.mark.parametrize("image", sorted(IMAGES))
def test_grey_equals_pillow(image):
    Image, _, _ = _pil()
    a = IMAGES[image]
    assert np.array_equal(np.asarray(Image.fromarray(a).convert("L").convert("RGB")), A.grey(a))


@pytest.fixture(scope="module")
def colours():
    return A.all_colours()


def test_rgb_to_hsv_equals_pillow_on_every_colour(colours):
    """S and V exact; H exact too (recorded share of differing colours: 0, asserted without margin - the input is exhaustive)."""
    Image, _, _ = _pil()
    ref = np.asarray(Image.fromarray(colours).convert("HSV"))
    mine = A.rgb2hsv(colours)
    assert np.array_equal(ref[..., 1], mine[..., 1]) and np.array_equal(ref[..., 2], mine[..., 2])
    d = np.abs(ref[..., 0].astype(np.int32) - mine[..., 0])
    share = float((d > 0).mean())
    print("RGB -> HSV: H differs on a share of %.6f of all colours, by at most %d" % (share, d.max()))
    assert d.max() <= 1 and share == A.HSV_H_DIFFERING_SHARE


def test_hsv_to_rgb_equals_pillow_on_every_triple(colours):
    Image, _, _ = _pil()
    hsv = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(colours[..., c])) for c in range(3)])
    assert np.array_equal(np.asarray(hsv.convert("RGB")), A.hsv2rgb(colours))


@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("factor", A.HUE_FACTORS + (0.0137,))
def test_hue_equals_the_pil_path(image, factor):
    a = IMAGES[image]
    _pil()
    row = A.row_of(True, (A.Hh, A.B, A.C, A.S), (1.0, 1.0, 1.0, factor))
    assert np.array_equal(AUG.augment_pil(a, row), A.hue(a, factor))


@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("sigma", A.SIGMAS)
def test_blur_equals_pillow(image, sigma):
    """The target is bit equality; the condition is at most 1 grey level, and the recorded share of differing values per sigma (0)."""
    Image, _, ImageFilter = _pil()
    a = IMAGES[image]
    ref = np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=float(np.float32(sigma))))).astype(np.int32)
    d = np.abs(ref - A.blur(a, sigma))
    share = float((d > 0).mean())
    print("blur sigma %g on %s: weights %r, differing share %.6f, max %d" % (sigma, image, A.box_weights(sigma), share, d.max()))
    assert d.max() <= 1 and share <= A.BLUR_DIFFERING_SHARE[sigma]


def test_box_radius_switches_at_sqrt_two():
    assert [A.box_weights(s)[0] for s in A.SIGMAS] == [0, 0, 0, 0, 0, 1, 1, 1]
    assert all(3 * (A.box_weights(s)[0] + 1) <= AUG.APRON for s in A.SIGMAS + (float(AUG.MAX_SIGMA),))


@pytest.mark.parametrize("name", A.GOLDEN_CASES)
def test_whole_chain_equals_augment_pil(name):
    """One row with everything on per case (contrast first, last, after hue, before hue; with and without grey): the restatement, Pillow
    now, and Pillow when the fixture was written agree."""
    _pil()
    image, row, expected = A.load_golden(name)
    assert row == dict(A.CHAIN_ROWS, **A.COLOUR_CHAIN_ROWS)[name]
    assert row.jitter and row.blur and sorted(row.order) == [0, 1, 2, 3]
    mine = A.apply_row(image, row)
    assert np.array_equal(mine, AUG.augment_pil(image, row))
    assert np.array_equal(mine, expected)


def test_chain_cases_place_contrast():
    pos = {k: (r.order.index(A.C), r.order.index(A.Hh)) for k, r in A.CHAIN_ROWS.items()}
    assert pos["contrast_first"][0] == 0 and pos["contrast_last"][0] == 3
    assert pos["contrast_after_hue"][0] == pos["contrast_after_hue"][1] + 1 and pos["contrast_before_hue"][0] + 1 == pos["contrast_before_hue"][1]


# ------------------------------------------------------------------------------------------------------------------ the sampler
def test_rows_are_keyed_by_seed_step_and_position():
    a, b = AUG.sample_params(8, seed=7, step=3), AUG.sample_params(5, seed=7, step=3, first=3)
    assert a.rows[3:].tobytes() == b.rows.tobytes()
    assert a.rows.tobytes() != AUG.sample_params(8, seed=7, step=4).rows.tobytes()
    assert a.rows.tobytes() != AUG.sample_params(8, seed=8, step=3).rows.tobytes()
    assert a.rows.tobytes() == AUG.sample_params(8, seed=7, step=3).rows.tobytes()


def test_sampled_distribution():
    n = 20000
    t = AUG.sample_params(n, seed=1, step=0).rows
    for flag, p in ((AUG.JITTER, 0.2), (AUG.GREY, 0.2), (AUG.BLUR, 0.5)):
        k = int(((t["flags"] & flag) != 0).sum())
        assert abs(k - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (flag, k)
    assert not (t["flags"] & ~(AUG.JITTER | AUG.GREY | AUG.BLUR)).any()
    ranges = list(AUG.FACTOR_RANGE) + [AUG.SIGMA_RANGE]
    values = [t["factor"][:, k] for k in range(4)] + [t["sigma"]]
    for (lo, hi), v in zip(ranges, values):
        assert v.dtype == np.float32 and (v >= np.float32(lo)).all() and (v <= np.float32(hi)).all()
        tenth = np.minimum(((v.astype(np.float64) - lo) / (hi - lo) * 10).astype(int), 9)
        counts = np.bincount(np.maximum(tenth, 0), minlength=10)
        assert (counts > 0).all() and abs(counts[0] - n / 10) <= 4 * np.sqrt(n * 0.09) and abs(counts[9] - n / 10) <= 4 * np.sqrt(n * 0.09)
    orders = {tuple(o) for o in t["order"].tolist()}
    assert orders == set(itertools.permutations(range(4)))
    # the draws of one row do not move together: flags are independent of each other
    both = int((((t["flags"] & AUG.GREY) != 0) & ((t["flags"] & AUG.BLUR) != 0)).sum())
    assert abs(both - n * 0.1) <= 4 * np.sqrt(n * 0.1 * 0.9)


def test_identity_and_table_layout():
    t = AUG.AugmentParams.identity(3)
    assert len(t) == 3 and t.rows.dtype.itemsize == ctypes.sizeof(_lib._HEADER.structs["nopesac_aug_row"]) == 40
    assert t.row(1) == A.IDENTITY
    image = A.noise_image(7, 5)
    assert np.array_equal(A.apply_row(image, t.row(0)), image)
    rows = [A.STAGE_ROWS["hue"], A.CHAIN_ROWS["contrast_last"]]
    back = AUG.AugmentParams.from_rows(rows)
    assert [back.row(i) for i in range(2)] == rows and back[1].row(0) == rows[1] and len(back[0:1]) == 1


# -------------------------------------------------------------------------------------------------------------------- C surface
def test_python_constants_equal_the_header():
    assert (AUG.BRIGHTNESS, AUG.CONTRAST, AUG.SATURATION, AUG.HUE) == (0, 1, 2, 3) == tuple(AUG.OPS.index(o) for o in AUG.OPS)
    assert (AUG.JITTER, AUG.GREY, AUG.BLUR) == (H.NPS_AUG_JITTER, H.NPS_AUG_GREY, H.NPS_AUG_BLUR) == (1, 2, 4)
    assert (AUG.MAX_SIGMA, AUG.APRON, AUG.TILE) == (H.NPS_AUG_MAX_SIGMA, H.NPS_AUG_APRON, H.NPS_AUG_TILE)
    assert AUG.SIGMA_RANGE[1] <= AUG.MAX_SIGMA and H.NPS_AUG_OPS == 4


def _size(L, n, h, w):
    out = ctypes.c_int64(-7)
    assert L.nopesac_augment_workspace_bytes(n, h, w, ctypes.byref(out)) == 0
    return out.value


def test_size_entry_is_its_header_formula_and_never_negative():
    from nopesac_amd import ops
    L = _lib.load()
    assert "nopesac_augment_workspace_bytes" in _lib.STATUS           # the size comes back through a host pointer
    for n, h, w in ((1, 1, 1), (5, 37, 53), (64, 480, 640), (65535, 4096, 4096)):
        assert _size(L, n, h, w) == n * H.NPS_AUG_PARTIALS * 4 == ops.augment_workspace_bytes(n, h, w)
    for bad in (0, -1, -(1 << 20)):
        for args in ((bad, 480, 640), (64, bad, 640), (64, 480, bad), (bad, bad, bad)):
            assert _size(L, *args) == 0
    assert L.nopesac_augment_workspace_bytes(1, 1, 1, None) == H.NPS_E_ARG


def test_launcher_refuses_before_any_launch():
    """No device needed: every refusal comes from the host table and the scalar arguments."""
    L = _lib.load()
    E = H.NPS_E_ARG
    assert "nopesac_augment_u8" in _lib.STATUS
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n, hh, ww = 2, 8, 8
    need = _size(L, n, hh, ww)

    def call(rows, C=3, ws_bytes=need, ws=p):
        t = AUG.AugmentParams.from_rows(rows).rows
        return L.nopesac_augment_u8(p, n, hh * ww * 3, hh, ww, C, t.ctypes.data, p, p, None, None, None, ws, ws_bytes, None)

    good = A.CHAIN_ROWS["contrast_first"]
    assert call([good, good._replace(order=(0, 1, 2, 2))]) == E and b"permutation" in L.nopesac_last_error()
    assert call([good._replace(order=(0, 1, 2, 4)), good]) == E and b"permutation" in L.nopesac_last_error()
    above = np.nextafter(np.float32(AUG.MAX_SIGMA), np.float32(10))
    assert call([good, good._replace(sigma=above)]) == E and b"sigma" in L.nopesac_last_error()
    assert call([good, good._replace(sigma=0.0)]) == E and b"sigma" in L.nopesac_last_error()
    assert call([good, good], C=4) == E and b"channels" in L.nopesac_last_error()
    assert call([good, good], ws_bytes=need - 1) == E and b"workspace" in L.nopesac_last_error()
    assert call([good, good], ws=None) == E and b"workspace" in L.nopesac_last_error()
    assert call([good, good._replace(factors=(1.0, 1.0, 1.0, 0.6))]) == E and b"hue" in L.nopesac_last_error()
    t = AUG.AugmentParams.from_rows([good, good]).rows
    assert L.nopesac_augment_u8(p, n, hh * ww * 3, hh, ww, 3, t.ctypes.data, p, None, None, None, None, p, need, None) == E   # no output
