"""The augmentation kernels (csrc/augment.hip) against the numpy restatement of tests/augment_forms.py, bit for bit - the arithmetic is
integer plus correctly rounded f32 / f64, so no allowance applies anywhere - against Pillow's committed outputs (tests/golden/augment),
and through data.PairMapper.  The restatement itself is held to Pillow in test_augment_cpu.py."""
import os

import numpy as np
import pytest
import torch

from nopesac_amd import augment as AUG
from tests import augment_forms as A

pytestmark = pytest.mark.gpu
T = AUG.TILE
SIZES = [(1, 1), (1, 9), (7, 5), (37, 53), (T, T), (T + 1, T - 1), (2 * T + 3, 5), (T + 1, T + 4)]      # the last: a width that is a multiple of 4 but not of the tile
MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)


def _run(device, images, rows):
    """uint8 [n,H,W,3] numpy images under AugmentRow tuples -> the kernels' uint8 [n,H,W,3] result (from the CHW output)."""
    src = torch.from_numpy(np.ascontiguousarray(images)).to(device)
    out = AUG.augment(src, AUG.AugmentParams.from_rows(rows))
    torch.cuda.synchronize()
    assert out.shape == (len(rows), 3) + images.shape[1:3] and out.dtype == torch.uint8
    return out.permute(0, 2, 3, 1).cpu().numpy()


def _images(n, h, w, seed):
    return np.stack([A.noise_image(h, w, seed + k) if k % 3 else A.ramp_image(h, w) + np.uint8(k) for k in range(n)])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_stage_alone_and_the_full_chains(device, size):
    rows = list(A.STAGE_ROWS.values()) + list(A.CHAIN_ROWS.values()) + list(A.COLOUR_CHAIN_ROWS.values())
    names = list(A.STAGE_ROWS) + list(A.CHAIN_ROWS) + list(A.COLOUR_CHAIN_ROWS)
    images = _images(len(rows), *size, seed=10)
    got = _run(device, images, rows)
    for k, (name, row) in enumerate(zip(names, rows)):
        assert np.array_equal(got[k], A.apply_row(images[k], row)), (name, size)


@pytest.mark.parametrize("h,w,pad", [(37, 53, 40), (T + 1, T + 4, 40), (T + 1, T + 4, 41)], ids=["odd_width", "aligned", "misaligned_stride"])
def test_batch_with_different_rows_and_a_strided_source(device, h, w, pad):
    """Five images `pad` bytes further apart than their size (a wrong image stride), rows that differ (a branch that is not uniform per
    image): identity, contrast only, a full chain, identity, blur only.  Strides that keep and that break 4-byte alignment."""
    rows = [A.IDENTITY, A.STAGE_ROWS["contrast"], A.FULL_CHAIN, A.IDENTITY, A.STAGE_ROWS["blur_r1"]]
    images = _images(5, h, w, seed=20)
    stride = h * w * 3 + pad
    buf = torch.full((5 * stride,), 77, dtype=torch.uint8, device=device)
    views = [buf[k * stride:k * stride + h * w * 3].view(h, w, 3) for k in range(5)]
    for v, im in zip(views, images):
        v.copy_(torch.from_numpy(im))
    out = AUG.augment(views, AUG.AugmentParams.from_rows(rows))
    got = out.permute(0, 2, 3, 1).cpu().numpy()
    for k, row in enumerate(rows):
        assert np.array_equal(got[k], A.apply_row(images[k], row)), k
    assert np.array_equal(got[0], images[0]) and np.array_equal(got[3], images[3])


@pytest.mark.parametrize("size", [(37, 53), (T, T), (T + 1, T - 1), (2 * T + 3, 5), (5, 2 * T + 3)], ids=lambda s: "%dx%d" % s)
def test_blur_at_every_sigma(device, size):
    """Image edges that fall inside a tile, and the box radius going from 0 to 1 between 1.4142 and 1.4143."""
    rows = [A.row_of(blur=True, sigma=s) for s in A.SIGMAS]
    images = _images(len(rows), *size, seed=30)
    got = _run(device, images, rows)
    for k, s in enumerate(A.SIGMAS):
        assert np.array_equal(got[k], A.blur(images[k], s)), (s, size)


def test_contrast_mean(device):
    """The pre-pass's integer: the largest sum (all 255 at 480 x 640), a mean of k + 0.5 exactly, a sum over clipped values (contrast
    behind brightness 1.8).  Contrast 0.2 moves nearly every value by 0.8 per unit of the mean."""
    c02 = A.row_of(True, (A.C, A.B, A.S, A.Hh), (1.0, 0.2, 1.0, 0.0))
    white = np.full((1, 480, 640, 3), 255, np.uint8)
    assert A.contrast_input_mean(white[0], c02) == 255
    assert np.array_equal(_run(device, white, [c02])[0], A.apply_row(white[0], c02))
    big = _images(1, 480, 640, seed=40)
    assert np.array_equal(_run(device, big, [c02])[0], A.apply_row(big[0], c02))
    half = np.full((1, 8, 6, 3), 10, np.uint8)                           # grey pixels: luma = value; 24 of 10, 24 of 11: mean 10.5
    half[0, 4:] = 11
    assert int(A.luma(half[0]).astype(np.int64).sum()) * 2 == 21 * 48 and A.contrast_mean(half[0]) == 11
    assert np.array_equal(_run(device, half, [c02])[0], A.apply_row(half[0], c02))
    clipped = A.row_of(True, (A.B, A.C, A.S, A.Hh), (1.8, 0.2, 1.0, 0.0))
    img = _images(2, 37, 53, seed=41)[1:]
    assert A.contrast_input_mean(img[0], clipped) < int(1.8 * A.contrast_mean(img[0]))          # the sum is over clipped values
    assert np.array_equal(_run(device, img, [clipped])[0], A.apply_row(img[0], clipped))


@pytest.fixture(scope="module")
def colour_hsv():
    colours = A.all_colours()
    return colours, A.rgb2hsv(colours)


@pytest.mark.parametrize("factor", (-0.2, 0.0137, 0.2))
def test_hue_over_every_colour(device, colour_hsv, factor):
    colours, hsv = colour_hsv
    want = hsv.copy()
    want[..., 0] += np.uint8(A.hue_shift(factor))
    want = A.hsv2rgb(want)
    got = _run(device, colours[None], [A.row_of(True, (A.Hh, A.B, A.C, A.S), (1.0, 1.0, 1.0, factor))])[0]
    assert np.array_equal(got, want)


def test_both_output_forms_and_guard_bytes(device):
    """CHW uint8 = the transposed HWC result; NHWC f32 = ops.preprocess of the float CHW image bit for bit, pad channel zero; nothing
    is written around either output or around a workspace of exactly the stated size."""
    from nopesac_amd import _lib, ops
    h, w, n = 37, 53, 3
    rows = [A.FULL_CHAIN, A.IDENTITY, A.CHAIN_ROWS["contrast_last"]]
    images = _images(n, h, w, seed=50)
    want = np.stack([A.apply_row(images[k], rows[k]) for k in range(n)])
    params = AUG.AugmentParams.from_rows(rows).to(device)
    mean, std = torch.tensor(MEAN, device=device), torch.tensor(STD, device=device)
    G = 256
    need = ops.augment_workspace_bytes(n, h, w)
    sizes = {"chw": n * 3 * h * w, "nhwc": n * h * w * 4 * 4, "ws": need}
    bufs = {k: torch.full((G + v + G,), 0xA5, dtype=torch.uint8, device=device) for k, v in sizes.items()}
    chw = bufs["chw"][G:G + sizes["chw"]].view(n, 3, h, w)
    nhwc = bufs["nhwc"][G:G + sizes["nhwc"]].view(torch.float32).view(n, h, w, 4)
    ws = bufs["ws"][G:G + need]
    src = torch.from_numpy(images).to(device)
    _lib.C.nopesac_augment_u8(src.data_ptr(), n, h * w * 3, h, w, 3, params.rows.ctypes.data, params.device_rows.data_ptr(), chw.data_ptr(),
                              nhwc.data_ptr(), mean.data_ptr(), std.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(chw.cpu().numpy(), want.transpose(0, 3, 1, 2))
    ref = ops.preprocess(torch.from_numpy(want.transpose(0, 3, 1, 2).copy()).to(device).float(), mean, std, 4, torch.float32)
    assert nhwc.view(torch.int32).equal(ref.view(torch.int32)) and not nhwc[..., 3].any()
    for k, b in bufs.items():
        assert bool((b[:G] == 0xA5).all()) and bool((b[-G:] == 0xA5).all()), k
    # each form alone gives the same values
    only_nhwc = AUG.augment(src, params, chw=False, normalized=True, mean=mean, std=std)
    assert only_nhwc.view(torch.int32).equal(ref.view(torch.int32))
    assert AUG.augment(src, params).equal(chw)


@pytest.mark.parametrize("name", A.GOLDEN_CASES)
def test_against_pillows_committed_outputs(device, name):
    """The restatement equals Pillow bit for bit (test_augment_cpu.py: every recorded differing share is 0), so the kernels must too."""
    image, row, expected = A.load_golden(name)
    assert np.array_equal(_run(device, image[None], [row])[0], expected)


# --------------------------------------------------------------------------------------------------------------------- the mapper
def _cfg(augmentation):
    from nopesac_amd.config import get_cfg
    from tests.util import ROOT
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "inference_scannet.yaml"))
    cfg.DATALOADER.AUGMENTATION = augmentation
    return cfg


def _write_pairs(tmp_path, pairs, sizes=((242, 324),)):
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(5)
    entries = []
    for i in range(pairs):
        pair = {}
        for v in "01":
            h, w = sizes[(2 * i + int(v)) % len(sizes)]
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
            a = np.stack([128 + 90 * np.sin(xx / (9 + i) + yy / 14), 128 + 70 * np.cos(yy / (7 + int(v))) * np.sin(xx / 20), 120 + 100 * ((xx // 16 + yy // 12) % 2)], -1)
            f = tmp_path / ("%d_%s.jpg" % (i, v))
            Image.fromarray(np.clip(a + rng.normal(0, 4.0, a.shape), 0, 255).astype(np.uint8)).save(f, format="JPEG", quality=88, subsampling=2)
            pair[v] = {"file_name": str(f), "image_id": "%d-%s" % (i, v)}
        entries.append(pair)
    return entries


def _stack(items):
    return torch.stack([d[v]["image"] for v in "01" for d in items])          # batch_paths order


@pytest.mark.parametrize("sizes", [((242, 324),), ((242, 324), (121, 162))], ids=["one_size", "two_sizes"])
def test_training_mapper_augments_the_batch(device, tmp_path, sizes):
    from nopesac_amd import data
    B, seed, step = 3, 11, 4
    entries = _write_pairs(tmp_path, B, sizes)
    plain = data.PairMapper(_cfg(True), "scannet_train", device=device, uint8=True)
    base = _stack(plain.map_batch(entries))
    assert base.shape == (2 * B, 3, 480, 640)
    params = AUG.sample_params(2 * B, seed, step)
    assert params.rows["flags"].any()
    want = AUG.augment(base.permute(0, 2, 3, 1).contiguous(), params)
    for uint8 in (True, False):
        m = data.PairMapper(_cfg(True), "scannet_train", device=device, uint8=uint8, train=True, seed=seed)
        got = _stack(m.map_batch(entries, step=step))
        assert got.dtype == (torch.uint8 if uint8 else torch.float32) and got.equal(want if uint8 else want.float())
    # other splits of the same pairs: every image keeps its transform
    pieces = m.map_batch(entries[:1], step=step, first=0, total=B) + m.map_batch(entries[1:], step=step, first=1, total=B)
    assert _stack(pieces).equal(want.float())
    singles = [m.map_batch(entries[i:i + 1], step=step, first=i, total=B)[0] for i in (2, 0, 1)]
    assert _stack([singles[1], singles[2], singles[0]]).equal(want.float())
    assert not _stack(m.map_batch(entries, step=step + 1)).equal(want.float())
    host = data.PairMapper(_cfg(True), "scannet_train", uint8=True, train=True, seed=seed)      # no device: images handed over on the host
    got = _stack(host.map_batch(entries, step=step))
    assert got.device.type == "cpu" and got.equal(want.cpu())


def test_mapper_without_training_or_flag_is_unchanged(device, tmp_path):
    from nopesac_amd import data
    entries = _write_pairs(tmp_path, 2)
    for uint8 in (True, False):
        today = _stack(data.PairMapper(_cfg(False), "scannet_test", device=device, uint8=uint8).map_batch(entries))
        for cfg, train in ((_cfg(True), False), (_cfg(False), True)):
            m = data.PairMapper(cfg, "scannet_test", device=device, uint8=uint8, train=train, seed=3)
            assert not m.augmentation
            assert _stack(m.map_batch(entries, step=7)).equal(today) and _stack(m.map_batch(entries)).equal(today)


def test_host_decoded_files_go_through_the_same_kernels(device, tmp_path):
    """PNG files (decoded on the host) are uploaded and augmented by the same kernels."""
    pytest.importorskip("PIL")
    from PIL import Image
    from nopesac_amd import data
    entries = []
    for i in range(2):
        pair = {}
        for v in "01":
            f = tmp_path / ("%d_%s.png" % (i, v))
            Image.fromarray(A.noise_image(480, 640, seed=60 + 2 * i + int(v))).save(f)
            pair[v] = {"file_name": str(f), "image_id": "%d-%s" % (i, v)}
        entries.append(pair)
    base = _stack(data.PairMapper(_cfg(True), "scannet_train", device=device, uint8=True).map_batch(entries))
    m = data.PairMapper(_cfg(True), "scannet_train", device=device, uint8=True, train=True, seed=2)
    want = AUG.augment(base.permute(0, 2, 3, 1).contiguous(), AUG.sample_params(4, 2, 9))
    assert _stack(m.map_batch(entries, step=9)).equal(want)
