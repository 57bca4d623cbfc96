"""tests/jpeg_streams.py on the CPU: every generated stream is a file libjpeg reads as the writer meant it (Pillow = the oracle's pixels,
the oracle's coefficients = the writer's), and the three host readers of its bytes (jpeg.parse(fast=False), nopesac_jpeg_prepare_scan,
csrc/jpeg_host.hip) agree with the oracle's parser and with each other.  Exact comparisons throughout."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from nopesac_amd import jpeg
from oracle import jpeg_oracle as J
from tests import jpeg_streams as S

FAMILIES = sorted(S.FAMILIES)


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("family", FAMILIES)
def test_pillow_and_the_oracle_read_what_the_writer_wrote(family):
    """J.decode = Pillow's decode and J.decode_coefficients = the writer's coefficients (which validates the writer); the one family
    inside the wrap region instead DIFFERS from Pillow: jidctint.c's range-limit table wraps where libjpeg-turbo's SIMD IDCT saturates"""
    for st in S.FAMILIES[family]():
        fr = J.parse(st.data)
        coef = J.decode_coefficients(fr)
        for got, want in zip(coef, st.natural()):
            assert got.shape == want.shape and np.array_equal(got, want), st.name
        px = J.reconstruct(fr, coef)
        assert px.shape == (st.H, st.W, 3) and np.array_equal(px, st.pixels()), st.name
        pil = _pillow(st.data)
        if st.wrap:
            d = np.abs(pil.astype(np.int32) - px.astype(np.int32))
            assert d.max() > 128, (st.name, int(d.max()))    # saturated against wrapped samples
        else:
            lo, hi = S.prelimit_range(st)
            assert -512 <= lo and hi <= 511, st.name
            assert np.array_equal(px, pil), st.name


@pytest.mark.parametrize("family", FAMILIES)
def test_host_readers_agree_with_the_oracle_parser(family):
    """as test_jpeg_cpu.test_product_parser_agrees_with_the_oracle_parser, on every generated stream; the writer's interval lengths on top"""
    for st in S.FAMILIES[family]():
        data = st.data
        a, b = jpeg.parse(data, fast=False), J.parse(data)
        g = J.geometry(b)
        fast = jpeg.parse(data)
        w, offs, cnts = jpeg._words(a.intervals)
        assert fast.intervals is None and np.array_equal(fast.words, w) and fast.seg_off == offs and fast.seg_cnt == cnts, st.name
        assert fast.seg_bytes == [len(q) for q in a.intervals] == st.seg_bytes, st.name
        assert (fast.width, fast.height, fast.dri, fast.mcux, fast.mcuy) == (a.width, a.height, a.dri, a.mcux, a.mcuy)
        assert (a.width, a.height, a.mcux, a.mcuy, a.dri) == (b["W"], b["H"], g["mcux"], g["mcuy"], b["dri"]) and (a.width, a.height) == (st.W, st.H)
        key = lambda c: (c["h"], c["v"], c["bw"], c["bh"], c["dw"], c["dh"], c["td"], c["ta"])
        assert [key(c) for c in a.comps] == [key(c) for c in b["comps"]] == [key(c) for c in fast.comps], st.name
        assert a.intervals == b["intervals"], st.name
        for c, d, q in zip(a.comps, b["comps"], st.qt):
            nat = np.zeros(64, np.int64)
            nat[S.ZIGZAG] = q
            assert np.array_equal(a.qt[c["tq"]].astype(np.int64), nat) and np.array_equal(b["q"][d["tq"]], nat), st.name
        assert n_lanes_of(fast) == S.n_lanes(st), st.name


def n_lanes_of(info):
    hb = jpeg.prepare_batch([info], True)
    return 0 if hb.n_lanes == 0 else int(hb.img32[0, 29])


@pytest.mark.parametrize("family", FAMILIES + ["mixed_batch"])
def test_native_batch_reader_equals_the_python_form(family, tmp_path):
    """csrc/jpeg_host.hip on the streams as files against parse() + prepare_batch(), array for array, one and four threads (as
    test_host_cpu.test_native_jpeg_batch_prepare_equals_the_python_form)"""
    sts = S.mixed_batch() if family == "mixed_batch" else S.FAMILIES[family]()
    paths = []
    for i, st in enumerate(sts):
        p = tmp_path / ("%03d_%s.jpg" % (i, st.name))
        p.write_bytes(st.data)
        paths.append(str(p))
    for parallel in (True, False):
        want = jpeg.prepare_batch([jpeg.parse(st.data) for st in sts], parallel)
        slow = jpeg.prepare_batch([jpeg.parse(st.data, fast=False) for st in sts], parallel)
        for thr in (1, 4):
            got, status = jpeg.prepare_files(paths, threads=thr, parallel=parallel)
            assert status is None and got is not None and got.n == want.n == len(sts)
            for name in ("img32", "img64", "tables", "seg32", "seg64", "words"):
                a, b, c = getattr(got, name), getattr(want, name), getattr(slow, name)
                assert a.shape == b.shape == c.shape and a.dtype == b.dtype, (name, parallel, thr)
                assert torch.equal(a, b) and torch.equal(b, c), (name, parallel, thr)
            assert (got.lane_img is None) == (want.lane_img is None) and (got.lane_img is None or torch.equal(got.lane_img, want.lane_img))
            assert (got.n_seg, got.n_lanes, got.n_blocks, got.max_px, got.coef_off, got.plane_off, got.out_off) == (
                want.n_seg, want.n_lanes, want.n_blocks, want.max_px, want.coef_off, want.plane_off, want.out_off)
            assert [(g.height, g.width) for g in got.infos] == [(st.H, st.W) for st in sts]
        if parallel:
            assert want.n_lanes == sum(-(-S.n_lanes(st) // 64) * 64 for st in sts)


def test_case_tables_name_every_threshold_from_the_library():
    """the thresholds of the lane families come from jpeg.py / the header, and the families reach what they are named after"""
    assert S.SUB_BITS == jpeg.SUB_WORDS * 32 and S.MIN_PAR == jpeg.PARALLEL_MIN_BYTES and S.PASSES == jpeg.SYNC_PASSES
    assert [S.n_lanes(s) for s in S.lane_counts()] == list(S.LANE_COUNTS)
    assert len(S.lane_boundary()) == 32 and all(S.n_lanes(s) > 0 for s in S.lane_boundary())
    assert len(S.upsample_sizes()) == 3 * 9 * 5 and {s.W % 4 for s in S.upsample_sizes()} == {0, 1, 2, 3}
    assert len(S.colour_values()) == 2 * 27 + 3 + 3


def test_which_colour_constants_one_unit_can_be_observed():
    """S.ycc with the true constants is the oracle's conversion on every Cb x Cr pair; a one-unit change of a 16-bit constant is
    observable on the 8-bit domain for -22554 and -46802 (both ways) and for 116130 - 1, and for NO input at all for 91881 +- 1 and
    116130 + 1: those libraries compute what the true one computes, so no decode test can fail on them (docs/kernels.md, JPEG sweep)"""
    v = np.arange(256)
    cb, cr = np.meshgrid(v, v)
    for y in (0, 128, 255):
        yy = np.full(cb.shape, y)
        assert np.array_equal(S.ycc(yy, cb, cr), J.ycc_to_rgb(yy, cb, cr))
    got = {(S.YCC[i], d): S.constant_observable(i, d) for i in range(4) for d in (-1, 1)}
    assert got == {(91881, -1): False, (91881, 1): False, (-22554, -1): True, (-22554, 1): True, (-46802, -1): True, (-46802, 1): True,
                   (116130, -1): True, (116130, 1): False}
