"""csrc/jpeg.hip held to libjpeg on written streams no encoder produces (tests/jpeg_streams.py; docs/kernels.md "JPEG sweep"): the device
coefficient buffer against the WRITER's coefficients (not a decoder), padding blocks included, and the pixels against
oracle.jpeg_oracle.reconstruct of those coefficients - every stream alone and its family as one batch, through the self-synchronising
lane decoder where a stream is long enough and through the one-wave-per-interval kernel.  Exact comparisons, no tolerance anywhere.
Reads nothing outside the repository."""
import numpy as np
import pytest
import torch

from tests import jpeg_streams as S

pytestmark = pytest.mark.gpu


def settle_pass(changed, i):
    """passes in which lanes of image i still moved (NOPESAC_JPEG_SYNC_PASSES: not settled)"""
    col = changed[:, i].tolist()
    return next((p for p, c in enumerate(col) if c == 0), len(col))


def check_batch(sts, device, parallel=True, bgr=False):
    """one decode chain; -> {name: (lanes, par_done, passes)} of the images that went to the lanes"""
    from nopesac_amd import jpeg
    stats = {}
    outs = jpeg.decode_batch([s.data for s in sts], device, bgr=bgr, parallel=parallel, stats=stats)
    torch.cuda.synchronize()
    coef, off = stats["coef"].cpu().numpy(), stats["coef_off"].numpy()
    assert len(outs) == len(sts)
    for i, (s, o) in enumerate(zip(sts, outs)):
        for ci, c in enumerate(s.coef):
            got = coef[off[i, ci]:off[i, ci] + c.size].reshape(c.shape)
            assert np.array_equal(got, c), ("coefficients", s.name, ci, parallel)
        got = o.cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (s.H, s.W, 3), s.name
        assert np.array_equal(got[..., ::-1] if bgr else got, s.pixels()), ("pixels", s.name, parallel, bgr)
    lanes = {}
    want_lanes = [S.n_lanes(s) if parallel else 0 for s in sts]
    assert ("par_done" in stats) == any(want_lanes)
    if any(want_lanes):
        done, changed = stats["par_done"].cpu(), stats["changed"].cpu()
        assert changed.shape == (S.PASSES, len(sts))
        for i, (s, n) in enumerate(zip(sts, want_lanes)):
            if n:                                          # settled exactly when no lane moved in the last pass
                assert int(done[i]) == (1 if int(changed[-1, i]) == 0 else 0), s.name
                lanes[s.name] = (n, int(done[i]), settle_pass(changed, i))
            else:
                assert int(done[i]) == 0 and int(changed[:, i].sum()) == 0, s.name
    return lanes


@pytest.mark.parametrize("parallel", [True, False], ids=["lanes", "serial"])
@pytest.mark.parametrize("family", sorted(S.ENTROPY))
def test_entropy_stage_gives_the_writers_coefficients(device, family, parallel):
    """code lengths behind the look-ahead, one-symbol tables, permuted table ids, both ends of every category, ZRL chains and blocks
    without EOB, DC prediction over more than 1024 blocks, stuffed FFs at every phase, restart intervals of every kind, the lane
    decoder's thresholds, lane counts and boundary sweep, periodic streams: every stream alone, then the family as one batch"""
    sts = S.ENTROPY[family]()
    seen = {}
    for s in sts:
        seen.update(check_batch([s], device, parallel))
    together = check_batch(sts, device, parallel)
    if parallel:
        assert set(seen) == set(together) == {s.name for s in sts if S.n_lanes(s)}
        for name, (n, done, passes) in sorted(together.items()):
            print("jpeg sweep: %-32s %4d lanes  %s after %2d passes (alone: %s after %d)" % (
                name, n, "settled" if done else "FELL THROUGH", passes, "settled" if seen[name][1] else "fell through", seen[name][2]))
        if family in ("lane_thresholds", "lane_counts"):   # random blocks re-align within a lane; whether a periodic or a constructed
            assert all(done for _, done, _ in together.values()), together        # stream settles is an observation (docs/kernels.md)


def test_all_zero_420_stream_falls_through_and_is_still_right(device):
    """periodic_flat_420 is an all-zero stream: from ANY bit, with ANY guess of the block phase, a lane reads (category 0, EOB) for ever,
    so its exit only ever carries its entry's phase along and the truth travels exactly one lane per pass from lane 0 - with more than
    NOPESAC_JPEG_SYNC_PASSES + 1 lanes, and a lane length (in blocks) that is no multiple of the six blocks of an MCU, lanes still move
    in the last pass: par_done stays 0 and the one-wave-per-interval kernel decodes the image on the device.  Coefficients and pixels
    are checked either way."""
    st = S.periodic()[1]
    assert st.name == "periodic_flat_420" and S.n_lanes(st) > S.PASSES + 1 and (S.SUB_BITS // 4) % 6 != 0
    lanes = check_batch([st], device, True)
    assert lanes[st.name][1:] == (0, S.PASSES), lanes


@pytest.mark.parametrize("family", sorted(S.IDCT))
def test_idct_gives_the_oracles_samples(device, family):
    """one coefficient of each sign at each zigzag position (amplitudes 1, 255, 1023, and through a 16-bit table), zero rows and columns,
    both clamps, dense blocks at the largest amplitude inside [-512, 511] before the range limit - and one block set beyond it, where
    the kernel follows jidctint.c's wrapping range-limit table (the oracle does; libjpeg-turbo's SIMD path saturates, no conforming
    encoder gets there)"""
    sts = S.IDCT[family]()
    for s in sts:
        check_batch([s], device)
    check_batch(sts, device, parallel=False)


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("family", sorted(S.COLOUR))
def test_upsampling_and_colour_give_the_oracles_pixels(device, family, bgr):
    """widths 1 .. 9 x heights 1 .. 5 in 4:4:4 / 4:2:2 / 4:2:0 (replication at dw <= 2, first and last column rules, clamped context
    rows, a thread's four pixels across a row end, the byte-wise tail, 16-byte image offsets in a batch of odd sizes); the 27 flat
    Y / Cb / Cr combinations and checkerboard chroma"""
    sts = S.COLOUR[family]()
    for s in sts:
        check_batch([s], device, bgr=bgr)
    check_batch(sts, device, bgr=bgr)
    check_batch(sts[::-1][:3] + sts[:3], device, bgr=bgr)


@pytest.mark.parametrize("parallel", [True, False], ids=["lanes", "serial"])
def test_mixed_batch_in_shuffled_order(device, parallel):
    """images for the lanes, images below the threshold, restart images and one image the lanes give up on, in one chain"""
    sts = S.mixed_batch()
    lanes = check_batch(sts, device, parallel, bgr=parallel)
    if parallel:
        assert lanes["periodic_flat_420"][1] == 0
        random = [name for name in lanes if name.startswith(("lanes_", "at_threshold", "multiple_of_sub"))]
        assert len(random) == 4 and all(lanes[name][1] for name in random), lanes
