"""GPU half of the packaging sweep (tests/rle_forms.py): rle_labels, rle_transitions (counting and writing pass), rle_compress (sizing,
writing and capped pass) and decode_masks of csrc/rle.hip, fed constructed label maps and constructed flip positions that put a flip,
a run or a box extreme on every seam of their partitions, and the reading kernels of plane_eval.hip on the strings that result.  Every
comparison is bit-exact; every output buffer is prefilled and compared whole, so a write outside a mask's own range fails the test."""
import numpy as np
import pytest
import torch

from tests import rle_forms as S

pytestmark = pytest.mark.gpu
CASES = S.compress_cases()
BATCH = S.batch_masks()


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------------------------- 1. rle_transitions
def _both_passes(lab, n_kept, nq, device, byte_offset=False):
    """Counting pass, then counting + writing pass into the sentinel layout; everything compared with the numpy reference."""
    from nopesac_amd import ops
    V, N = lab.shape
    counts, offsets, want = S.transition_layout(lab, n_kept, nq)
    if byte_offset:
        store = torch.empty(V * N + 1, device=device, dtype=torch.uint8)
        labels = store[1:].view(V, N, 1)
        labels.copy_(_dev(lab, device).view(V, N, 1))
        assert labels.data_ptr() % 16 == 1 and labels.is_contiguous()
    else:
        labels = _dev(lab, device).view(V, N, 1)
    nk = _dev(n_kept, device)
    c1 = ops.rle_transitions(labels, nk, nq)
    pos = torch.full((want.size,), S.SENTINEL, device=device, dtype=torch.int32)
    c2 = ops.rle_transitions(labels, nk, nq, offsets=_dev(offsets, device), positions=pos)
    return c1.cpu().numpy(), c2.cpu().numpy(), pos.cpu().numpy(), counts, offsets, want


def _assert_passes(got, names=None):
    c1, c2, pos, counts, offsets, want = got
    V, nq = counts.shape
    for v in range(V):
        for p in range(nq):
            tag = (names[v] if names else v, p)
            assert c1[v, p] == counts[v, p] and c2[v, p] == counts[v, p], tag
            lo = offsets[v, p]
            assert np.array_equal(pos[lo:lo + counts[v, p]], want[lo:lo + counts[v, p]]), tag
    assert np.array_equal(pos, want)                                    # and every gap and the tail still hold the sentinel


@pytest.mark.parametrize("N", S.TRANSITION_SIZES)
def test_transitions_patterns_on_every_seam(device, N):
    names, lab, n_kept, nq = S.transition_case(N)
    _assert_passes(_both_passes(lab, n_kept, nq, device), names)


@pytest.mark.parametrize("N", S.OFFSET_BYTE_SIZES)
def test_transitions_scalar_path_by_alignment_alone(device, N):
    names, lab, n_kept, nq = S.transition_case(N)
    aligned, shifted = _both_passes(lab, n_kept, nq, device), _both_passes(lab, n_kept, nq, device, byte_offset=True)
    _assert_passes(shifted, names)
    assert np.array_equal(aligned[2], shifted[2])


def test_transitions_byte_compare_every_value_against_every_plane(device):
    lab, n_kept, nq = S.byte_compare_case()
    _assert_passes(_both_passes(lab, n_kept, nq, device))


@pytest.mark.parametrize("N", (1025, 16400))
def test_transitions_slots(device, N):
    lab, n_kept, nq = S.slot_case(N)
    got = _both_passes(lab, n_kept, nq, device)
    _assert_passes(got)
    assert (got[0][0] == 0).all() and (got[0][1, 1:] == 0).all()        # planes p >= n_kept[v]: count 0 (and nothing written, above)


def test_transitions_worst_case_fills_the_pending_buffer_bound(device):
    from nopesac_amd import ops, rle
    from oracle import rle_oracle as R
    V, H, W = 2, 37, 53
    w, kept, n_kept = S.worst_case_winner(V, H, W)
    flags = np.zeros(V, np.int32)
    args = [_dev(a, device) for a in (w, kept, n_kept, flags)]
    counts = ops.rle_transitions(ops.rle_labels(*args), args[2], 2).cpu().numpy()
    assert counts.tolist() == [[H * W, H * W - 1]] * V
    assert counts.sum() == V * (2 * H * W - 1) <= V * 2 * H * W         # the bound rle.PendingRLE sizes its positions buffer by
    out = rle.encode_views(*args)
    pend = rle.PendingRLE(*args)
    torch.cuda.synchronize()
    assert pend.finish(n_kept.tolist()) == out
    for v in range(V):
        for p in range(2):
            ref = R.encode((w[v] & 0x7F) == p)
            assert out[v][p] == {"segmentation": ref, "bbox": R.to_bbox(ref).tolist()}


# ------------------------------------------------------------------------------------------------------------------------ 2. rle_labels
@pytest.mark.parametrize("nq", S.LABEL_NQ)
def test_labels_around_the_transpose_tile(device, nq):
    from nopesac_amd import ops
    for H in S.LABEL_H:
        for W in S.LABEL_W:
            w, kept, n_kept, flags = S.labels_case(H, W, nq)
            got = ops.rle_labels(*[_dev(a, device) for a in (w, kept, n_kept, flags)])
            assert got.shape == (3, W, H)
            assert np.array_equal(got.cpu().numpy(), S.labels_ref(w, kept, n_kept, flags)), (H, W)


def test_labels_clamp_n_kept_to_nq(device):
    from nopesac_amd import ops
    w, kept, passed, clamped, flags = S.clamp_case()
    got = ops.rle_labels(*[_dev(a, device) for a in (w, kept, passed, flags)]).cpu().numpy()
    same = ops.rle_labels(*[_dev(a, device) for a in (w, kept, clamped, flags)]).cpu().numpy()
    assert np.array_equal(got, same)
    assert np.array_equal(got, S.labels_ref(w, kept, clamped, flags))


# ---------------------------------------------------------------------------------------------------------------------- 3. rle_compress
def _compress_device(cases, device, cap=None):
    """Sizing pass, then the writing (cap None) or capped pass into a byte buffer prefilled with FILL that ends in a guard tail.
    -> (lens, out_off, bbox, total, bytes uint8 [total or cap, + GUARD])."""
    from nopesac_amd import ops
    H, W = cases[0]["H"], cases[0]["W"]
    pos, offsets, counts = S.positions_layout(cases)
    d_pos, d_off, d_cnt = _dev(pos, device), _dev(offsets, device), _dev(counts, device)
    n = len(cases)
    lens = torch.full((n,), -1, device=device, dtype=torch.int32)
    bbox = torch.full((n, 4), -1.0, device=device, dtype=torch.float64)
    ops._C.nopesac_rle_compress_device(d_pos.data_ptr(), d_off.data_ptr(), d_cnt.data_ptr(), n, H, W, lens.data_ptr(), bbox.data_ptr(), None, None,
                                       ops._stream())
    ends = torch.cumsum(lens.to(torch.int64), 0)
    out_off = (ends - lens).contiguous()
    total = int(ends[-1].item())
    out = torch.full(((total if cap is None else cap) + S.GUARD,), S.FILL, device=device, dtype=torch.uint8)
    if cap is None:
        ops._C.nopesac_rle_compress_device(d_pos.data_ptr(), d_off.data_ptr(), d_cnt.data_ptr(), n, H, W, None, None, out.data_ptr(),
                                           out_off.data_ptr(), ops._stream())
    else:
        ops._C.nopesac_rle_compress_device_capped(d_pos.data_ptr(), d_off.data_ptr(), d_cnt.data_ptr(), n, H, W, lens.data_ptr(), out.data_ptr(),
                                                  out_off.data_ptr(), cap, ops._stream())
    return lens.cpu().numpy(), out_off.cpu().numpy(), bbox.cpu().numpy(), total, out.cpu().numpy()


def test_compress_every_string_and_box_case(device):
    from nopesac_amd import ops
    for c in CASES:
        want = S.string_ref(c)
        lens, out_off, bbox, total, out = _compress_device([c], device)
        assert (lens.tolist(), out_off.tolist(), total) == ([len(want)], [0], len(want)), c["name"]
        assert out.tobytes() == want + bytes([S.FILL]) * S.GUARD, c["name"]
        assert bbox.tolist() == [S.bbox_ref(c)], c["name"]
        pos = S.positions_of(c["runs"]).view(np.int32)                  # the wrapper the packaging calls, on the same case
        data, _, _, box2 = ops.rle_compress(_dev(pos if pos.size else np.zeros(1, np.int32), device), torch.zeros(1, device=device, dtype=torch.int64),
                                            torch.tensor([pos.size], device=device, dtype=torch.int32), c["H"], c["W"])
        assert data.cpu().numpy().tobytes() == want and box2.tolist() == [S.bbox_ref(c)], c["name"]


def test_compress_batch_of_twelve(device):
    want = [S.string_ref(c) for c in BATCH]
    lens, out_off, bbox, total, out = _compress_device(BATCH, device)
    assert lens.tolist() == [len(s) for s in want] and total == sum(lens)
    assert out_off.tolist() == (np.cumsum(lens) - lens).tolist()
    assert out.tobytes() == b"".join(want) + bytes([S.FILL]) * S.GUARD
    assert bbox.tolist() == [S.bbox_ref(c) for c in BATCH]


def test_compress_capped_pass(device):
    from nopesac_amd import ops
    want = [S.string_ref(c) for c in BATCH]
    lens0, off0, _, total0, _ = _compress_device(BATCH, device)
    caps = S.capped_caps(lens0)
    assert caps == [0, off0[5] + lens0[5], off0[5] + lens0[5] - 1, total0 - 1, total0, total0 + 5]
    for cap in caps:
        lens, out_off, _, total, out = _compress_device(BATCH, device, cap=cap)
        assert (lens.tolist(), out_off.tolist(), total) == (lens0.tolist(), off0.tolist(), total0), cap
        assert np.array_equal(out, S.capped_expected(want, cap, cap + S.GUARD)), cap
    pos, offsets, counts = S.positions_layout(BATCH)                    # the wrapper: same tables, and the total it hands back
    cap = caps[1]
    data, out_off, lens, bbox, total = ops.rle_compress_capped(_dev(pos, device), _dev(offsets, device), _dev(counts, device), BATCH[0]["H"],
                                                               BATCH[0]["W"], cap)
    assert (lens.tolist(), out_off.tolist(), total.tolist()) == (lens0.tolist(), off0.tolist(), [total0])
    assert data.cpu().numpy().tobytes() == b"".join(want[:6])
    assert bbox.tolist() == [S.bbox_ref(c) for c in BATCH]


# ---------------------------------------------------------------------------------------------------------------------- 4. decode_masks
@pytest.mark.parametrize("H,W", S.DECODE_HW)
def test_decode_masks_sizes_and_misaligned_rows(device, H, W):
    from nopesac_amd import ops
    from nopesac_amd.modeling.meta_arch import decode_masks
    w, kept, n_kept, flags = S.decode_case(H, W)
    N, total = H * W, int(n_kept.sum())
    n64 = n_kept.astype(np.int64)
    d = [_dev(a, device) for a in (w, kept, n_kept, flags, np.cumsum(n64) - n64)]
    masks = torch.full((total * N + S.GUARD,), S.FILL, device=device, dtype=torch.uint8)
    ops._C.nopesac_decode_masks(*[t.data_ptr() for t in d], masks.data_ptr(), 3, H, W, 128, ops._stream())
    ref = torch.cat([decode_masks(torch.from_numpy(w[v]), torch.from_numpy(kept[v, :n_kept[v]]), bool(flags[v] & 2)) for v in range(3)])
    want = torch.cat([ref.to(torch.uint8).reshape(-1), torch.full((S.GUARD,), S.FILL, dtype=torch.uint8)])
    assert torch.equal(masks.cpu(), want)
    got = ops.decode_masks(*d[:4], total)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------------ 5. round trip
def test_device_decode_of_every_string_case(device):
    """rle.decode_bits (nopesac_rle_string_runs -> nopesac_rle_runs_to_bits) on the oracle's strings, 5- and 6-character counts among them."""
    from nopesac_amd import rle
    by_size = {}
    for c in CASES + BATCH:
        by_size.setdefault((c["H"], c["W"]), []).append(c)
    for (H, W), cases in by_size.items():
        bits, area = rle.decode_bits([{"size": [H, W], "counts": S.string_ref(c)} for c in cases], device)
        bits, area = bits.cpu().numpy(), area.cpu().numpy()
        for i, c in enumerate(cases):
            words, ones = S.bits_of(c)
            assert area[i] == ones and np.array_equal(bits[i], words), c["name"]
