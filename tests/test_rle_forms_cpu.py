"""CPU half of the packaging sweep (tests/rle_forms.py): the case tables sit on the seams they claim, the character-count table is
asserted, the host compressors (nopesac_rle_compress_host / _batch_host) pass every string and box case and their strings decode back
to the masks, and the two numpy emulations of the partitioned kernels equal the references on every case - and stop doing so, on a
named case, for each of thirteen planted errors.  Runs without a GPU."""
import numpy as np
import pytest

from oracle import rle_oracle as R
from tests import rle_forms as S

CASES = S.compress_cases()
BATCH = S.batch_masks()


# ---------------------------------------------------------------------------------------------------------------------------- tables
def test_character_count_table():
    for x, n in S.CHARS.items():
        assert S.chars_needed(x) == n, x
        if x >= 0:
            assert len(R.to_string([x])) == n, x
        else:                                                           # 0, 1 - x, 0, 1: the fourth count is stored as 1 - (1 - x) = x
            assert len(R.to_string([0, 1 - x, 0, 1])) == 1 + S.chars_needed(1 - x) + 1 + n, x
    assert sorted(set(S.CHARS.values())) == [1, 2, 3, 4, 5, 6]
    for n in range(1, 6):                                               # both sides of every step, on both signs
        assert S.CHARS[2**(5 * n - 1) - 1] == n and S.CHARS[2**(5 * n - 1)] == n + 1
        assert S.CHARS[-2**(5 * n - 1)] == n and S.CHARS[-2**(5 * n - 1) - 1] == n + 1
    assert S.chars_needed(S.MAX_PIXELS) == 6 and S.chars_needed(-S.MAX_PIXELS) == 6 and S.chars_needed(2**29) == 7


def test_compress_cases_sit_where_they_claim():
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES)
    assert [len(by["m=%d" % m]["runs"]) for m in S.RUN_COUNTS] == list(S.RUN_COUNTS)
    for m in (257, 258, 259, 513, 1025):                                # the deltas that reach into the previous chunk are not zero
        r = by["m=%d" % m]["runs"]
        assert all(r[j] != r[j - 2] for j in range(256, min(260, m)))
    for c in CASES + BATCH:
        assert sum(c["runs"]) == c["H"] * c["W"] <= S.MAX_PIXELS and len(c["runs"]) <= 1025
    for x, n in S.CHARS.items():                                        # every stored value is in its string, with its length
        for j in (3, 4):
            runs = by["delta %d at %d" % (x, j)]["runs"]
            assert runs[j] - runs[j - 2] == x
            assert len(R.to_string(runs[:j + 1])) - len(R.to_string(runs[:j])) == n
        for j in (0, 1, 2):
            if x > 0:
                runs = by["raw %d at %d" % (x, j)]["runs"]
                assert runs[j] == x and len(R.to_string(runs[:j + 1])) - len(R.to_string(runs[:j])) == n
    assert any(c["runs"][0] == 0 and len(c["runs"]) % 2 == 0 for c in CASES)          # starts with ones and ends with ones
    a, b = by["extremes: min-y run 395, max-y run 601"], by["extremes: crossing run 901"]
    assert len(a["runs"]) == len(b["runs"]) == 1025
    edges = np.cumsum(a["runs"])
    assert edges[394] % 64 == 3 and (edges[601] - 1) % 64 == 60         # min-y from run 394 / 395, max-y from run 601
    assert S.bbox_ref(a) == [0.0, 3.0, 512.0, 58.0]
    edges = np.cumsum(b["runs"])
    assert edges[900] // 64 == 450 and (edges[901] - 1) // 64 == 451    # run 901 alone crosses a column
    assert sum(edges[j - 1] // 64 < (edges[j] - 1) // 64 for j in range(1, 1024, 2)) == 1
    assert S.bbox_ref(b) == [0.0, 0.0, 513.0, 64.0]
    assert [len(c["runs"]) == 1 for c in BATCH] == [False, True, False, False, True, False, False, True, False, False, False, True]


def test_transition_cases_sit_where_they_claim():
    assert [S.wave_range(N) for N in (16384, 16385, 32768, 32784, 49168)] == [1024, 2048, 2048, 3072, 4096]
    assert 49168 - 12 * 4096 == 16                                      # the last wave in use holds 16 pixels
    for N in S.TRANSITION_SIZES:
        names, lab, n_kept, nq = S.transition_case(N)
        Q = S.wave_range(N)
        assert lab.shape == (len(names), N) and lab.size <= 34 * 49168
        row = dict(zip(names, lab))
        assert S.flips_ref(row["even / 1"], 0).size == N and S.flips_ref(row["all / none"], 0).tolist() == [0]
        for period, tag in ((16, "16"), (1024, "1024"), (Q, "Q")):
            for shift in (-1, 0, 1):
                want = {b for b in range(period + shift, N, period)} | ({0, 1} & set(range(N)) if shift == 1 else set())
                assert set(S.flips_ref(row["%s k %+d / none" % (tag, shift)], 0).tolist()) == want, (N, tag, shift)
    for N in S.OFFSET_BYTE_SIZES:
        assert N % 16 == 0 and N in S.TRANSITION_SIZES
    lab, n_kept, nq = S.byte_compare_case()
    assert lab.shape == (2, 4096 + 16) and nq == 128
    loads = lab[0, :4096].reshape(256, 16)
    for j in range(16):
        assert sorted(loads[:, j].tolist()) == list(range(256))         # every byte value at every position of a 16-byte load
    pairs = set(zip(lab[0, :-1].tolist(), lab[0, 1:].tolist()))
    assert {(0xFF, 0x00), (0x00, 0x01), (0xFF, 0x7F), (0x7F, 0xFF), (0x80, 0x00), (0x7F, 0x80)} <= pairs
    w, kept, n = S.worst_case_winner(2, 37, 53)
    lab = S.labels_ref(w, kept, n, np.zeros(2, np.int32))
    assert sum(S.flips_ref(lab[0].reshape(-1), p).size for p in (0, 1)) == 2 * 37 * 53 - 1


def test_transition_layout_keeps_gaps():
    lab, n_kept, nq = S.slot_case(1025)
    counts, offsets, want = S.transition_layout(lab.reshape(3, -1), n_kept, nq)
    assert (counts[0] == 0).all() and (counts[1, 1:] == 0).all() and (counts[2] > 0).all()
    flat_off, flat_cnt = offsets.reshape(-1), counts.reshape(-1)
    assert (flat_off[1:] - (flat_off[:-1] + flat_cnt[:-1]) == S.GAP).all() and flat_off[0] == S.GAP
    assert want.size == flat_off[-1] + flat_cnt[-1] + S.GAP + S.GUARD
    assert (want == S.SENTINEL).sum() == want.size - counts.sum()


def test_labels_reference_on_a_hand_worked_map():
    winner = np.array([[[0x80 | 3, 3, 0x80 | 9], [0x80 | 5, 0x80 | 127, 5]]], np.uint8)
    kept = np.array([[5, 3, 127, -1]], np.int32)
    plain = S.labels_ref(winner, kept, np.array([3], np.int32), np.array([0], np.int32))
    assert plain.tolist() == [[[1, 0], [0xFF, 2], [0xFF, 0xFF]]]
    fall = S.labels_ref(winner, kept, np.array([2], np.int32), np.array([2], np.int32))
    assert fall.tolist() == [[[1, 0], [1, 0xFF], [0xFF, 0]]]
    w, kept, passed, clamped, flags = S.clamp_case()
    assert passed[0] > kept.shape[1] and passed[0] * 1 <= kept.size     # strictly inside the kept_idx buffer
    assert set(kept[1, :2]) <= set(kept[0])
    assert np.array_equal(S.labels_ref(w, kept, passed, flags), S.labels_ref(w, kept, clamped, flags))


# ------------------------------------------------------------------------------------------------------------------ host compressors
def test_host_compressor_every_case():
    from nopesac_amd import rle
    for c in CASES + BATCH:
        s, bbox = rle.compress(S.positions_of(c["runs"]), c["H"], c["W"])
        assert s == S.string_ref(c), c["name"]
        assert bbox == S.bbox_ref(c), c["name"]
        assert R.from_string(s) == c["runs"], c["name"]


def test_host_batch_compressor_with_gaps():
    from nopesac_amd import rle
    pos, offsets, counts = S.positions_layout(BATCH)
    strings, bbox = rle.compress_batch(pos.view(np.uint32), offsets, counts, BATCH[0]["H"], BATCH[0]["W"])
    assert strings == [S.string_ref(c) for c in BATCH]
    assert bbox.tolist() == [S.bbox_ref(c) for c in BATCH]
    assert (counts == 0).sum() == 4


def test_host_round_trip_every_case():
    from nopesac_amd import rle
    for c in CASES + BATCH:
        got = rle.decode({"size": [c["H"], c["W"]], "counts": S.string_ref(c)})
        assert np.array_equal(got, S.mask_of(c)), c["name"]
        words, area = S.bits_of(c)
        assert area == int(got.sum()) and words.size == (c["H"] * c["W"] + 31) // 32


# ------------------------------------------------------------------------------------------------------------------------ emulations
def _transition_maps():
    for N in S.TRANSITION_SIZES:
        names, lab, n_kept, nq = S.transition_case(N)
        for name, row in zip(names, lab):
            yield "N=%d %s" % (N, name), row


MAPS = list(_transition_maps())


def _transition_misses(plant):
    bad = []
    for name, row in MAPS:
        for p in (0, 1):
            ref = S.flips_ref(row, p)
            total, out = S.emulate_transitions(row, p, plant)
            if total != ref.size or not np.array_equal(out[:total], ref) or out[total] != S.SENTINEL:
                bad.append("%s p=%d" % (name, p))
    return bad


def test_transition_emulation_equals_the_reference():
    assert _transition_misses(None) == []
    lab, n_kept, nq = S.byte_compare_case()
    for p in range(128):
        total, out = S.emulate_transitions(lab[0], p)
        assert out[:total].tolist() == S.flips_ref(lab[0], p).tolist()


@pytest.mark.parametrize("plant", S.TRANSITION_PLANTS)
def test_transition_cases_notice_a_planted_error(plant):
    bad = _transition_misses(plant)
    print("%s: %d of %d (map, plane) pairs differ, first %s" % (plant, len(bad), 2 * len(MAPS), bad[:3]))
    assert bad, plant


def _compress_misses(plant):
    bad = []
    for c in CASES + BATCH:
        s, bbox = S.emulate_compress(S.positions_of(c["runs"]), c["H"], c["W"], plant)
        what = ("string " if s != S.string_ref(c) else "") + ("box" if bbox != S.bbox_ref(c) else "")
        if what:
            bad.append("%s (%s)" % (c["name"], what.strip()))
    return bad


def test_compress_emulation_equals_the_reference():
    assert _compress_misses(None) == []


@pytest.mark.parametrize("plant", S.COMPRESS_PLANTS)
def test_compress_cases_notice_a_planted_error(plant):
    bad = _compress_misses(plant)
    print("%s: %d of %d cases differ, first %s" % (plant, len(bad), len(CASES) + len(BATCH), bad[:3]))
    assert bad, plant
    box_only = plant in ("full flag", "even runs", "- (j % 2)")
    assert all(("string" in b) != box_only for b in bad), plant         # a box error leaves every string alone, and the reverse
