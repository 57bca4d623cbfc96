"""csrc/plane_eval.hip on the GPU: the RLE string parser against rle.counts_of, the rasteriser against rle.decode, the popcount IoU
against rle.iou (all exact: integer-derived), the true-positive assignment against tests/plane_eval_ref.py (flags and gt_id exact,
errors at 1e-9), and the evaluator built on them against the numbers the reference function produced on the fixture seeds
(tests/golden/J_plane_eval_*.npz; tolerance = 4 x the reference-vs-float64 gap stored there, floored at 1e-12)."""
import numpy as np
import pytest
import torch

from nopesac_amd import _lib
from oracle import rle_oracle as R
from tests import plane_eval_inputs as PI
from tests import plane_eval_ref as REF
from tests.util import gold

pytestmark = pytest.mark.gpu


def _counts_rle(counts, size=(1, 1)):
    return {"size": list(size), "counts": R.to_string([int(c) for c in counts])}


def _device_runs(strings, device):
    from nopesac_amd import ops
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    data = torch.from_numpy(np.frombuffer(b"".join(strings) + b"\0", np.uint8).copy())[:int(off[-1])].to(device)
    runs, n_runs = ops.rle_string_runs(data, torch.from_numpy(off).to(device))
    runs, n_runs = runs.cpu().numpy(), n_runs.cpu().numpy()
    return [runs[off[i]:off[i] + n_runs[i]] for i in range(len(strings))]


def _packed(mask):
    """uint32 words of a dense mask: bit p & 31 of word p >> 5, p = x H + y."""
    b = np.packbits(np.asarray(mask, bool).reshape(-1, order="F"), bitorder="little")
    return np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view(np.uint32)


def _blobs(rng, h, w, n):
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    lab = np.argmin((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2, 0)
    return np.stack([lab == k for k in range(n)])


def _noisy_mask(rng, h, w, flips):
    m = _blobs(rng, h, w, 3)[0]
    p = rng.integers(0, h * w, flips)
    m.reshape(-1)[p] ^= True
    return m


STRING_CASES = {
    "one character numbers": [3, 2, 5, 1, 4, 7, 15, 2, 9],
    "runs of 16 and more": [16, 31, 17, 40, 100, 33, 511, 20],
    "runs of 512 and more": [512, 3, 1024, 5000, 70000, 6, 100000, 1 << 20],
    "negative differences": [5, 100, 7, 3, 2, 1, 900, 0, 1, 0, 600, 2],
    "one run": [35],
    "two runs": [5, 30],
    "three runs": [5, 7, 23],
    "first run 0": [0, 10, 5, 0, 0, 20],
    "empty mask": [48 * 64],
    "full mask": [0, 48 * 64],
}


def test_string_parser_cases(device):
    from nopesac_amd import rle
    rng = np.random.default_rng(5)
    rles = [_counts_rle(c) for c in STRING_CASES.values()]
    rles.append({"size": [1, 1], "counts": b""})                                        # a 0-byte string: no run
    rles.append(_counts_rle(rng.integers(0, 40, 1000)))                                  # numbers and characters beyond one 256-chunk
    rles.append(_counts_rle(rng.integers(0, 3000, 777) * rng.integers(0, 2, 777)))       # multi-character numbers across chunk borders
    rles.append(R.encode(_noisy_mask(rng, 480, 640, 1500)))                               # a 480x640 mask with a few thousand runs
    got = _device_runs([r["counts"] for r in rles], device)
    for name, r, g in zip(list(STRING_CASES) + ["0 bytes", "1000 small", "777 mixed", "480x640"], rles, got):
        want = rle.counts_of(r)
        assert len(g) == len(want) and np.array_equal(g.astype(np.int64), want), name
    assert len(got[-1]) > 2000
    # n_masks = 1 and = 0
    one = _device_runs([rles[3]["counts"]], device)
    assert np.array_equal(one[0].astype(np.int64), rle.counts_of(rles[3]))
    assert _device_runs([], device) == []


@pytest.fixture(scope="module")
def encoded_views(device):
    """rle.encode_views on a seeded winner map: (masks bool [V][n,H,W], RLE dicts [V][n])."""
    from nopesac_amd import rle
    rng = np.random.default_rng(7)
    V, H, W, nq, n = 2, 48, 64, 8, 5
    masks = [_blobs(rng, H, W, n + 1)[:n] for _ in range(V)]                               # the last blob stays unclaimed
    winner = np.full((V, H, W), 7, np.uint8)
    for v in range(V):
        for k in range(n):
            winner[v][masks[v][k]] = (k + 1) | 0x80
    kept = np.full((V, nq), -1, np.int32)
    kept[:, :n] = np.arange(1, n + 1)
    out = rle.encode_views(torch.from_numpy(winner).to(device), torch.from_numpy(kept).to(device),
                           torch.full((V,), n, dtype=torch.int32, device=device), torch.zeros(V, dtype=torch.int32, device=device))
    return masks, [[e["segmentation"] for e in row] for row in out]


def test_string_parser_reads_the_device_encoder(device, encoded_views):
    from nopesac_amd import rle
    masks, segs = encoded_views
    flat = [s for row in segs for s in row]
    assert len(flat) == 10
    for s, g, m in zip(flat, _device_runs([s["counts"] for s in flat], device), [m for v in masks for m in v]):
        assert np.array_equal(g.astype(np.int64), rle.counts_of(s))
        assert np.array_equal(g.astype(np.int64), np.asarray(R.run_lengths(m)))
    bits, area = rle.decode_bits(flat, device)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), np.stack([_packed(m) for v in masks for m in v]))
    assert area.tolist() == [int(m.sum()) for v in masks for m in v]


def _check_bits(rles, device):
    from nopesac_amd import rle
    bits, area = rle.decode_bits(rles, device)
    h, w = rles[0]["size"]
    assert bits.shape == (len(rles), (h * w + 31) // 32) and bits.dtype == torch.int32
    got = bits.cpu().numpy().view(np.uint32)
    for i, r in enumerate(rles):
        dense = rle.decode(r)
        want = np.packbits(dense.reshape(-1, order="F"), bitorder="little")
        assert np.array_equal(got[i].view(np.uint8)[:len(want)], want), i
        assert not got[i].view(np.uint8)[len(want):].any()
        assert int(area[i]) == int(dense.sum())


def test_rasteriser_small_sizes(device):
    rng = np.random.default_rng(9)
    # N = 35 (no multiple of 32): compressed and uncompressed in one call
    m57 = [rng.uniform(size=(5, 7)) < 0.5 for _ in range(4)] + [np.zeros((5, 7), bool), np.ones((5, 7), bool)]
    _check_bits([R.encode(m) if i % 2 else {"size": [5, 7], "counts": R.run_lengths(m)} for i, m in enumerate(m57)], device)
    # N = 32 and N = 64, runs ending exactly on word borders
    _check_bits([{"size": [4, 8], "counts": c} for c in ([32], [0, 32], [16, 16], [0, 16, 16], [31, 1], [1, 31])], device)
    _check_bits([{"size": [8, 8], "counts": c} for c in ([32, 32], [0, 32, 32], [0, 64], [64], [32, 0, 32], [31, 2, 31], [0, 0, 0, 32, 0, 32])],
                device)
    # checkerboard: every run is 1 (N runs, many words per thread); one run over several whole words
    yy, xx = np.mgrid[0:48, 0:64]
    board = (yy + xx) % 2 == 0
    assert len(R.run_lengths(board)) > 48 * 64 - 64
    _check_bits([R.encode(board), {"size": [48, 64], "counts": R.run_lengths(~board)}, {"size": [48, 64], "counts": [40, 200, 48 * 64 - 240]},
                 R.encode(np.zeros((48, 64), bool)), R.encode(np.ones((48, 64), bool))], device)


@pytest.mark.parametrize("seed", PI.SEEDS)
def test_rasteriser_fixture_masks(device, seed):
    views = [v for _, v in PI.unique_views(PI.plane_eval_case(seed))]
    _check_bits([R.encode(m) for v in views for m in list(v["pred"]) + list(v["gt"])], device)


def test_rasteriser_480x640(device):
    rng = np.random.default_rng(3)
    m = _noisy_mask(rng, 480, 640, 1500)
    assert len(R.run_lengths(m)) > 2000
    _check_bits([R.encode(m), {"size": [480, 640], "counts": R.run_lengths(~m)}], device)


def test_rasteriser_bad_runs(device):
    """Runs that sum to N - 1 or N + 1, a negative run, a mask without runs: bad is set, the words are zero, and neither the good
    masks laid out around them nor the guard words around the buffer change (the buffer is larger than what the kernel may touch)."""
    from nopesac_amd import ops, rle
    H, W = 5, 13                                                                          # N = 65: 3 words, the last one nearly empty
    N, words = H * W, 3
    rng = np.random.default_rng(2)
    good = [R.run_lengths(rng.uniform(size=(H, W)) < 0.5) for _ in range(5)]
    bads = [[10, 20, N - 31], [10, 20, N - 29], [40, -5, N - 35], [], [N, 1], [70, -5]]
    lists = [good[0], bads[0], good[1], bads[1], good[2], bads[2], good[3], bads[3], bads[4], bads[5], good[4]]
    is_bad = [0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 0]
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(c) for c in lists], out=off[1:])
    runs = torch.tensor([c for l in lists for c in l], dtype=torch.int32, device=device)
    n_runs = torch.tensor([len(l) for l in lists], dtype=torch.int32, device=device)
    guard, n = 64, len(lists)
    buf = torch.full((guard + n * words + guard,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    bits, area, bad = ops.rle_runs_to_bits(runs, torch.from_numpy(off).to(device), n_runs, H, W, bits=buf[guard:guard + n * words])
    assert bad.tolist() == is_bad
    host = buf.cpu().numpy()
    assert (host[:guard] == 0x5A5A5A5A).all() and (host[-guard:] == 0x5A5A5A5A).all()
    got = host[guard:guard + n * words].view(np.uint32).reshape(n, words)
    for i, (l, b) in enumerate(zip(lists, is_bad)):
        if b:
            assert not got[i].any() and int(area[i]) == 0, i
        else:
            dense = rle.decode({"size": [H, W], "counts": l})
            assert np.array_equal(got[i], _packed(dense)) and int(area[i]) == int(dense.sum()), i
    for l in bads:
        with pytest.raises(ValueError, match="do not cover"):
            rle.decode_bits([{"size": [H, W], "counts": good[0]}, {"size": [H, W], "counts": l}], device)
    with pytest.raises(ValueError, match="do not cover"):
        rle.decode_bits([R.encode(np.ones((H, W), bool)), {"size": [H, W], "counts": R.to_string([N - 1])}], device)
    with pytest.raises(ValueError, match="different sizes"):
        rle.decode_bits([R.encode(np.ones((H, W), bool)), R.encode(np.ones((W, H), bool))], device)


def _ragged_iou(views, device):
    """views: [(dt RLEs, gt RLEs, iscrowd list)] -> per-view (iou [n_dt, n_gt], inter) from ONE mask_iou_bits launch."""
    from nopesac_amd import ops, rle
    n_dt, n_gt = [len(v[0]) for v in views], [len(v[1]) for v in views]
    bits, area = rle.decode_bits([r for v in views for r in v[0]] + [r for v in views for r in v[1]], device)
    offs = np.zeros((3, len(views) + 1), np.int64)
    np.cumsum(n_dt, out=offs[0, 1:]); np.cumsum(n_gt, out=offs[1, 1:]); np.cumsum(np.multiply(n_dt, n_gt), out=offs[2, 1:])
    d = torch.from_numpy(offs).to(device)
    crowd = torch.tensor([int(c) for v in views for c in v[2]], dtype=torch.uint8, device=device)
    nd = sum(n_dt)
    iou, inter = ops.mask_iou_bits(bits[:nd], area[:nd], d[0], bits[nd:], area[nd:], d[1], crowd if crowd.numel() else None, d[2],
                                   int(offs[2, -1]), max(n_dt), max(n_gt))
    iou, inter = iou.cpu().numpy(), inter.cpu().numpy()
    return [(iou[offs[2, v]:offs[2, v + 1]].reshape(n_dt[v], n_gt[v]), inter[offs[2, v]:offs[2, v + 1]].reshape(n_dt[v], n_gt[v]))
            for v in range(len(views))]


@pytest.mark.parametrize("size", [(5, 7), (48, 64)])
def test_iou_ragged_views_equal_the_host(device, size):
    from nopesac_amd import rle
    h, w = size
    rng = np.random.default_rng(h)

    def masks(n):
        return [R.encode(rng.uniform(size=(h, w)) < rng.uniform(0.1, 0.9)) for _ in range(n)]
    views = []
    for n_dt, n_gt in [(0, 0), (0, 3), (3, 0), (1, 1), (3, 5), (128, 50)]:
        views.append((masks(n_dt), masks(n_gt), [int(rng.integers(0, 2)) for _ in range(n_gt)]))
    # disjoint, identical and empty-vs-empty pairs; a full mask
    a = np.zeros((h, w), bool); a[:, : w // 2] = True
    special = [R.encode(a), R.encode(~a), R.encode(np.zeros((h, w), bool)), R.encode(np.ones((h, w), bool))]
    views.append((special, special, [0, 0, 0, 1]))
    got = _ragged_iou(views, device)
    for (dt, gt, crowd), (iou, inter) in zip(views, got):
        want = rle.iou(dt, gt, crowd)
        assert iou.dtype == np.float64 and iou.shape == want.shape and (iou == want).all()
        if len(dt) and len(gt):
            D = np.stack([rle.decode(r).reshape(-1) for r in dt]).astype(np.int64)
            G = np.stack([rle.decode(r).reshape(-1) for r in gt]).astype(np.int64)
            assert np.array_equal(inter, D @ G.T)
    s = got[-1][0]
    assert s[0, 1] == 0.0 and s[0, 0] == 1.0 and s[2, 2] == 0.0 and s[1, 1] == 1.0
    # the public single-view form
    dt, gt, crowd = views[4]
    assert (rle.iou_device(dt, gt, crowd, device=device) == rle.iou(dt, gt, crowd)).all()
    assert (rle.iou_device(dt, gt, device=device) == rle.iou(dt, gt)).all()
    assert rle.iou_device([], gt, device=device).shape == (0, 5) and rle.iou_device(dt, [], device=device).shape == (3, 0)


def test_iou_480x640(device):
    from nopesac_amd import rle
    rng = np.random.default_rng(1)
    gt = [R.encode(m) for m in _blobs(rng, 480, 640, 20)]
    dt = [R.encode(np.roll(m, (3, -5), (0, 1))) for m in _blobs(rng, 480, 640, 20)]
    got, want = rle.iou_device(dt, gt, [0] * 19 + [1], device=device), rle.iou(dt, gt, [0] * 19 + [1])
    assert got.shape == (20, 20) and (got == want).all() and (want > 0).sum() > 40


# ---- assignment
def _assign(views, device, thresholds=(0.5, 30.0, 0.3)):
    """views: [(iou [n,m] f64, score f32, pred_label, pred_plane, gt_label, gt_plane)] -> rows of ONE plane_ap_assign launch."""
    from nopesac_amd import ops
    n_dt, n_gt = [len(v[1]) for v in views], [len(v[4]) for v in views]
    offs = np.zeros((3, len(views) + 1), np.int64)
    np.cumsum(n_dt, out=offs[0, 1:]); np.cumsum(n_gt, out=offs[1, 1:]); np.cumsum(np.multiply(n_dt, n_gt), out=offs[2, 1:])
    d = torch.from_numpy(offs).to(device)

    def cat(i, dtype, width=1):
        a = np.concatenate([np.asarray(v[i], dtype).reshape(-1) for v in views]) if views else np.zeros(0, dtype)
        return torch.from_numpy(np.concatenate([a, np.zeros(width, dtype)])).to(device)[:a.size]      # (never an empty allocation)
    rows = ops.plane_ap_assign(cat(0, np.float64), d[2], d[0], d[1], cat(1, np.float32), cat(2, np.int32), cat(3, np.float32, 3),
                               cat(4, np.int32), cat(5, np.float32, 3), max(n_dt, default=0), max(n_gt, default=0), *thresholds)
    return rows.cpu().numpy(), offs[0]


def _compare_rows(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 1, 2, 3, 4, 5, 8, 9]], want[:, [0, 1, 2, 3, 4, 5, 8, 9]])          # score, label, flags, best_iou, gt_id
    assert np.array_equal(np.isnan(got[:, 6:8]), np.isnan(want[:, 6:8]))
    ok = ~np.isnan(want[:, 6])
    assert np.abs(got[ok, 6:8] - want[ok, 6:8]).max(initial=0.0) <= 1e-9


def _plane(normal, offset):
    n = np.asarray(normal, np.float64)
    return (n / np.linalg.norm(n) * offset).astype(np.float32)


def _tilted(deg):
    return [np.sin(np.deg2rad(deg)), 0.0, np.cos(np.deg2rad(deg))]


def test_assignment_covered_sets(device):
    gt_plane = np.stack([_plane([0, 0, 1], 2.0), _plane([0, 1, 0], 3.0)])
    # predictions 0 and 1 both pick GT 0; 1 has the higher score but a 45 degree normal error: it takes GT 0 for the mask and the
    # offset criterion only, so prediction 0 is a false positive there and a true positive for plane and normal
    iou = np.array([[0.8, 0.1], [0.7, 0.2], [0.1, 0.9], [0.2, 0.6]])
    score = np.array([0.6, 0.9, 0.5, 0.4], np.float32)
    pred_plane = np.stack([_plane(_tilted(5), 2.1), _plane(_tilted(45), 2.05), _plane([0, 1, 0], 3.0), _plane([0, 1, 0], 3.05)])
    view = (iou, score, [1, 1, 1, 1], pred_plane, [1, 1], gt_plane)
    got, _ = _assign([view], device)
    _compare_rows(got, REF.assign(*view))
    assert got[:, 2:6].tolist() == [[0, 1, 1, 0], [1, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0]]
    assert got[:, 9].tolist() == [0, 0, 1, 1]
    # label mismatch, IoU at the threshold (given as the double 0.5), first maximum of a tied IoU row
    iou = np.array([[0.9, 0.9, 0.1], [0.5, 0.2, 0.1], [0.1, 0.2, 0.75]])
    view = (iou, np.array([0.9, 0.8, 0.7], np.float32), [1, 1, 2], np.stack([gt_plane[0]] * 3), [1, 1, 1], np.stack([gt_plane[0]] * 3))
    got, _ = _assign([view], device)
    _compare_rows(got, REF.assign(*view))
    assert got[:, 9].tolist() == [0, 0, 2] and got[:, 2].tolist() == [1, 0, 0]


def test_assignment_iou_exactly_half_from_integer_areas(device):
    """intersection 2, areas 3 and 3: union 4, IoU = 0.5 exactly - not a true positive (`>` is strict); with one more common pixel
    (3 / 5) it is."""
    from nopesac_amd import evaluation as E
    gt = np.zeros((5, 7), bool); gt[0, 0:3] = True
    half = np.zeros((5, 7), bool); half[0, 1:4] = True
    more = np.zeros((5, 7), bool); more[0, 0:4] = True; more[1, 0] = True                    # inter 3, union 5
    plane = [0.0, 0.0, 2.0]
    for pred, tp in ((half, 0.0), (more, 1.0)):
        view = {"instances": [{"segmentation": R.encode(pred), "score": 0.9, "category_id": 0}], "pred_plane": np.array([plane], np.float32),
                "annotations": [{"segmentation": R.encode(gt), "plane": plane, "category_id": 1}]}
        rows = E.plane_rows([view], device)
        assert rows.shape == (1, 10) and rows[0, 8] == (0.5 if tp == 0.0 else 0.6) and rows[0, 2:6].tolist() == [tp] * 4
        assert rows[0, 9] == 0.0 and rows[0, 6] < 1e-6 and rows[0, 7] < 1e-6


def test_assignment_random_views_up_to_the_limits(device):
    """One launch over ragged views: 1, 64, 65 and 128 predictions (a lane owns two from 65 on), 1 ... 255 GT planes, a view without
    GT, tied scores, tied IoU rows, two categories."""
    rng = np.random.default_rng(4)
    views = []
    for n, m in [(1, 1), (64, 255), (65, 50), (128, 7), (37, 0), (128, 255), (9, 3)]:
        iou = np.round(rng.uniform(0, 1, (n, m)), 2)                                         # two decimals: tied maxima happen
        score = np.round(rng.uniform(0, 1, n), 1 if n > 20 else 3).astype(np.float32)        # tied scores in the larger views
        gt_plane = rng.normal(size=(m, 3)).astype(np.float32) * 2
        g = iou.argmax(1) if m else np.zeros(n, np.int64)
        base = gt_plane[g] if m else rng.normal(size=(n, 3)).astype(np.float32)
        pred_plane = (base * rng.uniform(0.8, 1.25, (n, 1)) + rng.normal(size=(n, 3)) * rng.choice([0.02, 0.3, 1.0], (n, 1))).astype(np.float32)
        views.append((iou, score, rng.integers(1, 3, n), pred_plane, rng.integers(1, 3, m), gt_plane))
    assert any(len(np.unique(v[1])) < len(v[1]) for v in views)
    got, off = _assign(views, device)
    want = [REF.assign(*v) for v in views]
    for i, w in enumerate(want):
        _compare_rows(got[off[i]:off[i + 1]], w)
    assert np.isnan(want[4][:, 6]).all() and (want[4][:, 9] == -1).all() and not want[4][:, 2:6].any()
    allw = np.concatenate(want)
    assert 0 < allw[:, 2].sum() < len(allw) and 0 < allw[:, 3].sum() < allw[:, 2].sum()
    assert _assign([], device)[0].shape == (0, 10)


def test_assignment_limits_are_argument_errors(device):
    from nopesac_amd import ops
    z = torch.zeros(4, dtype=torch.int64, device=device)
    f, i, d = (torch.zeros(8, dtype=t, device=device) for t in (torch.float32, torch.int32, torch.float64))
    for max_dt, max_gt in ((_lib.H.NPS_PLANE_MAX_QUERIES + 1, 1), (1, 256)):
        with pytest.raises(_lib.HipKernelError, match="at most 128 predictions and 255 GT"):
            ops.plane_ap_assign(d, z[:2], z[:2], z[:2], f[:0], i[:0], f[:0], i[:0], f[:0], max_dt, max_gt, 0.5, 30.0, 0.3)


# ---- the evaluator
@pytest.fixture(scope="module", params=PI.SEEDS)
def fixture_case(request):
    pairs = PI.plane_eval_case(request.param)
    return pairs, gold(f"J_plane_eval_{request.param}"), PI.reference_order_rows(pairs)


def _check_table(got, g, ref64):
    keys = [str(k) for k in g["keys"]]
    assert list(got) == keys
    values, gaps = g["values"].numpy(), g["gap_values"].numpy()
    for k, want, gap in zip(keys, values, gaps):
        if k.startswith("%"):
            assert got[k] == want, k
        else:
            assert abs(got[k] - want) <= max(4 * gap, 1e-12), (k, got[k], want, gap)
        assert abs(got[k] - ref64[k]) <= 1e-9, k


def test_evaluate_for_planes_against_the_reference(device, fixture_case):
    from nopesac_amd import evaluation as E
    pairs, g, ref_rows = fixture_case
    preds, dataset = PI.product_inputs(pairs)
    views = [{"instances": pv["instances"], "pred_plane": pv["pred_plane"], "annotations": dataset[key][v]["annotations"]}
             for (key, p) in zip(dataset, preds) for v, pv in p.items()]
    seen, uniq = set(), []
    for p, view in zip([pv for p in preds for pv in p.values()], views):
        if p["image_id"] not in seen and len(view["instances"]):
            uniq.append(view)
        seen.add(p["image_id"])
    rows = E.plane_rows(uniq, device)
    # per prediction, in the reference's order: flags exact, errors within 4 x the reference's own float32 gap
    order = np.concatenate([o + np.argsort(-rows[o:o + len(v["instances"]), 0], kind="stable")
                            for o, v in zip(np.cumsum([0] + [len(v["instances"]) for v in uniq[:-1]]), uniq)])
    r = rows[order]
    assert np.array_equal(r[:, 0], g["score"].numpy()) and np.array_equal(r[:, 2:6], g["flags"].numpy())
    assert np.abs(r[:, 6] - g["normal"].numpy()).max() <= max(4 * float(g["gap_normal"]), 1e-12)
    assert np.abs(r[:, 7] - g["offset"].numpy()).max() <= max(4 * float(g["gap_offset"]), 1e-12)
    _compare_rows(r, ref_rows)
    ref64 = REF.table(ref_rows, PI.npos_of(pairs))
    _check_table(E.evaluate_for_planes(preds, dataset, device, categories=[{"id": 1, "name": "plane"}]), g, ref64)
    # the evaluator class: the same table from process() calls, one pair at a time and all at once
    for step in (1, 3):
        ev = E.PlaneEvaluator(device)
        inputs = [{v: {"image_id": dataset[key][v]["image_id"], "annotations": dataset[key][v]["annotations"]} for v in "01"} for key in dataset]
        outputs = [{v: {"instances": p[v]["instances"], "pred_plane": torch.from_numpy(p[v]["pred_plane"])} for v in "01"} for p in preds]
        for i in range(0, len(inputs), step):
            ev.process(inputs[i:i + step], outputs[i:i + step])
        _check_table(ev.evaluate(), g, ref64)
    with pytest.raises(TypeError, match="RLE dict"):
        bad = {k: {**e, "0": {**e["0"], "annotations": [{"segmentation": [[0, 0, 1, 1, 2, 2]], "plane": [0, 0, 1], "category_id": 1}]}}
               for k, e in dataset.items()}
        E.evaluate_for_planes(preds, bad, device)


def test_evaluate_for_matchings_on_the_device_equals_the_host(device):
    from nopesac_amd import evaluation as E
    from tests import golden_inputs as GI
    case = GI.matching_eval_case(3)
    keys = ("pred_assignment", "pred_assignment_afterRef0", "pred_assignment_beforeRef0")
    preds, dataset = [], {}
    for pi, pr in enumerate(case):
        ids = (f"a{pi}", f"b{pi}")
        pred, entry = {}, {"gt_corrs": pr["gt_corrs"]}
        for v, vid in zip("01", ids):
            view = pr["views"][int(v)]
            pred[v] = {"image_id": vid, "instances": [{"segmentation": R.encode(m)} for m in view["pred"]]}
            entry[v] = {"annotations": [{"segmentation": {"size": list(m.shape), "counts": R.run_lengths(m)}} for m in view["gt"]]}
        for k in keys:
            pred[k] = torch.from_numpy(pr[k])
        dataset[ids[0] + "__" + ids[1]] = entry
        preds.append(pred)
    assert E.evaluate_for_matchings(preds, dataset, device=device) == E.evaluate_for_matchings(preds, dataset)


def test_cli_eval_planes(device, tmp_path, caplog):
    """`python -m nopesac_amd.run --eval-planes`: the table under results["plane"] (the reference's keys) is the one the host
    restatement gives for the instances the run dumped and the annotations the pairs carried; the two tables are logged."""
    import logging
    import os
    from nopesac_amd import rle, run
    from nopesac_amd.synth import synth_pair
    from tests.util import ROOT
    rng = np.random.default_rng(8)
    pairs = [synth_pair(60 + i, structured=True) for i in range(2)]
    pairs[1]["0"] = dict(pairs[0]["1"])                                                      # one image in two pairs
    gts = {}
    for p in pairs:
        for v in "01":
            if p[v]["image_id"] not in gts:
                blobs = _blobs(rng, 480, 640, 5)
                gts[p[v]["image_id"]] = (blobs, (rng.normal(size=(5, 3)) * 2).astype(np.float32))
            blobs, planes = gts[p[v]["image_id"]]
            p[v]["annotations"] = [{"segmentation": R.encode(m), "plane": [float(x) for x in pl], "category_id": 1} for m, pl in zip(blobs, planes)]
    torch.save(pairs, tmp_path / "pairs.pt")
    with caplog.at_level(logging.INFO, logger="nopesac_amd"):
        res = run.main(["--config-file", os.path.join(ROOT, "configs", "inference_mp3d.yaml"), "--eval-only", "--synthetic-weights", "--eval-planes",
                        "--pairs-file", str(tmp_path / "pairs.pt"), "--pairs-per-batch", "2", "--dump-dir", str(tmp_path / "dump"),
                        "MODEL.DEVICE", str(device)])
    assert "Detection metrics" in caplog.text and "Plane metrics" in caplog.text
    preds = torch.load(tmp_path / "dump" / "NopeSAC_instances_predictions.pth", weights_only=False)
    seen, views = set(), []
    for pr in preds:
        for v in "01":
            image_id, ins = pr[v]["image_id"], pr[v].get("instances", [])
            if image_id in seen:
                continue
            seen.add(image_id)
            if len(ins):
                views.append({"pred": np.stack([rle.decode(i["segmentation"]) for i in ins]), "score": np.asarray([i["score"] for i in ins], np.float32),
                              "label": [i["category_id"] for i in ins], "pred_plane": pr[v]["pred_plane"].numpy(), "gt": gts[image_id][0],
                              "gt_label": [1] * 5, "gt_plane": gts[image_id][1]})
    assert len(seen) == 3 and sum(len(v["score"]) for v in views) >= 3
    want = REF.table(REF.evaluate(views), {1: 15.0})
    got = res["plane"]
    assert list(got) == list(want)
    for k in want:
        assert (got[k] == want[k]) if k.startswith("%") else abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])


def test_plane_evaluator_takes_a_view_without_annotations(device):
    """A view with predictions and `annotations: []` (the one divergence from the reference, which raises there): its rows get
    gt_id -1 and NaN errors, count as false positives in every AP and stay out of the error statistics; evaluate() works."""
    from nopesac_amd import evaluation as E
    pairs = PI.plane_eval_case(PI.SEEDS[0])
    preds, dataset = PI.product_inputs(pairs)
    donor = preds[0]["0"]
    extra = {"instances": [dict(i, score=s) for i, s in zip(donor["instances"][:2], (0.99, 0.5))], "pred_plane": donor["pred_plane"][:2]}
    inputs = [{v: {"image_id": dataset[key][v]["image_id"], "annotations": dataset[key][v]["annotations"]} for v in "01"} for key in dataset]
    outputs = [{v: {"instances": p[v]["instances"], "pred_plane": torch.from_numpy(p[v]["pred_plane"])} for v in "01"} for p in preds]
    inputs.append({"0": {"image_id": "Z0", "annotations": []}, "1": {"image_id": "Z1", "annotations": []}})
    outputs.append({"0": {"instances": extra["instances"], "pred_plane": torch.from_numpy(extra["pred_plane"])},
                    "1": {"instances": [], "pred_plane": torch.zeros(0, 3)}})
    ev = E.PlaneEvaluator(device)
    ev.process(inputs[:2], outputs[:2])
    ev.process(inputs[2:], outputs[2:])
    got = ev.evaluate()
    z = REF.assign(np.zeros((2, 0)), np.array([0.99, 0.5], np.float32), [1, 1], extra["pred_plane"], [], np.zeros((0, 3), np.float32))
    assert np.isnan(z[:, 6:8]).all() and (z[:, 9] == -1).all()
    rows = np.concatenate([PI.reference_order_rows(pairs), z])
    want, plain = REF.table(rows, PI.npos_of(pairs)), REF.table(rows[:-2], PI.npos_of(pairs))
    assert list(got) == list(want) and all(abs(got[k] - want[k]) <= 1e-9 for k in want)
    assert got["mask_ap@0.5"] < plain["mask_ap@0.5"] and abs(got["mean_normal"] - plain["mean_normal"]) <= 1e-9
    z_rows = np.concatenate(ev._rows)[-2:]
    assert np.isnan(z_rows[:, 6:8]).all() and (z_rows[:, 9] == -1).all() and not z_rows[:, 2:6].any() and not z_rows[:, 8].any()


def test_iou_device_views_mixed_sizes_in_one_call(device):
    from nopesac_amd import rle
    rng = np.random.default_rng(6)

    def masks(n, h, w):
        return [R.encode(rng.uniform(size=(h, w)) < 0.5) for _ in range(n)]
    views = [(masks(3, 5, 7), masks(2, 5, 7), None), (masks(4, 48, 64), masks(6, 48, 64), [0, 1, 0, 0, 1, 0]), ([], masks(2, 5, 7), None),
             (masks(1, 5, 7), masks(5, 5, 7), [1, 0, 0, 0, 0]), (masks(2, 48, 64), [], None)]
    got = rle.iou_device_views(views, device)
    assert len(got) == len(views)
    for (dt, gt, crowd), m in zip(views, got):
        want = rle.iou(dt, gt, crowd)
        assert m.dtype == np.float64 and m.shape == want.shape and (m == want).all()
