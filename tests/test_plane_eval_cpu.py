"""The host side of the plane detection evaluator (no GPU): plane_table against the table the reference's evaluate_for_planes
produced on the fixture seeds (tests/golden/J_plane_eval_*.npz, scripts/gen_plane_eval_golden.py), its edge cases, the numpy
restatement tests/plane_eval_ref.py against the reference's per-prediction results, the margins of the seeded inputs, and the C
surface of the four new entry points.

Tolerances: percentages, counts and flags are exact.  The reference computes compare_planes and compute_ap in float32; the fixture
stores, per quantity, the largest gap between the reference's value and the float64 restatement of the same formula on the same
inputs, and a float64 result is held to 4 x that gap (the factor covers reordered float32 sums), floored at 1e-12."""
import numpy as np
import pytest

from tests import plane_eval_inputs as PI
from tests import plane_eval_ref as REF
from tests.util import gold

QUIRK = "plane_ap@iou0.5offset30.0"
KEYS = ["%normal<10", "%normal<30", "%offset<0.5", "%offset<0.3", "mean_normal", "median_normal", "mean_offset", "median_offset",
        "mask_ap@0.5 - plane", "plane_ap@iou0.5normal30.0offset0.3 - plane", "plane_ap@iou0.5normal30.0 - plane",
        "plane_ap@iou0.5offset0.3 - plane", "mask_ap@0.5", "plane_ap@iou0.5normal30.0offset0.3", "plane_ap@iou0.5normal30.0", QUIRK]


@pytest.fixture(scope="module", params=PI.SEEDS)
def case(request):
    return PI.plane_eval_case(request.param), gold(f"J_plane_eval_{request.param}")


def _reference_rows(g):
    """[n, 10] rows from the stored per-prediction lists of the reference (label 1; best_iou and gt_id are not stored)."""
    n = len(g["score"])
    rows = np.zeros((n, 10), np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2:6] = g["score"].numpy(), 1.0, g["flags"].numpy()
    rows[:, 6], rows[:, 7] = g["normal"].numpy(), g["offset"].numpy()
    return rows


def test_plane_table_reproduces_the_reference_table(case):
    from nopesac_amd import evaluation as E
    pairs, g = case
    keys = [str(k) for k in g["keys"]]
    assert keys == KEYS and QUIRK in keys and "plane_ap@iou0.5offset0.3" not in keys
    got = E.plane_table(_reference_rows(g), PI.npos_of(pairs))
    assert list(got) == keys
    for k, want, gap in zip(keys, g["values"].numpy(), g["gap_values"].numpy()):
        if k.startswith("%"):
            assert got[k] == want, k
        else:
            assert abs(got[k] - want) <= max(4 * gap, 1e-12), (k, got[k], want, gap)
    assert got[QUIRK] == got["plane_ap@iou0.5offset0.3 - plane"]
    assert int(g["flags"].sum()) > 0 and 0 < got["mask_ap@0.5"] < 1
    # the vectorised AP against the looped restatement, and independence of the row order
    ref = REF.table(_reference_rows(g), PI.npos_of(pairs))
    assert list(ref) == keys and all(abs(got[k] - ref[k]) <= 1e-12 for k in keys)
    shuffled = E.plane_table(_reference_rows(g)[np.random.default_rng(0).permutation(len(g["score"]))], PI.npos_of(pairs))
    assert all(abs(shuffled[k] - got[k]) <= 1e-12 for k in keys)


def test_restatement_matches_the_reference_per_prediction(case):
    pairs, g = case
    rows = PI.reference_order_rows(pairs)
    assert np.array_equal(rows[:, 0], g["score"].numpy())
    assert np.array_equal(rows[:, 2:6], g["flags"].numpy())
    assert np.abs(rows[:, 6] - g["normal"].numpy()).max() <= max(4 * float(g["gap_normal"]), 1e-12)
    assert np.abs(rows[:, 7] - g["offset"].numpy()).max() <= max(4 * float(g["gap_offset"]), 1e-12)
    # the gaps are float32 rounding, far below the margins the inputs keep to the thresholds
    assert float(g["gap_normal"]) < PI.NORMAL_MARGIN / 4 and float(g["gap_offset"]) < PI.OFFSET_MARGIN / 4
    table = REF.table(rows, PI.npos_of(pairs))
    for k, want, gap in zip(g["keys"], g["values"].numpy(), g["gap_values"].numpy()):
        assert abs(table[str(k)] - want) <= max(4 * gap, 1e-12), k


def test_input_margins_and_shape_of_the_cases(case):
    pairs, _ = case
    assert len(pairs) == 3
    views = [v for p in pairs for v in p["views"]]
    for v in views:
        n, o, i = PI.margins(v)
        assert n > PI.NORMAL_MARGIN and o > PI.OFFSET_MARGIN and i > PI.IOU_MARGIN
        assert v["gt"].shape[1:] == (48, 64) and v["gt"].sum(0).min() == 1 and v["gt"].sum(0).max() == 1      # a partition
        assert len(np.unique(v["score"])) == len(v["score"])
    ids = [i for p in pairs for i in p["ids"]]
    assert len(ids) == 6 and len(set(ids)) == 5                                                    # one image in two pairs
    uniq = PI.unique_views(pairs)
    assert sum(len(v["score"]) == 0 and len(v["gt"]) > 0 for _, v in uniq) == 1                    # GT without predictions
    assert pairs[1]["views"][0]["gt"] is pairs[0]["views"][1]["gt"]
    assert not np.array_equal(pairs[1]["views"][0]["score"], pairs[0]["views"][1]["score"])        # the copy a de-duplication drops
    rows = PI.reference_order_rows(pairs)
    for col, edges in ((6, PI.NORMAL_EDGES), (7, PI.OFFSET_EDGES)):                                # both sides of every threshold
        for e in edges:
            assert (rows[:, col] < e).any() and (rows[:, col] > e).any()
    assert PI.npos_of(pairs)[1] == sum(len(v["gt"]) for _, v in uniq)


def test_plane_table_edge_cases():
    from nopesac_amd import evaluation as E
    none = E.plane_table(np.zeros((0, 10)), {1: 7.0})
    assert list(none) == KEYS and all(none[k] == 0.0 for k in KEYS if "ap@" in k or k.startswith("%"))
    assert all(np.isnan(none[k]) for k in ("mean_normal", "median_normal", "mean_offset", "median_offset"))

    def row(score, flags, normal=5.0, offset=0.1, label=1):
        return [score, label, *flags, normal, offset, 0.9, 0]
    fps = E.plane_table(np.array([row(0.9, [0] * 4, 50, 0.6), row(0.8, [0] * 4, 60, 0.7)]), {1: 3.0})
    assert all(fps[k] == 0.0 for k in KEYS if "ap@" in k) and fps["%normal<30"] == 0.0 and fps["mean_normal"] == 55.0
    one = E.plane_table(np.array([row(0.9, [1, 0, 1, 0])]), {1: 4.0})
    assert one["mask_ap@0.5"] == 0.25 and one["plane_ap@iou0.5normal30.0"] == 0.25 and one["plane_ap@iou0.5normal30.0offset0.3"] == 0.0
    assert one[QUIRK] == 0.0 and one["%normal<10"] == 100.0 and one["median_offset"] == 0.1
    # a TP, a FP, a TP of 2 GT planes: precision envelope 1, 2/3, 2/3 -> 0.5 * 1 + 0.5 * 2/3
    three = E.plane_table(np.array([row(0.9, [1] * 4), row(0.8, [0] * 4), row(0.7, [1] * 4)]), {1: 2.0})
    assert abs(three["mask_ap@0.5"] - (0.5 + 0.5 * 2 / 3)) < 1e-15
    assert abs(REF.compute_ap([0.9, 0.8, 0.7], [1, 0, 1], 2.0) - three["mask_ap@0.5"]) < 1e-15
    # two categories, none of the second in the dataset: it is skipped in the class mean and gets no key
    rows = np.array([row(0.9, [1] * 4), row(0.8, [1] * 4, label=2), row(0.7, [0] * 4)])
    two = E.plane_table(rows, {1: 2.0, 2: 0.0}, cat_names={2: "other"})
    assert list(two) == KEYS and two["mask_ap@0.5"] == two["mask_ap@0.5 - plane"] == 0.5
    both = E.plane_table(rows, {1: 2.0, 2: 1.0}, cat_names={2: "other"})
    assert both["mask_ap@0.5 - other"] == 1.0 and both["mask_ap@0.5"] == 0.75 and len(both) == len(KEYS) + 4
    assert all(v == 0.0 for k, v in E.plane_table(rows, {1: 0.0}).items() if "ap@" in k)
    # tied scores: the rows keep their order (stable sort), whatever else is in the table
    tied = np.array([row(0.5, [1] * 4), row(0.5, [0] * 4), row(0.5, [0] * 4), row(0.5, [1] * 4)])
    first = E.plane_table(tied, {1: 2.0})["mask_ap@0.5"]
    assert first == E.plane_table(tied.copy(), {1: 2.0})["mask_ap@0.5"] == REF.compute_ap(tied[:, 0], tied[:, 2], 2.0)
    assert abs(first - (0.5 * 1.0 + 0.5 * 0.5)) < 1e-15
    assert E.plane_table(tied[::-1], {1: 2.0})["mask_ap@0.5"] == first                    # (this table is symmetric)
    assert E.plane_table(tied[[1, 2, 0, 3]], {1: 2.0})["mask_ap@0.5"] == 0.5                  # FP FP TP TP: the envelope is 1/2 throughout
    # rows of a view without GT (NaN errors) stay out of the statistics but count as false positives
    nan = E.plane_table(np.array([row(0.9, [1] * 4), row(0.95, [0] * 4, np.nan, np.nan)]), {1: 1.0})
    assert nan["mean_normal"] == 5.0 and nan["%offset<0.3"] == 100.0 and nan["mask_ap@0.5"] == 0.5


def test_average_precision_against_the_looped_form():
    from nopesac_amd import evaluation as E
    rng = np.random.default_rng(1)
    for n in (1, 2, 17, 400):
        scores, tp = np.round(rng.uniform(size=n), 2), (rng.uniform(size=n) < 0.4).astype(np.float64)
        npos = float(tp.sum() + rng.integers(0, 5) + 1)
        assert abs(E.average_precision(scores, tp, npos) - REF.compute_ap(scores, tp, npos)) <= 1e-12
    assert E.average_precision(np.zeros(0), np.zeros(0), 3.0) == 0.0


def test_evaluators_refuse_polygons_and_cpu():
    from nopesac_amd import evaluation as E
    view = {"instances": [{"segmentation": {"size": [2, 2], "counts": [1, 3]}, "score": 0.5, "category_id": 0}], "pred_plane": np.ones((1, 3), np.float32),
            "annotations": [{"segmentation": [[0, 0, 1, 1, 2, 2]], "plane": [0, 0, 1], "category_id": 1}]}
    with pytest.raises(TypeError, match="RLE dict"):
        E.plane_rows([view], "cpu")
    ev = E.PlaneEvaluator("cpu")
    with pytest.raises(TypeError, match="RLE dict"):
        ev.process([{"0": {"image_id": "a", "annotations": view["annotations"]}, "1": {"image_id": "b", "annotations": []}}],
                   [{"0": view, "1": {"instances": [], "pred_plane": np.zeros((0, 3), np.float32)}}])
    assert E.plane_rows([], "cpu").shape == (0, 10)
    ev = E.PlaneEvaluator("cpu")                       # nothing with predictions: no device work, npos still counted
    rle = {"size": [2, 2], "counts": [1, 3]}
    ev.process([{"0": {"image_id": "a", "annotations": [{"segmentation": rle, "plane": [0, 0, 1], "category_id": 1}] * 3},
                 "1": {"image_id": "a", "annotations": [{"segmentation": rle, "plane": [0, 0, 1], "category_id": 1}] * 3}}],
               [{"0": {"instances": [], "pred_plane": np.zeros((0, 3), np.float32)}, "1": None}])
    out = ev.evaluate()
    assert list(out) == KEYS and out["mask_ap@0.5"] == 0.0 and np.isnan(out["mean_normal"])
    assert float(np.concatenate(ev._gt)[:, 2].sum()) == 3.0                                        # image "a" once


def test_c_surface_of_the_plane_evaluator():
    """The four entry points are declared nps_status, bound with the types the header states, exported by the library, and report
    argument errors before any device call."""
    from ctypes import c_double, c_int, c_void_p
    from nopesac_amd import _lib
    names = ("nopesac_rle_string_runs", "nopesac_rle_runs_to_bits", "nopesac_mask_iou_bits", "nopesac_plane_ap_assign")
    lib = _lib.load()
    for n in names:
        assert n in _lib.declared_symbols() and n in _lib.STATUS and _lib.RESTYPES[n] is c_int and hasattr(lib, n)
    p, i, d = c_void_p, c_int, c_double
    assert _lib.SIGNATURES["nopesac_rle_string_runs"] == [p, p, i, p, p, p]
    assert _lib.SIGNATURES["nopesac_rle_runs_to_bits"] == [p, p, p, i, i, i, p, p, p, p, p]
    assert _lib.SIGNATURES["nopesac_mask_iou_bits"] == [p] * 8 + [i] * 4 + [p] * 3
    assert _lib.SIGNATURES["nopesac_plane_ap_assign"] == [p] * 9 + [i] * 3 + [d] * 3 + [p, p]
    text = open(_lib.HEADER_PATH).read()
    old = "int max_dt, int max_gt, double iou_thresh,"
    assert text.count(old) == 1
    with pytest.raises(_lib.HeaderError, match="nopesac_plane_ap_assign.*long double"):
        _lib.read_header(text.replace(old, "int max_dt, int max_gt, long double iou_thresh,"))
    assert lib.nopesac_rle_string_runs(None, None, -1, None, None, None) == -1 and b"n_masks" in lib.nopesac_last_error()
    assert lib.nopesac_rle_string_runs(None, None, 3, None, None, None) == -1 and b"null pointer" in lib.nopesac_last_error()
    assert lib.nopesac_rle_string_runs(None, None, 0, None, None, None) == 0
    assert lib.nopesac_rle_runs_to_bits(None, None, None, 2, 0, 5, None, None, None, None, None) == -1 and b"H, W" in lib.nopesac_last_error()
    assert lib.nopesac_rle_runs_to_bits(None, None, None, 2, 65536, 65536, None, None, None, None, None) == -1
    assert lib.nopesac_rle_runs_to_bits(None, None, None, 2, 5, 7, None, None, None, None, None) == -1 and b"null pointer" in lib.nopesac_last_error()
    assert lib.nopesac_mask_iou_bits(None, None, None, None, None, None, None, None, 1, 0, 1, 1, None, None, None) == -1
    assert lib.nopesac_mask_iou_bits(None, None, None, None, None, None, None, None, 1, 3, 1, 1, None, None, None) == -1
    assert b"null pointer" in lib.nopesac_last_error()
    assert lib.nopesac_mask_iou_bits(None, None, None, None, None, None, None, None, 1, 3, 0, 1, None, None, None) == 0
    for max_dt, max_gt in ((129, 1), (1, 256), (-1, 0)):
        assert lib.nopesac_plane_ap_assign(None, None, None, None, None, None, None, None, None, 1, max_dt, max_gt, 0.5, 30.0, 0.3, None, None) == -1
    assert b"at most 128 predictions and 255 GT" in lib.nopesac_last_error()
    assert lib.nopesac_plane_ap_assign(None, None, None, None, None, None, None, None, None, 1, 4, 4, 0.5, 30.0, 0.3, None, None) == -1
    assert b"null pointer" in lib.nopesac_last_error()
    assert lib.nopesac_plane_ap_assign(None, None, None, None, None, None, None, None, None, 0, 4, 4, 0.5, 30.0, 0.3, None, None) == 0


def test_cli_refuses_eval_planes_with_the_stub_model(capsys):
    from nopesac_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--eval-only", "--eval-planes", "--stub-model", "--synthetic-pairs", "1"])
    assert e.value.code == 2 and "--eval-planes cannot run with --stub-model" in capsys.readouterr().err


def _no_gt_rows(rank):
    """Rows of a view with 2 (rank 0) or 3 (rank 1) predictions and no GT: gt_id -1, NaN errors, no true positive."""
    n = 2 + rank
    return REF.assign(np.zeros((n, 0)), np.linspace(0.99, 0.4 + 0.1 * rank, n).astype(np.float32), [1] * n, np.ones((n, 3), np.float32), [],
                      np.zeros((0, 3), np.float32))


def _gather_worker(rank, world, port, seed, q):
    import os
    import torch
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from nopesac_amd import runner
    from nopesac_amd.evaluation import PlaneEvaluator
    runner.init_distributed("gloo")
    pairs = PI.plane_eval_case(seed)
    # rank 0 sees pair 0 (images A, B), rank 1 pairs 1 and 2 (B again - with the predictions a de-duplication must drop - C, D, E)
    mine = pairs[:1] if rank == 0 else pairs[1:]
    index = {image_id: i for i, (image_id, _) in enumerate(PI.unique_views(pairs))}
    ev = PlaneEvaluator("cpu", image_index=index)
    plain = PlaneEvaluator("cpu")                      # several ranks and no image_index: integer ids only
    assert plain._number(7) == 7.0
    try:
        plain._number("s11A")
        raise AssertionError("a string id must be refused when ranks have to agree on image numbers")
    except ValueError as e:
        assert "image_index" in str(e)
    for image_id, view in PI.unique_views(mine):
        ev._register(float(index[image_id]), {1: len(view["gt"])})
        if len(view["score"]):
            rows = REF.evaluate([view])
            ev._rows.append(np.concatenate([rows, np.full((len(rows), 1), float(index[image_id]))], 1))
    # image Z has predictions and no annotation at all, and both ranks saw it (with different predictions)
    ev._register(float(len(index)), {})
    ev._rows.append(np.concatenate([_no_gt_rows(rank), np.full((2 + rank, 1), float(len(index)))], 1))
    res = ev.evaluate()
    torch.distributed.barrier()
    q.put((rank, res))
    torch.distributed.destroy_process_group()


def test_plane_evaluator_gather_keeps_the_lowest_ranks_copy_world2():
    """Two ranks over gloo, ragged row counts, image B on both ranks with different predictions, and an image without any
    annotation on both ranks: every rank gets the table of the single-process evaluation - rank 0's copies are kept, B's GT is
    counted once, the rows without GT count as false positives and stay out of the error statistics."""
    import multiprocessing as mp
    import socket
    seed = PI.SEEDS[0]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, seed, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = gold(f"J_plane_eval_{seed}")
    pairs = PI.plane_eval_case(seed)
    want = REF.table(np.concatenate([PI.reference_order_rows(pairs), _no_gt_rows(0)]), PI.npos_of(pairs))
    plain = REF.table(PI.reference_order_rows(pairs), PI.npos_of(pairs))
    assert want["mask_ap@0.5"] < plain["mask_ap@0.5"] and want["mean_normal"] == plain["mean_normal"]      # two more false positives
    for _, res in got:
        assert list(res) == KEYS
        for k, ref_value, gap in zip(KEYS, g["values"].numpy(), g["gap_values"].numpy()):
            assert abs(res[k] - want[k]) <= 1e-9, k
            if "ap@" not in k:                     # the error statistics leave the NaN rows out: still the reference's
                assert abs(res[k] - ref_value) <= max(4 * gap, 1e-12), k
