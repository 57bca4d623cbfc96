"""The host side of the two-view reconstruction AP (no GPU): the numpy restatement tests/recon_eval_ref.py against what the
reference's own functions produced on the fixture seeds (tests/golden/K_recon_eval_*.npz, scripts/gen_recon_eval_golden.py), what the
seeded cases cover, recon_table, ReconEvaluator's gather over gloo, the C surface of the new entry point and the CLI's refusals.

Tolerances: flags, scores and counts are exact.  The reference and the restatement are both float64; the fixture stores, per
quantity, the largest gap between them on these very inputs, and a float64 result is held to 4 x that gap, floored at 1e-12 (the rule
of the J_plane_eval fixtures)."""
import numpy as np
import pytest

from tests import recon_eval_inputs as RI
from tests import recon_eval_ref as REF
from tests.util import gold

KEYS = ["all", "-offset", "-normal", "-mask", "-normal-offset", "npos"]


@pytest.fixture(scope="module", params=RI.SEEDS)
def case(request):
    pairs = RI.recon_eval_case(request.param)
    return pairs, gold(f"K_recon_eval_{request.param}"), RI.reference_rows(pairs)


def _tol(gap):
    return max(4 * float(gap), 1e-12)


def test_restatement_matches_the_reference(case):
    pairs, g, (rows, n_ge, errs) = case
    assert np.array_equal(rows[:, 0], g["score"].numpy()) and np.array_equal(rows[:, 1:6], g["flags"].numpy())
    assert float(g["npos"]) == sum(n_ge)
    for i, e in enumerate(errs):
        want = g[f"err_{i}"].numpy()
        assert want.shape == (3, len(e["pred_entries"]), len(e["gt_entries"]))
        for m, (key, gap) in enumerate((("err_offsets", "gap_offset"), ("err_normals", "gap_normal"), ("mask_iou", "gap_iou"))):
            if want[m].size:
                assert np.abs(e[key] - want[m]).max() <= _tol(g[gap]), (i, key)
    table = REF.table(rows, sum(n_ge))
    assert list(table) == KEYS
    for k, want, gap in zip(REF.CRITERIA, g["ap"].numpy(), g["gap_ap"].numpy()):
        assert abs(table[k] / 100.0 - want) <= _tol(gap), k
    # the gaps are rounding, far below the margins the inputs keep to the thresholds
    assert float(g["gap_normal"]) < RI.NORMAL_MARGIN / 4 and float(g["gap_offset"]) < RI.OFFSET_MARGIN / 4 and float(g["gap_iou"]) == 0.0
    assert int(g["flags"].sum()) > 0 and 0 < g["ap"].numpy().min() and g["ap"].numpy().max() < 1


def test_cases_keep_their_margins_and_scores(case):
    pairs, _, (rows, _, _) = case
    assert 3 <= len(pairs) <= 4
    for p in pairs:
        assert RI.margins_ok(p) and RI.gt_agrees(p)
        a = p["assignment"]
        assert a.shape == (len(p["views"][0]["pred"]), len(p["views"][1]["pred"])) and a.sum(0).max(initial=0) <= 1 and a.sum(1).max(initial=0) <= 1
        for v in p["views"]:
            assert v["gt"].shape[1:] == (48, 64) and v["pred"].shape[1:] == (48, 64)
    score = np.concatenate([v["score"] for p in pairs for v in p["views"]])
    assert len(np.unique(score)) == len(score) and score.min() > 0.1
    assert len(np.unique(rows[:, 0])) == len(rows)                     # ... and so are the entries' (a merged entry has the larger one)


def test_cases_cover_every_situation():
    pairs = [p for s in RI.SEEDS for p in RI.recon_eval_case(s)]
    plans = [kw for s in RI.SEEDS for kw in RI.PLAN[s]]
    n = lambda p: (len(p["views"][0]["pred"]), len(p["views"][1]["pred"]))      # noqa: E731
    m = lambda p: (len(p["views"][0]["gt"]), len(p["views"][1]["gt"]))          # noqa: E731
    assert any(min(n(p)) > 0 and not p["assignment"].any() for p in pairs)                         # no predicted correspondence
    assert any(n(p)[0] > 0 and p["assignment"].sum() == n(p)[0] for p in pairs)                    # every view-0 prediction matched
    assert any(n(p)[0] > 0 and n(p)[1] == 0 for p in pairs) and any(n(p) == (0, 0) and sum(m(p)) > 0 for p in pairs)
    assert any(m(p)[0] == 0 and m(p)[1] > 0 and sum(n(p)) > 0 for p in pairs)                      # no GT in one view
    assert any(min(m(p)) > 0 and len(p["gt_corrs"]) == 0 and p["assignment"].any() for p in pairs)    # empty gt_corrs
    cols = [np.argwhere(p["assignment"])[:, 1] for p in pairs]
    assert any(len(c) > 1 and (np.diff(c) < 0).any() for c in cols)                                # row-major order is not column order
    assert sum(RI.has_trap(p) for p, kw in zip(pairs, plans) if kw.get("trap")) == 2
    assert sum(RI.has_negative_dot(p) for p, kw in zip(pairs, plans) if kw.get("negdot")) == 2
    norms = [np.linalg.norm(p[c]["rotation"]) for p in pairs for c in ("pred_cam", "gt_cam")]
    assert min(norms) < 0.7 and max(norms) > 1.5                                                   # non-unit quaternions, both ways
    angles = [2 * np.degrees(np.arccos(abs(p["gt_cam"]["rotation"][0]) / np.linalg.norm(p["gt_cam"]["rotation"]))) for p in pairs]
    assert max(angles) > 178.0
    # both sides of every threshold occur among the decisive quantities
    errs = [REF.pair_errors(*RI.pair_args(p)) for p in pairs]
    for key, t in (("mask_iou", 0.5), ("err_normals", 30.0), ("err_offsets", 1.0)):
        x = np.concatenate([e[key].reshape(-1) for e in errs])
        assert (x < t).any() and (x > t).any()


def test_walk_takes_the_first_flagged_entry_only():
    flags = np.array([[0, 1, 1], [0, 1, 1], [1, 0, 0], [0, 0, 0], [0, 0, 1]], bool)
    assert REF.walk(flags).tolist() == [1, 0, 1, 0, 1]                  # entry 1 does not move on to the free GT entry 2
    assert REF.walk(np.zeros((3, 0), bool)).tolist() == [0, 0, 0]


def test_recon_table_on_injected_rows():
    from nopesac_amd import evaluation as E
    assert E.RECON_ROW_COLS == REF.COLS and E.RECON_CRITERIA == REF.CRITERIA

    def row(score, flags):
        return [score, *flags, 0, -1]
    # a TP, a FP, a TP of 2 GT entries: precision envelope 1, 2/3, 2/3 -> 0.5 * 1 + 0.5 * 2/3; criterion 2 has no TP
    rows = np.array([row(0.7, [1, 1, 0, 1, 1]), row(0.9, [1, 1, 0, 0, 1]), row(0.8, [0, 0, 0, 0, 0])])
    got = E.recon_table(rows, 2.0)
    assert list(got) == KEYS and got["npos"] == 2.0
    assert abs(got["all"] - 100 * (0.5 + 0.5 * 2 / 3)) < 1e-12 and got["-normal"] == 0.0 and got["-normal-offset"] == got["-offset"] == got["all"]
    assert abs(got["-mask"] - 100 * 0.5 * (1 / 3)) < 1e-12               # FP FP TP: one of two GT entries at precision 1/3
    assert all(abs(got[k] - REF.table(rows, 2.0)[k]) <= 1e-12 for k in KEYS)
    # equal scores keep the order of the rows: FP before TP and TP before FP differ
    tied = np.array([row(0.5, [0] * 5), row(0.5, [1] * 5)])
    assert E.recon_table(tied, 1.0)["all"] == 50.0 and E.recon_table(tied[::-1], 1.0)["all"] == 100.0
    assert REF.table(tied, 1.0)["all"] == 50.0
    # nothing to find: every AP is 0 (the reference prints nan); no rows at all
    assert E.recon_table(rows, 0.0) == {**{k: 0.0 for k in REF.CRITERIA}, "npos": 0.0}
    assert E.recon_table(np.zeros((0, 8)), 5.0) == {**{k: 0.0 for k in REF.CRITERIA}, "npos": 5.0}
    rng = np.random.default_rng(3)
    big = np.concatenate([np.round(rng.uniform(size=(300, 1)), 2), (rng.uniform(size=(300, 5)) < 0.4).astype(np.float64), np.zeros((300, 2))], 1)
    want = REF.table(big, 140.0)
    assert all(abs(E.recon_table(big, 140.0)[k] - want[k]) <= 1e-10 for k in KEYS)


def test_recon_table_reproduces_the_reference_table(case):
    from nopesac_amd import evaluation as E
    _, g, _ = case
    rows = np.concatenate([g["score"].numpy()[:, None], g["flags"].numpy(), np.zeros((len(g["score"]), 2))], 1)
    got = E.recon_table(rows, float(g["npos"]))
    for k, want, gap in zip(REF.CRITERIA, g["ap"].numpy(), g["gap_ap"].numpy()):
        assert abs(got[k] / 100.0 - want) <= _tol(gap), k


TIED = {3: [[0.05, 0, 0, 0, 0, 0, 0, -1]], 7: [[0.05, 1, 1, 1, 1, 1, 0, -1]]}      # pair number -> rows with one score: pair 3's comes first


def _fill(ev, pairs, numbers):
    for p, num in zip(pairs, numbers):
        rows, n_ge, _ = REF.pair_rows(*RI.pair_args(p))
        ev._add([float(num)], rows, [len(rows)], [n_ge])


def _expected(pairs):
    numbers = [0, 1, 2, 5][:len(pairs)]
    rows, n_ge, _ = RI.reference_rows(pairs)
    split = np.cumsum([0] + [len(REF.pair_rows(*RI.pair_args(p))[0]) for p in pairs])
    parts = {num: rows[split[i]:split[i + 1]] for i, num in enumerate(numbers)}
    parts.update({k: np.asarray(v, np.float64) for k, v in TIED.items()})
    return numbers, REF.table(np.concatenate([parts[k] for k in sorted(parts)]), sum(n_ge) + 2)


def _gather_worker(rank, world, port, seed, q):
    import os
    import torch
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from nopesac_amd import runner
    from nopesac_amd.evaluation import ReconEvaluator
    runner.init_distributed("gloo")
    try:
        ReconEvaluator("cpu")._number("a__b")
        raise AssertionError("several ranks must agree on pair numbers: pair_index is required")
    except ValueError as e:
        assert "pair_index" in str(e)
    pairs = RI.recon_eval_case(seed)
    numbers, _ = _expected(pairs)
    ev = ReconEvaluator("cpu", pair_index={})
    # rank 0 holds the LATER pairs and the tied row of pair 7, rank 1 the first pair and the tied row of pair 3: rank order is not pair order
    if rank == 0:
        _fill(ev, pairs[1:], numbers[1:])
        ev._add([7.0], np.asarray(TIED[7], np.float64), [1], [1])
        ev._skipped = 2
    else:
        _fill(ev, pairs[:1], numbers[:1])
        ev._add([3.0], np.asarray(TIED[3], np.float64), [1], [1])
        ev._skipped = 1
    res = ev.evaluate()
    torch.distributed.barrier()
    q.put((rank, res))
    torch.distributed.destroy_process_group()


def test_recon_evaluator_gathers_the_same_table_at_world_sizes_1_and_2():
    """Injected rows (the restatement's), ragged over two gloo ranks with the later pairs on rank 0 and two rows of equal score whose
    order decides the AP: every rank gets the single-process table, which orders rows by (pair number, entry)."""
    import multiprocessing as mp
    import socket
    from nopesac_amd.evaluation import ReconEvaluator
    seed = RI.SEEDS[1]
    pairs = RI.recon_eval_case(seed)
    numbers, want = _expected(pairs)
    one = ReconEvaluator("cpu", pair_index={})
    _fill(one, pairs[::-1], numbers[::-1])                               # fed out of order
    one._add([7.0], np.asarray(TIED[7], np.float64), [1], [1])
    one._add([3.0], np.asarray(TIED[3], np.float64), [1], [1])
    one._skipped = 3
    single = one.evaluate()
    assert list(single) == KEYS + ["pairs", "skipped"] and single["pairs"] == len(pairs) + 2 and single["skipped"] == 3
    assert all(abs(single[k] - want[k]) <= 1e-9 for k in KEYS)
    swapped = REF.table(np.concatenate([RI.reference_rows(pairs)[0], TIED[7], TIED[3]]), want["npos"])
    assert swapped["all"] != want["all"]                                 # the order of the tied rows matters in this table
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
    for _, res in got:
        assert res == single


def test_evaluators_refuse_polygons_and_count_skipped_pairs():
    from nopesac_amd import evaluation as E
    rle = {"size": [2, 2], "counts": [1, 3]}
    ann = [{"segmentation": rle, "plane": [0, 0, 1], "category_id": 1}]
    out = {"0": {"instances": [{"segmentation": rle, "score": 0.5}], "pred_plane": np.ones((1, 3), np.float32)},
           "1": {"instances": [], "pred_plane": np.zeros((0, 3), np.float32)},
           "camera": {"tran": np.zeros(3), "rot": np.array([1.0, 0, 0, 0])}, "pred_assignment": np.zeros((1, 0))}
    full = {"0": {"image_id": "a", "annotations": ann}, "1": {"image_id": "b", "annotations": ann}, "gt_corrs": [[0, 0]],
            "rel_pose": {"position": [0, 0, 0], "rotation": [1, 0, 0, 0]}}
    polygon = {**full, "0": {"image_id": "a", "annotations": [{"segmentation": [[0, 0, 1, 1, 2, 2]], "plane": [0, 0, 1]}]}}
    ev = E.ReconEvaluator("cpu")
    with pytest.raises(TypeError, match="RLE dict"):
        ev.process([polygon], [out])
    ev = E.ReconEvaluator("cpu")
    lacking = [{k: v for k, v in full.items() if k != drop} for drop in ("rel_pose", "gt_corrs")] + [{**full, "1": {"image_id": "b"}}]
    ev.process(lacking, [out] * 3)                                          # nothing left for the device
    res = ev.evaluate()
    assert res == {**{k: 0.0 for k in REF.CRITERIA}, "npos": 0.0, "pairs": 0, "skipped": 3}
    assert E.recon_rows([], "cpu")[0].shape == (0, 8)
    rec = {"0": {"image_id": "a", **out["0"]}, "1": {"image_id": "b", **out["1"]}, "pred_assignment": out["pred_assignment"],
           "camera": {"pred": out["camera"], "gts": {"tran": None, "rot": None}}}
    with pytest.raises(TypeError, match="RLE dict"):
        E.evaluate_for_reconstruction([rec], {"a__b": polygon}, "cpu")
    res = E.evaluate_for_reconstruction([rec, rec], {"a__b": lacking[0], "x__y": full}, "cpu")       # no GT camera anywhere
    assert res["pairs"] == 0 and res["skipped"] == 2 and res["all"] == 0.0
    assert E.assignment_corrs(np.array([[0, 1, 0], [1, 0, 0]])).tolist() == [[0, 1], [1, 0]]
    assert E.assignment_corrs(np.zeros((0, 4))).shape == (0, 2)


def test_c_surface_of_the_recon_evaluator():
    """The entry point is declared nps_status, bound with the types the header states, exported by the library, and reports
    argument errors before any device call; P = 0 is a valid call that enqueues nothing."""
    from ctypes import c_int, c_int64, c_void_p
    from nopesac_amd import _lib, ops
    name = "nopesac_recon_ap_assign"
    lib = _lib.load()
    assert name in _lib.declared_symbols() and name in _lib.STATUS and _lib.RESTYPES[name] is c_int and hasattr(lib, name)
    p, i = c_void_p, c_int
    assert _lib.SIGNATURES[name] == [p] * 13 + [i] * 3 + [c_int64] + [p] * 6
    assert _lib.H.NPS_RECON_AP_COLS == len(ops.RECON_AP_COLS) == 8
    none = [None] * 13
    assert lib.nopesac_recon_ap_assign(*none, 0, 4, 4, 0, *[None] * 6) == 0
    assert lib.nopesac_recon_ap_assign(*none, -1, 4, 4, 0, *[None] * 6) == -1 and b"P < 0" in lib.nopesac_last_error()
    for max_dt, max_gt in ((129, 1), (1, 256), (-1, 0)):
        assert lib.nopesac_recon_ap_assign(*none, 1, max_dt, max_gt, 0, *[None] * 6) == -1
        assert b"at most 128 predictions and 255 GT" in lib.nopesac_last_error()
    assert lib.nopesac_recon_ap_assign(*none, 1, 4, 4, 0, *[None] * 6) == -1 and b"null pointer" in lib.nopesac_last_error()


def test_cli_refuses_eval_recon_with_the_stub_model(capsys):
    from nopesac_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--eval-only", "--eval-recon", "--stub-model", "--synthetic-pairs", "1"])
    assert e.value.code == 2 and "--eval-recon cannot run with --stub-model" in capsys.readouterr().err
    assert run.default_argument_parser().parse_args(["--eval-recon"]).eval_recon is True
