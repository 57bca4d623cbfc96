"""csrc/recon_eval.hip on the GPU: the per-pair kernel alone on IoU blocks given as numbers (no masks) against
tests/recon_eval_ref.py - flags, scores, entry maps and GT entry counts exact, the three error matrices (the kernel's debug output)
at 1e-9, the tolerance test_plane_eval_gpu.py uses for float64 against float64 - and the evaluator built on it against what the
reference's functions produced on the fixture seeds (tests/golden/K_recon_eval_*.npz; 4 x the stored gap, floored at 1e-12)."""
import numpy as np
import pytest
import torch

from tests import recon_eval_inputs as RI
from tests import recon_eval_ref as REF
from tests.util import gold

pytestmark = pytest.mark.gpu

ARGS = ("iou0", "iou1", "score0", "score1", "plane0", "plane1", "gt_plane0", "gt_plane1", "pred_cam", "gt_cam", "pred_corrs", "gt_corrs")


def _launch(specs, device, max_dt=None, max_gt=None):
    """ops.recon_ap_assign on pairs given as REF.pair_errors' arguments (tuples in ARGS order) -> (rows per pair, GT entry counts,
    bad flags, error matrices per pair [3, entries, GT entries])."""
    from nopesac_amd import ops
    P = len(specs)
    s = [dict(zip(ARGS, spec)) for spec in specs]
    n_dt = [len(x[k]) for x in s for k in ("score0", "score1")]
    n_gt = [len(np.asarray(x[k]).reshape(-1, 3)) for x in s for k in ("gt_plane0", "gt_plane1")]
    off = np.zeros((3, 2 * P + 1), np.int64)
    np.cumsum(n_dt, out=off[0, 1:]); np.cumsum(n_gt, out=off[1, 1:]); np.cumsum(np.multiply(n_dt, n_gt), out=off[2, 1:])
    corr = [[np.asarray(x[k], np.int32).reshape(-1, 2) for x in s] for k in ("pred_corrs", "gt_corrs")]
    coff = np.zeros((2, P + 1), np.int64)
    for a in range(2):
        np.cumsum([len(c) for c in corr[a]], out=coff[a, 1:])
    n_ent = [n_dt[2 * i] + n_dt[2 * i + 1] - len(corr[0][i]) for i in range(P)]
    n_ge = [n_gt[2 * i] + n_gt[2 * i + 1] - len(corr[1][i]) for i in range(P)]
    err_off = np.zeros(P + 1, np.int64)
    np.cumsum([3 * a * b for a, b in zip(n_ent, n_ge)], out=err_off[1:])
    cat = lambda keys, dt, w: np.concatenate([np.asarray(x[k], dt).reshape(-1, w) for x in s for k in keys]).reshape(-1)      # noqa: E731
    cam = lambda key: np.stack([np.concatenate([np.asarray(x[key]["position"], np.float64), np.asarray(x[key]["rotation"], np.float64)]) for x in s])   # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    rows, nge, bad, errs = ops.recon_ap_assign(
        dev(cat(("iou0", "iou1"), np.float64, 1)), dev(off[2]), dev(off[0]), dev(off[1]), dev(cat(("score0", "score1"), np.float32, 1)),
        dev(cat(("plane0", "plane1"), np.float32, 3)), dev(cat(("gt_plane0", "gt_plane1"), np.float32, 3)), dev(cam("pred_cam")), dev(cam("gt_cam")),
        dev(np.concatenate(corr[0]).reshape(-1)), dev(coff[0]), dev(np.concatenate(corr[1]).reshape(-1)), dev(coff[1]), int(sum(n_ent)),
        max(n_dt) if max_dt is None else max_dt, max(n_gt) if max_gt is None else max_gt, err_off=dev(err_off), err_total=int(err_off[-1]))
    rows, errs = rows.cpu().numpy(), errs.cpu().numpy()
    split = np.cumsum([0] + n_ent)
    return ([rows[split[i]:split[i + 1]] for i in range(P)], nge.cpu().numpy(), bad.cpu().numpy(),
            [errs[err_off[i]:err_off[i + 1]].reshape(3, n_ent[i], n_ge[i]) for i in range(P)])


def _check_pair(rows, nge, errs, spec):
    want, want_nge, e = REF.pair_rows(*spec)
    assert rows.shape == want.shape and nge == want_nge
    assert np.array_equal(rows, want), np.argwhere(rows != want)[:8]       # score, five flags, both entry maps: exact
    for m, key in enumerate(("err_offsets", "err_normals", "mask_iou")):
        assert errs[m].shape == e[key].shape
        if e[key].size:
            assert np.abs(errs[m] - e[key]).max() <= (0.0 if key == "mask_iou" else 1e-9), key


@pytest.mark.parametrize("seed", RI.SEEDS)
def test_kernel_on_the_fixture_cases_without_masks(device, seed):
    """Every situation the seeds cover (tests/test_recon_eval_cpu.py::test_cases_cover_every_situation), all pairs of a seed in
    one launch, the IoU blocks computed on the host from the dense masks."""
    specs = [RI.pair_args(p) for p in RI.recon_eval_case(seed)]
    rows, nge, bad, errs = _launch(specs, device)
    assert not bad.any()
    for i, spec in enumerate(specs):
        _check_pair(rows[i], int(nge[i]), errs[i], spec)


def _random_spec(rng, n, m, n_pc, n_gc):
    """A pair from numbers alone: n = (n0, n1) predictions, m = (m0, m1) GT planes, n_pc / n_gc correspondences; the predictions are
    GT planes (through the GT camera) turned and shifted, the IoU blocks uniform draws with a few high values."""
    cam = RI._camera(rng)
    glob = [RI._unit(rng.normal(size=3)) * rng.uniform(1.5, 4.0) for _ in range(max(m[0], 1) + m[1])]
    gt = [np.asarray([RI._local_in_view0(g, cam)[0] for g in glob[:m[0]]], np.float32).reshape(-1, 3),
          np.asarray([g * RI.FLIP for g in glob[max(m[0], 1):]], np.float32).reshape(-1, 3)]
    planes, ious = [], []
    for v in range(2):
        src = rng.integers(0, max(m[v], 1), n[v])
        planes.append(np.asarray([RI._perturbed(rng, gt[v][k].astype(np.float64)) if m[v] else rng.normal(size=3) * 2 for k in src], np.float32).reshape(-1, 3))
        iou = rng.uniform(0.0, 0.45, (n[v], m[v]))
        if m[v]:
            iou[np.arange(n[v]), src] = rng.uniform(0.55, 1.0, n[v]) * (rng.uniform(size=n[v]) < 0.8)
        ious.append(iou)
    score = rng.permutation(np.linspace(0.15, 0.95, n[0] + n[1])).astype(np.float32)
    pc = np.stack([rng.permutation(n[0])[:n_pc], rng.permutation(n[1])[:n_pc]], 1)
    pc = pc[np.lexsort((pc[:, 1], pc[:, 0]))]                             # row-major order of the assignment matrix
    gc = np.stack([rng.permutation(m[0])[:n_gc], rng.permutation(m[1])[:n_gc]], 1)
    pred_cam = {"position": cam["position"] + rng.normal(size=3) * 0.1, "rotation": cam["rotation"] * 1.3}
    return (ious[0], ious[1], score[:n[0]], score[n[0]:], planes[0], planes[1], gt[0], gt[1], pred_cam, cam, pc, gc)


def _clear_of_thresholds(spec) -> bool:
    """No error of the pair within 1e-6 of its threshold and no matched normals within 1e-3 of perpendicular: 1e-9 of rounding
    cannot flip a flag.  No normal error below 1e-3 degrees either: acos next to 1 turns one ulp of the dot product into 1e-8
    radians, which says nothing about the kernel."""
    e = REF.pair_errors(*spec)
    n0, n1 = REF.global_planes(spec[4], spec[8])[1], REF.global_planes(spec[5], REF.IDENTITY)[1]
    dots = [abs(float(n0[a] @ n1[b])) for a, b in spec[10]]
    return (np.abs(e["err_normals"] - 30.0).min(initial=1.0) > 1e-6 and np.abs(e["err_offsets"] - 1.0).min(initial=1.0) > 1e-6
            and min(dots, default=1.0) > 1e-3 and e["err_normals"].min(initial=1.0) > 1e-3)


def _specs(seed, shapes):
    out = []
    for k, shape in enumerate(shapes):
        for attempt in range(50):
            spec = _random_spec(np.random.default_rng(1000 * seed + 50 * k + attempt), *shape)
            if _clear_of_thresholds(spec):
                out.append(spec)
                break
        else:
            raise RuntimeError("no draw clear of the thresholds")
    return out


def test_kernel_entry_counts_beyond_one_and_two_waves(device):
    """70 + 70 predictions with 5 correspondences (135 entries: the walk's lanes stride past 64 and 128) against 40 + 40 GT planes
    with 10 correspondences (70 GT entries: the ballot loop takes two chunks), next to small pairs in the same launch, one of them
    at the per-view limits of 128 predictions."""
    specs = _specs(5, [((3, 2), (2, 2), 1, 1), ((70, 70), (40, 40), 5, 10), ((128, 128), (3, 4), 100, 2), ((1, 0), (0, 1), 0, 0)])
    rows, nge, bad, errs = _launch(specs, device)
    assert not bad.any() and [len(r) for r in rows] == [4, 135, 156, 1] and nge.tolist() == [3, 70, 5, 1]
    for i, spec in enumerate(specs):
        _check_pair(rows[i], int(nge[i]), errs[i], spec)
    assert rows[1][:, 1:6].sum() > 20                                      # (true positives exist beyond the first wave's entries)
    assert rows[1][64:, 1:6].sum() > 0 and rows[1][128:, 5].sum() > 0


def test_kernel_the_walk_does_not_move_on(device):
    """Two predictions of view 1 whose first flagged GT entry is the same while a later flagged GT entry stays free: the second is a
    false positive under every criterion - written out by hand, apart from the seeds' drawn traps."""
    cam = {"position": [0.0, 0.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.0]}
    gt1 = np.array([[0, 0, 2.0], [0, 0, 2.3]], np.float32)                 # two parallel GT planes 0.3 apart, both in view 1
    p1 = np.array([[0, 0, 2.05], [0, 0, 2.1]], np.float32)
    iou1 = np.array([[0.9, 0.8], [0.7, 0.95]])                            # both overlap both
    none = np.zeros((0, 3), np.float32)
    spec = (np.zeros((0, 0)), iou1, np.zeros(0, np.float32), np.array([0.9, 0.8], np.float32), none, p1, none, gt1, cam, cam,
            np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32))
    rows, nge, bad, errs = _launch([spec], device)
    assert rows[0][:, 1:6].tolist() == [[1.0] * 5, [0.0] * 5] and nge.tolist() == [2] and rows[0][:, 6:].tolist() == [[-1, 0], [-1, 1]]
    _check_pair(rows[0], 2, errs[0], spec)


def test_kernel_flags_malformed_correspondences(device):
    """An index out of range (either side, either sign), a plane in two correspondences (predicted and GT): the pair is flagged, its
    rows stay zero and its GT entries are not counted; its neighbours in the launch are untouched."""
    good = _specs(9, [((4, 5), (3, 3), 2, 1), ((2, 2), (2, 3), 1, 2)])
    base = _specs(10, [((4, 4), (3, 3), 2, 2)])[0]

    def with_corrs(pc=None, gc=None):
        s = list(base)
        s[10], s[11] = (base[10] if pc is None else np.asarray(pc)), (base[11] if gc is None else np.asarray(gc))
        return tuple(s)
    broken = [with_corrs(pc=[[0, 1], [1, 4]]), with_corrs(pc=[[-1, 1], [1, 2]]), with_corrs(pc=[[0, 1], [2, 1]]), with_corrs(pc=[[3, 0], [3, 2]]),
              with_corrs(gc=[[0, 0], [0, 1]]), with_corrs(gc=[[1, 2], [3, 0]])]
    specs = [good[0]] + broken + [good[1]]
    rows, nge, bad, _ = _launch(specs, device)
    assert bad.tolist() == [0] + [1] * len(broken) + [0]
    for i in range(1, 1 + len(broken)):
        assert not rows[i].any() and nge[i] == 0
    for i in (0, len(specs) - 1):
        assert np.array_equal(rows[i], REF.pair_rows(*specs[i])[0])


def test_kernel_empty_launches_and_limits(device):
    from nopesac_amd import ops
    z64 = torch.zeros(1, device=device, dtype=torch.int64)
    f32, f64, i32 = (torch.zeros(0, device=device, dtype=t) for t in (torch.float32, torch.float64, torch.int32))
    rows, nge, bad = ops.recon_ap_assign(f64, z64, z64, z64, f32, f32, f32, f64, f64, i32, z64, i32, z64, 0, 0, 0)      # P = 0
    assert rows.shape == (0, 8) and nge.numel() == 0 and bad.numel() == 0
    # a pair with nothing in it, and one with GT only: no rows, the GT entries are counted
    cam = {"position": [0.1, 0.2, 0.3], "rotation": [0.5, 0.5, 0.5, 0.5]}
    none, nocorr = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.int32)
    empty = (np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0, np.float32), np.zeros(0, np.float32), none, none, none, none, cam, cam, nocorr, nocorr)
    gt_only = (np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.float32), np.zeros(0, np.float32), none, none, np.ones((2, 3), np.float32),
               np.ones((3, 3), np.float32), cam, cam, nocorr, np.array([[1, 2]], np.int32))
    rows, nge, bad, _ = _launch([empty, gt_only, empty], device)
    assert [len(r) for r in rows] == [0, 0, 0] and nge.tolist() == [0, 4, 0] and not bad.any()
    for max_dt, max_gt in ((129, 1), (1, 256)):
        with pytest.raises(ops._lib.HipKernelError, match="at most 128 predictions and 255 GT"):
            _launch([empty], device, max_dt=max_dt, max_gt=max_gt)


# ---- the evaluator
@pytest.fixture(scope="module", params=RI.SEEDS)
def fixture_case(request):
    pairs = RI.recon_eval_case(request.param)
    return pairs, gold(f"K_recon_eval_{request.param}"), RI.reference_rows(pairs)


def _check_table(got, g):
    assert list(got)[:6] == list(REF.CRITERIA) + ["npos"] and got["npos"] == float(g["npos"])
    for k, want, gap in zip(REF.CRITERIA, g["ap"].numpy(), g["gap_ap"].numpy()):
        assert abs(got[k] / 100.0 - want) <= max(4 * float(gap), 1e-12), (k, got[k], want)


def _product_pairs(pairs):
    from nopesac_amd import evaluation as E
    preds, dataset = RI.product_inputs(pairs)
    return [E._recon_pair((p["0"], p["1"]), [dataset[k]["0"]["annotations"], dataset[k]["1"]["annotations"]], p["camera"]["pred"],
                          dataset[k]["rel_pose"], p["pred_assignment"], dataset[k]["gt_corrs"], "test") for p, k in zip(preds, dataset)]


def test_recon_rows_from_masks_against_the_reference(device, fixture_case):
    """RLE masks in (compressed strings and run lists), rows out: flags as the reference's, the error matrices within 1e-9 of the
    reference's (float64 against float64), and the same rows bit for bit whether the pairs go in one batch or one by one."""
    from nopesac_amd import evaluation as E
    pairs, g, (ref_rows, ref_nge, _) = fixture_case
    todo = _product_pairs(pairs)
    rows, n_ent, n_ge, errs = E.recon_rows(todo, device, with_errors=True)
    assert np.array_equal(rows[:, 0], g["score"].numpy()) and np.array_equal(rows[:, 1:6], g["flags"].numpy())
    assert np.array_equal(rows, ref_rows) and n_ge.tolist() == ref_nge and int(n_ent.sum()) == len(rows)
    for i, e in enumerate(errs):
        want = g[f"err_{i}"].numpy()
        assert e.shape == want.shape
        if want.size:
            assert np.abs(e[:2] - want[:2]).max() <= 1e-9 and np.array_equal(e[2], want[2]), i
    one_by_one = [E.recon_rows([t], device) for t in todo]
    assert np.array_equal(np.concatenate([r[0] for r in one_by_one]), rows)
    assert [int(r[2][0]) for r in one_by_one] == n_ge.tolist() and [int(r[1][0]) for r in one_by_one] == n_ent.tolist()
    twisted = dict(todo[0], pred_corrs=np.array([[0, 0], [0, 1]], np.int32))      # plane 0 of view 0 in two correspondences
    with pytest.raises(ValueError, match=r"pair\(s\) \[1\]"):
        E.recon_rows([todo[1], twisted], device)


def test_evaluators_against_the_reference_table(device, fixture_case):
    from nopesac_amd import evaluation as E
    pairs, g, _ = fixture_case
    preds, dataset = RI.product_inputs(pairs)
    table = E.evaluate_for_reconstruction(preds, dataset, device)
    _check_table(table, g)
    assert table["pairs"] == len(pairs) and table["skipped"] == 0
    assert E.evaluate_for_reconstruction(preds, dataset, device, pairs_per_launch=1) == table
    less = {k: v for k, v in list(dataset.items())[1:]}                       # a record without its dataset pair is skipped and counted
    assert E.evaluate_for_reconstruction(preds, less, device)["skipped"] == 1
    inputs, outputs = RI.evaluator_batches(pairs)
    for step in (1, len(pairs)):
        ev = E.ReconEvaluator(device)
        for i in range(0, len(inputs), step):
            ev.process(inputs[i:i + step], outputs[i:i + step])
        assert ev.evaluate() == table
    ev = E.ReconEvaluator(device, pair_index={k: 10 - i for i, k in enumerate(dataset)})      # numbered against the feeding order
    ev.process(inputs + [{k: v for k, v in inputs[0].items() if k != "gt_corrs"}], outputs + outputs[:1])
    got = ev.evaluate()
    _check_table(got, g)
    assert got["skipped"] == 1 and got["pairs"] == len(pairs)


def test_cli_eval_recon(device, tmp_path, caplog):
    """`python -m nopesac_amd.run --eval-recon`: the table under results["recon"] is the one the host restatement gives for the
    instances, planes, camera and assignment the run dumped and the GT the pairs carried; the five rows are logged; a pair without
    gt_corrs is skipped and counted."""
    import logging
    import os
    from nopesac_amd import rle, run
    from nopesac_amd.synth import synth_pair
    from oracle import rle_oracle as R
    from tests.plane_eval_ref import mask_iou
    from tests.util import ROOT
    rng = np.random.default_rng(8)
    pairs = [synth_pair(70 + i, structured=True) for i in range(3)]
    gts = []
    for i, p in enumerate(pairs):
        cam = RI._camera(rng)
        p["rel_pose"] = {"position": [float(x) for x in cam["position"]], "rotation": [float(x) for x in cam["rotation"]]}
        blobs = [RI._blobs(rng, 480, 640, 4), RI._blobs(rng, 480, 640, 5)]
        planes = [(rng.normal(size=(len(b), 3)) * 2).astype(np.float32) for b in blobs]
        for v in "01":
            p[v]["annotations"] = [{"segmentation": R.encode(m), "plane": [float(x) for x in pl], "category_id": 1}
                                   for m, pl in zip(blobs[int(v)], planes[int(v)])]
        if i < 2:
            p["gt_corrs"] = [[0, 1], [2, 0]]
        gts.append((blobs, planes))
    torch.save(pairs, tmp_path / "pairs.pt")
    with caplog.at_level(logging.INFO, logger="nopesac_amd"):
        res = run.main(["--config-file", os.path.join(ROOT, "configs", "inference_mp3d.yaml"), "--eval-only", "--synthetic-weights", "--eval-recon",
                        "--pairs-file", str(tmp_path / "pairs.pt"), "--pairs-per-batch", "2", "--dump-dir", str(tmp_path / "dump"),
                        "MODEL.DEVICE", str(device)])
    assert "Reconstruction AP (2 pairs, 1 skipped" in caplog.text and "-normal-offset:" in caplog.text
    preds = torch.load(tmp_path / "dump" / "NopeSAC_instances_predictions.pth", weights_only=False)
    rows, npos = [], 0
    for pr, p, (blobs, planes) in list(zip(preds, pairs, gts))[:2]:
        dense = [np.stack([rle.decode(i["segmentation"]) for i in pr[v]["instances"]]) if pr[v]["instances"] else np.zeros((0, 480, 640), bool)
                 for v in "01"]
        cam = {"position": pr["camera"]["pred"]["tran"], "rotation": pr["camera"]["pred"]["rot"]}
        r, n_ge, _ = REF.pair_rows(mask_iou(dense[0], blobs[0]), mask_iou(dense[1], blobs[1]), [i["score"] for i in pr["0"]["instances"]],
                                   [i["score"] for i in pr["1"]["instances"]], pr["0"]["pred_plane"].numpy(), pr["1"]["pred_plane"].numpy(),
                                   planes[0], planes[1], cam, p["rel_pose"], np.argwhere(pr["pred_assignment"].numpy()), p["gt_corrs"])
        rows.append(r)
        npos += n_ge
    assert npos == 14 and sum(len(r) for r in rows) >= 2
    want = REF.table(np.concatenate(rows), npos)
    got = res["recon"]
    assert got["pairs"] == 2 and got["skipped"] == 1
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
