"""csrc/plane_eval.hip on the GPU: nopesac_poly_to_bits against tests/poly_reference.py (cocoapi's rleFrPoly + merge in its own sort /
difference form) - bit equality everywhere, the results are integers - then rle.polygon_bits / rle.segmentation_bits and the three
evaluators with gt_polygons=True against the same calls on GT converted to uncompressed RLE dicts by the reference.

Shapes: the smallest that reach every path.  Vertex counts 3 .. 2049 cross the 256-edge chunk of the kernel (63 / 64 / 65 the wave, 300
one chunk boundary, 2049 eight of them and a last chunk of one edge); image sizes 5 x 6 (one word), 7 x 9 and 33 x 31 (last word
partly used), 64 x 64 (full words, 128 of them: half a step of the 256-word parity scan) and 480 x 640 (9600 words: 38 steps, where a
wrong carry from step to step shows)."""
import numpy as np
import pytest
import torch

from oracle import rle_oracle as R
from tests import poly_reference as PR

pytestmark = pytest.mark.gpu

KINDS = ("integer", "half", "random", "outside", "closed", "duplicates", "collinear")
COUNTS = (3, 4, 63, 64, 65, 300, 2049)
GUARD, FILL = 64, 0x5A5A5A5A


def _star(rng, k, h, w, integer=False):
    """k points around a centre at sorted angles: a contour-like outline."""
    cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.15, 0.5, k) * min(h, w)
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return np.round(pts) if integer else pts


def _polygon(rng, kind, k, h, w):
    """A flat polygon of exactly k vertices."""
    if kind == "integer":
        pts = rng.integers(0, [w + 1, h + 1], (k, 2)).astype(np.float64)
    elif kind == "half":
        pts = rng.integers(0, [2 * w + 1, 2 * h + 1], (k, 2)) / 2.0
    elif kind == "random":
        pts = rng.uniform(0, [w, h], (k, 2))
    elif kind == "outside":                      # the truncating cast, dropped columns, y clamped to H
        pts = rng.uniform(-3, max(h, w) + 3, (k, 2))
    elif kind == "closed":                       # a contour that repeats its first point
        pts = _star(rng, k - 1, h, w)
        pts = np.concatenate([pts, pts[:1]])
    elif kind == "duplicates":                   # consecutive duplicate vertices (edges of length 0), also across the closing edge
        base = _star(rng, k - k // 3, h, w, integer=bool(k % 2))
        idx = np.sort(np.concatenate([np.arange(len(base)), rng.integers(0, len(base), k - len(base) - 1), [0]]))
        pts = np.roll(base[idx], -1, axis=0) if k > 3 else base[idx]
    else:                                        # collinear: the midpoints of an integer outline's edges are vertices too
        base = _star(rng, (k + 1) // 2, h, w, integer=True)
        mid = (base + np.roll(base, -1, axis=0)) / 2.0
        pts = np.stack([base, mid], 1).reshape(-1, 2)[:k]
    assert pts.shape == (k, 2)
    return pts.reshape(-1).tolist()


def _grid_masks(h, w, seed):
    """70 masks: every kind with every vertex count (49), then 21 more; 1, 2 or 5 polygons per mask, the further ones small."""
    rng = np.random.default_rng(seed)
    masks = []
    for i in range(70):
        kind, k = KINDS[i % 7], COUNTS[(i // 7) % 7]
        polys = [_polygon(rng, kind, k, h, w)]
        for extra in range((1, 2, 5)[i % 3] - 1):
            polys.append(_polygon(rng, KINDS[(i + extra + 1) % 7], (3, 4, 63, 65)[(i + extra) % 4], h, w))
        masks.append(polys)
    return masks


def _few_masks(h, w, seed, big=300):
    """21 masks: every kind with 1, 2 and 5 polygons (overlapping outlines and disjoint boxes), vertex counts cycling; one outline of
    2049 vertices."""
    rng = np.random.default_rng(seed)
    masks = []
    for i in range(21):
        kind, n = KINDS[i % 7], (1, 2, 5)[i // 7]
        polys = [_polygon(rng, kind, (3, 4, 63, 64, 65, big)[(i + j) % 6] if j == 0 else (3, 4, 65)[(i + j) % 3], h, w) for j in range(n)]
        if n == 5:                               # two disjoint boxes among them
            polys[3] = [0, 0, w / 4, 0, w / 4, h / 4, 0, h / 4]
            polys[4] = [w / 2 + 0.5, h / 2, w, h / 2, w, h, w / 2 + 0.5, h]
        masks.append(polys)
    masks[4] = [_polygon(rng, "closed", 2049, h, w)]
    return masks


def _large_masks():
    h, w = 480, 640
    rng = np.random.default_rng(7)
    return [
        [_polygon(rng, "closed", 300, h, w)],
        [_polygon(rng, "random", 5, h, w)],
        [[0, 0, w, 0, w, h, 0, h]],                                             # every pixel: the carry runs through all 9600 words
        [_polygon(rng, "collinear", 64, h, w), [10, 10, 200.5, 10, 200.5, 90, 10, 90], [500, 400, 630, 400, 630, 470, 500, 470],
         _polygon(rng, "half", 4, h, w), _polygon(rng, "duplicates", 65, h, w)],
        [_polygon(rng, "outside", 4, h, w)],
        [[600.3, 470.2, 639.6, 471.0, 639.9, 479.9, 601.0, 478.5]],              # only the last columns
        [[-2, -2, 0.6, -2, 0.6, h + 2, -2, h + 2], [w - 0.6, 3, w + 3, 3, w + 3, h - 3]],      # the first and the last column
    ]


def _flatten(masks):
    polys = [np.asarray(p, np.float64) for m in masks for p in m]
    poly_off = np.zeros(len(polys) + 1, np.int64)
    np.cumsum([p.size // 2 for p in polys], out=poly_off[1:])
    mask_off = np.zeros(len(masks) + 1, np.int64)
    np.cumsum([len(m) for m in masks], out=mask_off[1:])
    return np.concatenate(polys) if polys else np.zeros(0), poly_off, mask_off


def _run_raw(masks, h, w, device):
    """One launch through ops.poly_to_bits into a guarded buffer -> (words uint32 [n, words], area, bad, whole buffer)."""
    from nopesac_amd import ops
    xy, poly_off, mask_off = _flatten(masks)
    n, words = len(masks), (h * w + 31) // 32
    buf = torch.full((GUARD + n * words + GUARD,), FILL, dtype=torch.int32, device=device)
    bits, area, bad = ops.poly_to_bits(torch.from_numpy(xy).to(device), torch.from_numpy(poly_off).to(device), torch.from_numpy(mask_off).to(device),
                                       h, w, bits=buf[GUARD:GUARD + n * words])
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "guard words changed"
    return host[GUARD:GUARD + n * words].view(np.uint32).reshape(n, words), area.cpu().numpy(), bad.cpu().numpy(), host


def _check_raw(masks, h, w, device, want=None):
    got, area, bad, host = _run_raw(masks, h, w, device)
    assert not bad.any(), np.flatnonzero(bad)
    for i, polys in enumerate(masks):
        dense = PR.mask_dense(polys, h, w) if want is None else want[i]
        exp = PR.packed(dense)
        assert np.array_equal(got[i], exp), (i, h, w, [len(p) // 2 for p in polys], int(np.flatnonzero(got[i] != exp)[0]))
        assert int(area[i]) == int(dense.sum()) == int(sum(bin(int(x)).count("1") for x in got[i])), i
    if (h * w) % 32:
        assert not (got[:, -1] >> np.uint32((h * w) % 32)).any()
    again = _run_raw(masks, h, w, device)
    assert np.array_equal(again[3], host) and np.array_equal(again[1], area), "a second call gives other bytes"
    return got


GRID = {"size": (7, 9), "seed": 101}
FEW = {(5, 6): 102, (33, 31): 103, (64, 64): 104}


@pytest.fixture(scope="module")
def reference():
    """The reference's dense masks, computed once: {name: (masks, h, w, dense list)}."""
    out = {}
    h, w = GRID["size"]
    out["grid"] = (_grid_masks(h, w, GRID["seed"]), h, w)
    for (h, w), seed in FEW.items():
        out[f"few{h}x{w}"] = (_few_masks(h, w, seed, big=2049 if (h, w) == (5, 6) else 300), h, w)
    out["large"] = (_large_masks(), 480, 640)
    return {k: (m, h, w, [PR.mask_dense(p, h, w) for p in m]) for k, (m, h, w) in out.items()}


def test_hand_worked_rectangle_one_mask(device):
    got = _check_raw([[[1, 1, 4, 1, 4, 3, 1, 3]]], 5, 6, device)
    want = np.zeros((5, 6), bool)
    want[1:3, 1:4] = True
    assert np.array_equal(got[0], PR.packed(want))


def test_every_kind_with_every_vertex_count_70_masks_in_one_launch(device, reference):
    masks, h, w, dense = reference["grid"]
    assert len(masks) == 70 and {(KINDS[i % 7], len(m[0]) // 2) for i, m in enumerate(masks)} >= {(a, b) for a in KINDS for b in COUNTS}
    assert {len(m) for m in masks} == {1, 2, 5}
    _check_raw(masks, h, w, device, dense)


@pytest.mark.parametrize("size", list(FEW))
def test_sizes_and_polygons_per_mask(device, reference, size):
    masks, h, w, dense = reference["few%dx%d" % size]
    assert any(d.any() for d in dense) and not all(d.all() for d in dense)
    _check_raw(masks, h, w, device, dense)


def test_480x640(device, reference):
    masks, h, w, dense = reference["large"]
    assert dense[2].all() and dense[5][:, :600].sum() == 0 and dense[5].any() and dense[6][:, 0].all() and dense[6][:, -1].any()
    _check_raw(masks, h, w, device, dense)


def test_bad_flags_are_values(device):
    """A NaN coordinate, a coordinate of 1e12, a 2-point polygon, a mask without polygons, and a single far-away vertex (more boundary
    points than the cap; the coordinate itself is within the bound): bad is set for that mask only, its words are zero, the masks
    around it are right and the guards untouched.  rle.polygon_bits raises ValueError naming the masks."""
    from nopesac_amd import _lib, rle
    h, w = 7, 9
    cap = _lib.H.NPS_POLY_POINT_FACTOR * (h * w + h + w) + _lib.H.NPS_POLY_POINT_FLOOR
    assert cap >= 8 * h * w + 8 * (h + w) and 5 * 1e7 < _lib.H.NPS_POLY_COORD_MAX and 5 * 1e7 > cap
    rng = np.random.default_rng(9)
    good = [[_polygon(rng, KINDS[i], (4, 65, 5, 300, 3, 64)[i], h, w)] for i in range(6)]
    tri = [1.0, 1.0, 6.0, 2.0, 3.0, 6.0]
    bads = [[tri, [1.0, float("nan"), 5.0, 1.0, 5.0, 5.0]], [[1.0, 1.0, 1e12, 2.0, 3.0, 6.0]], [tri, [1.0, 1.0, 5.0, 5.0]], [],
            [[1.0, 1.0, 1e7, 2.0, 3.0, 6.0], tri], [[float("inf"), 1.0, 6.0, 2.0, 3.0, 6.0]]]
    masks = [good[0], bads[0], good[1], bads[1], good[2], bads[2], bads[3], good[3], bads[4], good[4], bads[5], good[5]]
    is_bad = [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0]
    got, area, bad, _ = _run_raw(masks, h, w, device)
    assert bad.tolist() == is_bad
    for i, (polys, b) in enumerate(zip(masks, is_bad)):
        if b:
            assert not got[i].any() and int(area[i]) == 0, i
        else:
            dense = PR.mask_dense(polys, h, w)
            assert np.array_equal(got[i], PR.packed(dense)) and int(area[i]) == int(dense.sum()), i
    got, area, bad, _ = _run_raw([[], []], h, w, device)                                 # no coordinate at all
    assert bad.tolist() == [1, 1] and not got.any()
    for k, polys in enumerate(bads):
        if k == 2:
            continue                                                                       # (refused on the host: test_poly_cpu.py)
        with pytest.raises(ValueError, match=r"masks \[1\] of 3"):
            rle.polygon_bits([good[0], polys, good[1]], h, w, device)
    bits, area = rle.polygon_bits([good[0], good[1]], h, w, device)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), np.stack([PR.packed(PR.mask_dense(g, h, w)) for g in good[:2]]))
    bits, area = rle.polygon_bits([], h, w, device)
    assert bits.shape == (0, 2) and area.shape == (0,)


def test_segmentation_bits_mixes_rle_and_polygons(device):
    from nopesac_amd import rle
    h, w = 33, 31
    rng = np.random.default_rng(4)
    polys = [[_polygon(rng, "closed", 40, h, w)], [_polygon(rng, "half", 5, h, w), _polygon(rng, "outside", 4, h, w)], [[0, 0, w, 0, w, h, 0, h]]]
    dense = [rng.uniform(size=(h, w)) < 0.4 for _ in range(3)]
    segs = [polys[0], R.encode(dense[0]), {"size": [h, w], "counts": R.run_lengths(dense[1])}, polys[1], polys[2], R.encode(dense[2])]
    want = [PR.mask_dense(polys[0], h, w), dense[0], dense[1], PR.mask_dense(polys[1], h, w), PR.mask_dense(polys[2], h, w), dense[2]]
    bits, area = rle.segmentation_bits(segs, device)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), np.stack([PR.packed(d) for d in want]))
    assert area.tolist() == [int(d.sum()) for d in want]
    one, a1 = rle.segmentation_bits(polys, device, size=(h, w))                             # polygons only: the size is given
    assert torch.equal(one, bits[[0, 3, 4]]) and torch.equal(a1, area[[0, 3, 4]])
    two, a2 = rle.segmentation_bits([segs[1], segs[2], segs[5]], device)                    # RLE only: decode_bits
    assert torch.equal(two, bits[[1, 2, 5]]) and torch.equal(a2, area[[1, 2, 5]])
    with pytest.raises(ValueError, match="need an image size"):
        rle.segmentation_bits(polys, device)
    m = rle.iou_device([segs[1], R.encode(want[0])], [polys[0], segs[2], polys[2]], device=device)
    assert np.array_equal(m, rle.iou([segs[1], R.encode(want[0])], [R.encode(want[0]), segs[2], R.encode(want[4])]))


# ---- the evaluators --------------------------------------------------------------------------------------------------------------
H, W = 48, 64


def _unit(v):
    return v / np.linalg.norm(v)


def _eval_view(rng, with_preds=True):
    """GT: 2 - 4 annotations of one or two polygons (outlines and boxes); predictions: shifted copies of the GT masks and stripes."""
    yy, xx = np.mgrid[0:H, 0:W]
    gt = []
    for k in range(int(rng.integers(2, 5))):
        x0, y0 = rng.uniform(0, W - 12), rng.uniform(0, H - 12)
        box = [x0, y0, x0 + rng.uniform(4, 12), y0, x0 + rng.uniform(4, 12), y0 + rng.uniform(4, 12), x0, y0 + rng.uniform(4, 12)]
        gt.append([_polygon(rng, "closed", int(rng.integers(8, 40)), H, W)] + ([box] if k % 2 else []))
    dense = [PR.mask_dense(p, H, W) for p in gt]
    preds = []
    if with_preds:
        for d in dense:
            if rng.uniform() < 0.85:
                preds.append(np.roll(d, int(rng.integers(-2, 3)), axis=int(rng.integers(0, 2))))
        preds.append((xx + yy) % 7 == 0)
    n = len(preds)
    return {"gt_polys": gt, "gt_dense": dense, "gt_plane": (rng.normal(size=(len(gt), 3)) * 2).astype(np.float32),
            "pred": preds, "pred_plane": (rng.normal(size=(n, 3)) * 2).astype(np.float32)}


def _annotations(view, form):
    """form(k) -> "poly" | "rle" | "string": how annotation k carries its mask."""
    out = []
    for k, (polys, dense, plane) in enumerate(zip(view["gt_polys"], view["gt_dense"], view["gt_plane"])):
        seg = {"poly": polys, "rle": PR.mask_rle(polys, H, W), "string": R.encode(dense)}[form(k)]
        out.append({"segmentation": seg, "plane": [float(x) for x in plane], "category_id": 1})
    return out


@pytest.fixture(scope="module")
def eval_case():
    """Four pairs; the last one has no prediction in view 1.  -> build(form) = (predictions, dataset_dict)."""
    rng = np.random.default_rng(31)
    pairs = []
    for i in range(4):
        views = (_eval_view(rng), _eval_view(rng, with_preds=i < 3))
        n0, n1 = len(views[0]["pred"]), len(views[1]["pred"])
        A = np.zeros((n0, n1), np.uint8)
        for d in range(min(n0, n1, 2)):
            A[d, (d + i) % n1] = 1
        m = min(len(views[0]["gt_polys"]), len(views[1]["gt_polys"]))
        cam = lambda: {"position": rng.uniform(-1, 1, 3), "rotation": _unit(rng.normal(size=4))}     # noqa: E731
        pairs.append({"ids": (f"q{i}a", f"q{i}b"), "views": views, "A": A, "gt_corrs": [[k, (k + 1) % m] for k in range(m - 1)],
                      "pred_cam": cam(), "gt_cam": cam()})
    total = sum(len(v["pred"]) for p in pairs for v in p["views"])
    score = iter((np.linspace(0.95, 0.2, total)[rng.permutation(total)]).astype(np.float32).tolist())

    for p in pairs:
        for v in p["views"]:
            v["instances"] = [{"segmentation": R.encode(m), "score": next(score), "category_id": 0} for m in v["pred"]]

    def build(form):
        preds, dataset = [], {}
        for p in pairs:
            pred = {"camera": {"pred": {"tran": np.asarray(p["pred_cam"]["position"]), "rot": np.asarray(p["pred_cam"]["rotation"])},
                               "gts": {"tran": list(p["gt_cam"]["position"]), "rot": list(p["gt_cam"]["rotation"])}},
                    "pred_assignment": torch.from_numpy(p["A"].copy())}
            entry = {"gt_corrs": [list(c) for c in p["gt_corrs"]],
                     "rel_pose": {"position": list(p["gt_cam"]["position"]), "rotation": list(p["gt_cam"]["rotation"])}}
            for v, image_id, view in zip("01", p["ids"], p["views"]):
                pred[v] = {"image_id": image_id, "pred_plane": torch.from_numpy(view["pred_plane"].copy()), "instances": view["instances"]}
                entry[v] = {"image_id": image_id, "annotations": _annotations(view, form)}
            dataset[p["ids"][0] + "__" + p["ids"][1]] = entry
            preds.append(pred)
        return preds, dataset
    return build


FORMS = {"polygons": lambda k: "poly", "mixed": lambda k: ("poly", "rle", "string")[k % 3]}


def _plane_views(preds, dataset):
    return [{"instances": p[v]["instances"], "pred_plane": p[v]["pred_plane"], "annotations": dataset[key][v]["annotations"]}
            for p, key in zip(preds, dataset) for v in "01" if p[v]["instances"]]


def _recon_pairs(preds, dataset, E):
    return [E._recon_pair((p["0"], p["1"]), [dataset[key]["0"]["annotations"], dataset[key]["1"]["annotations"]], p["camera"]["pred"],
                          dataset[key]["rel_pose"], p["pred_assignment"], dataset[key]["gt_corrs"], "test", True) for p, key in zip(preds, dataset)]


@pytest.mark.parametrize("form", list(FORMS))
def test_rows_and_tables_with_polygon_gt_equal_those_with_rle_gt(device, eval_case, form):
    from nopesac_amd import evaluation as E
    preds, rle_set = eval_case(lambda k: "rle")
    _, poly_set = eval_case(FORMS[form])
    want = E.plane_rows(_plane_views(preds, rle_set), device)
    got = E.plane_rows(_plane_views(preds, poly_set), device, gt_polygons=True)
    assert want.shape[0] > 10 and (want[:, 8] > 0.5).any() and np.array_equal(got, want, equal_nan=True)
    want = E.recon_rows(_recon_pairs(preds, rle_set, E), device, with_errors=True)
    got = E.recon_rows(_recon_pairs(preds, poly_set, E), device, with_errors=True, gt_polygons=True)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and want[0].shape[0] > 10
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[3], want[3]))
    want = E.evaluate_for_matchings(preds, rle_set, device=device)
    assert E.evaluate_for_matchings(preds, poly_set, device=device, gt_polygons=True) == want
    assert want["pred_assignment"]["Pred. Num."] > 0 and want["pred_assignment"]["GT Num."] > 0
    want = E.evaluate_for_planes(preds, rle_set, device)
    got = E.evaluate_for_planes(preds, poly_set, device, gt_polygons=True)
    assert list(got) == list(want) and all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in want)
    assert E.evaluate_for_reconstruction(preds, poly_set, device, gt_polygons=True) == E.evaluate_for_reconstruction(preds, rle_set, device)
    with pytest.raises(TypeError, match="frPyObjects"):
        E.plane_rows(_plane_views(preds, poly_set), device)


def test_evaluator_classes_with_polygon_gt(device, eval_case):
    """PlaneEvaluator / ReconEvaluator with gt_polygons=True: fed one pair at a time and all at once, and on RLE GT - one table."""
    from nopesac_amd import evaluation as E
    preds, rle_set = eval_case(lambda k: "rle")
    _, poly_set = eval_case(FORMS["mixed"])
    outputs = [{"0": {k: p["0"][k] for k in ("instances", "pred_plane")}, "1": {k: p["1"][k] for k in ("instances", "pred_plane")},
                "camera": p["camera"]["pred"], "pred_assignment": p["pred_assignment"]} for p in preds]

    def tables(dataset, at_once, **kw):
        inputs = [dataset[key] for key in dataset]
        out = []
        for ev in (E.PlaneEvaluator(device, **kw), E.ReconEvaluator(device, **kw)):
            if at_once:
                ev.process(inputs, outputs)
            else:
                for i, o in zip(inputs, outputs):
                    ev.process([i], [o])
            out.append(ev.evaluate())
        return out
    want = tables(rle_set, True)
    assert want[0]["mask_ap@0.5"] > 0 and want[1]["npos"] > 0 and want[1]["pairs"] == 4
    for at_once in (True, False):
        got = tables(poly_set, at_once, gt_polygons=True)
        for g, t in zip(got, want):
            assert list(g) == list(t) and all(g[k] == t[k] or (np.isnan(g[k]) and np.isnan(t[k])) for k in t)
    with pytest.raises(TypeError, match="frPyObjects"):
        tables(poly_set, True)


def test_no_prediction_at_all_with_polygon_gt(device, eval_case):
    """Only empty IoU blocks: nothing is rasterised, so no image size is needed and none is asked for."""
    from nopesac_amd import evaluation as E
    preds, rle_set = eval_case(lambda k: "rle")
    _, poly_set = eval_case(FORMS["polygons"])
    bare = [{**p, "0": {**p["0"], "instances": [], "pred_plane": torch.zeros(0, 3)}, "1": {**p["1"], "instances": [], "pred_plane": torch.zeros(0, 3)},
             "pred_assignment": torch.zeros(0, 0, dtype=torch.uint8)} for p in preds]
    assert E.plane_rows([{"instances": [], "pred_plane": np.zeros((0, 3)), "annotations": poly_set[key]["0"]["annotations"]} for key in poly_set],
                        device, gt_polygons=True).shape == (0, 10)
    got = E.recon_rows(_recon_pairs(bare, poly_set, E), device, gt_polygons=True)
    want = E.recon_rows(_recon_pairs(bare, rle_set, E), device)
    assert got[0].shape == (0, 8) and all(np.array_equal(a, b) for a, b in zip(got, want)) and want[2].sum() > 0
    assert E.evaluate_for_matchings(bare, poly_set, device=device, gt_polygons=True) == E.evaluate_for_matchings(bare, rle_set, device=device)
    assert E.evaluate_for_planes(bare, poly_set, device, gt_polygons=True)["mask_ap@0.5"] == 0.0
    assert E.evaluate_for_reconstruction(bare, poly_set, device, gt_polygons=True) == E.evaluate_for_reconstruction(bare, rle_set, device)
