"""The host side of the polygon rasteriser (no GPU): tests/poly_reference.py - cocoapi's rleFrPoly + merge restated in its own sort /
difference form, the yardstick of tests/test_poly_gpu.py - against hand-worked masks, its round trip through rle.decode, the C surface
of nopesac_poly_to_bits, and the checks rle.polygon_bits and evaluate_for_matchings make before any device is touched."""
import numpy as np
import pytest

from tests import poly_reference as PR


def test_hand_worked_rectangle():
    """[1,1, 4,1, 4,3, 1,3] on 5 x 6: upsampled x crosses the column boundaries 5 k + 2.5 at x = 1, 2, 3 (5 -> 20 covers 7.5, 12.5,
    17.5; 2.5 and 22.5 lie outside), on the top edge at y = ceil((5 + .5) / 5 - .5) = 1 and on the bottom edge at y = ceil(2.6) = 3:
    columns 1..3, rows 1..2.  Column-major runs: 6 zeros (column 0 and row 0 of column 1), then 2 ones / 3 zeros per column."""
    assert PR.poly_runs([1, 1, 4, 1, 4, 3, 1, 3], 5, 6) == [6, 2, 3, 2, 3, 2, 12]
    dense = PR.mask_dense([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6)
    want = np.zeros((5, 6), bool)
    want[1:3, 1:4] = True
    assert np.array_equal(dense, want)
    assert sorted(PR.crossings([1, 1, 4, 1, 4, 3, 1, 3], 5, 6)) == [6, 8, 11, 13, 16, 18]


@pytest.mark.parametrize("h,w", [(5, 6), (7, 9), (33, 31)])
def test_full_frame_and_degenerate(h, w):
    assert PR.poly_runs([0, 0, w, 0, w, h, 0, h], h, w) == [0, h * w]
    assert PR.mask_dense([[0, 0, w, 0, w, h, 0, h]], h, w).all()
    for pt in ((2.0, 3.0), (0.0, 0.0), (w + 2.0, -1.0)):
        assert PR.poly_runs(list(pt) * 3, h, w) == [h * w]                # every point the same: no crossing, one run of zeros
    assert PR.mask_rle([[2, 3] * 4], h, w) == {"size": [h, w], "counts": [h * w]}


def test_negative_coordinates_truncate_toward_zero():
    """(int)(5 x + .5) truncates: x = -0.5 gives (int)(-2.0) = -2 and x = -0.7 gives (int)(-3.0) = -3, but x = -0.6 gives (int)(-2.5) =
    -2, not floor's -3; an edge that starts at a negative coordinate does not end on its vertex."""
    u, v = PR.boundary_points([-0.6, -0.6, 3, -0.6, 3, 2])
    assert (u[0], v[0]) == (-2, -1)              # the vertex is (-2, -2); the edge's first point is (int)(-2 + 0 + .5) = (int)(-1.5) = -1
    assert PR._upsampled([-0.6, -0.7, -0.5, 0])[0][:2] == [-2, -2] and PR._upsampled([-0.6, -0.7, -0.5, 0])[1][:2] == [-3, 0]


def test_runs_cover_the_image_and_round_trip():
    from nopesac_amd import rle
    rng = np.random.default_rng(5)
    for trial in range(60):
        h, w = int(rng.integers(3, 40)), int(rng.integers(3, 40))
        k = int(rng.integers(3, 12))
        kind = trial % 4
        pts = rng.uniform(-3, max(h, w) + 3, (k, 2))
        if kind == 1:
            pts = np.round(pts)
        elif kind == 2:
            pts = np.round(pts * 2) / 2
        polys = [pts.reshape(-1).tolist()]
        if trial % 3 == 0:
            polys.append(rng.uniform(0, [w, h], (4, 2)).reshape(-1).tolist())
        runs = PR.mask_runs(polys, h, w)
        assert sum(runs) == h * w and all(r > 0 for r in runs[1:])
        for xy in polys:
            single = PR.poly_runs(xy, h, w)
            assert sum(single) == h * w and all(r > 0 for r in single[1:])
            # cocoapi's sort / difference / fuse is the parity of the crossings at or before a pixel
            toggles = np.bincount(np.asarray([p for p in PR.crossings(xy, h, w) if p < h * w], np.int64), minlength=h * w)
            assert np.array_equal(np.cumsum(toggles) % 2 == 1, PR._dense_flat(single))
        dense = rle.decode(PR.mask_rle(polys, h, w))
        assert np.array_equal(dense, PR.mask_dense(polys, h, w))
        union = np.zeros((h, w), bool)
        for xy in polys:
            union |= rle.decode({"size": [h, w], "counts": PR.poly_runs(xy, h, w)})
        assert np.array_equal(dense, union)
        assert np.array_equal(PR.packed(dense)[: (h * w) // 32].view(np.uint8), np.packbits(dense.reshape(-1, order="F"), bitorder="little")[: (h * w) // 32 * 4])


def test_c_surface_of_the_polygon_rasteriser():
    """nopesac_poly_to_bits is declared nps_status, bound with the types the header states, exported by the library, and reports
    argument errors before any device call; n_masks = 0 is a valid call that enqueues nothing."""
    from ctypes import c_int, c_int64, c_void_p
    from nopesac_amd import _lib
    name = "nopesac_poly_to_bits"
    lib = _lib.load()
    assert name in _lib.declared_symbols() and name in _lib.STATUS and _lib.RESTYPES[name] is c_int and hasattr(lib, name)
    p, i, l = c_void_p, c_int, c_int64
    assert _lib.SIGNATURES[name] == [p, p, p, l, l, i, i, i, p, p, p, p, p]
    assert _lib.H.NPS_POLY_COORD_MAX == 1 << 29 and _lib.H.NPS_POLY_POINT_FACTOR >= 8 and _lib.H.NPS_POLY_POINT_FLOOR >= 0
    fn = lib.nopesac_poly_to_bits
    none = (None,) * 5
    assert fn(None, None, None, 0, 0, -1, 5, 6, *none) == -1 and b"n_masks" in lib.nopesac_last_error()
    assert fn(None, None, None, -1, 0, 1, 5, 6, *none) == -1 and fn(None, None, None, 0, -1, 1, 5, 6, *none) == -1
    assert fn(None, None, None, 3, 1, 2, 0, 5, *none) == -1 and b"H, W" in lib.nopesac_last_error()
    assert fn(None, None, None, 3, 1, 2, 5, -1, *none) == -1 and b"H, W" in lib.nopesac_last_error()
    assert fn(None, None, None, 3, 1, 2, 65536, 65536, *none) == -1 and b"H, W" in lib.nopesac_last_error()
    assert fn(None, None, None, 3, 1, 2, 5, 7, *none) == -1 and b"null pointer" in lib.nopesac_last_error()
    assert fn(None, None, None, 0, 0, 0, 5, 7, *none) == 0
    with pytest.raises(_lib.HipKernelError, match="null pointer"):
        _lib.C.nopesac_poly_to_bits(None, None, None, 3, 1, 2, 5, 7, *none)


def test_polygon_bits_checks_its_polygons_on_the_host():
    """Odd-length and too-short polygons are refused before anything is uploaded: device "cpu" would raise OpsArgumentError (there is
    no CPU path) if the call got as far as the library."""
    from nopesac_amd import rle
    good = [1, 1, 4, 1, 4, 3]
    with pytest.raises(ValueError, match="mask 1 has 7 numbers"):
        rle.polygon_bits([[good], [good + [2]]], 5, 6, "cpu")
    with pytest.raises(ValueError, match="mask 0 has 4 numbers"):
        rle.polygon_bits([[[1, 1, 4, 3]]], 5, 6, "cpu")                   # (cocoapi would read a list of 4-number entries as boxes)
    with pytest.raises(ValueError, match="mask 2 has 0 numbers"):
        rle.polygon_bits([[good], [good, good], [good, []]], 5, 6, "cpu")
    with pytest.raises(ValueError, match="need an image size"):
        rle.segmentation_bits([[good]], "cpu")
    with pytest.raises(ValueError, match="size"):
        rle.segmentation_bits([[good], {"size": [5, 6], "counts": [30]}], "cpu", size=(6, 5))
    with pytest.raises(TypeError, match="RLE dict or a list of polygons"):
        rle.segmentation_bits([[good], "abc"], "cpu", size=(5, 6))


def test_evaluators_take_gt_polygons_only_on_request_and_only_on_a_device():
    from nopesac_amd import evaluation as E
    poly = [[0, 0, 3, 0, 3, 3]]
    dataset = {"a__b": {"0": {"annotations": [{"segmentation": poly}]}, "1": {"annotations": []}, "gt_corrs": []}}
    preds = [{"0": {"image_id": "a", "instances": []}, "1": {"image_id": "b", "instances": []}, "pred_assignment": np.zeros((0, 0))}]
    with pytest.raises(ValueError, match="gt_polygons=True needs a device"):
        E.evaluate_for_matchings(preds, dataset, gt_polygons=True, device=None)
    with pytest.raises(TypeError, match="must be an RLE dict \\(polygons need cocoapi frPyObjects\\)"):
        E.evaluate_for_matchings(preds, dataset)
    assert E._rle_of(poly, "x", True) is poly and E._rle_of({"size": [1, 1], "counts": [1]}, "x", True)
    with pytest.raises(TypeError, match="RLE dict or a list of polygons"):
        E._rle_of("abc", "x", True)
    # nothing with predictions: no device work, polygon GT still counts in npos
    ev = E.PlaneEvaluator("cpu", gt_polygons=True)
    ev.process([{"0": {"image_id": "a", "annotations": [{"segmentation": poly, "category_id": 1, "plane": [0, 0, 1]}]},
                 "1": {"image_id": "b", "annotations": []}}], [{"0": {"instances": []}, "1": None}])
    assert float(np.concatenate(ev._gt)[:, 2].sum()) == 1.0 and ev.evaluate()["mask_ap@0.5"] == 0.0
    with pytest.raises(TypeError, match="frPyObjects"):
        E.PlaneEvaluator("cpu").process([{"0": {"image_id": "a", "annotations": [{"segmentation": poly, "category_id": 1}]},
                                          "1": {"image_id": "b", "annotations": []}}], [{"0": {"instances": []}, "1": None}])
    import inspect
    for fn in (E.plane_rows, E.recon_rows, E.evaluate_for_planes, E.evaluate_for_reconstruction, E.evaluate_for_matchings,
               E.PlaneEvaluator.__init__, E.ReconEvaluator.__init__):
        assert inspect.signature(fn).parameters["gt_polygons"].default is False
