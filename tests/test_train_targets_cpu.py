"""Training targets without a device: the numpy restatement (tests/train_targets_forms.py) against the reference's own outputs
(tests/golden/train_targets/*.npz, scripts/gen_train_targets_golden.py), the host side of nopesac_amd/targets.py - padding and filter of
the correspondences, the pose sign, both readers, every ValueError - and the argument refusals of the five launchers through the C ABI."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from tests import train_targets_forms as F


def _lib():
    from nopesac_amd import _lib
    return _lib


# ---- the restatement against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.GOLDEN_CASES))
def test_restatement_matches_the_reference_fixture(name):
    labels, K = F.golden_case(name)
    H, W = labels.shape
    g = np.load(os.path.join(F.GOLD, name + ".npz"))
    ids, n_all, n, bad = F.label_ids(labels[None], _lib().H.NPS_LABEL_MAX_IDS)
    assert not bad[0] and int(n[0]) == int(g["n"]) == min(int(n_all[0]), 50)
    masks, centers, pixel = F.label_targets(labels[None], ids, n, int(n[0]))
    assert np.array_equal(np.packbits(masks[0].reshape(int(n[0]), -1), axis=1), g["masks"])
    c64 = F.centers64(masks, n)[0]
    assert np.abs(g["plane_centers"] - c64).max() <= float(g["gap_plane_centers"])
    p64 = (c64[:, :, None, None] * masks[0][:, None].astype(np.float64)).sum(0)
    assert np.abs(g["pixel_centers"] - p64).max() <= float(g["gap_pixel_centers"])
    k64, mag = F.coordinate_map(K, H, W)
    assert (np.abs(g["k_inv_dot_xy1"] - k64).reshape(3, -1).max(1) <= g["gap_k_inv_dot_xy1"]).all()
    # the gaps are rounding, not a different formula: a few f32 ulps of the values
    assert float(g["gap_plane_centers"]) <= 4 * 2.0 ** -24 and (g["gap_k_inv_dot_xy1"] <= 4 * 2.0 ** -24 * mag.reshape(3, -1).max(1)).all()
    # f32 centres of the restatement: the correctly rounded float64 quotient
    assert np.array_equal(centers[0], c64.astype(np.float32))


def test_restatement_on_the_edge_cases():
    H = _lib().H
    cases = F.label_cases(H.NPS_LABEL_MAX_IDS, H.NPS_LABEL_TABLE_SLOTS)
    want = {"zeros": 0, "one_id": 1, "ids50": 50, "ids51": 51, "ids1000": 1000, "collide": 40, "collide_neg": 15, "negative": 5, "int_max": 4,
            "last_pixel": 3, "exactly_cap": H.NPS_LABEL_MAX_IDS}
    for name, count in want.items():
        ids, n_all, n, bad = F.label_ids(cases[name], H.NPS_LABEL_MAX_IDS)
        assert (int(n_all[0]), int(n[0]), int(bad[0])) == (count, min(count, 50), 0), name
    for name in ("too_many", "cap_with_zero"):
        ids, n_all, n, bad = F.label_ids(cases[name], H.NPS_LABEL_MAX_IDS)
        assert (int(n_all[0]), int(n[0]), int(bad[0])) == (0, 0, 1) and not ids.any(), name
    ids, n_all, n, bad = F.label_ids(cases["negative"], H.NPS_LABEL_MAX_IDS)
    assert ids[0, :5].tolist() == [-5, -1, 0, 3, 9]                                         # 0 is not first: it stays a plane
    ids, *_ = F.label_ids(cases["int_max"], H.NPS_LABEL_MAX_IDS)
    assert ids[0, :4].tolist() == [-2**31, 0, 1, 2**31 - 1]
    assert F.label_ids(cases["ragged"], H.NPS_LABEL_MAX_IDS)[2].tolist() == [3, 50, 1]
    assert int((cases["last_pixel"] == 77).sum()) == 1 and cases["last_pixel"][0, -1, -1] == 77
    assert (cases["collide"][cases["collide"] != 0] % H.NPS_LABEL_TABLE_SLOTS == 0).all()
    big = F.big_case()
    assert [F.unique_ids(m).size for m in big] == [20, 50]
    m = F.mask_views(17, 33, 3)[0][0]
    bits = np.zeros((1, (17 * 33 + 31) // 32), np.int32)
    flat = m.reshape(-1, order="F")
    for p in np.flatnonzero(flat):
        bits.view(np.uint32)[0, p >> 5] |= np.uint32(1) << np.uint32(p & 31)
    assert np.array_equal(F.unpack_bits(bits, 17, 33)[0], m)
    from nopesac_amd import rle
    assert np.array_equal(rle.decode(F.to_rle(m)), m)


# ---- host side of the mapper ------------------------------------------------------------------------------------------------------------
def test_correspondences_are_filtered_and_padded():
    from nopesac_amd.targets import pad_corrs
    got = pad_corrs([[(0, 1), (50, 2), (3, 49), (7, 60)], [], [(1, 1), (2, 2), (49, 49)]])
    assert got.dtype == np.int32 and got.shape == (3, 3, 2)
    assert got[0].tolist() == [[0, 1], [3, 49], [-1, -1]] and (got[1] == -1).all() and got[2].tolist() == [[1, 1], [2, 2], [49, 49]]
    assert pad_corrs([[], []]).shape == (2, 1, 2)                                            # K >= 1: the launcher takes no empty table
    assert pad_corrs([np.zeros((0, 2), np.int64)]).tolist() == [[[-1, -1]]]


def test_pose_rows_follow_process_camera():
    from nopesac_amd.targets import pose_rows
    poses = [{"position": [1.0, -2.0, 0.5], "rotation": [-0.5, 0.5, -0.5, 0.5]}, {"position": [0, 0, 0], "rotation": [0.9, 0.1, 0.2, -0.3]},
             {"position": [3, 2, 1], "rotation": [0.0, -1.0, 0.0, 0.0]}]
    got = pose_rows(poses)
    assert got.dtype == np.float32 and got.shape == (3, 7)
    assert got[0].tolist() == [1.0, -2.0, 0.5, 0.5, -0.5, 0.5, -0.5]                         # w < 0: negated
    assert np.array_equal(got[1], np.float32([0, 0, 0, 0.9, 0.1, 0.2, -0.3])) and got[2].tolist() == [3, 2, 1, 0, -1, 0, 0]      # w == 0 stays
    assert pose_rows(poses, flip_negative_w=False)[0, 3:].tolist() == [-0.5, 0.5, -0.5, 0.5]
    from nopesac_amd.config import get_cfg
    from nopesac_amd.targets import TargetMapper
    cfg = get_cfg()
    assert TargetMapper.from_cfg(cfg, "cpu").flip_negative_w is (not cfg.MODEL.CAMERA_HEAD.CLASSIFICATION_ON)


def test_readers(tmp_path):
    from PIL import Image
    from nopesac_amd.targets import read_mp3d_observation, read_scannet_view
    rng = np.random.default_rng(0)
    sem, dep = rng.integers(0, 9, (6, 8)).astype(np.int64), rng.random((6, 8))
    with open(tmp_path / "obs.pkl", "wb") as f:
        pickle.dump({"semantic_sensor": sem, "depth_sensor": dep, "color_sensor": np.zeros((6, 8, 4), np.uint8)}, f)
    got = read_mp3d_observation(str(tmp_path / "obs.pkl"))
    assert got["semantic_map"].dtype == np.int32 and np.array_equal(got["semantic_map"], sem)
    assert got["depth"].dtype == np.float32 and np.array_equal(got["depth"], dep.astype(np.float32))
    d16 = rng.integers(0, 65536, (6, 8)).astype(np.uint16)
    d16[0, :2] = 0, 65535
    Image.fromarray(d16).save(tmp_path / "depth.png")
    K = np.array([[577.0, 0, 319.5], [0, 577.0, 239.5], [0, 0, 1]])
    with open(tmp_path / "ann.pkl", "wb") as f:
        pickle.dump({"plane_masks": rng.random((3, 6, 8)) < 0.5, "camera_K": K}, f)
    got = read_scannet_view(str(tmp_path / "ann.pkl"), str(tmp_path / "depth.png"))
    assert got["depth"].dtype == np.uint16 and np.array_equal(got["depth"], d16)             # millimetres, unconverted
    assert got["plane_masks"].dtype == np.uint8 and got["plane_masks"].shape == (3, 6, 8) and np.array_equal(got["camera_K"], K)
    Image.fromarray(np.zeros((6, 8), np.uint8)).save(tmp_path / "d8.png")
    with pytest.raises(ValueError, match="16-bit"):
        read_scannet_view(str(tmp_path / "ann.pkl"), str(tmp_path / "d8.png"))


def _annos(k, seg=None):
    return [dict({"plane": [0.1 * j, 1.0, 2.0], "category_id": 0}, **({"segmentation": seg} if seg is not None else {})) for j in range(k)]


def _restated_label_ids(labels, nmax_limit=50, out=None):
    """ops.label_ids on the host: the numpy restatement behind the wrapper's interface"""
    from nopesac_amd import ops
    res = [torch.from_numpy(a) for a in F.label_ids(labels.numpy(), ops.LABEL_MAX_IDS, nmax_limit)]
    for dst, src in zip(out or (), res):
        if dst is not None:
            dst.copy_(src)
    return res


def test_every_value_error(monkeypatch):
    from nopesac_amd import ops
    from nopesac_amd.targets import TargetMapper, inverse_intrinsics
    monkeypatch.setattr(ops, "label_ids", _restated_label_ids)
    tm = TargetMapper("cpu")
    H, W = 16, 16
    sem = F.partition(H, W, [3, 5, 9], 1)
    depth = np.ones((H, W), np.float32)
    ok = {"image_id": "house_7", "semantic_map": sem, "depth": depth, "annotations": _annos(3)}

    def fails(records, *words):
        with pytest.raises(ValueError) as e:
            tm.view_targets(records)
        assert all(w in str(e.value) for w in words), (words, str(e.value))
    fails([], "no record")
    # the three the issue names, on the label route, each naming the view
    fails([ok, dict(ok, image_id="house_8", annotations=_annos(2))], "view 1 (house_8)", "3 planes", "2 annotations")
    fails([dict(ok, semantic_map=np.zeros((H, W), np.int32), annotations=[])], "view 0 (house_7)", "no plane")
    many = (np.arange(40 * 40) % (ops.LABEL_MAX_IDS + 1) + 1).astype(np.int32).reshape(40, 40)
    fails([dict(ok, semantic_map=many, depth=np.ones((40, 40), np.float32))], "view 0 (house_7)", "distinct labels")
    # crowd annotations do not count, as in the reference's mapper
    fails([dict(ok, annotations=_annos(3) + [dict(_annos(1)[0], iscrowd=1)]), dict(ok, annotations=_annos(4))], "view 1", "4 annotations")
    # the other routes: the same two checks before anything is uploaded
    pm = np.zeros((2, H, W), np.uint8)
    fails([{"plane_masks": pm, "depth": depth, "annotations": _annos(3)}], "view 0", "2 planes", "3 annotations")
    fails([{"plane_masks": pm[:0], "depth": depth, "annotations": []}], "view 0", "no plane")
    fails([{"plane_masks": np.zeros((2, H, W + 1), np.uint8), "depth": depth, "annotations": _annos(2)}], "plane_masks")
    fails([{"depth": depth, "annotations": _annos(2, [[0.0, 0.0, 4.0, 0.0, 4.0, 4.0]])[:1] + _annos(1)}], "without a segmentation")
    # the record itself
    fails([dict(ok, plane_masks=pm)], "exactly one")
    fails([{"depth": depth, "annotations": _annos(2)}], "no ground-truth masks")
    fails([ok, {"plane_masks": pm, "depth": depth, "annotations": _annos(2)}], "one kind")
    fails([{k: v for k, v in ok.items() if k != "depth"}], "no depth")
    fails([ok, dict(ok, depth=np.ones((H, W), np.uint16))], "uint16")
    fails([dict(ok, depth=np.ones((H, W + 2), np.float32))], "semantic_map")
    with pytest.raises(ValueError, match="3 x 3"):
        inverse_intrinsics(np.eye(4))
    with pytest.raises(ValueError, match="max_targets"):
        TargetMapper("cpu", max_targets=51)


def test_launchers_refuse_bad_arguments_without_a_device():
    L = _lib()
    lib, E, H = L.load(), L.H.NPS_E_ARG, L.H
    err = lambda: lib.nopesac_last_error().decode()
    P = 4096                                                   # never dereferenced: the checks come before any HIP call
    assert lib.nopesac_label_ids(None, 1, 8, 8, 50, P, P, P, P, None) == E and "label_ids" in err() and "null input" in err()
    assert lib.nopesac_label_ids(P, 1, 8, 8, 50, P, None, P, P, None) == E and "null output" in err()
    assert lib.nopesac_label_ids(P, 0, 8, 8, 50, P, P, P, P, None) == E and "bad dims" in err()
    assert lib.nopesac_label_ids(P, 1, 8, 0, 50, P, P, P, P, None) == E and "bad dims" in err()
    assert lib.nopesac_label_ids(P, 1, 1 << 16, 1 << 16, 50, P, P, P, P, None) == E and "bad dims" in err()
    assert lib.nopesac_label_ids(P, 1, 8, 8, 0, P, P, P, P, None) == E and "nmax_limit" in err()
    assert lib.nopesac_label_ids(P, 1, 8, 8, H.NPS_LABEL_MAX_IDS + 1, P, P, P, P, None) == E and "nmax_limit" in err()
    assert lib.nopesac_label_ids(P + 2, 1, 8, 8, 50, P, P, P, P, None) == E and "aligned" in err()
    from nopesac_amd import ops
    need = ops.label_targets_workspace_bytes(2, 50, 480, 640)
    assert need == 2 * 75 * 50 * 3 * 4 and ops.label_targets_workspace_bytes(0, 50, 480, 640) == 0
    assert ops.label_targets_workspace_bytes(2, 50, 1, 1) == 2 * 50 * 3 * 4
    assert lib.nopesac_label_targets_workspace_bytes(2, 50, 480, 640, None) == E and "null result" in err()
    lt = lambda **o: lib.nopesac_label_targets(*[o.get(k, d) for k, d in (("labels", P), ("ids", P), ("n", P), ("B", 2), ("nmax", 50), ("H", 480), ("W", 640),
                                                                            ("masks", P), ("centers", P), ("pixel", P), ("ws", P), ("ws_bytes", need), ("stream", None))])
    assert lt(ids=None) == E and "label_targets" in err() and "null input" in err()
    assert lt(pixel=None) == E and "null output" in err()
    assert lt(nmax=0) == E and "nmax" in err()
    assert lt(nmax=51) == E and "nmax" in err()
    assert lt(B=70000) == E and "bad dims" in err()
    assert lt(ws_bytes=need - 1) == E and "workspace" in err()
    assert lt(ws=None) == E and "workspace" in err()
    assert lt(labels=P + 1) == E and "aligned" in err()
    assert lib.nopesac_bits_to_masks(None, 3, P, 1, 5, 8, 8, P, None) == E and "bits_to_masks" in err() and "null input" in err()
    assert lib.nopesac_bits_to_masks(P, 3, None, 1, 5, 8, 8, P, None) == E and "null input" in err()
    assert lib.nopesac_bits_to_masks(P, -1, P, 1, 5, 8, 8, P, None) == E and "null input" in err()
    assert lib.nopesac_bits_to_masks(P, 3, P, 1, 5, 8, 8, None, None) == E and "null output" in err()
    assert lib.nopesac_bits_to_masks(P, 3, P, 1, 51, 8, 8, P, None) == E and "nmax" in err()
    assert lib.nopesac_bits_to_masks(P, 3, P, 1, 5, 0, 8, P, None) == E and "bad dims" in err()
    assert lib.nopesac_depth_u16_to_f32(None, 8, 1000.0, P, None) == E and "depth_u16_to_f32" in err() and "null input" in err()
    assert lib.nopesac_depth_u16_to_f32(P, 8, 1000.0, None, None) == E and "null output" in err()
    assert lib.nopesac_depth_u16_to_f32(P, 0, 1000.0, P, None) == E and "n=0" in err()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.nopesac_depth_u16_to_f32(P, 8, scale, P, None) == E and "scale" in err()
    assert lib.nopesac_depth_u16_to_f32(P + 1, 8, 1000.0, P, None) == E and "aligned" in err()
    assert lib.nopesac_coordinate_map(None, 1, 8, 8, P, None) == E and "coordinate_map" in err() and "null input" in err()
    assert lib.nopesac_coordinate_map(P, 1, 8, 8, None, None) == E and "null output" in err()
    assert lib.nopesac_coordinate_map(P, 1, 8, -3, P, None) == E and "bad dims" in err()
    assert lib.nopesac_coordinate_map(P, 1, 8, 8, P + 2, None) == E and "aligned" in err()
    # the wrappers refuse host tensors before the library is asked
    with pytest.raises(ops.OpsArgumentError):
        ops.label_ids(torch.zeros(1, 4, 4, dtype=torch.int32))
    with pytest.raises(ops.OpsArgumentError):
        ops.depth_from_u16(torch.zeros(4, 4, dtype=torch.float32))
