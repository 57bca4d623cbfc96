"""csrc/recon_mesh.hip and nopesac_amd/mesh.py on the GPU against tests/recon_mesh_ref.py (which tests/test_recon_mesh_cpu.py holds
against the reference's own functions).  Every comparison is the same:
  * counts, offsets, faces and view_of_instance exact;
  * uvs equal to the float32 rounding of the restatement's value;
  * vertices per component within 2^-22 (|camera position|_inf + |local vertex|_2): the result carries one float32 rounding, at most
    2^-24 relative to that scale, the two float64 routes differ by orders of magnitude less under the conditioning the cases keep
    (|n . ray| >= 0.2, offsets in [0.5, 6]) - a fourfold margin;
  * merged planes within 1e-9 absolute: eigh and the closed form differ by about 1e-16 / (2 DOT_MARGIN), the parameters are below 10.
Shapes are the smallest at which each mechanism can go wrong; one case runs at the real size, 480 x 640."""
import os

import numpy as np
import pytest
import torch

from oracle import rle_oracle as R
from tests import poly_reference as PR
from tests import recon_mesh_inputs as MI
from tests import recon_mesh_ref as REF
from tests.plane_eval_inputs import _rotate
from tests.recon_eval_inputs import FLIP, _camera, _local_in_view0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda")


def _host(mesh):
    return {k: getattr(mesh, k).cpu().numpy() for k in ("verts", "uvs", "faces", "vert_off", "face_off", "view_of_instance", "planes", "bad")}


def _compare(mesh, pair, stride, merge=True, instance=None):
    got, want = _host(mesh), REF.pair_mesh(pair, stride, merge, instance=instance)
    assert not got["bad"].any() and mesh.stride == stride
    for k in ("vert_off", "face_off", "faces", "view_of_instance"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["uvs"].dtype == np.float32 and np.array_equal(got["uvs"], want["uvs"].astype(np.float32))
    assert got["planes"].shape == want["planes"].shape
    plane_err = float(np.abs(got["planes"] - want["planes"]).max(initial=0.0))
    t = np.abs(np.asarray(pair["camera"]["position"], np.float64)).max()
    scale = np.where(np.repeat(want["view_of_instance"], np.diff(want["vert_off"])) == 0, t, 0.0) + np.sqrt((want["local"] ** 2).sum(1))
    ratio = float((np.abs(got["verts"].astype(np.float64) - want["verts"]).max(1) / scale).max(initial=0.0))
    print(f"stride {stride}: {len(want['verts'])} vertices, {len(want['faces'])} faces, vertex error {ratio * 2 ** 24:.3f} x 2^-24 of the scale, "
          f"plane error {plane_err:.3g}")
    assert got["verts"].dtype == np.float32 and ratio <= 2.0 ** -22
    assert plane_err <= 1e-9
    return got, want


def _meshes(pairs, device, stride=1, merge=True, **kw):
    from nopesac_amd import mesh
    return mesh.pair_meshes(MI.product_pairs(pairs), device, stride=stride, merge=merge, **kw)


@pytest.mark.parametrize("stride", (1, 2, 3))
@pytest.mark.parametrize("seed", MI.SEEDS)
def test_seeded_cases_at_every_stride(device, seed, stride):
    """24 x 36: neither H - 1 nor W - 1 is a multiple of 2 or 3.  The seeds cover K given and None, a non-unit quaternion, a view
    without instances, a pair without correspondences and the `negdot` rule."""
    pairs = MI.recon_mesh_case(seed, 24, 36)
    for m, p in zip(_meshes(pairs, device, stride), pairs):
        _compare(m, p, stride)


@pytest.mark.parametrize("seed", MI.SEEDS)
def test_seeded_blobs_48x64_merged_and_not(device, seed):
    pairs = MI.recon_mesh_case(seed, 48, 64)
    for merge in (True, False):
        for m, p in zip(_meshes(pairs, device, 1, merge), pairs):
            got, want = _compare(m, p, 1, merge)
            if not merge or len(p["corrs"]) == 0:                     # planes pass through, widened
                assert np.array_equal(got["planes"], np.concatenate([v["planes"] for v in p["views"]]).astype(np.float64))


def test_negdot_follows_the_stated_rule(device):
    """The merged normal of a correspondence with n0 . n1 < 0 points like n0 - n1: like view 0's plane, against view 1's."""
    pairs = [p for seed in (32, 33) for p in MI.recon_mesh_case(seed, 24, 36) if p["negdot"] is not None]
    assert len(pairs) == 2
    for m, p in zip(_meshes(pairs, device), pairs):
        got, _ = _compare(m, p, 1)
        a, b = p["negdot"]
        n0 = len(p["views"][0]["planes"])
        g0, g1 = REF.global_params(got["planes"][:n0], p["camera"]), REF.global_params(got["planes"][n0:], REF.IDENTITY)
        before0, before1 = REF.global_params(p["views"][0]["planes"], p["camera"]), REF.global_params(p["views"][1]["planes"], REF.IDENTITY)
        assert np.abs(g0[a] - g1[b]).max() <= 1e-9 and g0[a] @ before0[a] > 0 and g1[b] @ before1[b] < 0


@pytest.mark.parametrize("seed,qscale", ((41, 1.0), (42, 1.0), (43, 1.0), (44, 1.0), (41, 1.7)))
def test_merge_axis_aligned_planes_and_zero_components(device, seed, qscale):
    """Floors and walls seen from an upright camera: view 1's planes have components that are exactly zero (one of them -0.0), which
    no seeded case has; the identity view takes them without a rotation.  ops.recon_mesh_merge alone, no masks.  View 0's planes
    0..2 are view 1's seen from the camera, turned by 1 to 8 degrees (n0 . n1 >= 0.99, far from DOT_MARGIN) and shifted by at most 0.1."""
    from nopesac_amd import ops
    rng = np.random.default_rng(seed)
    cam = _camera(rng)
    p1 = np.array([[0, 0, 2], [1.5, 0, 0], [0, -2.5, 0], [0, 3, -0.0]], np.float32)
    p0 = []
    for k in range(3):
        p, _ = _local_in_view0(p1[k].astype(np.float64) * FLIP, cam)
        off = np.linalg.norm(p)
        p0.append(_rotate(p / off, rng.uniform(1.0, 8.0), rng) * (off + rng.uniform(-0.1, 0.1)))
    p0 = np.asarray(p0 + [[0.0, 0.0, 1.25]], np.float32)
    camera = {"position": cam["position"], "rotation": cam["rotation"] * qscale}
    corrs = np.array([[0, 0], [1, 1], [2, 2]], np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    merged, bad = ops.recon_mesh_merge(dev(np.concatenate([p0, p1])), dev(np.array([0, 4, 8], np.int64)),
                                       dev(np.concatenate([camera["position"], camera["rotation"]])[None]), dev(corrs.reshape(-1)),
                                       dev(np.array([0, 3], np.int64)), 4)
    assert bad.tolist() == [0]
    err = np.abs(merged.cpu().numpy() - np.concatenate(REF.merged_local_planes(p0, p1, camera, corrs))).max(1)
    print(f"seed {seed}, qscale {qscale}: merged planes within {err[[0, 1, 2, 4, 5, 6]].max():.3g}, unmatched within {err[[3, 7]].max():.3g}")
    assert err[[0, 1, 2, 4, 5, 6]].max() <= 1e-9                              # the merged planes, both views
    assert err[[3, 7]].max() <= 1e-9                                          # the unmatched ones come back


def _special_masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    blob = (yy - h / 2) ** 2 + (xx - w / 3) ** 2 < (h / 3) ** 2
    edge = (yy == h - 1) | (xx == w - 1)
    return [np.stack([blob, np.zeros((h, w), bool), (yy + xx) % 2 == 0]), np.stack([np.ones((h, w), bool), edge, ~blob])]


@pytest.mark.parametrize("stride", (1, 2, 3))
def test_special_masks_23x37(device, stride):
    """H W is no multiple of 32 (a partial last word).  An empty mask between two others, a checkerboard (every second pixel a vertex,
    no face), a full mask (every face), a mask that touches only the last row and the last column."""
    m0, m1 = _special_masks(23, 37)
    pair = MI.custom_pair(1, m0, m1, corrs=[(0, 2)], qscale=1.3)
    (mesh,) = _meshes([pair], device, stride)
    got, want = _compare(mesh, pair, stride)
    nv, nf = np.diff(got["vert_off"]), np.diff(got["face_off"])
    hs, ws = -(-23 // stride), -(-37 // stride)
    assert nv[1] == 0 and nf[1] == 0 and nv[3] == hs * ws and nf[3] == 2 * (hs - 1) * (ws - 1)
    if stride == 1:
        assert nv[2] == (23 * 37 + 1) // 2 and nf[2] == 0 and nv[4] == 23 + 37 - 1 and nf[4] == 0


@pytest.mark.parametrize("shape", ((1, 40), (40, 1)))
def test_single_row_and_single_column(device, shape):
    ones = np.ones((1,) + shape, bool)
    part = ones.copy()
    part.reshape(-1)[5:9] = False
    pair = MI.custom_pair(2, np.concatenate([ones, part]), part, K=np.array([[30.0, 0.0, shape[1] / 2], [0.0, 30.0, shape[0] / 2], [0.0, 0.0, 1.0]]))
    for stride in (1, 3):
        (mesh,) = _meshes([pair], device, stride)
        got, _ = _compare(mesh, pair, stride)
        assert got["faces"].shape == (0, 3) and got["vert_off"][-1] > 0


def test_the_most_instances_a_view_may_have(device):
    from nopesac_amd import ops
    n = ops.PLANE_MAX_QUERIES
    yy, xx = np.mgrid[0:12, 0:16]
    m0 = np.stack([((yy * 16 + xx) % n == k) | ((yy // 3 == k % 4) & (xx // 4 == k // 4 % 4)) for k in range(n)])
    m1 = np.stack([xx < 8, xx >= 8])
    pair = MI.custom_pair(3, m0, m1, corrs=[(n - 1, 1), (0, 0)])
    (mesh,) = _meshes([pair], device)
    got, _ = _compare(mesh, pair, 1)
    assert len(got["vert_off"]) == n + 3


def test_two_pairs_in_one_call_equal_two_single_calls(device):
    pairs = MI.recon_mesh_case(31, 24, 36)[:2] + MI.recon_mesh_case(33, 24, 36)[:1]
    together = _meshes(pairs, device, 2)
    for m, p in zip(together, pairs):
        (alone,) = _meshes([p], device, 2)
        a, b = _host(m), _host(alone)
        assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]


def test_bad_correspondences(device):
    """A correspondence that names a missing plane, or a plane twice: ValueError from pair_meshes; at the kernel the pair's flag is
    set, nothing of it is written, and the other pairs of the launch come out as they do alone."""
    from nopesac_amd import mesh, ops
    pairs = MI.recon_mesh_case(31, 24, 36)
    n = [len(v["planes"]) for v in pairs[1]["views"]]
    for bad_corrs in ([[0, n[1]]], [[-1, 0]], [[0, 0], [1, 0]], [[0, 1], [0, 0]]):
        broken = [pairs[0], {**pairs[1], "corrs": np.asarray(bad_corrs, np.int64)}, pairs[2]]
        assert not REF.check_corrs(n[0], n[1], bad_corrs)
        with pytest.raises(ValueError, match=r"pair\(s\) \[1\]"):
            mesh.pair_meshes(MI.product_pairs(broken), device)
        planes = np.concatenate([v["planes"] for p in broken for v in p["views"]]).astype(np.float32)
        counts = [len(v["planes"]) for p in broken for v in p["views"]]
        view_off, corr_off = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum([len(p["corrs"]) for p in broken])])
        cams = np.stack([np.concatenate([p["camera"]["position"], p["camera"]["rotation"]]) for p in broken])
        corr = np.concatenate([np.asarray(p["corrs"], np.int32).reshape(-1, 2) for p in broken]).reshape(-1)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
        merged, bad = ops.recon_mesh_merge(dev(planes), dev(view_off), dev(cams), dev(corr), dev(corr_off), max(counts))
        assert bad.tolist() == [0, 1, 0]
        merged = merged.cpu().numpy()
        assert not merged[view_off[2]:view_off[4]].any()                          # the wrapper's zeros
        for i in (0, 2):
            want = np.concatenate(REF.merged_local_planes(broken[i]["views"][0]["planes"], broken[i]["views"][1]["planes"], broken[i]["camera"],
                                                          broken[i]["corrs"]))
            assert np.abs(merged[view_off[2 * i]:view_off[2 * i + 2]] - want).max() <= 1e-9


def test_fill_refuses_offsets_that_disagree_with_the_counts(device):
    """An instance whose offset range is not its counted range sets its flag; its neighbour is filled as usual."""
    from nopesac_amd import ops
    pair = MI.custom_pair(4, np.ones((1, 8, 8), bool), np.ones((1, 8, 8), bool))
    from nopesac_amd import rle
    bits, _ = rle.decode_bits([R.encode(m) for v in pair["views"] for m in v["masks"]], device)
    nv, nf = ops.recon_mesh_count(bits, 8, 8, 1)
    assert nv.tolist() == [64, 64] and nf.tolist() == [98, 98]
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=device)      # noqa: E731
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)      # noqa: E731
    planes = f64(np.concatenate([v["planes"] for v in pair["views"]]))
    kinv = f64(np.tile(np.linalg.inv(REF.default_K(8, 8)).reshape(1, 9), (2, 1)))
    cams = f64(np.stack([np.concatenate([pair["camera"]["position"], pair["camera"]["rotation"]]), [0, 0, 0, 1, 0, 0, 0]]))
    view = torch.tensor([0, 1], dtype=torch.int32, device=device)
    verts, _, faces, bad = ops.recon_mesh_fill(bits, 8, 8, 1, planes, view, kinv, cams, i64([0, 63, 127]), i64([0, 98, 196]), 128, 196)
    assert bad.tolist() == [1, 0]                                             # 63 vertices claimed, 64 counted
    verts, _, faces, bad = ops.recon_mesh_fill(bits, 8, 8, 1, planes, view, kinv, cams, i64([0, 64, 128]), i64([0, 98, 200]), 128, 200)
    assert bad.tolist() == [0, 1]
    want = REF.pair_mesh(pair, 1)
    assert np.array_equal(faces[:98].cpu().numpy(), want["faces"][:98])
    view[1] = 2                                                               # a view the tables do not have
    assert ops.recon_mesh_fill(bits, 8, 8, 1, planes, view, kinv, cams, i64([0, 64, 128]), i64([0, 98, 196]), 128, 196)[3].tolist() == [0, 1]


def test_polygon_segmentations(device):
    from nopesac_amd import mesh
    h, w = 23, 37
    polys = [[[3.0, 2.0, 30.5, 4.0, 25.0, 20.0, 6.0, 18.5]], [[1.0, 1.0, 12.0, 1.0, 12.0, 9.0, 1.0, 9.0], [20.0, 10.0, 35.0, 12.0, 28.0, 22.0]]]
    dense = np.stack([PR.mask_dense(p, h, w) for p in polys])
    assert dense.any(axis=(1, 2)).all()
    pair = MI.custom_pair(6, dense[:1], dense[1:], corrs=[(0, 0)])
    product = MI.product_pairs([pair])
    product[0]["views"][0]["instances"][0]["segmentation"] = polys[0]             # a polygon list next to an RLE dict ...
    (m,) = mesh.pair_meshes(product, device, stride=2)
    _compare(m, pair, 2)
    product[0]["views"][1]["instances"][0]["segmentation"] = polys[1]             # ... and polygons only: the size comes with the call
    (m,) = mesh.pair_meshes(product, device, stride=1, size=(h, w))
    _compare(m, pair, 1)


def test_real_size_480x640(device):
    """One full mask and one blob at stride 1: 38400 bytes of mask in LDS, vertex offsets past 2^16 (307200 and more), 612162 faces of
    the full mask.  Compared with the whole-array route of the restatement."""
    yy, xx = np.mgrid[0:480, 0:640]
    blob = ((yy - 200) / 150.0) ** 2 + ((xx - 400) / 230.0) ** 2 < 1.0
    pair = MI.custom_pair(7, np.ones((1, 480, 640), bool), blob[None], corrs=[(0, 0)], qscale=0.8)
    (mesh,) = _meshes([pair], device)
    got, _ = _compare(mesh, pair, 1, instance=REF.instance_mesh_arrays)
    assert got["vert_off"].tolist()[1] == 480 * 640 and got["face_off"].tolist()[1] == 2 * 479 * 639 and got["vert_off"][2] > 400000


def _records(pairs):
    """Prediction records as PoseEvaluator keeps them, from a seeded case."""
    from nopesac_amd.evaluation import PoseEvaluator
    records = []
    for k, (p, q) in enumerate(zip(pairs, MI.product_pairs(pairs))):
        A = np.zeros((1, len(p["views"][0]["planes"]), len(p["views"][1]["planes"])), np.float32)
        for a, b in p["corrs"]:
            A[0, a, b] = 1
        inp = {v: {"image_id": f"m{k}v{v}", "file_name": f"m{k}v{v}.png"} for v in "01"}
        out = {v: {"instances": q["views"][int(v)]["instances"], "pred_plane": torch.from_numpy(p["views"][int(v)]["planes"].copy())} for v in "01"}
        out.update(camera={"tran": np.asarray(p["camera"]["position"], np.float32), "rot": np.asarray(p["camera"]["rotation"], np.float32)},
                   pred_assignment=torch.from_numpy(A))
        records.append((inp, out, PoseEvaluator.prediction_record(inp, out)))
    return records


def test_meshes_from_dump_and_exporter(device, tmp_path):
    """The records dump_predictions writes come back as the meshes pair_meshes builds from the same pairs (the dump keeps the camera
    in float32), through meshes_from_dump and through the MeshExporter; the stub model's records, which hold no instances, give empty
    meshes."""
    from nopesac_amd import mesh, run
    from nopesac_amd.evaluation import PoseEvaluator, dump_predictions
    pairs = [p for p in MI.recon_mesh_case(31, 24, 36) if p["K"] is None]
    for p in pairs:                                                               # the camera as the dump holds it
        p["camera"] = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in p["camera"].items()}
    records = _records(pairs)
    dump_predictions([r[2] for r in records], str(tmp_path / "dump"))
    meshes = mesh.meshes_from_dump(str(tmp_path / "dump"), device, stride=2)
    assert len(meshes) == len(pairs)
    for m, p in zip(meshes, pairs):
        _compare(m, p, 2)
    assert len(mesh.meshes_from_dump(str(tmp_path / "dump"), device, limit=1)) == 1
    exporter = mesh.MeshExporter(device, str(tmp_path / "obj"), stride=2, limit=1)
    exporter.process([r[0] for r in records], [r[1] for r in records])
    assert exporter.evaluate() == {"exported": 1, "stride": 2} and sorted(os.listdir(tmp_path / "obj")) == ["m0v0__m0v1.mtl", "m0v0__m0v1.obj"]
    n_v = int(_host(meshes[0])["vert_off"][-1])
    text = open(tmp_path / "obj" / "m0v0__m0v1.obj").read()
    assert text.count("\nv ") == n_v and "map_Kd m0v0.png" in open(tmp_path / "obj" / "m0v0__m0v1.mtl").read()
    stub, ev = run._StubModel(), PoseEvaluator(keep_predictions=True)
    batch = [run.synth_pair(i, 8, 8) for i in range(2)]
    ev.process(batch, stub(batch))
    dump_predictions(ev._predictions, str(tmp_path / "stub"))
    for m in mesh.meshes_from_dump(str(tmp_path / "stub"), device):
        assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.vert_off.tolist() == [0]


def test_meshes_from_gt(device):
    from nopesac_amd import mesh
    pair = MI.recon_mesh_case(31, 24, 36)[0]
    entry = {"gt_corrs": pair["corrs"].tolist(), "rel_pose": pair["camera"]}
    for v in "01":
        view = pair["views"][int(v)]
        entry[v] = {"height": 24, "width": 36, "annotations": [{"segmentation": R.encode(m), "plane": [float(x) for x in pl]}
                                                               for m, pl in zip(view["masks"], view["planes"])]}
    _compare(mesh.meshes_from_gt(entry, device, stride=3), pair, 3)


def test_write_obj_round_trip(device, tmp_path):
    from nopesac_amd import mesh
    pair = MI.recon_mesh_case(33, 24, 36)[0]
    (m,) = _meshes([pair], device, 2)
    got = _host(m)
    obj, mtl = mesh.write_obj(str(tmp_path), "p", m, ["a.png", "b.png"])
    lines = open(obj).read().split("\n")
    v = np.array([[float(x) for x in line.split()[1:]] for line in lines if line.startswith("v ")])
    vt = np.array([[float(x) for x in line.split()[1:]] for line in lines if line.startswith("vt ")])
    f = np.array([[int(tok.split("/")[0]) for tok in line.split()[1:]] for line in lines if line.startswith("f ")])
    assert all(a == b for line in lines if line.startswith("f ") for a, b in (tok.split("/") for tok in line.split()[1:]))
    assert v.shape == got["verts"].shape and np.abs(v - got["verts"]).max() <= 0.5e-10 and np.abs(vt - got["uvs"]).max() <= 0.5e-10
    base = np.repeat(got["vert_off"][:-1], np.diff(got["face_off"]))[:, None] + 1
    assert np.array_equal(f[0::2], got["faces"] + base) and np.array_equal(f[1::2], (got["faces"] + base)[:, ::-1])
    assert [line for line in lines if line.startswith("# mesh")] == [f"# mesh {k}" for k in range(len(got["view_of_instance"]))]
    assert [line for line in lines if line.startswith("usemtl")] == [f"usemtl p_view{k}" for k in got["view_of_instance"]]
    assert open(mtl).read().count("newmtl") == 2
