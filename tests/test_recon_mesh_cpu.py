"""The reconstruction meshes without a GPU: tests/recon_mesh_ref.py against what the reference's own functions produced on the
fixture seeds (tests/golden/K_recon_mesh_*.npz, scripts/gen_recon_mesh_golden.py) - faces and counts equal, float values within 4 x the
gap the fixture records (the gap is the measurement against the reference; the factor covers another summation order) - the case
generator, write_obj's text on a hand-made mesh, the C surface of csrc/recon_mesh.hip and the checks made before any device work."""
import os

import numpy as np
import pytest
import torch

from tests import recon_mesh_inputs as MI
from tests import recon_mesh_ref as REF

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY_POINTS = ("nopesac_recon_mesh_merge", "nopesac_recon_mesh_count", "nopesac_recon_mesh_fill")


@pytest.mark.parametrize("seed", MI.SEEDS)
def test_restatement_against_the_reference(seed):
    g = np.load(os.path.join(GOLD, f"K_recon_mesh_{seed}.npz"))
    case = MI.recon_mesh_case(seed)
    kept = g["pairs"].tolist()
    assert kept == [i for i, p in enumerate(case) if p["negdot"] is None] and kept
    strides = sorted({int(k.rsplit("_", 1)[1]) for k in g.files if k.startswith("faces_")})
    assert strides == [1, 2]
    for i in kept:
        for s in strides:
            mine = REF.pair_mesh(case[i], s)
            for k in ("vert_off", "face_off", "faces"):
                assert np.array_equal(mine[k], g[f"{k}_{i}_{s}"]), (i, s, k)
            for k in ("local", "verts", "uvs"):
                want, gap = g[f"{k}_{i}_{s}"].astype(np.float64), float(g[f"gap_{k}"])
                assert mine[k].shape == want.shape
                if want.size:
                    err = float(np.abs(mine[k] - want).max())
                    print(f"seed {seed} pair {i} stride {s} {k}: {err:.3g} (recorded gap {gap:.3g})")
                    assert err <= 4 * gap, (i, s, k, err, gap)
            assert np.abs(mine["planes"] - g[f"planes_{i}"]).max(initial=0.0) <= 4 * float(g["gap_planes"])


def test_generator_terminates_and_keeps_its_conditions():
    for seed in MI.SEEDS:
        for h, w in ((24, 32), (48, 64)):
            case = MI.recon_mesh_case(seed, h, w)
            assert len(case) == len(MI.PLAN[seed])
            for p, kw in zip(case, MI.PLAN[seed]):
                assert MI.conditions_ok(p) and REF.check_corrs(kw["n"][0], kw["n"][1], p["corrs"])
                assert [len(v["planes"]) for v in p["views"]] == list(kw["n"]) and len(p["corrs"]) == kw["ncorr"]
                assert (p["negdot"] is not None) == bool(kw.get("negdot")) and (p["K"] is not None) == bool(kw.get("K"))
                for corr, d in zip(p["corrs"].tolist(), MI.matched_dots(p)):
                    assert d <= -MI.NEG_DOT if corr == p["negdot"] else d >= MI.DOT_MARGIN


def test_array_route_of_the_restatement_equals_the_loops():
    """instance_mesh_arrays (what the GPU test at 480 x 640 compares with) against the loops: integers equal, floats to rounding."""
    for seed in MI.SEEDS:
        for p in MI.recon_mesh_case(seed):
            for s in (1, 2, 3):
                a, b = REF.pair_mesh(p, s), REF.pair_mesh(p, s, instance=REF.instance_mesh_arrays)
                assert all(np.array_equal(a[k], b[k]) for k in ("faces", "vert_off", "face_off", "uvs"))
                assert all(np.abs(a[k] - b[k]).max(initial=0.0) <= 1e-13 for k in ("verts", "local"))


def test_negative_dot_rule_of_the_restatement():
    """n0 . n1 < 0: the eigenvector oriented like n0 - n1; n0 . n1 >= 0: like n0 + n1."""
    n0, n1 = np.array([0.0, 0.6, 0.8]), np.array([0.0, 0.6, -0.8])
    assert np.allclose(REF.merged_normal(n0, n1), [0.0, 0.0, 1.0]) and np.allclose(REF.merged_normal(n1, n0), [0.0, 0.0, -1.0])
    n1 = np.array([0.6, 0.0, 0.8])
    assert np.allclose(REF.merged_normal(n0, n1), (n0 + n1) / np.linalg.norm(n0 + n1))


def _hand_mesh():
    from nopesac_amd.mesh import PairMesh
    t = torch.tensor
    verts = t([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 1.0], [0.5, -2.0, 3.25], [-1.0, 2.0, 3.0], [0.125, 0.0, 1e-4]])
    uvs = t([[0.0, 1.0], [0.5, 1.0], [0.5, 0.5], [0.0, 0.5], [0.25, 0.75], [1.0, 0.0], [1.0 / 3.0, 0.5]])
    faces = t([[0, 2, 1], [0, 3, 2], [0, 1, 2]], dtype=torch.int32)
    return PairMesh(verts, uvs, faces, t([0, 4, 7]), t([0, 2, 3]), t([0, 1], dtype=torch.int32), torch.zeros(2, 3, dtype=torch.float64),
                    torch.zeros(2, dtype=torch.int32), (2, 2), 1)


@pytest.mark.parametrize("double_sided", (True, False))
def test_write_obj_layout(tmp_path, double_sided):
    from nopesac_amd.mesh import write_obj
    mesh = _hand_mesh()
    obj, mtl = write_obj(str(tmp_path), "pair", mesh, ["images/a.png", "b.jpg"], double_sided=double_sided)
    lines = open(obj).read().split("\n")
    assert lines[0] == "mtllib pair.mtl" and lines[1] == "" and lines[-1] == ""
    body = lines[2:-1]
    heads = [k for k, line in enumerate(body) if line.startswith("# mesh")]
    assert [body[k] for k in heads] == ["# mesh 0", "# mesh 1"]
    n_seen = 0
    for inst, (v0, v1, f0, f1) in enumerate(((0, 4, 0, 2), (4, 7, 2, 3))):
        block = body[heads[inst] + 1:heads[inst + 1] if inst + 1 < len(heads) else len(body)]
        nv, nf = v1 - v0, f1 - f0
        kinds = [line.split(" ")[0] for line in block]
        assert kinds == ["v"] * nv + ["vt"] * nv + ["usemtl"] + ["f"] * (nf * (2 if double_sided else 1))
        for row, line in zip(mesh.verts[v0:v1].tolist(), block[:nv]):
            assert line == "v " + " ".join("%.10f" % x for x in row)
        for row, line in zip(mesh.uvs[v0:v1].tolist(), block[nv:2 * nv]):
            assert line == "vt " + " ".join("%.10f" % x for x in row)
        assert block[2 * nv] == f"usemtl pair_view{inst}"
        f_lines = block[2 * nv + 1:]
        for k, face in enumerate(mesh.faces[f0:f1].tolist()):
            ids = [x + v0 + 1 for x in face]                          # 1-based, into the whole file
            fwd = "f " + " ".join(f"{x}/{x}" for x in ids)
            rev = "f " + " ".join(f"{x}/{x}" for x in reversed(ids))
            if double_sided:
                assert f_lines[2 * k:2 * k + 2] == [fwd, rev]
            else:
                assert f_lines[k] == fwd
        n_seen += nv
    assert n_seen == 7
    text = open(mtl).read()
    assert text.count("newmtl ") == 2 and "newmtl pair_view0\nmap_Kd images/a.png\n" in text and "newmtl pair_view1\nmap_Kd b.jpg\n" in text
    with pytest.raises(ValueError, match="image_files"):
        write_obj(str(tmp_path), "pair", mesh, ["a.png"])
    mesh.bad[1] = 1
    with pytest.raises(RuntimeError, match=r"instance\(s\) \[1\]"):
        write_obj(str(tmp_path), "pair", mesh, ["a.png", "b.png"])


def test_c_surface_of_the_mesh_kernels():
    """Every new entry point is declared nps_status, bound with the types the header states, exported by the library, and reports
    argument errors - null pointers, negative sizes, stride < 1, a mask over the LDS bound - before any device call; P = 0 / n = 0 are
    valid calls that enqueue nothing."""
    from ctypes import c_int, c_int64, c_void_p
    from nopesac_amd import _lib, ops
    lib = _lib.load()
    p, i, l = c_void_p, c_int, c_int64
    want = {"nopesac_recon_mesh_merge": [p] * 5 + [i, i, l, p, p, p],
            "nopesac_recon_mesh_count": [p, i, i, i, i, p, p, p],
            "nopesac_recon_mesh_fill": [p, i, i, i, i, p, p, i, p, p, p, p, l, l, p, p, p, p, p]}
    for name in ENTRY_POINTS:
        assert name in _lib.declared_symbols() and name in _lib.STATUS and _lib.RESTYPES[name] is c_int and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == want[name], name
    assert _lib.H.NPS_MESH_LDS_WORDS == ops.MESH_LDS_WORDS and 4 * ops.MESH_LDS_WORDS <= 64 * 1024
    assert ops.mesh_lds_words(480, 640, 1) == 11042 <= ops.MESH_LDS_WORDS
    err = lib.nopesac_last_error
    N5, N3 = [None] * 5, [None] * 3
    assert lib.nopesac_recon_mesh_merge(*N5, 0, 4, 0, *N3) == 0
    assert lib.nopesac_recon_mesh_merge(*N5, -1, 4, 0, *N3) == -1 and b"P < 0" in err()
    assert lib.nopesac_recon_mesh_merge(*N5, 1, 4, -1, *N3) == -1 and b"total < 0" in err()
    assert lib.nopesac_recon_mesh_merge(*N5, 1, 129, 0, *N3) == -1 and b"at most 128 planes" in err()
    assert lib.nopesac_recon_mesh_merge(*N5, 1, 4, 0, *N3) == -1 and b"null pointer" in err()
    count = lambda n, H, W, s: lib.nopesac_recon_mesh_count(None, n, H, W, s, None, None, None)      # noqa: E731
    assert count(0, 480, 640, 1) == 0
    assert count(-1, 480, 640, 1) == -1 and b"n < 0" in err()
    assert count(1, 0, 640, 1) == -1 and b"H, W > 0" in err()
    assert count(1, 480, 640, 0) == -1 and b"stride >= 1" in err()
    assert count(1, 480, 640, -3) == -1 and b"stride >= 1" in err()
    assert count(1, 1024, 1024, 1) == -1 and b"NPS_MESH_LDS_WORDS" in err()
    assert count(0, 1024, 1024, 2) == 0                                   # the same mask fits at stride 2
    assert count(1, 480, 640, 1) == -1 and b"null pointer" in err()
    fill = lambda n, H, W, s, nv=0, nf=0, views=1: lib.nopesac_recon_mesh_fill(None, n, H, W, s, None, None, views, *[None] * 4, nv, nf, *[None] * 5)   # noqa: E731
    assert fill(0, 480, 640, 1) == 0
    assert fill(-1, 480, 640, 1) == -1 and b"n < 0" in err()
    assert fill(1, 480, 640, 0) == -1 and b"stride >= 1" in err()
    assert fill(1, 2048, 2048, 2) == -1 and b"NPS_MESH_LDS_WORDS" in err()
    assert fill(1, 480, 640, 1, nv=-1) == -1 and b"n_verts" in err()
    assert fill(1, 480, 640, 1, views=-1) == -1 and b"n_views" in err()
    assert fill(1, 480, 640, 1) == -1 and b"null pointer" in err()
    with pytest.raises(_lib.HipKernelError, match="stride >= 1"):
        _lib.C.nopesac_recon_mesh_count(None, 1, 4, 4, 0, None, None, None)


def test_wrappers_check_their_arguments_without_a_gpu():
    from nopesac_amd import ops
    bits = torch.zeros((1, 1), dtype=torch.int32)
    for call in (lambda s, H=4, W=4: ops.recon_mesh_count(bits, H, W, s),
                 lambda s, H=4, W=4: ops.recon_mesh_fill(bits, H, W, s, *[None] * 6, 0, 0)):
        with pytest.raises(ops.OpsArgumentError, match="stride >= 1"):
            call(0)
        with pytest.raises(ops.OpsArgumentError, match="NPS_MESH_LDS_WORDS"):
            call(1, 1024, 1024)
        with pytest.raises(ops.OpsArgumentError, match="H, W > 0"):
            call(1, 0, 4)
        with pytest.raises(ops.OpsArgumentError, match="no CPU path"):
            call(1)
    with pytest.raises(ops.OpsArgumentError, match="at most 128 planes"):
        ops.recon_mesh_merge(*[None] * 5, 129)
    with pytest.raises(ops.OpsArgumentError, match="no CPU path"):
        ops.recon_mesh_merge(torch.zeros(3), *[None] * 4, 1)


def test_pair_meshes_checks_before_any_device_work():
    from nopesac_amd import mesh
    view = lambda n_inst, n_planes: {"instances": [{"segmentation": {"size": [2, 2], "counts": [0, 4]}}] * n_inst,     # noqa: E731
                                     "pred_plane": np.ones((n_planes, 3), np.float32)}
    cam = {"position": [0.0, 0.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.0]}
    with pytest.raises(ValueError, match="1 instances but 2 pred_plane rows"):
        mesh.pair_meshes([{"views": (view(1, 1), view(1, 2)), "camera": cam, "corrs": []}], "cpu")
    with pytest.raises(ValueError, match="stride >= 1"):
        mesh.pair_meshes([{"views": (view(1, 1), view(1, 1)), "camera": cam, "corrs": []}], "cpu", stride=0)
    with pytest.raises(ValueError, match="at most 128 instances"):
        mesh.pair_meshes([{"views": (view(129, 129), view(0, 0)), "camera": cam, "corrs": []}], "cpu")
    assert mesh.pair_meshes([], "cpu") == []
    (m,) = mesh.pair_meshes([{"views": (view(0, 0), view(0, 0)), "camera": cam, "corrs": []}], "cpu")      # nothing for the device
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.vert_off.tolist() == [0] and m.view_of_instance.numel() == 0
    assert np.array_equal(mesh.default_K(480, 640), REF.default_K(480, 640))


def test_cli_flags_and_stub_export(tmp_path):
    from nopesac_amd import run
    args = run.default_argument_parser().parse_args([])
    assert (args.export_meshes, args.mesh_stride, args.mesh_limit) == ("", 4, 16)
    args = run.default_argument_parser().parse_args(["--export-meshes", "out", "--mesh-stride", "2", "--mesh-limit", "0"])
    assert (args.export_meshes, args.mesh_stride, args.mesh_limit) == ("out", 2, 0)
    # the stub model's records hold no instances: the exporter's plumbing runs without a device and writes a header-only pair of files
    res = run.main(["--eval-only", "--stub-model", "--synthetic-pairs", "3", "--export-meshes", str(tmp_path / "m"), "--mesh-limit", "2"])
    assert res["meshes"] == {"exported": 2, "stride": 4}
    names = sorted(os.listdir(tmp_path / "m"))
    assert len(names) == 4 and [n.rsplit(".", 1)[1] for n in names] == ["mtl", "obj"] * 2
    assert open(tmp_path / "m" / names[1]).read() == "mtllib " + names[0] + "\n\n"
    assert "meshes" not in run.main(["--eval-only", "--stub-model", "--synthetic-pairs", "1"])
