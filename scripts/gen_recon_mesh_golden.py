"""Pin the reconstruction meshes to the reference: run the reference's own functions (vis_NopeSAC.py save_pair_objects on its dense
route) on the seeded cases of tests/recon_mesh_inputs.py and write tests/golden/K_recon_mesh_<seed>.npz.  CPU only.  Compiled from the
reference tree with oracle.ref_shim.load_reference_function, each on its own because their modules import numpy-quaternion,
pytorch3d, cv2 and imageio: merge_plane_params_from_local_params and merge_plane_params_from_global_params (vis_NopeSAC.py),
get_plane_params_in_global, get_plane_params_in_local and transform_meshes (utils/mesh_utils.py), get_pcd (utils/vis.py); and, with the
small AST step below, the dense branch of get_single_image_mesh (utils/vis.py: the `else` of `if reduce_size`), wrapped into a function
of one instance.  Their namespace gets numpy with np.quaternion, scipy.linalg.eigh, a quaternion stand-in (from_float_array,
as_rotation_matrix = q v q^-1 by Hamilton products, inverse), a Meshes stand-in that carries lists of tensors, a polygons_to_bitmask
that hands back the mask it is given, and get_pcd with K bound (the dense branch calls it without K, which drops into pdb).

What is run how:
  * the planes go in as float64 (a pair without correspondences would otherwise take |p| and p / |p| in float32, the dtype of the
    prediction: the port computes them in float64 throughout);
  * stride s: the reference has none, so its dense branch runs on m[::s, ::s] with K' = diag(1 / s, 1 / s, 1) K (pixel coordinates
    multiplied back by s inside K'^-1) and height, width = H / s, W / s for the texture coordinates; the fixture sizes divide by s;
  * the vertex lists are cast to float32 and transform_meshes works in float32, as in the reference;
  * webvis stays off (that branch is broken in the reference);
  * a pair with a `negdot` correspondence is left out: the reference's sign is a rounding accident there and the port defines the
    case (tests/recon_mesh_ref.py states the rule; the GPU tests check the kernels against it).
What cannot be run this way: the Textures / Meshes packing around the dense branch (pytorch3d) and save_obj's file writing (imageio,
cv2); tests/recon_mesh_ref.py and the tests of write_obj's layout alone stand for them.

RESULTS ONLY (the inputs are regenerated from their seeds), per kept pair i of the seed and stride s in STRIDES:
  planes_<i> [n, 3] float64            merge_plane_params_from_local_params, view 0's planes then view 1's
  vert_off_<i>_<s>, face_off_<i>_<s>   int64 [n + 1], faces_<i>_<s> int32 [F, 3] (ids local to the instance)
  local_<i>_<s> float64 [V, 3]         get_pcd;  verts_<i>_<s> float32 [V, 3] transform_meshes;  uvs_<i>_<s> float32 [V, 2]
  pairs int64 [k]                      the indices of the kept pairs in the seed's case
  gap_planes, gap_local, gap_verts, gap_uvs
                                       the largest absolute gap between the reference's value and tests/recon_mesh_ref.py on the same
                                       inputs - the tests derive their tolerances from them (4 x the gap)
Counts, offsets and faces must equal the restatement's exactly (asserted).
Needs the reference tree (NOPESAC_REFERENCE_ROOT); nothing of the reference's text is committed.  Not imported by any test."""
import ast
import os
import sys
from collections import defaultdict

import numpy as np
import torch
from scipy.linalg import eigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import recon_mesh_inputs as MI  # noqa: E402
from tests import recon_mesh_ref as REF  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STRIDES = (1, 2)


class Quat:
    def __init__(self, w, x, y, z):
        self.c = (float(w), float(x), float(y), float(z))

    def __mul__(self, o):
        a, b, c, d = self.c
        e, f, g, h = o.c
        return Quat(a * e - b * f - c * g - d * h, a * f + b * e + c * h - d * g, a * g - b * h + c * e + d * f, a * h + b * g - c * f + d * e)

    def inverse(self):
        w, x, y, z = self.c
        n = w * w + x * x + y * y + z * z
        return Quat(w / n, -x / n, -y / n, -z / n)


def as_rotation_matrix(q):
    """Columns q e_k q^-1."""
    inv = q.inverse()
    return np.array([(q * Quat(0, *e) * inv).c[1:] for e in np.eye(3)], np.float64).T


class NumpyWithQuaternion:
    quaternion = Quat

    def __getattr__(self, name):
        return getattr(np, name)


class Meshes:
    """What transform_meshes touches of pytorch3d's Meshes."""

    def __init__(self, verts, faces, textures=None):
        self._verts, self._faces, self.textures = list(verts), list(faces), textures

    def verts_packed(self):
        return torch.cat(self._verts) if self._verts else torch.zeros((0, 3))

    def verts_list(self):
        return self._verts

    def faces_list(self):
        return self._faces

    def num_verts_per_mesh(self):
        return torch.tensor([len(v) for v in self._verts], dtype=torch.int64)


def load_dense_branch(namespace):
    """The `else` of `if reduce_size` in get_single_image_mesh's loop as dense(segm, normal, offset, height, width, webvis,
    verts_3d, faces, uvs) -> (verts_3d, faces, uvs), compiled in `namespace`."""
    path = os.path.join(ref_shim.REFERENCE_ROOT, "NopeSAC_Net/utils/vis.py")
    tree = ast.parse(open(path).read(), filename=path)
    (fn,) = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_single_image_mesh"]
    branches = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Name) and n.test.id == "reduce_size"]
    assert len(branches) == 1 and branches[0].orelse
    shell = ast.parse("def dense(segm, normal, offset, height, width, webvis, verts_3d, faces, uvs):\n    pass\n    return verts_3d, faces, uvs\n")
    shell.body[0].body[0:1] = branches[0].orelse
    exec(compile(ast.fix_missing_locations(shell), path, "exec"), namespace)
    return namespace["dense"]


def reference_functions():
    quaternion = type("quaternion", (), {"from_float_array": staticmethod(lambda a: Quat(*np.asarray(a, np.float64).reshape(4))),
                                         "as_rotation_matrix": staticmethod(as_rotation_matrix)})
    ns = {"np": NumpyWithQuaternion(), "quaternion": quaternion, "eigh": eigh, "torch": torch, "Meshes": Meshes, "defaultdict": defaultdict,
          "polygons_to_bitmask": lambda segm, height, width: segm}
    for name in ("get_plane_params_in_global", "get_plane_params_in_local", "transform_meshes"):
        ref_shim.load_reference_function("NopeSAC_Net/utils/mesh_utils.py", name, ns)
    for name in ("merge_plane_params_from_global_params", "merge_plane_params_from_local_params"):
        ref_shim.load_reference_function("vis_NopeSAC.py", name, ns)
    ns["reference_get_pcd"] = ref_shim.load_reference_function("NopeSAC_Net/utils/vis.py", "get_pcd", {"np": np})
    load_dense_branch(ns)
    return ns


def reference_pair(ns, pair, stride):
    """The reference's functions on one pair -> the dict tests/recon_mesh_ref.pair_mesh returns (verts and uvs float32)."""
    planes = {v: np.asarray(pair["views"][int(v)]["planes"], np.float32).astype(np.float64) for v in "01"}
    camera = {"position": np.asarray(pair["camera"]["position"], np.float64), "rotation": Quat(*pair["camera"]["rotation"])}
    identity = {"position": np.array([0, 0, 0]), "rotation": Quat(1, 0, 0, 0)}
    corrs = [list(c) for c in pair["corrs"].tolist()]
    if len(corrs) != 0:                                              # (save_pair_objects merges only then)
        planes = ns["merge_plane_params_from_local_params"](planes, corrs, camera)
    out = {k: [] for k in ("verts", "local", "uvs", "faces", "view_of_instance", "planes")}
    vert_off, face_off = [0], [0]
    for v, cam in zip("01", (camera, identity)):
        masks = pair["views"][int(v)]["masks"]
        H, W = masks.shape[1:]
        K = REF.default_K(H, W) if pair["K"] is None else np.asarray(pair["K"], np.float64)
        K_s = np.diag([1.0 / stride, 1.0 / stride, 1.0]) @ K
        ns["get_pcd"] = lambda verts, normal, offset, K_s=K_s: ns["reference_get_pcd"](verts, normal, offset, K=K_s)
        p = np.array(planes[v])
        offsets = np.linalg.norm(p, ord=2, axis=1)                   # (the head of get_single_image_mesh)
        norms = p / offsets.reshape(-1, 1)
        verts_list, faces_list = [], []
        for mask, normal, offset in zip(masks, norms, offsets):
            verts_3d, faces, uvs = ns["dense"](mask[::stride, ::stride], normal, offset, H / stride, W / stride, False, [], [], [])
            out["local"].append(np.asarray(verts_3d, np.float64).reshape(-1, 3))
            verts_list.append(torch.tensor(np.asarray(verts_3d).reshape(-1, 3), dtype=torch.float32))
            faces_list.append(np.asarray(faces, np.int64).reshape(-1, 3))
            out["uvs"].append(torch.tensor(np.asarray(uvs).reshape(-1, 2), dtype=torch.float32).numpy())
            out["view_of_instance"].append(int(v))
            vert_off.append(vert_off[-1] + len(verts_list[-1])); face_off.append(face_off[-1] + len(faces_list[-1]))
        if verts_list:
            moved = ns["transform_meshes"](Meshes(verts_list, faces_list), cam)
            out["verts"] += [t.numpy() for t in moved.verts_list()]
        out["faces"] += faces_list
        out["planes"].append(p.reshape(-1, 3))
    cat = lambda parts, cols, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros((0, cols), dtype)      # noqa: E731
    return {"verts": cat(out["verts"], 3, np.float32), "local": cat(out["local"], 3, np.float64), "uvs": cat(out["uvs"], 2, np.float32),
            "faces": cat(out["faces"], 3, np.int32), "vert_off": np.asarray(vert_off, np.int64), "face_off": np.asarray(face_off, np.int64),
            "view_of_instance": np.asarray(out["view_of_instance"], np.int32), "planes": np.concatenate(out["planes"])}


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not found at %s" % ref_shim.REFERENCE_ROOT)
    os.makedirs(GOLD, exist_ok=True)
    ns = reference_functions()
    for seed in MI.SEEDS:
        case = MI.recon_mesh_case(seed)
        kept = [i for i, p in enumerate(case) if p["negdot"] is None]
        out, gaps = {"pairs": np.asarray(kept, np.int64)}, {k: 0.0 for k in ("planes", "local", "verts", "uvs")}
        for i in kept:
            for s in STRIDES:
                ref, mine = reference_pair(ns, case[i], s), REF.pair_mesh(case[i], s)
                for k in ("vert_off", "face_off", "faces", "view_of_instance"):
                    assert np.array_equal(ref[k], mine[k]), f"seed {seed} pair {i} stride {s}: {k} differs from the restatement: it, or the reading of the reference, is wrong"
                for k in gaps:
                    if ref[k].size:
                        gaps[k] = max(gaps[k], float(np.abs(ref[k].astype(np.float64) - mine[k]).max()))
                out[f"planes_{i}"] = ref["planes"]
                out.update({f"{k}_{i}_{s}": ref[k] for k in ("vert_off", "face_off", "faces", "local", "verts", "uvs")})
        out.update({f"gap_{k}": np.float64(g) for k, g in gaps.items()})
        path = os.path.join(GOLD, f"K_recon_mesh_{seed}.npz")
        np.savez_compressed(path, **out)
        print(f"seed {seed}: pairs {kept}, {os.path.getsize(path)} bytes; gaps " + " ".join(f"{k} {g:.3g}" for k, g in gaps.items()))


if __name__ == "__main__":
    main()
