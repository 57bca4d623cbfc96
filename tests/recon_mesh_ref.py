"""Host restatement (numpy, float64, plain loops and dicts) of the two-view reconstruction meshes, written from their description -
the reference's vis_NopeSAC.py save_pair_objects on its dense route: merge_plane_params_from_local_params (get_plane_params_in_global,
merge_plane_params_from_global_params, get_plane_params_in_local), get_pcd, get_single_image_mesh(reduce_size=False) and the arithmetic
of transform_meshes.  The CPU tests hold it against what the reference functions themselves produced on the fixture seeds
(tests/golden/K_recon_mesh_*.npz); the GPU tests compare the kernels against it at shapes the fixture does not cover.  Nothing here is
shared with nopesac_amd.mesh, and the routes differ from the kernels' on purpose: a rotation MATRIX from the quaternion,
np.linalg.eigh for the merged normal, a dict for the vertex ids.

The one rule that is this project's and not the reference's: a correspondence with n0 . n1 < 0 (the reference's sign is a rounding
accident there) merges to the eigenvector oriented like n0 - n1, the orientation of view 0's plane."""
import math

import numpy as np

from tests.recon_eval_ref import IDENTITY, rotation_matrix

FLIP = np.array([1.0, -1.0, -1.0])
DEFAULT_FOCAL = 517.97


def default_K(H, W):
    return np.array([[DEFAULT_FOCAL, 0.0, W / 2], [0.0, DEFAULT_FOCAL, H / 2], [0.0, 0.0, 1.0]], np.float64)


def _camera(camera):
    t = np.asarray(camera["position"] if "position" in camera else camera["tran"], np.float64).reshape(3)
    q = np.asarray(camera["rotation"] if "rotation" in camera else camera["rot"], np.float64).reshape(4)
    return t, rotation_matrix(q)


def global_params(planes, camera):
    """get_plane_params_in_global: [n, 3] float64, the foot point of the origin on every plane in the common frame."""
    t, R = _camera(camera)
    out = np.zeros((len(planes), 3))
    for k, p in enumerate(np.asarray(planes, np.float64).reshape(-1, 3)):
        end = R @ (p * FLIP) + t
        b = end - t
        out[k] = (end @ b) / (math.sqrt(b @ b) ** 2) * b
    return out


def local_params(planes, camera):
    """get_plane_params_in_local: the planes of the common frame as the camera sees them."""
    t, R = _camera(camera)
    out = np.zeros((len(planes), 3))
    for k, b in enumerate(np.asarray(planes, np.float64).reshape(-1, 3)):
        world = t + b - (t @ b) / (math.sqrt(b @ b) ** 2) * b
        out[k] = (R.T @ (world - t)) * FLIP
    return out


def merged_normal(n0, n1):
    """The top eigenvector of n0 n0^T + n1 n1^T; its sign by n0 + n1 for n0 . n1 >= 0 (the reference's rule) and by n0 - n1 below."""
    pair = np.vstack([n0, n1])
    w, v = np.linalg.eigh(pair.T @ pair)
    avg = v[:, int(np.argmax(w))]
    toward = n0 + n1 if float(n0 @ n1) >= 0.0 else n0 - n1
    return -avg if float(avg @ toward) < 0.0 else avg


def merge_global(g0, g1, corrs):
    g0, g1 = np.array(g0, np.float64), np.array(g1, np.float64)
    off = [np.maximum(np.sqrt((g * g).sum(1)), 1e-5) for g in (g0, g1)]
    nrm = [g / o[:, None] for g, o in zip((g0, g1), off)]
    for a, b in corrs:
        plane = merged_normal(nrm[0][a], nrm[1][b]) * ((off[0][a] + off[1][b]) / 2)
        g0[a] = plane
        g1[b] = plane
    return g0, g1


def merged_local_planes(planes0, planes1, camera, corrs):
    """merge_plane_params_from_local_params -> (view 0's planes, view 1's) float64; without correspondences the planes as they are."""
    p0, p1 = (np.asarray(p, np.float32).reshape(-1, 3).astype(np.float64) for p in (planes0, planes1))
    corrs = [(int(a), int(b)) for a, b in np.asarray(corrs).reshape(-1, 2)]
    if not corrs:
        return p0, p1
    g0, g1 = merge_global(global_params(p0, camera), global_params(p1, IDENTITY), corrs)
    return local_params(g0, camera), local_params(g1, IDENTITY)


def check_corrs(n0, n1, corrs):
    corrs = [(int(a), int(b)) for a, b in np.asarray(corrs).reshape(-1, 2)]
    ok = all(0 <= a < n0 and 0 <= b < n1 for a, b in corrs)
    return ok and len({a for a, _ in corrs}) == len(corrs) and len({b for _, b in corrs}) == len(corrs)


def instance_mesh(mask, plane, K, stride=1):
    """The dense mesh of one instance in its view's frame -> (verts float64 [V, 3], uvs float64 [V, 2], faces int [F, 3])."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    m = mask[::stride, ::stride]
    hs, ws = m.shape
    K_inv = np.linalg.inv(np.asarray(K, np.float64))
    plane = np.asarray(plane, np.float64)
    offset = math.sqrt(plane @ plane)
    normal = plane / offset
    ids, verts, uvs = {}, [], []
    for y in range(hs):
        for x in range(ws):
            if m[y, x]:
                ids[(y, x)] = len(verts)
                ray = K_inv @ np.array([float(x * stride), float(y * stride), 1.0])
                verts.append(offset / (normal @ ray) * ray)
                uvs.append([x * stride / W, 1.0 - y * stride / H])
    faces = []
    for (y, x) in ids:                                   # insertion order = vertex order
        if y < hs - 1 and x < ws - 1:
            if m[y, x + 1] and m[y + 1, x + 1]:
                faces.append([ids[(y, x)], ids[(y + 1, x + 1)], ids[(y, x + 1)]])
            if m[y + 1, x] and m[y + 1, x + 1]:
                faces.append([ids[(y, x)], ids[(y + 1, x)], ids[(y + 1, x + 1)]])
    return np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(uvs, np.float64).reshape(-1, 2), np.asarray(faces, np.int64).reshape(-1, 3)


def instance_mesh_arrays(mask, plane, K, stride=1):
    """instance_mesh by whole-array numpy (ids from a running sum, faces by boolean selection in (y, x, upper / lower) order): the
    route for masks too large for the loops.  tests/test_recon_mesh_cpu.py holds it equal to instance_mesh."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    m = mask[::stride, ::stride]
    ys, xs = np.nonzero(m)
    ids = (np.cumsum(m.reshape(-1)) - 1).reshape(m.shape)
    plane = np.asarray(plane, np.float64)
    offset = math.sqrt(plane @ plane)
    ray = (np.linalg.inv(np.asarray(K, np.float64)) @ np.stack([xs * float(stride), ys * float(stride), np.ones(len(xs))])).T
    verts = (offset / (ray @ (plane / offset)))[:, None] * ray
    uvs = np.stack([xs * stride / W, 1.0 - ys * stride / H], 1)
    a, right, below, diag = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
    i_a, i_right, i_below, i_diag = ids[:-1, :-1], ids[:-1, 1:], ids[1:, :-1], ids[1:, 1:]
    tris = np.stack([np.stack([i_a, i_diag, i_right], -1), np.stack([i_a, i_below, i_diag], -1)], 2)      # [hs - 1, ws - 1, 2, 3]
    flags = np.stack([a & right & diag, a & below & diag], 2)
    return verts.reshape(-1, 3), uvs.reshape(-1, 2), tris[flags].astype(np.int64).reshape(-1, 3)


def to_common(verts, camera):
    """transform_meshes: flip y and z, rotate, shift."""
    t, R = _camera(camera)
    if len(verts) > 4096:                                # (the large masks: one product instead of a loop)
        return (R @ (np.asarray(verts, np.float64) * FLIP).T).T + t
    return np.asarray([R @ (v * FLIP) + t for v in verts], np.float64).reshape(-1, 3)


def pair_mesh(pair, stride=1, merge=True, instance=None):
    """pair: {"views": ({"masks" bool [n, H, W], "planes" f32 [n, 3]}, x 2), "camera", "corrs" [k, 2], "K" 3 x 3 or None} -> dict of
    verts (common frame), local (the same vertices in their view's frame), uvs, faces, vert_off, face_off, view_of_instance, planes.
    instance: instance_mesh (the default) or instance_mesh_arrays."""
    v0, v1 = pair["views"]
    corrs = np.asarray(pair["corrs"]).reshape(-1, 2) if merge else np.zeros((0, 2), np.int64)
    planes = merged_local_planes(v0["planes"], v1["planes"], pair["camera"], corrs)
    verts, local, uvs, faces, view_of, vert_off, face_off = [], [], [], [], [], [0], [0]
    for v, (view, cam) in enumerate(zip((v0, v1), (pair["camera"], IDENTITY))):
        for mask, plane in zip(view["masks"], planes[v]):
            K = default_K(*mask.shape) if pair.get("K") is None else pair["K"]
            lv, uv, f = (instance or instance_mesh)(mask, plane, K, stride)
            local.append(lv); verts.append(to_common(lv, cam)); uvs.append(uv); faces.append(f); view_of.append(v)
            vert_off.append(vert_off[-1] + len(lv)); face_off.append(face_off[-1] + len(f))
    cat = lambda parts, cols, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros((0, cols), dtype)      # noqa: E731
    return {"verts": cat(verts, 3, np.float64), "local": cat(local, 3, np.float64), "uvs": cat(uvs, 2, np.float64),
            "faces": cat(faces, 3, np.int64), "vert_off": np.asarray(vert_off, np.int64), "face_off": np.asarray(face_off, np.int64),
            "view_of_instance": np.asarray(view_of, np.int32), "planes": np.concatenate(planes).reshape(-1, 3)}
