"""Seeded inputs of the reconstruction meshes (nopesac_amd/mesh.py), shared by scripts/gen_recon_mesh_golden.py (which runs the
reference's functions on them and stores only their results, tests/golden/K_recon_mesh_<seed>.npz) and the tests.  Built on the
geometry of tests/recon_eval_inputs.py: a camera from its _camera, a view's masks a partition of the image into its _blobs, the two
views of a matched plane derived from ONE plane of the common frame through the camera (its _local_in_view0) and then turned and
shifted a little, so that merging has something to do; matched planes keep n0 . n1 >= DOT_MARGIN unless the pair is a `negdot` one,
whose first correspondence joins two unrelated planes with n0 . n1 <= -NEG_DOT.

Two conditions hold for every instance of every case, on the planes that are meshed (merged and not): the plane meets the rays of
its mask's pixels with |n . ray| >= FACING, and its offset lies in [OFFSET_LO, OFFSET_HI].  They bound the conditioning of
depth = offset / (n . ray), which the tests' tolerances rely on.  A draw that misses either is rejected and drawn again with the next
sub-seed."""
import numpy as np

from tests import recon_mesh_ref as REF
from tests.plane_eval_inputs import _rotate
from tests.recon_eval_inputs import DOT_MARGIN, FLIP, _blobs, _camera, _local_in_view0, _unit

SEEDS = (31, 32, 33)
FACING, OFFSET_LO, OFFSET_HI, NEG_DOT = 0.2, 0.5, 6.0, 0.3

# What the pairs of a seed are.  n: instances per view;  ncorr: correspondences (the first `ncorr` planes of view 1 are seen in view
# 0 too, listed there in another order);  negdot: the first correspondence joins planes whose global normals point apart;
# qscale: camera quaternion scale;  K: the pair carries its own intrinsics (else None: the default ones)
PLAN = {
    31: [dict(n=(3, 3), ncorr=2), dict(n=(2, 3), ncorr=0), dict(n=(3, 2), ncorr=1, qscale=1.7, K=True)],
    32: [dict(n=(3, 3), ncorr=2, negdot=True, K=True), dict(n=(0, 2), ncorr=0), dict(n=(2, 2), ncorr=2, qscale=0.6)],
    33: [dict(n=(4, 3), ncorr=3), dict(n=(2, 2), ncorr=1, negdot=True)],
}


def rays(mask, K):
    ys, xs = np.nonzero(mask)
    return (np.linalg.inv(K) @ np.stack([xs, ys, np.ones_like(xs)]).astype(np.float64)).T


def plane_ok(plane, mask, K) -> bool:
    off = float(np.linalg.norm(plane))
    if not (OFFSET_LO <= off <= OFFSET_HI):
        return False
    r = rays(mask, K)
    return len(r) == 0 or float(np.abs(r @ (np.asarray(plane, np.float64) / off)).min()) >= FACING


def _facing_plane(rng, mask, K):
    """A plane in front of the camera that meets every ray of the mask well."""
    for _ in range(200):
        p = _unit(rng.normal(size=3) * np.array([0.6, 0.6, 0.2]) + np.array([0.0, 0.0, 1.0])) * rng.uniform(0.8, 5.0)
        if plane_ok(p, mask, K):
            return p
    return None


def _pair(rng, h, w, n=(3, 3), ncorr=2, negdot=False, qscale=1.0, K=False):
    cam = _camera(rng)
    Kp = np.array([[517.97 * w / 640 * rng.uniform(0.9, 1.1), 0.0, w / 2 + 0.7], [0.0, 517.97 * w / 640, h / 2 - 0.4], [0.0, 0.0, 1.0]]) if K else None
    Ku = REF.default_K(h, w) if Kp is None else Kp
    masks = [_blobs(rng, h, w, n[0]), _blobs(rng, h, w, n[1])]
    planes = [[None] * n[0], [None] * n[1]]
    order0 = list(rng.permutation(n[0]))                      # view 0 lists the shared planes in another order
    corrs = []
    for k in range(ncorr):
        a, b = int(order0[k]), k
        for _ in range(500):
            if negdot and k == 0:
                p0, p1 = _facing_plane(rng, masks[0][a], Ku), _facing_plane(rng, masks[1][b], Ku)
                if p0 is None or p1 is None:
                    continue
            else:
                p1 = _facing_plane(rng, masks[1][b], Ku)
                if p1 is None:
                    continue
                p0, _ = _local_in_view0(p1 * FLIP, cam)
                off = np.linalg.norm(p0)
                p0 = _rotate(p0 / off, rng.uniform(1.0, 8.0), rng) * (off + rng.uniform(-0.1, 0.1))
                p1 = p1 * (1.0 + rng.uniform(-0.03, 0.03))
            if plane_ok(p0, masks[0][a], Ku) and plane_ok(p1, masks[1][b], Ku):
                break
        else:
            return None
        planes[0][a], planes[1][b] = p0, p1
        corrs.append([a, b])
    for v in range(2):
        for k in range(n[v]):
            if planes[v][k] is None:
                planes[v][k] = _facing_plane(rng, masks[v][k], Ku)
                if planes[v][k] is None:
                    return None
    neg = list(corrs[0]) if negdot else None
    corrs.sort()
    camera = {"position": cam["position"], "rotation": cam["rotation"] * qscale}
    return {"views": tuple({"masks": masks[v], "planes": np.asarray(planes[v], np.float32).reshape(-1, 3)} for v in range(2)),
            "camera": camera, "corrs": np.asarray(corrs, np.int64).reshape(-1, 2), "K": Kp, "negdot": neg}


def custom_pair(seed, masks0, masks1, corrs=(), qscale=1.0, K=None):
    """A pair on masks the caller made (bool [n, h, w] per view): every plane meets the rays of the WHOLE image well, the two planes of
    a correspondence come from one plane of the common frame, and both conditions hold as for the seeded cases."""
    masks = [np.asarray(masks0, bool), np.asarray(masks1, bool)]
    h, w = masks[0].shape[1:]
    Ku = REF.default_K(h, w) if K is None else np.asarray(K, np.float64)
    whole = np.ones((h, w), bool)
    for attempt in range(400):
        rng = np.random.default_rng(100003 * seed + attempt)
        cam = _camera(rng)
        planes = [[_facing_plane(rng, whole, Ku) for _ in m] for m in masks]
        if any(p is None for v in planes for p in v):
            continue
        for a, b in corrs:
            p0, _ = _local_in_view0(planes[1][b] * FLIP, cam)
            off = np.linalg.norm(p0)
            planes[0][a] = _rotate(p0 / off, rng.uniform(1.0, 8.0), rng) * (off + rng.uniform(-0.1, 0.1))
        pair = {"views": tuple({"masks": masks[v], "planes": np.asarray(planes[v], np.float32).reshape(-1, 3)} for v in range(2)),
                "camera": {"position": cam["position"], "rotation": cam["rotation"] * qscale},
                "corrs": np.asarray(sorted(list(c) for c in corrs), np.int64).reshape(-1, 2), "K": K, "negdot": None}
        whole_pair = {**pair, "views": tuple({"masks": np.broadcast_to(whole, m.shape), "planes": v["planes"]} for m, v in zip(masks, pair["views"]))}
        if conditions_ok(whole_pair) and all(d >= DOT_MARGIN for d in matched_dots(pair)):
            return pair
    raise RuntimeError("no pair with the conditions found")


def matched_dots(pair):
    g0, g1 = REF.global_params(pair["views"][0]["planes"], pair["camera"]), REF.global_params(pair["views"][1]["planes"], REF.IDENTITY)
    return [float(_unit(g0[a]) @ _unit(g1[b])) for a, b in pair["corrs"]]


def conditions_ok(pair) -> bool:
    """Both conditions on every instance, for the merged planes and for the planes as they are."""
    for merge in (True, False):
        planes = REF.merged_local_planes(pair["views"][0]["planes"], pair["views"][1]["planes"], pair["camera"],
                                         pair["corrs"] if merge else np.zeros((0, 2), np.int64))
        for v in range(2):
            K = REF.default_K(*pair["views"][v]["masks"].shape[1:]) if pair["K"] is None else pair["K"]
            if not all(plane_ok(p, m, K) for p, m in zip(planes[v], pair["views"][v]["masks"])):
                return False
    return True


def recon_mesh_case(seed: int, h: int = 24, w: int = 32):
    """The pairs of PLAN[seed]: [{"views": ({"masks" bool [n, h, w], "planes" f32 [n, 3]}, x 2), "camera": {"position", "rotation"
    wxyz}, "corrs" int64 [k, 2], "K": 3 x 3 or None, "negdot": the correspondence [a, b] whose normals point apart, or None}]."""
    for attempt in range(400):
        rng = np.random.default_rng(1000 * seed + attempt)
        pairs = [_pair(rng, h, w, **kw) for kw in PLAN[seed]]
        if any(p is None for p in pairs):
            continue
        ok = all(conditions_ok(p) for p in pairs)
        for p in pairs:
            for corr, d in zip(p["corrs"].tolist(), matched_dots(p)):
                ok = ok and (d <= -NEG_DOT if corr == p["negdot"] else d >= DOT_MARGIN)
        if ok:
            return pairs
    raise RuntimeError("no case with the conditions found")


def product_pairs(pairs):
    """The case as nopesac_amd.mesh.pair_meshes takes it: masks as compressed COCO strings."""
    from oracle import rle_oracle as R
    return [{"views": tuple({"instances": [{"segmentation": R.encode(m)} for m in v["masks"]], "pred_plane": v["planes"]} for v in p["views"]),
             "camera": p["camera"], "corrs": p["corrs"], "K": p["K"]} for p in pairs]
