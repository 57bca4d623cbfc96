"""The training-target kernels (csrc/train_targets.hip) and nopesac_amd/targets.py on the device against the numpy restatement of
tests/train_targets_forms.py: bit for bit on ids, n, n_all, bad, masks, plane centres, the centre map and the depth; the coordinate map
within |out - f64| <= 2^-22 (|a x| + |b y| + |c|) (one rounding per coefficient of K^-1, three in the fused sum); against the
reference's own outputs (tests/golden/train_targets) within the stored reference-to-float64 gap on top of that.  Every output lies
between guard elements."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import plane_criterion_inputs as PI
from tests import plane_criterion_ref as R
from tests import train_targets_forms as F

pytestmark = pytest.mark.gpu

PAD = 64
FILL = {torch.uint8: 0xA5, torch.int32: -1515870811, torch.float32: float("nan")}


def guarded(numel, dtype, device, shift=0):
    """-> (buffer, view of numel elements): PAD + shift guard elements in front, PAD behind; shift = 0 leaves the view 16-byte aligned"""
    buf = torch.full((numel + 2 * PAD + shift,), FILL[dtype], dtype=dtype, device=device)
    view = buf[PAD + shift:PAD + shift + numel]
    assert (view.data_ptr() % 16 == 0) == (shift * buf.element_size() % 16 == 0)
    return buf, view


def taken(buf, numel, what, shift=0):
    """the view's content on the host: every element written, no guard element touched"""
    is_fill = lambda t: torch.isnan(t) if t.dtype == torch.float32 else t == FILL[t.dtype]
    b = buf.cpu()
    lo = PAD + shift
    assert bool(is_fill(b[:lo]).all()) and bool(is_fill(b[lo + numel:]).all()), what + ": a write outside the extent"
    assert not bool(is_fill(b[lo:lo + numel]).any()), what + ": an element left unwritten"
    return b[lo:lo + numel].clone().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _consts():
    from nopesac_amd import ops
    return ops.LABEL_MAX_IDS, ops.LABEL_TABLE_SLOTS


@functools.lru_cache(maxsize=None)
def _cases():
    cap, slots = _consts()
    c = F.label_cases(cap, slots)
    c["big_480x640"] = F.big_case()
    return c


@functools.lru_cache(maxsize=None)
def _reference(name):
    """ids, n_all, n, bad, nmax, masks, centres, centre map of the restatement: computed once per case"""
    labels = _cases()[name]
    ids, n_all, n, bad = F.label_ids(labels, _consts()[0])
    nmax = max(int(n.max()), 1)
    return (ids, n_all, n, bad, nmax) + F.label_targets(labels, ids, n, nmax)


def _run_labels(labels, device, nmax=None, shift=0):
    from nopesac_amd import ops
    cap = ops.LABEL_MAX_IDS
    B, H, W = labels.shape
    d = torch.from_numpy(labels).to(device)
    g = [guarded(B * cap, torch.int32, device)] + [guarded(B, torch.int32, device) for _ in range(3)]
    ids, n_all, n, bad = ops.label_ids(d, 50, out=tuple(v for _, v in g))
    got = [taken(b, k, w) for (b, _), k, w in zip(g, (B * cap, B, B, B), ("ids", "n_all", "n", "bad"))]
    got[0] = got[0].reshape(B, cap)
    nmax = nmax or max(int(got[2].max()), 1)
    t = [guarded(B * nmax * H * W, torch.uint8, device, shift), guarded(B * nmax * 2, torch.float32, device), guarded(B * 2 * H * W, torch.float32, device)]
    dev = ops.label_targets(d, ids, n, nmax, out=tuple(v for _, v in t))
    got += [taken(t[0][0], B * nmax * H * W, "masks", shift).reshape(B, nmax, H, W), taken(t[1][0], B * nmax * 2, "plane_centers").reshape(B, nmax, 2),
            taken(t[2][0], B * 2 * H * W, "pixel_centers").reshape(B, 2, H, W)]
    return got, dev, n


@pytest.mark.parametrize("name", ["zeros", "one_id", "ids50", "ids51", "ids1000", "collide", "collide_neg", "negative", "int_max", "too_many", "exactly_cap",
                                  "cap_with_zero", "last_pixel", "ragged"] + ["size_%dx%d" % s for s in F.SIZES] + ["big_480x640"])
def test_label_kernels_bit_for_bit(device, name):
    from nopesac_amd import ops
    labels = _cases()[name]
    ids, n_all, n, bad, nmax, masks, centers, pixel = _reference(name)
    got, dev, n_dev = _run_labels(labels, device)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], n_all) and np.array_equal(got[2], n) and np.array_equal(got[3], bad), name
    assert got[4].shape == masks.shape and np.array_equal(got[4], masks), name
    assert np.array_equal(bits(got[5]), bits(centers)) and np.array_equal(bits(got[6]), bits(pixel)), name
    assert not got[4][np.arange(nmax)[None, :] >= n[:, None]].any() and not got[5][np.arange(nmax)[None, :] >= n[:, None]].any()
    if name in ("too_many", "cap_with_zero"):
        assert bad.tolist() == [1] and n.tolist() == [0] and not got[4].any() and not got[6].any()
    if name == "zeros":
        assert n.tolist() == [0] and not got[4].any()
    if int(n.min()) >= 1:                                           # the same bits as the general route on the masks this kernel wrote
        c2, p2 = ops.plane_targets(dev[0], torch.from_numpy(n), n_dev)
        assert np.array_equal(bits(c2.cpu().numpy()), bits(got[5])) and np.array_equal(bits(p2.cpu().numpy()), bits(got[6])), name
    again, _, _ = _run_labels(labels, device)                       # deterministic: two runs, the same bits
    assert all(np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b) for a, b in zip(got, again)), name


def test_label_targets_with_unaligned_masks_and_a_larger_nmax(device):
    """an output that is not 16-byte aligned takes the byte-store path at a size the wide path would take; nmax above every n"""
    labels = _cases()["ragged"]
    ids, n_all, n, bad = F.label_ids(labels, _consts()[0])
    masks, centers, pixel = F.label_targets(labels, ids, n, 50)
    got, _, _ = _run_labels(labels, device, nmax=50, shift=3)
    assert np.array_equal(got[4], masks) and np.array_equal(bits(got[5]), bits(centers)) and np.array_equal(bits(got[6]), bits(pixel))


def test_centres_against_the_reference_fixture(device):
    """within the stored reference-to-float64 gap plus one f32 ulp: the kernel's value is the correctly rounded float64 quotient"""
    for name in F.GOLDEN_CASES:
        labels, _ = F.golden_case(name)
        g = np.load(os.path.join(F.GOLD, name + ".npz"))
        got, _, _ = _run_labels(labels[None], device)
        k = int(g["n"])
        assert int(got[2][0]) == k and np.array_equal(np.packbits(got[4][0].reshape(k, -1), axis=1), g["masks"]), name
        for mine, ref, gap in ((got[5][0], g["plane_centers"], g["gap_plane_centers"]), (got[6][0], g["pixel_centers"], g["gap_pixel_centers"])):
            err, tol = np.abs(mine.astype(np.float64) - ref), float(gap) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            print("%s: centre error %.3e, gap %.3e" % (name, err.max(), float(gap)))
            assert (err <= tol).all(), (name, err.max(), float(gap))


def _offsets(counts, device):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(device)


@pytest.mark.parametrize("size", [(17, 33), (16, 16), (3, 5)])
def test_bits_to_masks_against_rle_decode(device, size):
    from nopesac_amd import ops, rle
    H, W = size
    assert (H, W) != (17, 33) or (H * W) % 32 != 0
    views = F.mask_views(H, W, 7 + H)
    rles = [F.to_rle(m) for v in views for m in v]
    packed, _ = rle.segmentation_bits(rles, device)
    counts = [len(v) for v in views]
    assert counts == [3, 0, 5]
    for nmax, shift in ((3, 0), (6, 0), (3, 5)):                    # fewer rows than the last view holds; more than any holds; unaligned
        buf, view = guarded(3 * nmax * H * W, torch.uint8, device, shift)
        ops.bits_to_masks(packed, _offsets(counts, device), nmax, H, W, out=view)
        got = taken(buf, 3 * nmax * H * W, "masks", shift).reshape(3, nmax, H, W)
        want = np.zeros_like(got)
        for b, v in enumerate(views):
            for j, m in enumerate(v[:nmax]):
                want[b, j] = rle.decode(F.to_rle(m))
        assert np.array_equal(got, want), (size, nmax)
        assert not got[1].any() and want[2, :3].any()


@pytest.mark.parametrize("size", [(30, 40), (17, 33)])
def test_bits_to_masks_of_overlapping_polygons(device, size):
    from nopesac_amd import ops, rle
    H, W = size
    views = F.polygon_views(H, W)
    packed, _ = rle.segmentation_bits([s for v in views for s in v], device, size=(H, W))
    host = F.unpack_bits(packed.cpu().numpy(), H, W)
    assert (host[:3].sum(0) > 1).any()                              # the polygons of the first view overlap
    buf, view = guarded(3 * 3 * H * W, torch.uint8, device)
    ops.bits_to_masks(packed, _offsets([3, 0, 5], device), 3, H, W, out=view)
    got = taken(buf, 3 * 3 * H * W, "masks").reshape(3, 3, H, W)
    assert np.array_equal(got[0], host[:3]) and not got[1].any() and np.array_equal(got[2], host[3:6])
    assert all(m.any() for m in host)


def test_depth_of_every_uint16_value(device):
    from nopesac_amd import ops
    v = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    want = F.depth_metres(v)
    buf, view = guarded(65536, torch.float32, device)
    ops.depth_from_u16(torch.from_numpy(v).to(device), out=view)
    assert np.array_equal(bits(taken(buf, 65536, "depth")), bits(want.reshape(-1)))
    # a source that is not 16-byte aligned, of an odd length: the one-value-per-thread path
    src = torch.from_numpy(v.reshape(-1)).to(device)[1:]
    buf, view = guarded(65535, torch.float32, device, shift=1)
    ops.depth_from_u16(src, out=view)
    assert np.array_equal(bits(taken(buf, 65535, "depth", 1)), bits(want.reshape(-1)[1:]))
    assert np.array_equal(bits(ops.depth_from_u16(torch.from_numpy(v[:3, :5].copy()).to(device), 256.0).cpu().numpy()), bits(v[:3, :5].astype(np.float32) / np.float32(256)))


@pytest.mark.parametrize("size", F.SIZES + [(480, 640)])
def test_coordinate_map_bound(device, size):
    from nopesac_amd import ops
    from nopesac_amd.targets import inverse_intrinsics
    H, W = size
    Ks = [F.DEFAULT_K] + F.SCANNET_KS
    kinv = torch.from_numpy(np.stack([inverse_intrinsics(K) for K in Ks])).to(device)
    buf, view = guarded(3 * 3 * H * W, torch.float32, device)
    ops.coordinate_map(kinv, H, W, out=view)
    got = taken(buf, 3 * 3 * H * W, "k_inv_dot_xy1").reshape(3, 3, H, W).astype(np.float64)
    for b, K in enumerate(Ks):
        want, mag = F.coordinate_map(K, H, W)
        err, tol = np.abs(got[b] - want), 2.0 ** -22 * mag
        print("%dx%d K %d: worst error / bound %.3f" % (H, W, b, float((err / tol).max())))
        assert (err <= tol).all(), (size, b, float((err / tol).max()))


def test_coordinate_map_against_the_reference_fixture(device):
    from nopesac_amd import ops
    from nopesac_amd.targets import inverse_intrinsics
    for name in F.GOLDEN_CASES:
        labels, K = F.golden_case(name)
        H, W = labels.shape
        g = np.load(os.path.join(F.GOLD, name + ".npz"))
        got = ops.coordinate_map(torch.from_numpy(inverse_intrinsics(K)[None]).to(device), H, W)[0].cpu().numpy().astype(np.float64)
        _, mag = F.coordinate_map(K, H, W)
        err, tol = np.abs(got - g["k_inv_dot_xy1"]), 2.0 ** -22 * mag + g["gap_k_inv_dot_xy1"][:, None, None]
        assert (err <= tol).all(), (name, float((err / tol).max()))


# ---- the mapper ---------------------------------------------------------------------------------------------------------------------------
CHAIN = "s1"                                                        # the smallest shape of tests/plane_criterion_inputs.py: 6 x 8 targets
CHAIN_K = np.array([[640.0, 0, 320], [0, 480.0, 240], [0, 0, 1]])   # K^-1 . (x, y, 1) = (col / W - 0.5, row / H - 0.5, 1): the case's own map


def _chain_records():
    """the case's targets as dataset records: a label map (plane j carries the label 3 j + 2), uint16 depth, annotations"""
    _, t = PI.make(CHAIN)
    masks, n = t["masks"].numpy(), t["n"]
    records = []
    for b in range(len(n)):
        sem = np.zeros(masks.shape[2:], np.int32)
        for j in range(n[b]):
            sem[masks[b, j] > 0] = 3 * j + 2
        d16 = np.clip(np.rint(t["depth"][b].numpy() * 1000.0), 0, 65535).astype(np.uint16)
        records.append({"image_id": "case_%d" % b, "semantic_map": sem, "depth": d16, "camera_K": CHAIN_K,
                        "annotations": [{"plane": t["plane_params"][b, j].tolist(), "category_id": 0} for j in range(n[b])]})
    return records


def _restated_targets(records, device, k_map):
    labels = np.stack([r["semantic_map"] for r in records])
    ids, n_all, n, bad = F.label_ids(labels, _consts()[0])
    nmax = int(n.max())
    masks, centers, pixel = F.label_targets(labels, ids, n, nmax)
    params = np.zeros((len(records), nmax, 3), np.float32)
    for b, r in enumerate(records):
        params[b, :n[b]] = np.asarray([a["plane"] for a in r["annotations"]], np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {"masks": up(masks), "n": torch.from_numpy(n.astype(np.int32)), "plane_params": up(params), "plane_centers": up(centers),
            "pixel_centers": up(pixel), "depth": up(F.depth_metres(np.stack([r["depth"] for r in records]))), "k_inv_dot_xy1": k_map}


def test_view_targets_feed_the_criterion_unchanged(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.targets import TargetMapper
    from nopesac_amd.training import PlaneCriterion
    cfg = get_cfg()
    records = _chain_records()
    mine = TargetMapper.from_cfg(cfg, device).view_targets(records)
    assert set(mine) == {"masks", "n", "n_host", "plane_params", "plane_centers", "pixel_centers", "depth", "k_inv_dot_xy1", "labels"}
    n = PI.CASES[CHAIN][6]
    assert mine["n_host"].tolist() == n and mine["n"].cpu().tolist() == n and mine["masks"].shape[1] == max(n)
    assert mine["labels"].cpu().tolist() == [[0] * k + [-1] * (max(n) - k) for k in n]
    # the coordinate map is the one field held to a bound, not to bits: the restated targets take the mapper's, after the bound is checked
    want_k, mag = F.coordinate_map(CHAIN_K, 6, 8)
    assert (np.abs(mine["k_inv_dot_xy1"].cpu().numpy().astype(np.float64) - want_k[None]) <= 2.0 ** -22 * mag[None]).all()
    theirs = _restated_targets(records, device, mine["k_inv_dot_xy1"])
    for k in ("masks", "plane_params", "plane_centers", "pixel_centers", "depth"):
        assert np.array_equal(mine[k].cpu().numpy().view(np.uint8), theirs[k].cpu().numpy().view(np.uint8)), k
    outputs, _ = PI.cast(*PI.make(CHAIN), torch.float32, device)
    res = []
    for t in (mine, theirs):
        crit = PlaneCriterion.from_cfg(cfg)
        losses, indices = crit(outputs, t)
        res.append(({k: v.detach().cpu() for k, v in losses.items()}, indices["match_q"].cpu(), indices["match_gt"].cpu()))
    assert set(res[0][0]) == set(res[1][0]) and all(torch.equal(res[0][0][k].view(torch.int32), res[1][0][k].view(torch.int32)) for k in res[0][0])
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert float(res[0][0]["loss_q"]) > 0 and float(res[0][0]["loss_mask"]) > 0      # live: the depth satisfies the planes under CHAIN_K


def test_the_three_routes_agree_and_default_intrinsics_are_cached(device):
    from nopesac_amd.targets import TargetMapper
    tm = TargetMapper(device)
    H, W = 30, 40
    sems = [F.partition(H, W, [3, 5, 9], 31), F.partition(H, W, [2, 4, 6, 8, 10], 32)]
    recs = []
    for s in sems:
        ids = F.unique_ids(s)
        recs.append({"semantic_map": s, "depth": np.full((H, W), 2.5, np.float32), "annotations": [{"plane": [0.0, 1.0, float(i)], "category_id": 0} for i in ids]})
    a = tm.view_targets(recs)
    stacks = [(F.unique_ids(s)[:, None, None] == s[None]).astype(np.uint8) for s in sems]
    b = tm.view_targets([dict({k: v for k, v in r.items() if k != "semantic_map"}, plane_masks=m) for r, m in zip(recs, stacks)])
    c = tm.view_targets([{"depth": r["depth"], "annotations": [dict(an, segmentation=F.to_rle(m)) for an, m in zip(r["annotations"], st)]}
                         for r, st in zip(recs, stacks)])
    for other in (b, c):
        for k in a:
            x, y = a[k].cpu().numpy(), other[k].cpu().numpy()
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    assert a["n_host"].tolist() == [3, 5] and float(a["depth"][0, 0, 0]) == 2.5
    assert len(tm._default_map) == 1 and np.array_equal(a["k_inv_dot_xy1"][0].cpu().numpy(), a["k_inv_dot_xy1"][1].cpu().numpy())
    want, mag = F.coordinate_map(F.DEFAULT_K, H, W)
    assert (np.abs(a["k_inv_dot_xy1"][0].cpu().numpy().astype(np.float64) - want) <= 2.0 ** -22 * mag).all()
    # the refusals that need the kernel's answer
    with pytest.raises(ValueError, match=r"view 1.*5 planes.*4 annotations"):
        tm.view_targets([recs[0], dict(recs[1], annotations=recs[1]["annotations"][:4])])
    many = (np.arange(H * W) % (_consts()[0] + 1) + 1).astype(np.int32).reshape(H, W)
    with pytest.raises(ValueError, match=r"view 0 \(v7\).*distinct labels"):
        tm.view_targets([dict(recs[0], image_id="v7", semantic_map=many)])
    with pytest.raises(ValueError, match="no plane"):
        tm.view_targets([dict(recs[0], semantic_map=np.zeros((H, W), np.int32), annotations=[])])


def test_pair_targets_feed_the_corr_matrix(device):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.targets import TargetMapper
    from nopesac_amd.training import PlaneCriterion, plane_corr_matrix
    cfg = get_cfg()
    r = _chain_records()
    n = PI.CASES[CHAIN][6]
    nq = PI.CASES[CHAIN][2]
    corrs = [[(0, 1), (3, 0), (2, 5), (51, 0), (1, 60)], [(1, 2), (0, 0)]]            # an index past n, two past 50
    entries = [{"0": r[0], "1": r[1], "gt_corrs": corrs[0], "rel_pose": {"position": [1.0, 2.0, 3.0], "rotation": [-0.5, 0.5, 0.5, 0.5]}},
               {"0": r[1], "1": r[0], "gt_corrs": corrs[1], "rel_pose": {"position": [0.0, 0.5, 0.0], "rotation": [0.5, -0.5, 0.5, 0.5]}}]
    out = TargetMapper.from_cfg(cfg, device).pair_targets(entries)
    t = out["targets"]
    assert t["n_host"].tolist() == [n[0], n[1], n[1], n[0]]                           # view-1 records first
    assert out["gt_pose"].cpu().tolist() == [[1.0, 2.0, 3.0, 0.5, -0.5, -0.5, -0.5], [0.0, 0.5, 0.0, 0.5, -0.5, 0.5, 0.5]]
    assert out["gt_corrs"].dtype == torch.int32 and out["gt_corrs"].cpu().tolist() == [[[0, 1], [3, 0], [2, 5]], [[1, 2], [0, 0], [-1, -1]]]
    o, _ = PI.cast(*PI.make(CHAIN), torch.float32, device)
    outputs = {k: torch.cat([v, v.flip(0)]) for k, v in o.items() if k != "aux_outputs"}
    _, indices = PlaneCriterion.from_cfg(cfg)(outputs, t)
    mq = indices["match_q"][0]
    got = plane_corr_matrix(out["gt_corrs"], mq[:2], mq[2:], nq)
    as_ref = lambda m, counts: [(m[b, :k].long().cpu(), torch.arange(k)) for b, k in enumerate(counts)]
    want = R.plane_corr_matrix(corrs, as_ref(mq[:2], [n[0], n[1]]), as_ref(mq[2:], [n[1], n[0]]), nq)
    assert torch.equal(got.cpu().bool(), want) and bool(want[:, :nq, :nq].any())
