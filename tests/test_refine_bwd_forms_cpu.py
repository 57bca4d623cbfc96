"""CPU half of the camera head's backward sweep (tests/refine_bwd_forms.py): the inputs meet the conditions the GPU half relies on, the
committed float32 constants are what the module measures, the float64 restatements reproduce the forward references of
tests/stage_forms.py (and the oracle's loss lines), a float32 emulation of the kernels' own backward formulas stays within the limit,
and the same emulation with one planted error does not."""
import pytest
import torch

from tests import refine_bwd_forms as R
from tests import stage_forms as S

F64 = torch.float64


def _worst(family, key, got):
    return max(q for q, _ in R.worst_ratio(family, key, got).values())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def test_case_lists():
    assert R.NQS == (1, 2, 50, 64, 100, 128) and R.LOSS_BS == (1, 64, 65) and R.TRANS_EPS == (0.0, 1e-3)
    assert R.case_ms(1) == [1, 0] and R.case_ms(2) == [1, 2, 0] and R.case_ms(50) == [1, 2, 25, 49, 50, 0] and R.case_ms(128) == [1, 2, 64, 127, 128, 0]
    assert R.LOSS_WEIGHT != 1.0 and R.POSE_WEIGHT != 1.0
    assert set(R.F32_WORST) == set(R.FAMILIES) == set(R.EMULATE) == set(R.PLANTS)


@pytest.mark.parametrize("nq", R.NQS)
def test_geometry_inputs_meet_their_conditions(nq):
    c = R.geometry_inputs(nq)
    ms, B = c["ms"], len(c["ms"])
    assert ms == R.case_ms(nq) and ms[-1] == 0 and c["m"].tolist() == ms
    assert int((c["rot_raw"].norm(dim=-1) < 1e-12).sum()) == (2 if nq > 1 else 1)              # the g / 1e-12 branch
    sm = R.margins("score_maps", nq)
    assert sm["dist"] > R.DIST_MARGIN, sm["dist"]                                                # dn, dl2: exactly 0 or above the margin
    for b, m in enumerate(ms):
        assert float(c["geo_local"][b, m:].abs().sum()) == 0 or b % 2 == 1
        assert b % 2 == 0 or m == nq or float(c["geo_local"][b, m:].abs().min()) > 0
    v = R.margins("vote", nq)
    assert v["clamp"] >= R.CLAMP_MARGIN, v
    assert v["all_clamped"] >= 1 and v["none_clamped"] >= 1 and v["above_0.9"] >= 1, v
    NH = nq + 1
    for k in R.FAMILIES["score_maps"]["cots"]:
        g = c[k]
        assert (g == 0).any() and (nq <= 2 or ((g < 0).any() and (g > 0).any()))                  # (four or twelve entries at nq = 1, 2)
        for b, m in enumerate(ms):                                                               # nonzero where the forward is masked
            assert m == nq or (g[b, :, m:] != 0).any()
            assert (g[b, m + 1:] != 0).any() or (m + 1 == NH) or (b, NH - 1) in c["no_cotangent"] and m + 2 == NH
        for b, h in c["no_cotangent"]:
            assert float(g[b, h].abs().sum()) == 0
    for k in ("g_score_rot", "g_score_trans"):
        assert all(m + 1 == NH or (c[k][b, m + 1:] != 0).any() for b, m in enumerate(ms))
    for k in R.FAMILIES["vote"]["cots"]:
        assert float(c[k].abs().max()) != 1.0 and (c[k] < 0).any()


@pytest.mark.parametrize("key", R.family_keys("losses"), ids=lambda k: "nq%d_B%d" % k)
def test_loss_inputs_meet_their_conditions(key):
    nq, B = key
    c = R.loss_inputs(nq, B)
    mg = R.margins("losses", key)
    assert mg["argmin"] >= R.ARGMIN_MARGIN and mg["score"] >= R.SCORE_MARGIN, mg
    assert c["weight"] != 1.0 and int((c["g_loss"] == 0).sum()) == 1 and (c["g_loss"] < 0).any()
    assert c["m"].tolist().count(0) == (1 if B > 1 else 0) and set(c["m"].tolist()) - {0} <= set(R.case_ms(nq))
    assert (c["gt_pose"][:, 3:].norm(dim=-1) - 1).abs().min() > 1e-3                              # normalised inside, on both sides
    if B > 3:
        assert torch.equal(c["pred_rot"][2], c["gt_pose"][2, 3:]) and torch.equal(c["avg_trans"][2], c["gt_pose"][2, :3])
        cos = torch.nn.functional.cosine_similarity(c["pred_rot"][3].double(), c["gt_pose"][3, 3:].double(), dim=0)
        assert float(cos) < -1 + 1e-12
        ref, _ = R.reference("losses", key)
        row = c["live"].tolist().index(2)
        for k in ("g_pred_rot", "g_pred_trans", "g_avg_rot", "g_avg_trans"):
            assert float(ref[k][row].abs().sum()) == 0


def test_loss_inputs_cover_both_sides_of_one():
    sides = set()
    for key in R.family_keys("losses"):
        sides |= R.margins("losses", key)["sides"]
    assert sides == {-1, 0, 1}


@pytest.mark.parametrize("key", R.family_keys("pose_loss"), ids=lambda k: "B%d_eps%g" % k)
def test_pose_inputs_meet_their_conditions(key):
    c = R.pose_inputs(*key)
    assert c["gt_trans"].stride(0) == 7 and c["gt_rot"].stride(0) == 7 and c["gt_rot"].data_ptr() == c["pose"].data_ptr() + 12
    assert c["weight"] != 1.0 and (c["g_out"] < 0).any() and (c["g_out"] > 0).any()
    if c["B"] > 3:
        assert torch.equal(c["est_rot"][2], c["gt_rot"][2]) and torch.equal(c["est_trans"][2], c["gt_trans"][2])
        assert float(torch.nn.functional.cosine_similarity(c["est_rot"][3].double(), c["gt_rot"][3].double(), dim=0)) < -1 + 1e-12
        if key[1] == 0.0:
            ref, _ = R.reference("pose_loss", key)
            assert all(float(v[2].abs().sum()) == 0 for v in ref.values())


# ---- constants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_f32_constants_are_what_the_module_measures(family):
    measured = R.f32_worst(family)
    assert 0.5 <= measured / R.F32_WORST[family] <= 2.0, (family, measured, R.F32_WORST[family])
    assert R.limit(family) == 8.0 * R.F32_WORST[family]


# ---- references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", R.NQS)
def test_f64_forwards_reproduce_the_stage_references(nq):
    c = R.geometry_inputs(nq)
    x, aux, _ = R.problem("score_maps", nq)
    got = R.score_maps_fwd({k: v.double() for k, v in x.items()}, aux)
    for b, m in enumerate(c["ms"]):
        r = S.score_maps_reference(c["geo_local"][b], c["rot_raw"][b], c["trans_raw"][b], c["init_rot"][b], c["init_trans"][b], m)
        for o, k in zip(got, ("normal_score", "param_score", "l2_dist")):
            assert float((o[b] - r[k]).abs().max()) <= 1e-12 * max(float(r[k].abs().max()), 1.0), (nq, m, k)
    x, aux, _ = R.problem("vote", nq)
    got = R.vote_fwd({k: v.double() for k, v in x.items()}, aux)
    for b, m in enumerate(c["ms"][:-1]):
        r = S.soft_vote_reference(c, b, {}, S.VOTE_TRAIN)
        for o, k in zip(got, ("pred_rot", "pred_trans", "avg_rot", "avg_trans", "score_rot", "score_trans")):
            assert float((o[b] - r[k]).abs().max()) <= 1e-12, (nq, m, k)


@pytest.mark.parametrize("key", [(1, 1), (2, 64), (50, 65), (128, 65)], ids=lambda k: "nq%d_B%d" % k)
def test_f64_losses_reproduce_the_oracle_lines(key):
    """The seven losses pair by pair, as the oracle's ransac_refine_train writes them (with its camera_pose_loss), over the live pairs."""
    from oracle import nopesac_oracle as O
    c = R.loss_inputs(*key)
    x, aux, _ = R.problem("losses", key)
    x = {k: v.double() for k, v in x.items()}
    got = R.losses_fwd(x, aux)[0]
    acc = torch.zeros(7, dtype=F64)
    for i in range(len(c["live"])):
        m, gt = int(aux["m"][i]), x["gt_pose"][i:i + 1]
        acc[0], acc[1] = (a + v for a, v in zip(acc[:2], O.camera_pose_loss(torch.cat((x["avg_trans"][i:i + 1], x["avg_rot"][i:i + 1]), -1), gt)))
        acc[2], acc[3] = (a + v for a, v in zip(acc[2:4], O.camera_pose_loss(torch.cat((x["pred_trans"][i:i + 1], x["pred_rot"][i:i + 1]), -1), gt)))
        rot_err = (torch.nn.functional.normalize(gt[:, 3:], dim=-1) - torch.nn.functional.normalize(c["rots_all"][c["live"][i]].double(), dim=-1)).norm(dim=-1)
        tr_err = (gt[:, :3] - c["trans_all"][c["live"][i]].double()).norm(dim=-1)
        acc[4] += (1.0 - x["score_rot"][i, rot_err[:m + 1].argmin()]).abs()
        acc[5] += (1.0 - x["score_trans"][i, tr_err[:m + 1].argmin()]).abs()
        acc[6] += torch.diag(x["l2_dist"][i, 1:]).sum() / m
    ref = acc / c["B"] * torch.tensor([1, 1, 1, 1, 0.01, 0.02, 0.1], dtype=F64) * c["weight"]
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize("key", R.family_keys("pose_loss"), ids=lambda k: "B%d_eps%g" % k)
def test_f64_pose_loss_reproduces_the_oracle(key):
    from oracle import nopesac_oracle as O
    x, aux, _ = R.problem("pose_loss", key)
    x = {k: v.double() for k, v in x.items()}
    got = R.pose_loss_fwd(x, aux)[0]
    lx, lq = O.camera_pose_loss(torch.cat((x["est_trans"], x["est_rot"]), -1), torch.cat((x["gt_trans"] + aux["eps"], x["gt_rot"]), -1))
    assert float((got - torch.stack([lx, lq]) * aux["weight"]).abs().max()) <= 1e-14


# ---- emulation and planted errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_f32_emulation_of_the_kernel_formulas_stays_within_the_limit(family):
    for key in R.family_keys(family):
        w = R.worst_ratio(family, key, R.EMULATE[family](key))
        assert all(q <= R.limit(family) for q, _ in w.values()), (family, key, w)


# where each planted error must show: every key of the family that reaches the faulty term
# (the renormalisation's dot product is the same for every hypothesis, and the softmax backward removes what is common to all of them: it
# shows only where some probabilities of a pair are clamped and others are not, which needs more than the two hypotheses of nq = 1)
PLANT_KEYS = {("vote", "renorm_dot"): list(R.NQS[1:]),
              ("losses", "inv_b_64"): [(nq, B) for nq in R.NQS for B in (1, 65)],
              ("losses", "diag_j_below_m"): [(nq, B) for nq in R.NQS[1:] for B in (64, 65)],
              ("pose_loss", "eps_ignored"): [(B, 1e-3) for B in R.LOSS_BS]}


@pytest.mark.parametrize("family,plant", [(f, p) for f in sorted(R.PLANTS) for p in R.PLANTS[f]])
def test_planted_errors_do_not_stay_within_the_limit(family, plant):
    for key in PLANT_KEYS.get((family, plant), R.family_keys(family)):
        assert _worst(family, key, R.EMULATE[family](key, plant)) > R.limit(family), (family, plant, key)
