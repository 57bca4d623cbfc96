"""CPU half of the stage sweep (tests/stage_forms.py): the forms tables are complete and every build, bench leg and edge is a GPU case; the
float64 references reproduce the reference fixtures and the oracle; the designed inputs keep their decisions away from the margins."""
import pytest
import torch

from oracle import nopesac_oracle as O
from tests import golden_inputs as GI
from tests import head_forms as HF
from tests import stage_forms as S
from tests.util import gold, rel_err

CFG = O.OracleConfig()


# ------------------------------------------------------------------------------------------------------------------------ forms tables
def test_sinkhorn_table_names_one_build_per_size_and_every_build_is_a_gpu_case():
    for nq in range(1, 129):
        for no_w4 in (False, True):
            for no_wg in (False, True):
                assert S.sinkhorn_build(nq, no_w4, no_wg) in S.SINK_BUILDS
    # the boundaries of the dispatch (matcher.hip): the last size of a build and the first of the next
    plain = {nq: S.sinkhorn_build(nq) for nq in range(1, 129)}
    for last, build, nxt in ((51, "w4<13>", "w4<16>"), (63, "w4<16>", "wg<2,17>"), (67, "wg<2,17>", "wg<2,26>"), (103, "wg<2,26>", "wg<2,32>"),
                             (127, "wg<2,32>", "wg<3,33>")):
        assert plain[last] == build and plain[last + 1] == nxt
    assert {S.sinkhorn_build(nq, True, True) for nq in range(1, 128)} == {"k1024<16>"} and S.sinkhorn_build(128, True, True) == "k1024<36>"
    assert S.sinkhorn_build(50, True, False) == "wg<2,17>"          # one switch alone reaches the row-group form, not the 1024 threads
    assert {b for _, b in S.SINK_GPU_CASES} == set(S.SINK_BUILDS)
    for nq, build in S.SINK_GPU_CASES:
        S.sinkhorn_switches(nq, build)
        assert nq in S.SINK_FLOOR
    for nq, build in plain.items():                                  # first and last size of every default build is a case
        if nq == 1 or nq == 128 or plain[nq - 1] != build or plain[nq + 1] != build:
            assert (nq, build) in S.SINK_GPU_CASES, (nq, build)


def test_bench_legs_are_cases_of_all_three_families():
    legs = set(HF.LEG_NQ.values()) | {HF.ONE_PAIR_NQ}
    assert legs <= {nq for nq, b in S.SINK_GPU_CASES if not b.startswith("k1024")}
    assert legs <= {c[0] for c in S.PS_GPU_CASES} and legs <= set(S.NQS)
    for nq in S.NQS:
        assert set(S.ransac_ms(nq)) >= {0, 1, 2, nq - 1, nq}


def test_sinkhorn_pairs_hold_the_edges():
    for nq in sorted({n for n, _ in S.SINK_GPU_CASES}):
        p = S.sinkhorn_pairs(nq)
        assert len(p) <= 12 and (nq, nq) in p and (1, 1) in p and (0, 0) in p and any(a == 0 < b for a, b in p) and any(b == 0 < a for a, b in p)
        assert (nq, min(2, nq)) in p and (min(3, nq), nq) in p
        if nq >= 65:
            assert {63, 64, 65} <= {a for a, _ in p} and {63, 64, 65} <= {b for _, b in p}


def test_postselect_cases_reach_every_build_the_refusal_and_both_count_registers():
    forms = {}
    for c in S.PS_GPU_CASES:
        nq, geom, pair = c
        forms.setdefault(S.postselect_form(nq, *S.PS_GEOMETRIES[geom]), []).append(c)
    assert S.REFUSED in forms and all(c[0] == 128 for c in forms[S.REFUSED])
    assert {f[1:] for f in forms if f != S.REFUSED} == set(S.PS_BUILDS)
    assert S.postselect_form(50, 12, 24, 24, 48) == (8, 2, False)           # the host loop halves the 16-row tile once
    assert S.postselect_form(50, 120, 160, 480, 640) == (16, 4, True)      # the architecture's shape
    for build in S.PS_BUILDS:                                               # every build also with more than 64 valid queries
        assert any(max(c[2]) > 64 for f, cs in forms.items() if f != S.REFUSED and f[1:] == build for c in cs), build
    for nq in S.NQS:
        nvs = {abs(v) for c in S.PS_GPU_CASES if c[0] == nq for v in c[2]}
        assert nvs >= {v for v in S.PS_NV if v <= nq}, (nq, nvs)
    x4 = [c for c in forms[(16, 4, True)]]
    assert any(S.PS_GEOMETRIES[c[1]][3] % 64 for c in x4) and any(S.PS_GEOMETRIES[c[1]][2] % 16 for c in x4)   # ragged tiles each way
    assert any(min(c[2]) < 0 for c in S.PS_GPU_CASES)                       # the max-overlap fallback
    nv_mod = {max(v, 1) % 4 for c in S.PS_GPU_CASES for v in c[2] if v >= 0}
    assert nv_mod == {0, 1, 2, 3}                                           # every list padding


# ------------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("nq", [7, 50, 128])
def test_sinkhorn_reference_meets_the_marginals(nq):
    """Columns of exp(scores + norm) after the 200 iterations the kernels run (the column potential is updated last), rows once the
    iteration has converged (3000 iterations; thin pairs such as (50, 2) are still 1e-7 away from the row marginals after 200)."""
    c = S.sinkhorn_inputs(nq)
    for b, r in enumerate(S.matcher_references(nq, 200)):
        if r["ls"] is None or not (r["n1"] and r["n2"]):
            continue
        n1, n2 = r["n1"], r["n2"]
        norm = -torch.log(torch.tensor(float(n1 + n2), dtype=torch.float64))
        P = torch.exp(r["block"] + norm)
        mu = torch.cat([torch.full((n1,), 1.0), torch.tensor([float(n2)])]).double() / (n1 + n2)
        nu = torch.cat([torch.full((n2,), 1.0), torch.tensor([float(n1)])]).double() / (n1 + n2)
        assert float((P.sum(0) - nu).abs().max()) < 1e-9, (n1, n2)
        if nq < 128:
            P = torch.exp(S.matcher_reference(c, b, 3000, 0.0)["block"] + norm)
            assert float((P.sum(1) - mu).abs().max()) < 1e-9 and float((P.sum(0) - nu).abs().max()) < 1e-9, (n1, n2)


@pytest.mark.parametrize("n1,n2,seed", [(1, 1, 50), (5, 3, 51), (17, 40, 52), (32, 32, 53), (50, 50, 54)])
def test_matcher_reference_against_the_fixtures_and_the_oracle(sd50, n1, n2, seed):
    """The descriptor dot products of the oracle's matcher (its scores with its own f32 geometric terms taken back out) through the f64
    geometry + Sinkhorn + assignment: the fixtures' log scores and assignment, and oracle.log_sinkhorn in f32."""
    case = GI.matcher_case(n1, n2, seed)
    app1, app2, cam7, p1, p2 = case
    with torch.no_grad():
        s32 = O.matcher_scores(sd50, *case, CFG)
        ang, off = O._geometric_dists(p1, p2, cam7[3:], cam7[:3], 1e-10, 5.0)
        dot = s32 + off / CFG.offset_multiplier + ang / CFG.normal_multiplier
        ls32 = O.log_sinkhorn(s32, sd50["matching_head.bin_score"], 200)
    c = {"nq": 50, "n1": [n1], "n2": [n2], "dot": torch.zeros(1, 50, 50), "p1": torch.zeros(1, 50, 3), "p2": torch.zeros(1, 50, 3), "cam7": cam7[None]}
    c["dot"][0, :n1, :n2], c["p1"][0, :n1], c["p2"][0, :n2] = dot, p1, p2
    bin_score = float(sd50["matching_head.bin_score"])
    old = S.BIN_SCORE
    S.BIN_SCORE = bin_score
    try:
        r = S.matcher_reference(c, 0, 200, 1e-4)
    finally:
        S.BIN_SCORE = old
    g = gold(f"E_matcher_{n1}x{n2}")
    assert rel_err(r["block"], g["log_scores"]) < 2e-5 and rel_err(r["block"], ls32) < 2e-5
    assert torch.equal(r["A"][:n1, :n2].float(), g["assignment"]) and float(r["A"].sum()) == float(g["assignment"].sum())
    ls = r["ls"]
    assert bool((ls[n1:50] == -1e30).all()) and bool((ls[:, n2:50] == -1e30).all()) and torch.equal(ls[50, 50], r["block"][n1, n2])


@pytest.mark.parametrize("kind,seed", [("multi", 31), ("none_pass", 32), ("all_overlap_rejected", 33), ("full", 34)])
def test_postselect_reference_reproduces_the_fixtures(kind, seed):
    logits, params, mask, feat = GI.postselect_case(kind, seed)
    r = S.postselect_reference(logits, torch.sigmoid(mask), params, feat, 480, 640)
    g = gold(f"C_postselect_{kind}")
    n = r["n_kept"]
    idx = r["kept_idx"][:n]
    assert idx.tolist() == g["idx"].tolist() and int(r["kept_idx"][n:].max() if n < 50 else -1) == -1
    assert torch.equal(r["planes"][:n], g["planes"])
    n_out = int((r["margin"] < S.PS_MARGIN).sum())
    assert (r["areas"][:n] - g["areas"]).abs().max() <= n_out
    assert rel_err(r["centers"][:n], g["centers"]) < 2e-4 and rel_err(r["scores"][:n], g["scores"]) < 1e-6
    from nopesac_amd.modeling import decode_masks
    rows = decode_masks(r["winner"], idx, bool(r["flags"] & 2)).sum(2).to(torch.int32)
    assert (rows - g["mask_rowsum"]).abs().sum() <= 2 * n_out
    assert r["flags"] == {"multi": 0, "none_pass": 1, "all_overlap_rejected": 2, "full": 0}[kind]


@pytest.mark.parametrize("m,cam_type", [(0, "soft"), (1, "soft"), (2, "soft"), (7, "soft"), (32, "soft"), (50, "soft"), (7, "avg-all"),
                                        (7, "min-cost"), (7, "max-score")])
def test_ransac_references_reproduce_the_fixtures(sd50, m, cam_type):
    """geo_sequence, the score maps and the vote in f64 on the refine fixtures' inputs; the MLP stacks between them come from the oracle."""
    nq = 50
    rc = GI.refine_case(nq, m, 60 + m)
    n1, n2 = rc["A"].shape
    c = {"nq": nq, "ms": [m], "A": torch.zeros(1, nq, nq), "p1": torch.zeros(1, nq, 3), "p2": torch.zeros(1, nq, 3),
         "n1": torch.tensor([n1]), "n2": torch.tensor([n2]), "init_rot": rc["init_rot"][None], "init_trans": rc["init_trans"][None]}
    c["A"][0, :n1, :n2], c["p1"][0, :n1], c["p2"][0, :n2] = rc["A"], rc["planes1"], rc["planes2"]
    g = gold(f"F_refine_nq{nq}_m{m}_{cam_type}")
    seq = S.geo_sequence_reference(c, 0, True)
    assert seq["m"] == m and rel_err(seq["geo_global"], g["geo_global"]) < 1e-5 and torch.equal(seq["sig"].float(), g["sig"][:, 0])
    gl, _ = O.geo_sequence(rc["planes1"], rc["planes2"], rc["A"], nq)
    assert torch.equal(seq["geo_local"].float(), gl)
    enc_l = S.geo_sequence_reference(c, 0, False)["geo_enc"]
    o = gl[:, :3].norm(dim=-1, keepdim=True)
    assert rel_err(enc_l[:, :4], torch.cat([gl[:, :3] / (o + 1e-10), o], -1)) < 1e-6
    if m < 2:
        return
    p = "camera_head_list.0"
    lin = lambda x, n: torch.nn.functional.linear(x, sd50[f"{p}.{n}.weight"], sd50[f"{p}.{n}.bias"])
    with torch.no_grad():
        geo = O.mlp(seq["geo_enc"].float(), sd50, p + ".geo_encoder")
        s1 = O.mlp(geo, sd50, p + ".geo_proj_s1")
        f_rot = O.mlp(s1, sd50, p + ".decoder_rot")
        f_tran = O.mlp(O.mlp(torch.cat([s1, f_rot], -1), sd50, p + ".geo_proj_s2"), sd50, p + ".decoder_tran")
        fused_rot = torch.relu(O.mlp(torch.cat((rc["rot_feat"].expand(nq, -1), f_rot), -1), sd50, p + ".decoder_rot2"))
        fused_tran = torch.relu(O.mlp(torch.cat((rc["trans_feat"].expand(nq, -1), f_tran), -1), sd50, p + ".decoder_tran2"))
        maps = S.score_maps_reference(gl, lin(fused_rot, "rots"), lin(fused_tran, "trans"), rc["init_rot"], rc["init_trans"], m)
        sf_r = O.mlp(maps["normal_score"].float(), sd50, p + ".normal_score_proj")
        sf_t = O.mlp(maps["param_score"].float(), sd50, p + ".param_score_proj")
    assert rel_err(maps["rots_all"][:m + 1], g["all_pred_rots"]) < 5e-5 and rel_err(maps["trans_all"][:m + 1], g["all_pred_trans"]) < 5e-5
    assert rel_err(maps["l2_dist"][:m + 1, :m], g["l2_dist"]) < 5e-5 and rel_err(maps["normal_angle"][:m + 1, :m], g["normal_dist"]) < 1e-3
    assert rel_err(maps["offset_dist"][:m + 1, :m], g["offset_dist"]) < 5e-5
    w = lambda n: sd50[f"{p}.{n}"]
    c.update(sf_rot=sf_r[None], sf_trans=sf_t[None], reg_rot_w=w("rot_score_reg.weight")[0], reg_rot_b=w("rot_score_reg.bias"),
             reg_trans_w=w("trans_score_reg.weight")[0], reg_trans_b=w("trans_score_reg.bias"), init_rot_feat=rc["rot_feat"][None],
             init_trans_feat=rc["trans_feat"][None], fused_rot=fused_rot[None], fused_trans=fused_tran[None], rots_w=w("rots.weight"),
             rots_b=w("rots.bias"), trans_w=w("trans.weight"), trans_b=w("trans.bias"))
    mode = {"soft": 0, "avg-all": 1, "min-cost": 2, "max-score": 3}[cam_type]
    v = S.soft_vote_reference(c, 0, maps, mode)
    for mine, key in (("pred_trans", "pred_trans"), ("pred_rot", "pred_rot"), ("avg_trans", "pred_trans_avg"), ("avg_rot", "pred_rot_avg")):
        assert rel_err(v[mine], g[key]) < 5e-5, key
    assert rel_err(v["score_rot"][:m + 1], g["score_soft_rot"][:, 0]) < 1e-4 and rel_err(v["score_trans"][:m + 1], g["score_soft_offset"][:, 0]) < 1e-4


# ------------------------------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("nq", sorted({n for n, _ in S.SINK_GPU_CASES}))
def test_matcher_inputs_decide_something_and_stay_off_the_margins(nq):
    c = S.sinkhorn_inputs(nq)
    for iters in S.SINK_ITERS:
        refs = S.matcher_references(nq, iters)
        pairs = sum(r["n1"] * r["n2"] for r in refs)
        rows = sum(r["n1"] + r["n2"] for r in refs if r["n1"] and r["n2"])
        for r in refs:
            lo = min(r["n1"], r["n2"])
            if lo >= 4:
                assert int(r["A"].sum()) >= lo // 4, (iters, r["n1"], r["n2"])
            assert float(r["A"][r["n1"]:].sum() + r["A"][:, r["n2"]:].sum()) == 0
        assert sum(r["n_out_pairs"] for r in refs) <= S.PAIR_CAP * pairs, (iters, "pairs")
        assert sum(r["n_out_rows"] for r in refs) <= S.ROW_CAP * rows, (iters, "rows")
    assert c["n1"].tolist() == [p[0] for p in c["pairs"]]


@pytest.mark.parametrize("nq", sorted({n for n, _ in S.SINK_GPU_CASES}))
def test_sinkhorn_floor_constants_are_what_the_oracle_measures(nq):
    floor = S.oracle_f32_sinkhorn_floor(nq)
    print("nq %d: f32 oracle vs f64 %.3g (recorded %.3g)" % (nq, floor, S.SINK_FLOOR[nq]))
    assert S.SINK_FLOOR[nq] / 2 <= floor <= S.SINK_FLOOR[nq] * 2
    assert S.sinkhorn_bound(50) <= 5e-5


@pytest.mark.parametrize("case", [c for c in S.PS_GPU_CASES if S.postselect_form(c[0], *S.PS_GEOMETRIES[c[1]]) != S.REFUSED], ids=S.ps_case_id)
def test_postselect_inputs_stay_off_the_margins(case):
    assert S.postselect_case_ok(case)
    _, refs = S.postselect_case(case)
    assert refs[0]["kept_idx"].tolist() != refs[1]["kept_idx"].tolist() or case[2][0] == case[2][1]


@pytest.mark.parametrize("nq", S.NQS)
def test_ransac_inputs_stay_off_the_margins(nq):
    c = S.ransac_inputs(nq)
    n_out = n_all = 0
    for b, m in enumerate(c["ms"]):
        n1, n2 = int(c["n1"][b]), int(c["n2"][b])
        assert int(c["A"][b, :n1, :n2].sum()) == m and (m < 2 or int(c["A"][b, :n1, :n2].sum(1).max()) == 2)
        for wir in (True, False):
            seq = S.geo_sequence_reference(c, b, wir)
            assert seq["m"] == m and seq["sig_margin"] > S.SIG_MARGIN
        maps = S.score_maps_reference(seq["geo_local"].float(), c["rot_raw"][b], c["trans_raw"][b], c["init_rot"][b], c["init_trans"][b], m)
        assert float(maps["offset_out"].float().mean()) <= S.PAIR_CAP
        for mode in (2, 3):
            assert S.soft_vote_reference(c, b, maps, mode)["select_gap"] > S.SELECT_MARGIN, (m, mode)
        _, keep = S.refilter_reference(c["refilter_A"][b], c["p1"][b], c["p2"][b], n1, n2, c["init_rot"][b], c["init_trans"][b])
        n_out += int((~keep).sum())
        n_all += n1 * n2
    assert float(c["rot_raw"].norm(dim=-1).min()) < 1e-12
    assert n_out <= S.PAIR_CAP * n_all
