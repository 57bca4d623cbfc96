"""The CPU half of the plane criterion sweep (tests/plane_criterion_forms.py): the case lists reach the paths they claim, every input
condition holds in float64 and in float32, F32_WORST is what the float32 restatement measures, the assignment emulation reproduces
scipy's optimum on every hand-made cost (and stops on the non-finite ones), and a planted error leaves the limit."""
import numpy as np
import pytest
import torch

from tests import plane_criterion_forms as P
from tests import plane_criterion_ref as R


def test_cost_cases_reach_every_chunk_walk_wave_and_size():
    walks = {(c.h, c.w): P.chunk_walk(c) for c in P.COST_CASES}
    assert walks[(6, 8)] == ([1], 48)                                            # one partial chunk
    assert walks[(8, 8)] == ([1], 64)                                            # one full chunk
    assert walks[(5, 13)] == ([1, 1], 1)                                         # a second chunk with one live lane
    assert walks[(32, 32)] == ([1] * 16, 64)                                     # 16 full chunks, one per workgroup
    assert walks[(25, 41)] == ([2] + [1] * 15, 1)                                # a 17th chunk with one lane
    assert walks[(46, 46)] == ([3, 3] + [2] * 14, 4)                             # 34 chunks: workgroups 0 and 1 walk three
    by_hw = {}
    for c in P.COST_CASES:
        by_hw.setdefault((c.h, c.w), set()).add(c.s)
    assert all(v >= {1, 2} for v in by_hw.values()) and all(4 in by_hw[k] for k in ((6, 8), (8, 8), (5, 13)))
    assert {c.nq for c in P.COST_CASES} >= {1, 2, 3, 4, 5, 63, 64, 65, 100, 128}
    assert any(c.nq == 3 for c in P.COST_CASES)                                  # wave 3 of the cost kernel owns no query
    assert {(c.L, c.B) for c in P.COST_CASES} == {(1, 1), (3, 2), (2, 3), (8, 1)}
    ns = {n for c in P.COST_CASES for n in c.n}
    assert {1, 50} <= ns and any(c.nq <= 50 and c.nq in c.n for c in P.COST_CASES)
    assert any(c.nmax > max(c.n) for c in P.COST_CASES) and any(c.nmax == 50 for c in P.COST_CASES)
    assert {c.match for c in P.COST_CASES} == set(P.MATCHES)
    for c in P.COST_CASES:                                                       # the matches are what they are called
        mq = P.inputs(c.name)["match_q"]
        if c.match == "reversed":
            assert int(mq[0, 0]) == c.nq - 1                                     # the last query
        if c.match == "high" and c.nq - max(c.n) >= 64:
            assert int(mq[:, :1].min()) >= 64                                    # the second column of each lane
        if c.match == "perlayer" and c.L > 1 and c.nq > 3:
            assert not torch.equal(mq[:c.B], mq[c.B:2 * c.B])
    assert any(c.match == "high" and c.nq - max(c.n) >= 64 for c in P.COST_CASES)


def test_mask_and_q_cases_reach_every_band_and_scale():
    names = {c.name for c in P.MASK_CASES}
    assert all("mask_%dx%d_s%d" % (h, w, s) in names for h in P.MASK_HS for w in P.MASK_WS for s in P.MASK_SS) and "mask_9x160_s4" in names
    assert {P.bands(c) for c in P.MASK_CASES} == {(1, 1), (1, 2), (1, 7), (1, 8), (2, 1), (2, 8), (3, 1)}      # ragged, full and seam bands
    assert all(c.s * c.h * c.s * c.w <= 36 * 640 for c in P.CASES.values())
    for c in P.MASK_CASES:
        x = P.inputs(c.name)
        H, W = c.s * c.h, c.s * c.w
        m = x["masks"][0]
        assert bool(m[0].all()) and bool(m[1].any(1).all())                      # the whole image; a plane across every row (every band seam)
        assert [int(m[j].sum()) for j in range(2, 6)] == [1] * 4 and all(int(m[j][y, xx]) for j, (y, xx) in zip(range(2, 6), ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))))
        assert bool((x["mlog"] == 30).any()) or c.h * c.w < 4
    sweep = [c for c in P.MASK_CASES if c.name != "mask_9x160_s4"]
    for flag in (lambda c: c.pixel, lambda c: c.num_masks == 2.5, lambda c: bool(c.no_valid)):      # no flag follows s, h or w: every scale,
        for key, values in ((lambda c: c.s, P.MASK_SS), (lambda c: c.h, P.MASK_HS), (lambda c: c.w, P.MASK_WS)):      # every band shape and
            for v in values:                                                                         # h, w of 1 and 2 run with and without
                assert {flag(c) for c in sweep if key(c) == v} == {True, False}, v
    for key, values in ((lambda c: c.s, P.MASK_SS), (lambda c: c.h, P.MASK_HS), (lambda c: c.w, P.MASK_WS)):
        for v in values:
            assert {c.match for c in sweep if key(c) == v} == set(P.MATCHES), v
    for c in sweep:                                                             # the centre map's pixel at distance exactly 0 and the tied pairs
        x = P.inputs(c.name)
        assert len(x["tied"]["params"]) == 2 and len(x["tied"]["centers"]) == 1      # image 0 (n = 6) and the last image (n = 2)
        for key, tkey in (("params", "tparams"), ("centers", "tcenters")):
            assert all(torch.equal(x[key][i, q], x[tkey][b, j]) for i, q, b, j in x["tied"][key])
    hw = {c.s * c.h * c.s * c.w for c in P.CASES.values()}
    assert {48, 4096, 4097, 36 * 640} <= hw
    assert all(name in P.CASES for name in P.PADDED + P.CHAIN)


@pytest.mark.parametrize("group", ["cost", "q"] + ["mask_%d" % h for h in P.MASK_HS])
def test_input_conditions_hold_in_f64_and_f32(group):
    names = [n for n in P.CASES if n.startswith(group + ("x" if group.startswith("mask_") else "_"))]
    assert names
    for name in names:
        case = P.CASES[name]
        for dtype in (P.F64, P.F32):
            m = P.margins(name, dtype)
            assert m["gd"] >= P.GD_MARGIN and m["res"] >= P.RES_MARGIN and m["diff"] >= P.DIFF_MARGIN and m["norm"] >= P.NORM_MARGIN, (name, m)
            assert m["dist"] > P.DIST_MARGIN and m["zero_diff"] >= 3 and m["zero_dist"] >= (1 if case.pixel else 0), (name, m)
            for b, v in enumerate(m["valid"]):
                assert v == 0 if b in case.no_valid else (v > 0 or case.h * case.w * case.s ** 2 < 64), (name, m)      # cnt = 0 where the depth is tripled
                if case.n[b] == 1 and b not in case.no_valid:
                    assert v == case.s * case.h * case.s * case.w                # all pixels valid
            assert m["covered_twice"] > 0 or max(case.n) == 1
        x = P.inputs(name)
        assert all(bool((g == 0).any()) for g in x["gs"]) and bool((x["gs"][0] < 0).any())
        if case.s >= 2 and max(case.n) >= 6:                                     # a plane that is empty at the sampled resolution
            assert int(x["masks"][0, 5][::case.s, ::case.s].sum()) == 0 and int(x["masks"][0, 5].sum()) == 1


def test_f32_worst_is_what_the_restatement_measures():
    """also: the reference alone, restated in float32, sits inside the limit on every case (by the factor LIMIT_FACTOR)"""
    got = P.f32_worst()
    for fam, v in got.items():
        assert v <= 1.02 * P.F32_WORST[fam] and v >= 0.5 * P.F32_WORST[fam], (fam, v, P.F32_WORST[fam])
    assert set(got) == set(P.F32_WORST)


def _images():
    for name, (nq, nmax, images) in P.assign_launches().items():
        assert len(images) <= 24
        for b, (kind, C) in enumerate(images):
            yield "%s[%d]" % (name, b), kind, C.numpy()


def test_assignment_emulation_reproduces_scipys_optimum():
    shapes = set()
    for what, kind, C in _images():
        mq, mg, failed = P.assign_emulate(C)
        assert not failed, what
        total = P.check_match(mq, mg, C)
        q, j = P.scipy_assign(C)
        best = float(C.astype(np.float64)[q, j].sum())
        if kind == "continuous":
            assert P.optimum_gap(C) > 1e-6, what                                 # the optimum is unique ...
            assert np.array_equal(mq[j], q), what                                # ... and the emulation finds it
        else:
            assert total == best, (what, total, best)
        shapes.add(C.shape)
    assert {(128, 50), (50, 50), (1, 1), (128, 1)} <= shapes
    launches = P.assign_launches()
    assert all(len({C.shape[1] for _, C in images}) > 1 for images in (v[2] for k, v in launches.items() if k != "q1"))
    planted = launches["q128"][2][5][1].numpy()
    assert (P.assign_emulate(planted)[0] >= 64).all()                            # the optimum sits on the second column of each lane


def test_assignment_emulation_with_the_row_duals_dropped_leaves_the_optimum():
    worse = 0
    for what, kind, C in _images():
        if kind == "continuous":
            continue
        mq, mg, failed = P.assign_emulate(C, plant="row_duals")
        q, j = P.scipy_assign(C)
        best = float(C.astype(np.float64)[q, j].sum())
        got = float(C.astype(np.float64)[mq, np.arange(C.shape[1])].sum()) if not failed and (mq >= 0).all() and len(set(mq.tolist())) == len(mq) else float("inf")
        worse += got > best
    assert worse >= 2, worse


def test_assignment_emulation_stops_on_non_finite_costs():
    nq, nmax, images = P.refusal_launch()
    for (kind, fail), C in images:
        mq, mg, failed = P.assign_emulate(C.numpy())
        assert failed == (fail is not None), kind
        P.check_match(mq, mg, np.nan_to_num(C.numpy(), nan=0.0, posinf=1e30), upto=fail)
        if kind == "inf_column":
            assert 3 not in mq.tolist()


def test_corr_cases_are_what_they_claim():
    cases = P.corr_cases()
    assert any(max(len(c) for c in v[4]) == 1 for v in cases.values()) and any(max(len(c) for c in v[4]) > 256 for v in cases.values())
    assert {1, 128} <= {v[0] for v in cases.values()}
    nq, nmax, _, _, corrs = cases["small_nmax"]
    assert nmax < 50 and any(nmax <= a < 50 or nmax <= c < 50 for a, c in corrs[0])
    assert any(len(set(c)) < len(c) for v in cases.values() for c in v[4]) and any(not c for v in cases.values() for c in v[4])
    for name in cases:
        corrs, pad, m1, m2, idx1, idx2 = P.corr_inputs(name)
        want = R.plane_corr_matrix(corrs, idx1, idx2, cases[name][0])
        assert want.shape == (len(corrs), cases[name][0] + 1, cases[name][0] + 1)


def test_target_references_agree_with_the_restatement():
    for name in P.TARGET_CASES:
        masks, n = P.target_inputs(name)
        c64, p64 = R.prepare_targets(masks, n, P.F64)
        exact = P.exact_centroids(masks, n)
        for b in range(len(n)):
            for j in range(n[b]):
                assert abs(float(exact[b][j][0]) - float(c64[b, j, 0])) < 1e-12 and abs(float(exact[b][j][1]) - float(c64[b, j, 1])) < 1e-12
        assert float((P.centre_map_f32(masks, n, c64.float()).double() - p64).abs().max()) < 1e-5
    assert {(v[0], v[1]) for v in P.TARGET_CASES.values()} == {(1, 1), (3, 5), (24, 32), (36, 640)}
    masks, n = P.target_inputs("3x5", True)
    assert int(masks[0, 1].sum()) == 0 and P.exact_centroids(masks, n)[0][1] is None


@pytest.mark.parametrize("group", ["cost", "q"] + ["mask_%d" % h for h in P.MASK_HS])
def test_f32_emulation_of_the_kernels_order_stays_within_the_limit(group):
    for name in [n for n in P.CASES if n.startswith(group + ("x" if group.startswith("mask_") else "_"))]:
        ref, A = P.reference(name)
        got = P.emulate(name)
        assert torch.equal(got["q_valid"], ref["q_valid"]), name
        for fam, v in P.worst(got, ref, A, P.CASES[name]).items():
            assert v <= P.limit(fam), (name, fam, v / P.limit(fam))


@pytest.mark.parametrize("plant", [p for p in P.PLANTS if p != "row_duals"])
def test_a_planted_error_leaves_the_limit_on_every_case_that_reaches_it(plant):
    reached = [name for name in P.CASES if P.plant_reaches(plant, P.CASES[name])]
    assert len(reached) >= 9, (plant, reached)
    hidden = [name for name in reached if not P.plant_shows(name, plant)]
    assert not hidden, (plant, hidden)
