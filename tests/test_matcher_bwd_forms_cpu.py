"""CPU half of the matching head's backward sweep (tests/matcher_bwd_forms.py): the case lists reach the builds, lane-group widths, LDS
sizes and row-block counts they claim, the inputs meet the conditions the GPU half relies on, the committed float32 constants are what the
module measures, the float64 restatements reproduce the oracle and the signed Sinkhorn recursion reproduces autograd, a float32 emulation
of each kernel's own formulas stays within the limit, and the same emulation with one planted error does not."""
import pytest
import torch

from tests import matcher_bwd_forms as M

F64 = torch.float64


def _worst(family, key, got):
    return max(q for q, _ in M.worst_ratio(family, key, {k: got[k] for k in M.OUTPUTS[family]}).values())


# ---- case lists -----------------------------------------------------------------------------------------------------------------------
def test_attention_cases_reach_what_they_claim():
    assert M.ATT_SHAPES == ((1, 1), (1, 128), (128, 1), (2, 3), (50, 50), (64, 65), (121, 121), (122, 122), (128, 128))
    assert M.attention_lds_bytes(121, 121) <= 64 * 1024 < M.attention_lds_bytes(122, 122)                # the LDS opt-in edge
    assert M.attention_lds_bytes(128, 128) <= 160 * 1024 - 256
    tags = [k[2] for k in M.ATT_CASES]
    assert {(lq, lk) for lq, lk, t in M.ATT_CASES if t == "base"} == set(M.ATT_SHAPES) and {"peaked", "nolen", "h1"} <= set(tags)
    packed = padded = 0
    for key in M.ATT_CASES:
        c = M.attention_inputs(key)
        Lq, Lk = key[:2]
        assert 4 <= c["B"] <= 6 and c["heads"] == (1 if key[2] == "h1" else 8) and c["null_lens"] == (key[2] == "nolen")
        assert all(0 <= a <= Lq and 0 <= b <= Lk for a, b in c["lens"]) and c["lens"][0] == (Lq, Lk)
        if not c["null_lens"]:
            assert any(b == 0 and a > 0 for a, b in c["lens"]) and any(a == 0 and b > 0 for a, b in c["lens"])
        if key[2] == "base" and min(Lq, Lk) >= 2:
            assert any(a % 2 == 1 for a, _ in c["lens"]) and any(b % 2 == 0 and b for _, b in c["lens"]) and (1, Lk) in c["lens"] and (Lq, 1) in c["lens"]
        if key[2] == "peaked":
            assert any(a % 2 == 0 and a for a, _ in c["lens"]) and any(b % 2 == 1 for _, b in c["lens"])
            assert float(c["q"].std()) > 3.5 and float(c["k"].std()) > 3.5 and float(c["v"].std()) < 1.5
        if c["packed"]:
            assert c["q"].stride(0) == 768 and c["k"].data_ptr() == c["qkv"].data_ptr() + 4 * 256
        packed, padded = packed + c["packed"], padded + (c["out_pad"] > 0)
        d = c["dout"]
        assert (d < 0).any() and ((d.abs().sum(1) == 0).any() or d.shape[0] < 3)
    assert 0 < packed < len(M.ATT_CASES) and 0 < padded < len(M.ATT_CASES)


def test_peaked_attention_rows_hold_probabilities_that_underflow():
    c = M.attention_inputs((128, 128, "peaked"))
    q, k = c["q"][:128].view(128, 8, 32), c["k"][:128].view(128, 8, 32)
    s = torch.einsum("lhd,shd->lsh", q, k) * c["scale"]
    p = torch.exp(s - s.max(1, keepdim=True).values)
    assert (p == 0).any() and float(torch.softmax(s.double(), 1).max(1).values.median()) > 0.9


def test_layernorm_cases_reach_what_they_claim():
    assert M.LN_ROWS == (1, 3, 4, 5, 31, 32, 33, 64, 65, 257, 1025) and M.LN_RATIOS == (0.0, 2.5, 30.0)
    blocks = lambda r: (r + M.LN_BLOCK - 1) // M.LN_BLOCK
    assert sorted({blocks(r) for r in M.LN_ROWS}) == [1, 2, 3, 9, 33]
    idle = lambda r: (r - 1) % M.LN_BLOCK + 1 < 4                      # the last block has fewer rows than waves
    assert [r for r in M.LN_ROWS if idle(r)] == [1, 3, 33, 65, 257, 1025]
    for key in M.family_keys("layernorm"):
        c = M.layernorm_inputs(key)
        x = c["x"].double()
        ordinary = [r for r in range(c["rows"]) if r != 1 or c["rows"] < 3]
        ratio = x[ordinary].mean(1) / x[ordinary].std(1)
        assert abs(float(ratio.median()) - key[1]) < 0.35 + 0.05 * key[1] and float((ratio - key[1]).abs().max()) < 0.5 + 0.25 * key[1], (key, ratio)
        assert (c["gamma"] == 0).any() and (c["gamma"] < 0).any()
        if c["rows"] >= 3:
            assert float(x[1].std()) == 0 and float(x[1, 0]) != 0 and float(c["dy"][2].abs().sum()) == 0 and float(c["dy"][1].abs().sum()) > 0


def test_sinkhorn_cases_reach_every_build_and_lane_group_width():
    assert M.SINK_NQS == (1, 2, 7, 63, 64, 128)
    assert [M.sink_nt(nq) for nq in M.SINK_NQS] == [256, 256, 256, 256, 1024, 1024]
    assert M.SINK_PAIRS[63] == [(3, 3), (4, 2), (7, 7), (8, 8), (15, 15), (16, 1), (31, 31), (32, 32), (63, 63), (1, 63)]
    assert M.SINK_PAIRS[128] == [(15, 3), (16, 16), (31, 5), (32, 32), (63, 63), (64, 10), (127, 127), (128, 128), (128, 1), (1, 128)]
    assert [M.sink_tg(63, *p) for p in M.SINK_PAIRS[63]] == [64, 32, 32, 16, 16, 8, 8, 4, 4, 4]              # both sides of 4|5, 8|9, 16|17, 32|33
    assert [M.sink_tg(128, *p) for p in M.SINK_PAIRS[128]] == [64, 32, 32, 16, 16, 8, 8, 4, 4, 4]           # both sides of 16|17, 32|33, 64|65, 128|129
    assert [M.sink_tg(64, *p) for p in M.SINK_PAIRS[64]] == [64, 32, 32, 16, 16, 8, 8, 8, 8]
    assert (63 + 1) % 2 == 0 and (128 + 1) % 2 == 1                                                         # LD = R + 1 at nq = 63, LD = R at 128
    cases = M.sink_cases()
    for nq in M.SINK_NQS:
        assert {k[1] for k in cases if k[0] == nq and k[3] == "std"} == set(M.sink_iters(nq))
        assert {k[2] for k in cases if k[0] == nq} >= {1.0, -0.37, 0.0}
        pairs = M.sink_pairs(nq)
        assert (0, min(5, nq)) in pairs and (min(5, nq), 0) in pairs and all(max(p) <= nq for p in pairs)
    assert {k[0] for k in cases if k[3] == "none_selected"} == {7, 64} and {k[0] for k in cases if k[1] == 200} == {63, 128}


@pytest.mark.parametrize("nq", M.SINK_NQS)
def test_sinkhorn_inputs_meet_their_conditions(nq):
    c = M.sink_inputs(nq)
    pairs, R = c["pairs"], nq + 1
    last = len(pairs) - 1
    for b, (n1, n2) in enumerate(pairs):
        dead = torch.ones(R, R, dtype=torch.bool)
        if n1 and n2:
            dead[M._live_index(n1, nq)[:, None], M._live_index(n2, nq)[None]] = False
        assert not dead.any() or (c["gt"][b][dead] > 0).any(), b                       # bits outside the live region, to be ignored
        if n1 and n2:
            assert int(M._sel_mask(c, b).sum()) > 0 or b == last
    assert int(M._sel_mask(c, last).sum()) == 0 and min(pairs[last]) > 0                # the live pair with nothing selected
    assert float(c["dd"][last, pairs[last][0]:].abs().min() if pairs[last][0] < nq else 1.0) > 0       # noise outside the live blocks
    none = M.sink_inputs(7, "none_selected")
    assert all(int(M._sel_mask(none, b).sum()) == 0 for b, (n1, n2) in enumerate(none["pairs"]) if n1 and n2) and int(none["gt"].sum()) > 0


@pytest.mark.parametrize("key", M.sink_cases(), ids=str)
def test_sinkhorn_decision_margins(key):
    """In float64 and in the f32 restatement.  No score of nq = 1 can be positive after an iteration: the exponentials of the dustbin
    column sum to n1 = 1.  The launches with bin_score = -6 and those in which nothing is selected are not there for a positive score."""
    nq, iters, _, variant = key
    m = M.sink_margins(key)
    assert m["agree"] and m["score"] >= M.SCORE_MARGIN, m
    assert m["ntn_rt"] >= M.GEO_MARGIN and m["clamp"] >= M.GEO_MARGIN and m["angle"] >= M.ANGLE_MIN, m
    assert m["designated_angle"] < 0.1, m                                               # there the conditioning term carries the prior
    if variant == "std":
        assert m["dustbin_selected"] >= 1 and (m["positive"] >= 1 or (nq == 1 and iters >= 1)), m
    if variant == "neg_bin":
        c = M.sink_problem(key)
        ref, _ = M.reference("sinkhorn_fwd", key)
        assert any(bool(((M.live_block(ref["log_scores"][b], n1, n2, nq) <= 0) & M._sel_mask(c, b))[n1].any())
                   for b, (n1, n2) in enumerate(c["pairs"]) if n1 and n2)                # a gradient reaches the dustbin row


def test_embedding_loss_and_descriptor_dot_cases():
    assert [k[1] for k in M.EMB_CASES if k[0] == "hand"] == [1, 5, 300] and M.DOT_NQS == (1, 50, 128)
    for key in M.EMB_CASES:
        c = M.emb_inputs(key)
        sel = torch.cat([M._emb_selected(c, b, c["ls"]) for b in range(len(c["pairs"]))])
        assert (sel < 0).any() and float(sel.min()) > -1e29
        if key[0] == "hand":
            assert (sel == 0).any() and (sel > 0).any()
        if key != ("hand", 1):
            assert any(bool(((c["ls"][b] < -1e29) & (c["gt"][b] > 0)).any()) for b in range(len(c["pairs"])))
    assert M.dot_pairs(50) == [(50, 50), (1, 50), (50, 1), (0, 3), (3, 0), (49, 17)]
    for nq in M.DOT_NQS[1:]:
        c = M.dot_inputs(nq)
        assert all(float(c["G"][b, n1:].abs().min()) > 0 for b, (n1, n2) in enumerate(c["pairs"]) if n1 < nq)
        assert (c["G"] == 0).any() and (c["G"] < 0).any()


# ---- constants and references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(M.F32_WORST))
def test_f32_constants_are_what_the_module_measures(family):
    measured = M.f32_worst(family)
    assert 0.5 <= measured / M.F32_WORST[family] <= 2.0, (family, measured, M.F32_WORST[family])
    assert M.limit(family) == 8.0 * M.F32_WORST[family]


@pytest.mark.parametrize("nq", M.SINK_NQS)
def test_f64_sinkhorn_restatement_reproduces_the_oracle(nq):
    """The priors against oracle._geometric_dists, the potentials against oracle.log_sinkhorn."""
    from oracle import nopesac_oracle as O
    c = M.sink_problem((nq, 3, 1.0, "std"))
    with M._default_dtype(F64):
        for b, (n1, n2) in enumerate(c["pairs"]):
            if n1 == 0 or n2 == 0:
                continue
            p1, p2, cam = c["p1"][b, :n1].double(), c["p2"][b, :n2].double(), c["cam7"][b].double()
            ang, off = O._geometric_dists(p1, p2, cam[3:], cam[:3], 1e-10, 5.0)
            a, o, _, _ = M.priors(p1, p2, cam)
            assert float((a - ang).abs().max()) < (1e-5 if b == c["designated"] else 1e-9) and float((o.clamp(1e-10, 5.0) - off).abs().max()) < 1e-12
            Z = M.couplings(c["dd"][b, :n1, :n2].double(), p1, p2, cam, c["bin"].double(), F64)
            norm, lmu, lnu = M.marginals(n1, n2, F64)
            u, v = M.potentials(Z, lmu, lnu, 3)[-1]
            ref = O.log_sinkhorn(Z[:n1, :n2], c["bin"].double()[0], 3)
            assert float((Z + u[:, None] + v[None] - norm - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("key", [k for k in M.sink_cases() if k[1] != 200 or k[0] == 63], ids=str)
def test_signed_sinkhorn_recursion_reproduces_autograd(key):
    c = M.sink_problem(key)
    x = {k: c[k].double() for k in M.FLOATS["sinkhorn_bwd"]}
    ref, _ = M.reference("sinkhorn_bwd", key)
    got = M.sinkhorn_by_recursion(c, x, F64, signed=True)
    mags = M.sinkhorn_by_recursion(c, x, F64, signed=False)
    for k in ref:
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(float(mags[k].max()), 1e-300), (key, k)
        assert bool((mags[k] >= got[k].abs() * (1 - 1e-12)).all())


# ---- emulation and planted errors -----------------------------------------------------------------------------------------------------
EMU_WORST = {}


@pytest.mark.parametrize("family", sorted(M.F32_WORST))
def test_f32_emulation_of_the_kernel_formulas_stays_within_the_limit(family):
    for key in M.family_keys(family):
        w = M.worst_ratio(family, key, {k: v for k, v in M.EMULATE[family](key).items() if k in M.OUTPUTS[family]})
        EMU_WORST[family] = max(EMU_WORST.get(family, 0.0), max(q for q, _ in w.values()))
        assert all(q <= M.limit(family) for q, _ in w.values()), (family, key, w, M.limit(family))
    print(family, "emulation worst error / A", EMU_WORST[family], "limit", M.limit(family))


def _gradient_flows(key):
    ref, _ = M.reference("sinkhorn_bwd", key)
    return float(ref["d_desc_dot"].abs().max()) > 0


def _reaches(family, plant, key):
    """Whether the case reaches the faulty term."""
    if family == "attention":                          # a single live key: P = 1, dS = 0, dq = dk = 0, no odd key, l = 1
        return plant == "delta_dropped" or key[1] > 1
    if family == "layernorm":
        return plant != "block_partial_dropped" or key[0] > M.LN_BLOCK
    if family == "desc_dot":                           # a 1 x 1 block is its own transpose
        return plant == "div_16_dropped" or key > 1
    if family == "emb_loss":                           # the one full pair of ("hand", 1) has no dead region
        return plant != "dead_bits_counted" or key != ("hand", 1)
    nq, iters, g_loss, variant = key
    if not _gradient_flows(key):                       # g_loss = 0, nothing selected, or no selected score <= 0
        return False
    if plant in ("du_not_reset", "dv_without_sign"):
        return iters >= 2
    if plant == "v_t_for_v_t_minus_1":                 # (at 200 iterations v^t = v^(t-1) to rounding)
        return 2 <= iters <= 3
    if plant == "lnu_lmu_swapped":                     # the two dustbin marginals differ only where n1 != n2
        return iters >= 1 and nq >= 2
    if plant == "dustbin_row_left_out":                # see sink_cases: the dustbin row of dZ sums to zero from one iteration on
        return variant == "neg_bin"
    return True


@pytest.mark.parametrize("family,plant", [(f, p) for f in sorted(M.PLANTS) for p in M.PLANTS[f]])
def test_planted_errors_do_not_stay_within_the_limit(family, plant):
    keys = [k for k in M.family_keys(family) if _reaches(family, plant, k)]
    assert len(keys) >= 2
    for key in keys:
        assert _worst(family, key, M.EMULATE[family](key, plant)) > M.limit(family), (family, plant, key)
