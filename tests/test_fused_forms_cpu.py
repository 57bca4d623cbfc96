"""CPU half of the fused sweep (tests/fused_forms.py): for every case of the GPU sweep a float32 emulation of the kernel's algorithm - the
same rounding points, another summation order - stays within the per-element bound of the float64 reference (the bound is reachable by
correct f32 arithmetic), the same emulation with one planted arithmetic error per kernel feature exceeds it (negative controls; nothing
is planted in a kernel), and the inputs keep every ReLU / LeakyReLU pre-activation and every pool decision off its margin."""
import pytest
import torch

from tests import fused_forms as FF

WORST = {}


def _note(fam, q, case):
    if q > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (q, case)


# ---------------------------------------------------------------------------------------------------------------------------- stem
_stem_id = lambda c: "%dx%d_B%d_%s%s" % (c[0], c[1], c[2], "pos" if c[3] > 0 else "neg", "_frac" if c[4] else "")


@pytest.mark.parametrize("case", FF.stem_cases(), ids=_stem_id)
def test_stem_emulation_within_bound_and_inputs_off_margin(case):
    c = FF.stem_case(*case)
    H, W, B = case[:3]
    CH, CW, PH, PW = FF.stem_dims(H, W)
    zmin, gmin = FF.stem_margin(c)
    assert zmin > FF.MARGIN and gmin > FF.MARGIN, (zmin, gmin)
    if not case[4]:
        assert bool((c.raw == c.raw.round()).all()) and 0 <= float(c.raw.min()) and float(c.raw.max()) <= 255      # 8-bit pixel values
    for build in (0, 1, 2):
        ref = FF.stem_reference(c, build)
        y = FF.stem_emulate(c, build)
        assert y.shape == ref.v.shape == ref.E.shape == (B, PH, PW, 64)          # every element is compared
        q = FF.stem_ratio(y, ref)
        _note("stem build %d" % build, q, _stem_id(case))
        assert q <= 1.0, (build, q)
    assert torch.equal(FF.stem_emulate(c, 0), FF.stem_emulate(c, 1))              # preprocess + stem and the raw stem: the same bits


# fault -> the cases of the sweep that reach the feature (seams need a second tile column / row; the pad value only matters to build 2)
STEM_FAULT_CASES = {
    "outside_conv_in_pool": [(7, 7, 1, 1, False), (13, 157, 1, 1, False), (13, 161, 1, 1, False), (17, 33, 3, 1, False)],   # positive shifts: relu(shift) > 0 outside
    "pad_zero": [(7, 7, 1, 1, False), (8, 9, 1, -1, False), (100, 172, 1, -1, False), (8, 9, 1, 1, True)],
    "kw7_tap_nonzero": [(7, 7, 1, 1, False), (8, 9, 1, -1, False), (17, 33, 1, -1, False)],
    "seam_col_20": [(13, 157, 1, 1, False), (13, 161, 1, -1, False), (13, 161, 1, 1, False), (100, 172, 1, -1, False)],
    "seam_row_4": [(17, 33, 1, 1, False), (17, 33, 1, -1, False), (100, 172, 1, -1, False)],
}


@pytest.mark.parametrize("fault", FF.STEM_FAULTS)
def test_stem_planted_error_exceeds_bound(fault):
    for case in STEM_FAULT_CASES[fault]:
        assert case in FF.stem_cases()
        c = FF.stem_case(*case)
        for build in ((2,) if fault == "pad_zero" else (0, 1, 2)):
            q = FF.stem_ratio(FF.stem_emulate(c, build, fault), FF.stem_reference(c, build))
            print("control stem %-22s %-18s build %d  worst / tol %.3g" % (fault, _stem_id(case), build, q))
            assert q > 1.0, (fault, case, build, q)


# ---------------------------------------------------------------------------------------------------------------------------- pose-net
@pytest.mark.parametrize("case", FF.PB_CASES + FF.PB_ISO_CASES, ids=lambda c: "B%d_%s" % c)
def test_posenet_emulation_within_bound_and_inputs_off_margin(case):
    c = FF.pb_case(*case)
    assert FF.pb_margin(c) > FF.MARGIN
    live = FF._pb_live(case[1])
    for br in range(2):
        x = c.x[br].float()
        assert bool((x[:, ~live] == 0).all()) and bool((x[:, live] != 0).any())
    ref = FF.pb_forward(c)
    ys = FF.pb_forward(c, torch.float32)
    for y, r in zip(ys, ref):
        assert y.shape == r.v.shape == (case[0], 2, 3, 128)
    q = FF.pb_ratio(ys, ref)
    _note("pose-net branch tail" + (", one layer" if case in FF.PB_ISO_CASES else ""), q, "B%d_%s" % case)
    assert q <= 1.0, q
    if case in FF.PB_ISO_CASES and not case[1].endswith("mixed"):              # a band of 1e-3 of the value at most, on most elements
        tol = FF.out_tol(ref[0].v, ref[0].E, torch.float32)
        assert float((tol / ref[0].v.abs()).median()) < 1e-3


@pytest.mark.parametrize("fault", sorted(FF.PB_ISO_FAULTS))
def test_posenet_small_planted_error_at_one_layer_exceeds_bound(fault):
    """One wrong channel or pixel at the far corner of a layer's input, 2 % on its input, one stale channel in its top halo row: each of
    the five layers, on the routing that carries the affected output pixels to the output."""
    for case in FF.PB_ISO_CASES:
        routing = FF.PB_ISO_FAULTS[fault]
        if routing is not None and not case[1].endswith(routing):
            continue
        c = FF.pb_case(*case)
        q = FF.pb_ratio(FF.pb_forward(c, torch.float32, fault), FF.pb_forward(c))
        print("control pose-net %-30s %-12s worst / tol %.3g" % (fault, case[1], q))
        assert q > 1.0, (fault, case, q)


@pytest.mark.parametrize("fault", FF.PB_FAULTS)
def test_posenet_planted_error_exceeds_bound(fault):
    for case in FF.PB_CASES:
        c = FF.pb_case(*case)
        q = FF.pb_ratio(FF.pb_forward(c, torch.float32, fault), FF.pb_forward(c))
        print("control pose-net %-30s B%d_%-7s worst / tol %.3g" % ((fault,) + case + (q,)))
        assert q > 1.0, (fault, case, q)


# ---------------------------------------------------------------------------------------------------------------------------- MLP chain
@pytest.mark.parametrize("name", sorted(FF.MLP_CASES))
def test_mlp_emulation_within_bound_and_inputs_off_margin(name):
    c = FF.mlp_case(name)
    zs = FF.mlp_preacts(c)
    assert len(zs) == sum(1 for l in c.layers if l[1] in ("relu", "leaky"))
    assert all(float(z.abs().min()) > FF.MARGIN for z in zs)
    bufs = FF.mlp_emulate(c)
    q, per = FF.mlp_ratio(c, bufs)
    assert [l for l, _ in per] == [l for l, lay in enumerate(c.layers) if lay[2] is not None] and c.layers[-1][2] is not None
    for l, (N, act, tap, restart, bias) in enumerate(c.layers):
        if tap is not None:
            assert bufs[l][1].shape == (c.rows, N)                                # every element of every tap is compared
    _note("mlp chain", q, name)
    assert q <= 1.0, (name, per)


def test_mlp_cases_reach_every_path_of_the_issue():
    cs = FF.MLP_CASES.values()
    assert {1, 31, 32, 33, 65} <= {c.rows for c in cs}
    assert {1, 32, 33, 256, 257, 512, 513, 1024, 288, 800} <= {l[0] for c in cs for l in c.layers}
    pairs = set()
    for c in cs:
        k = c.kx + c.kb
        for (N, act, tap, restart, bias) in c.layers:
            k = c.kx + c.kb if restart else k
            pairs.add((k, FF.mlp_tpw(N)))
            k = N
    assert {(512, 1), (513, 1), (256, 2), (257, 2), (128, 4), (129, 4), (1280, 4), (1, 1), (3, 2), (50, 4)} <= pairs
    assert max(len(c.layers) for c in cs) == 12
    assert {1, 7} <= {c.rows_per for c in cs if c.kb} and any(c.kb and c.rows_per > c.rows for c in cs)
    assert any(c.x_off % 4 and c.kx % 2 for c in cs)
    assert {"none", "relu", "leaky", "sigmoid"} == {l[1] for c in cs for l in c.layers}
    assert {2, 3} <= {1 + sum(l[3] for l in c.layers) for c in cs}
    assert any(l[2] is not None and l[2] % 4 for c in cs for l in c.layers)


# fault -> cases with the feature (a narrow layer with K > 64; a broadcast prefix; a restart; a ragged last tile; N no multiple of 32)
MLP_FAULT_CASES = {
    "ksplit_partial_dropped": ["n_edges_k50", "k512_n256", "k513_n256", "k256_n512", "k257_n512", "twelve_layers"],
    "bcast_row_modulo": ["bcast_rows_per_1", "bcast_rows_per_7", "restart_three_stacks"],
    "restart_reads_previous": ["restart_two_stacks", "restart_three_stacks"],
    "rows_beyond_rows_leak": ["n_edges_k50", "n_edges_k3", "k1_one_row", "k128_n1024", "bcast_rows_per_7"],
    "tap_columns_past_n": ["n_edges_k50", "k256_n512", "twelve_layers", "restart_two_stacks"],
}


@pytest.mark.parametrize("fault", FF.MLP_FAULTS)
def test_mlp_planted_error_exceeds_bound(fault):
    for name in MLP_FAULT_CASES[fault]:
        c = FF.mlp_case(name)
        q = FF.mlp_ratio(c, FF.mlp_emulate(c, fault))[0]
        print("control mlp %-26s %-22s worst / tol %.3g" % (fault, name, q))
        assert q > 1.0, (fault, name, q)


# ---------------------------------------------------------------------------------------------------------------------------- mask head
_mh_id = lambda c: "B%d_%dx%d_nq%d" % c


@pytest.mark.parametrize("case", FF.MH_CASES, ids=_mh_id)
def test_mask_head_emulation_within_bound_and_inputs_off_margin(case):
    B, H, W, nq = case
    c = FF.mh_case(*case)
    assert FF.mh_margin(c) > FF.MARGIN
    ref = FF.mh_reference(c)
    prob, p1 = FF.mh_emulate(c)
    logit, _ = FF.mh_emulate(c, sigmoid=False)
    assert prob.shape == logit.shape == ref.prob.shape == ref.logit.shape == (B, H, W, nq) and p1.shape == ref.p1.shape == (B, H, W, 256)
    for fam, q in (("mask head prob", FF.mh_ratio(ref, prob=prob)), ("mask head logit", FF.mh_ratio(ref, logit=logit)),
                   ("mask head p1", FF.mh_ratio(ref, p1=p1)), ("mask head GEMM on own p1", FF.mh_own_p1_ratio(c, p1, prob=prob, logit=logit))):
        _note(fam, q, _mh_id(case))
        assert q <= 1.0, (fam, q)


# fault -> cases with the feature (a t1 with more than one row / column; more than one image; the 128-plane build)
MH_FAULT_CASES = {
    "clamp_last_row": [(1, 64, 2, 50), (1, 64, 6, 64), (1, 8, 48, 66), (1, 16, 32, 128)],
    "clamp_last_col": [(1, 2, 64, 2), (1, 64, 6, 64), (1, 8, 48, 66), (3, 16, 32, 50)],
    "bias_of_image_0": [(3, 16, 32, 50), (3, 8, 48, 128)],
    "planes_64_up_dropped": [(1, 8, 48, 66), (1, 16, 32, 128), (3, 8, 48, 128)],
    "planes_64_up_duplicated": [(1, 8, 48, 66), (1, 16, 32, 128), (3, 8, 48, 128)],
    "p1_not_rounded": [(1, 64, 6, 64), (1, 16, 32, 128), (3, 16, 32, 50)],
}


@pytest.mark.parametrize("fault", FF.MH_FAULTS)
def test_mask_head_planted_error_exceeds_bound(fault):
    for case in MH_FAULT_CASES[fault]:
        assert case in FF.MH_CASES
        c = FF.mh_case(*case)
        ref = FF.mh_reference(c)
        prob, p1 = FF.mh_emulate(c, fault)
        logit, _ = FF.mh_emulate(c, fault, sigmoid=False)
        qp, ql, q1 = FF.mh_ratio(ref, prob=prob), FF.mh_ratio(ref, logit=logit), FF.mh_ratio(ref, p1=p1)
        print("control mask head %-24s %-18s prob %.3g logit %.3g p1 %.3g" % (fault, _mh_id(case), qp, ql, q1))
        assert qp > 1.0 and ql > 1.0, (fault, case, qp, ql)
        if fault.startswith("clamp"):
            assert q1 > 1.0, (fault, case, q1)
        else:                                                  # a fault of the mask GEMM: also against float64 on the emulation's own p1
            qo = FF.mh_own_p1_ratio(c, p1, prob=prob, logit=logit)
            print("        on own p1 %.3g" % qo)
            assert qo > 1.0, (fault, case, qo)


def test_zz_worst_ratio_per_family(capsys):
    with capsys.disabled():
        print("\nfused sweep, CPU float32 emulations: worst |emulation - f64| / tolerance per family")
        for fam in sorted(WORST):
            print("  %-24s %.3f  %s" % ((fam,) + WORST[fam]))
    assert WORST and all(q <= 1.0 for q, _ in WORST.values())
