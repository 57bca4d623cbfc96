"""CPU half of the two-view training forms (tests/two_view_forms.py): the input conditions of every case, the restatement pinned to the
oracle, the recorded float32 figures re-measured, the sharpness of the bound (planted errors change the verdict), the new launchers'
argument checks through the C ABI (no device needed) and the random-pose sampler."""
import numpy as np
import pytest
import torch

from tests import two_view_forms as T


@pytest.mark.parametrize("nq", T.NQS)
def test_input_conditions_hold(nq):
    c, mg = T.inputs(nq), T.margins(nq)
    print(nq, c["m"].tolist(), c["redraws"], mg)
    assert mg["sig"] >= T.SIG_MARGIN and mg["norm"] > T.NORM_MARGIN and mg["dist"] > T.DIST_MARGIN, mg
    kinds = dict((k, b) for b, (k, _) in enumerate(c["kinds"]))
    ms = c["m"].tolist()
    assert ms[kinds["empty"]] == 0 and 1 in ms and nq in ms
    if nq >= 8:
        A = c["A"][kinds["fan"]]
        assert int(A.sum(1).max()) == 3 and int(A.sum(0).max()) == 3                       # one row in three pairs, one column in three pairs
        b = kinds["ragged"]
        n1, n2 = int(c["n1"][b]), int(c["n2"][b])
        assert n1 < nq and n2 < nq and bool(c["A"][b, n1:].any()) and bool(c["A"][b, :, n2:].any())
        assert int(c["seq"][b][0].max()) < n1 and int(c["seq"][b][1].max()) < n2
    if nq == 2:
        b = kinds["overflow"]
        assert int((c["A"][b] != 0).sum()) == 4 and ms[b] == 2
    z0, z1, z2 = T.expected_zero(nq)
    assert bool(z0.any()) and bool(z1.any())                                                # the zero contract is exercised


def test_restatement_is_pinned_to_the_oracle():
    """float64: the restated _Aux pass equals the oracle's (run under a float64 default dtype) to rounding.  float32: it agrees with
    oracle._refine_train_from_assignment in the seven losses and in both plane gradients within the oracle's own float32 error
    against its float64 self (the reference's own error; factor 2)."""
    from oracle import nopesac_oracle as O
    from nopesac_amd.synth import synth_state_dict
    c, sd = T.aux_case(), synth_state_dict(T.AUX_CASE["nq"])

    def oracle(dtype):
        with T._default_dtype(dtype):
            p1, p2 = c["planes1"].to(dtype).requires_grad_(True), c["planes2"].to(dtype).requires_grad_(True)
            sdd = {k: v.to(dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
            cv = lambda k: c[k].to(dtype)
            losses, _ = O._refine_train_from_assignment(sdd, p1, p2, cv("A"), cv("init_trans"), cv("init_rot"), cv("trans_feat"), cv("rot_feat"),
                                                        cv("gt_pose"), O.OracleConfig(num_queries=T.AUX_CASE["nq"], out_cam_type="soft"),
                                                        "initCamRef_Aux", T.AUX_CASE["weight"], "camera_head_list.0")
            g1, g2 = torch.autograd.grad(sum(losses.values()), [p1, p2])
        return {k: v.detach() for k, v in losses.items()}, g1, g2

    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    m64, m32 = T.aux_restated(torch.float64), T.aux_restated(torch.float32)
    assert set(m64[0]) == set(o64[0]) and len(m64[0]) == 7
    for k in o64[0]:
        assert abs(float(m64[0][k]) - float(o64[0][k])) <= 1e-12 * abs(float(o64[0][k])), k
        assert abs(float(m32[0][k]) - float(o32[0][k])) <= 1e-5 * abs(float(o32[0][k])), k                 # (f32: some hundred roundings)
    for i in (1, 2):
        assert T.scale_error(m64[i], o64[i]) <= 1e-12
        own = T.scale_error(o32[i], o64[i])
        print("view", i, "oracle f32 against its f64:", own, "restatement f32 against the oracle's f32:", T.scale_error(m32[i], o32[i]))
        assert T.scale_error(m32[i], o32[i]) <= 2 * own
        live = (o64[i].abs().sum(-1) > 0).sum()
        assert int(live) == 92                                                              # every matched row of the five pairs gets a gradient
    assert abs(float(o64[1].abs().max()) - 5.4e-2) < 1e-3 and abs(float(o64[2].abs().max()) - 7.4e-2) < 1e-3


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_recorded_f32_worst_is_current(family):
    got = T.f32_worst(family)
    print(family, got, T.F32_WORST[family])
    assert T.F32_WORST[family] / 2 <= got <= T.F32_WORST[family] * 2


def test_recorded_trainer_f32_error_is_current():
    got = T.trainer_f32_error()
    print(got, T.TRAINER_F32_ERR)
    for k, v in T.TRAINER_F32_ERR.items():
        assert v / 2 <= got[k] <= v * 2, (k, got[k], v)


@pytest.mark.parametrize("nq", T.NQS)
def test_reference_is_zero_where_the_contract_says_zero(nq):
    z0, z1, z2 = T.expected_zero(nq)
    ref, _ = T.reference("score_maps_geo", nq)
    assert bool((ref["g_geo_local"][z0] == 0).all())
    for w in T.WARPS:
        ref, _ = T.reference("geo_sequence", (nq, w))
        assert bool((ref["g_planes1"][z1] == 0).all()) and bool((ref["g_planes2"][z2] == 0).all())
        assert bool((ref["g_planes1"][~z1].abs().sum(-1) > 0).all())


@pytest.mark.parametrize("key", T.family_keys("geo_sequence"))
def test_emulation_passes_and_planted_errors_fail(key):
    """The float32 emulation of geo_sequence_bwd_kernel's formulas meets the limit; each planted error misses it wherever the case can
    show it: a missing flip under warp_in_ref, the fan summed once where a plane occurs in several pairs, the cut ignored at nq = 2."""
    nq, wir = key
    lim = T.limit("geo_sequence")
    worst = lambda plant: max(q for q, _ in T.worst_ratio("geo_sequence", key, T.emulate_geo_sequence(key, plant)).values())
    assert worst(None) <= lim
    shows = {"missing_flip": wir, "fan_summed_once": nq >= 8 or nq == 2, "cut_ignored": nq == 2}
    for plant in T.PLANTS:
        w = worst(plant)
        assert (w > lim) == shows[plant], (plant, w, lim)


def test_compact_restatement_properties():
    for nq, nmax in ((2, 2), (50, 20), (128, 50)):
        c = T.compact_case(nq, nmax)
        x_c, p_c, order, rank, bad = T.match_compact_np(c["x"], c["params"], c["match_q"], c["n"])
        assert not bad.any()
        for i, n in enumerate(c["n"]):
            assert (np.diff(order[i, :n]) > 0).all() and (order[i, n:] == -1).all() and (x_c[i, n:] == 0).all()
            assert sorted(order[i, :n].tolist()) == sorted(c["match_q"][i, :n].tolist())
            assert all(rank[i, order[i, r]] == r for r in range(n)) and int((rank[i] >= 0).sum()) == n
            assert np.array_equal(x_c[i, :n], c["x"][i, order[i, :n]]) and np.array_equal(p_c[i, :n], c["params"][i, order[i, :n]])
    mq = np.array([[0, 0], [5, 1], [0, 1]], np.int32)
    _, _, _, _, bad = T.match_compact_np(np.zeros((3, 2, 256), np.float32), np.zeros((3, 2, 3), np.float32), mq, np.array([2, 2, 3], np.int32))
    assert bad.tolist() == [1, 1, 1]


def test_new_launchers_refuse_bad_arguments_without_a_device():
    from nopesac_amd import _lib
    lib = _lib.load()
    err = lambda: lib.nopesac_last_error().decode()
    E = _lib.H.NPS_E_ARG
    P = 16                                                        # a non-null pointer that is never dereferenced: the checks come first
    geo = lambda **o: lib.nopesac_refine_score_maps_backward_geo(*[o.get(k, d) for k, d in (("geo", P), ("rr", P), ("tr", P), ("ir", P), ("it", P),
                                                                 ("m", P), ("B", 2), ("nq", 50), ("g1", P), ("g2", P), ("g3", P), ("out", P))], None)
    assert geo(nq=129) == E and "nq" in err() and "refine_score_maps_backward_geo" in err()
    assert geo(nq=0) == E and geo(B=0) == E
    assert geo(out=None) == E and "null output" in err()
    assert geo(g2=None) == E and "null input" in err()
    seq = lambda **o: lib.nopesac_geo_sequence_backward(*[o.get(k, d) for k, d in (("A", P), ("p1", P), ("p2", P), ("n1", P), ("n2", P), ("it", P),
                                                        ("ir", P), ("B", 2), ("nq", 50), ("w", 1), ("gl", P), ("ge", P), ("o1", P), ("o2", P))], None)
    assert seq(nq=129) == E and "nq" in err() and "geo_sequence_backward" in err()
    assert seq(B=0) == E and seq(o2=None) == E and "null output" in err()
    assert seq(ge=None) == E and "null input" in err()
    mc = lambda **o: lib.nopesac_match_compact(*[o.get(k, d) for k, d in (("x", P), ("p", P), ("mq", P), ("n", P), ("N", 4), ("nq", 50), ("nmax", 20),
                                                ("xc", P), ("pc", P), ("order", P), ("rank", P), ("bad", P))], None)
    assert mc(nq=129) == E and "nq" in err() and "match_compact" in err()
    assert mc(nmax=0) == E and "nmax" in err() and mc(nmax=129) == E and mc(N=0) == E
    assert mc(bad=None) == E and "null output" in err() and mc(mq=None) == E and "null input" in err()
    assert lib.nopesac_match_compact_backward(P, P, 4, 129, P, None) == E and "nq" in err()
    assert lib.nopesac_match_compact_backward(P, P, 4, 50, None, None) == E and "null output" in err()
    assert lib.nopesac_match_compact_backward(None, P, 4, 50, P, None) == E and "null input" in err()
    assert lib.nopesac_corr_compact(P, P, P, P, P, 2, 129, P, None) == E and "nq" in err()
    assert lib.nopesac_corr_compact(P, P, P, P, P, 0, 50, P, None) == E
    assert lib.nopesac_corr_compact(P, P, P, P, P, 2, 50, None, None) == E and "null output" in err()
    assert lib.nopesac_corr_compact(P, None, P, P, P, 2, 50, P, None) == E and "null input" in err()


def test_wrappers_refuse_shapes_and_dtypes_before_any_launch():
    """The Python wrappers check shapes and dtypes like their neighbours; CPU tensors are refused (there is no CPU path)."""
    from nopesac_amd import ops
    f = lambda *s: torch.zeros(*s)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    B, nq = 2, 5
    calls = [lambda: ops.ransac_score_maps_backward_geo(f(B, nq, 6), f(B, nq, 4), f(B, nq, 3), f(B, 4), f(B, 3), i32(B), f(B, nq + 1, nq),
                                                        f(B, nq + 1, nq), f(B, nq + 1, nq)),
             lambda: ops.geo_sequence_backward(f(B, nq, nq), f(B, nq, 3), f(B, nq, 3), i32(B), i32(B), f(B, 3), f(B, 4), f(B, nq, 6), f(B, nq, 8)),
             lambda: ops.match_compact(f(B, nq, 256), f(B, nq, 3), i32(B, 3), i32(B)),
             lambda: ops.match_compact_backward(f(B, nq, 256), i32(B, nq)),
             lambda: ops.corr_compact(torch.zeros(B, nq + 1, nq + 1, dtype=torch.uint8), i32(B, nq), i32(B, nq), i32(B), i32(B))]
    for call in calls:
        with pytest.raises(ops.OpsArgumentError):
            call()


def test_sample_rand_poses():
    from nopesac_amd.training import sample_rand_poses
    rot, trans = sample_rand_poses(64, seed=3, step=7)
    assert rot.shape == (64, 4) and trans.shape == (64, 3) and rot.dtype == trans.dtype == torch.float32
    assert float((rot.norm(dim=1) - 1).abs().max()) < 1e-6
    assert float(trans.abs().max()) < 2.5 and float(trans.abs().max()) > 2.0             # 192 uniforms on (-2.5, 2.5)
    angle = 2 * torch.acos(rot[:, 0].clamp(-1, 1))                                        # |rotation vector| <= 2.5 sqrt(3)
    assert float(angle.max()) <= 2.5 * 3 ** 0.5 + 1e-5 and float(angle.max()) > 2.0
    r2, t2 = sample_rand_poses(8, seed=3, step=7)                                         # a row depends on (seed, step, row) alone
    assert torch.equal(r2, rot[:8]) and torch.equal(t2, trans[:8])
    for other in (sample_rand_poses(8, seed=4, step=7), sample_rand_poses(8, seed=3, step=8)):
        assert not torch.equal(other[0], r2) and not torch.equal(other[1], t2)
    assert len({tuple(r.tolist()) for r in rot}) == 64
