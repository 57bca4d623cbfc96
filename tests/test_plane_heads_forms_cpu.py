"""tests/plane_heads_forms.py and tests/plane_heads_ref.py proved on the CPU: the case list covers the shapes the kernels can go wrong
at, the float64 autograd equals the closed-form VJPs, F32_WORST is what the float32 restatement measures, planted errors exceed the
limit (the bound is sharp), the reference fixtures agree with the float64 restatement of the heads, and the criterion cases of
tests/test_plane_heads_training_gpu.py keep their float64 assignment under noise."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import plane_heads_forms as H
from tests import plane_heads_ref as PR
from tests.util import GOLD, rel_err


def test_cases_cover_the_shapes():
    rows, sizes, batches, flags = set(), set(), set(), set()
    for name, (L, B, nq, h, w, centre, splits, fl, seed) in H.CASES.items():
        assert 1 <= L <= 3 and 1 <= nq <= 128 and nq in (7, 50, 128) and L in (1, 3), name
        rows.add(L * nq); sizes.add((h, w)); batches.add(B); flags.update(fl)
    assert rows >= {7, 21, 50, 150, 384}
    assert sizes >= {(5, 7), (6, 8), (30, 40), (120, 160)} and batches >= {1, 3}
    for hw in ((5, 7), (6, 8), (30, 40)):
        assert {c[1] for c in H.CASES.values() if (c[3], c[4]) == hw} >= {1, 3}, hw
    assert H.CASES["q50_120x160"][:5] == (1, 1, 50, 120, 160)
    assert flags >= {"zero_rows", "slice"}
    assert len({c[-1] for c in H.CASES.values()}) == len(H.CASES)                  # one seed per case
    # a forced split count that leaves the last pixel range short / more ranges than 256-pixel blocks / ranges beyond the map
    L, B, nq, h, w, _, S, _, _ = H.CASES["q21_30x40_b3_short_split"]
    chunk = -(-(-(-h * w // S)) // 32) * 32
    assert 0 < h * w - (S - 1) * chunk < chunk
    L, B, nq, h, w, _, S, _, _ = H.CASES["q50_30x40_many_splits"]
    assert S > h * w // 256
    L, B, nq, h, w, _, S, _, _ = H.CASES["q7_6x8_empty_splits"]
    assert (S - 1) * 32 >= h * w
    assert {c[5] for c in H.CASES.values()} == {True, False}                        # with and without the centre rows
    x = H.inputs("q21_6x8_zero_rows")
    assert float(x["dM"][:, :, 1::2].abs().max()) == 0.0 and float(x["dM"][:, :, 0::2].abs().max()) > 0


@pytest.mark.parametrize("name", [n for n in H.CASES if n != "q50_120x160"])
def test_f64_autograd_equals_the_closed_forms(name):
    x = H.cast(H.inputs(name), H.F64)
    a, c = H.vjp_autograd(x), H.vjp_closed(x)
    assert set(a) == set(c)
    for k in a:
        assert float((a[k] - c[k]).abs().max()) <= 1e-12 * float(c[k].abs().max()), (name, k)
    ref = H.reference(name)
    for k in a:
        assert bool((ref["A"][k] > 0).all()) or "zero_rows" in H.CASES[name][7]
        assert bool((ref["S"][k] >= ref["g"][k].abs() * (1 - 1e-12)).all())


def test_f32_worst_is_what_the_restatement_measures():
    worst = H.measure_f32_worst()
    print(worst)
    for fam, v in worst.items():
        assert H.F32_WORST[fam] / 2 <= v <= H.F32_WORST[fam] * 2, (fam, v, H.F32_WORST[fam])
    assert all(H.limit(f) >= H.LIMIT_FACTOR for f in H.FAMILIES)


@pytest.mark.parametrize("plant,keys", [("drop_block", ("d_fold", "d_beta", "d_p1", "d_wc", "d_bc")), ("swap_layer", ("d_fold", "d_beta", "d_p1")),
                                        ("no_dbeta", ("d_beta",))])
def test_planted_errors_exceed_the_limit(plant, keys):
    fam_of = {k: f for f, ks in H.FAMILIES.items() for k in ks}
    checked = 0
    for name, case in H.CASES.items():
        if name == "q50_120x160" or (plant == "swap_layer" and case[0] < 2):
            continue
        r = H.ratios(H.f32_restatement(name, plant), name)
        for k in keys:
            if k in r:
                assert r[k] > 100 * H.limit(fam_of[k]), (plant, name, k, r[k])
                checked += 1
        for k in r:                                               # ... and what the plant does not touch stays inside
            if k not in keys:
                assert r[k] <= H.limit(fam_of[k]), (plant, name, k, r[k])
    assert checked >= 5


def test_fixtures_agree_with_the_f64_heads():
    """tests/golden/L_plane_heads_*.npz (written by scripts/gen_plane_heads_golden.py from the reference in training mode) against
    PR.heads in float64 with the synthetic checkpoint's tensors: rel_err < 3e-4, the gate of test_stages_gpu.py::test_plane_head."""
    from nopesac_amd.synth import synth_state_dict
    paths = sorted(glob.glob(os.path.join(GOLD, "L_plane_heads_*.npz")))
    assert paths, "no L_plane_heads_* fixture"
    for path in paths:
        assert os.path.getsize(path) < 382 * 1024, path
        g = {k: torch.from_numpy(v) for k, v in np.load(path).items()}
        nq = int(g["nq"])
        sd = {k: v.double() for k, v in synth_state_dict(nq).items() if k.startswith("sem_seg_head.") and v.is_floating_point()}
        L, B = g["hs"].shape[:2]
        assert L == 3 and g["hs"].shape[2:] == (nq, 256)
        out = PR.heads(sd, g["hs"].double(), g["p1_sub"].double())          # p1 at the [::4, ::4] positions only: the heads are per pixel
        for l in range(L):
            for k in ("pred_logits", "pred_params", "pred_centers"):
                assert rel_err(out[k][l], g[k][l].double()) < 3e-4, (path, l, k)
            assert rel_err(out["pred_mask_logits"][l], g["mask_logits_sub"][l].double()) < 3e-4, (path, l)
        assert rel_err(out["pixel_centers"], g["pixel_centers_sub"].double()) < 3e-4, path


@pytest.mark.parametrize("name", PR.CRITERION_CASES)
def test_criterion_cases_keep_their_match_under_noise(name):
    """The float64 assignment of every layer stays the same under five draws of 1e-4 relative noise on the heads' inputs, and the
    float32 restatement (given the float64 indices) agrees with float64 on d hs and d p1 - no case may be skipped."""
    from nopesac_amd.synth import synth_state_dict
    sd = synth_state_dict(7)
    r64 = PR.through_criterion(name, sd, torch.float64)
    assert r64["idx"] and all(len(layer) == PR.PI.CASES[name][1] for layer in r64["idx"])
    g = torch.Generator().manual_seed(77)
    for _ in range(5):
        noisy = PR.through_criterion(name, sd, torch.float64, noise=(1e-4, g), grads=False)
        for la, lb in zip(r64["idx"], noisy["idx"]):
            for (sa, ta), (sb, tb) in zip(la, lb):
                assert torch.equal(sa, sb) and torch.equal(ta, tb), name
    r32 = PR.through_criterion(name, sd, torch.float32, indices=r64["idx"])
    for k in ("hs", "p1"):
        e = float((r32["input_grads"][k].double() - r64["input_grads"][k]).abs().max())
        print(name, "d", k, "f32 vs f64", e, "max", float(r64["input_grads"][k].abs().max()))
        assert e <= 1e-5 * float(r64["input_grads"][k].abs().max()) and float(r64["input_grads"][k].abs().max()) > 0
