"""CPU half of the plane criterion: the float64 restatement (tests/plane_criterion_ref.py) against the fixtures captured from the reference's
HungarianMatcher + SetCriterion (scripts/gen_plane_criterion_golden.py), the config weights, the argument checks of the new entry points
(no device needed) and the unique-optimum condition the GPU index comparisons rest on."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import plane_criterion_inputs as PI
from tests import plane_criterion_ref as R
from tests.util import GOLD, ROOT

OUT_KEYS = ("pred_logits", "pred_mask_logits", "pred_centers", "pred_params", "pixel_centers")


def _criterion(config=None):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.training import PlaneCriterion
    cfg = get_cfg()
    if config:
        cfg.merge_from_file(os.path.join(ROOT, "configs", config))
    return PlaneCriterion.from_cfg(cfg)


@pytest.mark.parametrize("name", PI.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    g = np.load(os.path.join(GOLD, "H_plane_criterion_%s.npz" % name))
    crit = _criterion()
    outputs, targets = PI.make(name)
    layers = [outputs] + list(outputs.get("aux_outputs", []))
    leaves = [(l, k, o[k].requires_grad_(True)) for l, o in enumerate(layers) for k in OUT_KEYS if k in o]
    losses, indices, _ = R.criterion(outputs, targets, crit.weights)
    assert sorted(losses) == list(g["loss_names"]) and len(losses) == 6 * len(layers) + 2
    for k, want in zip(g["loss_names"], g["loss_values"]):
        assert abs(float(losses[k].detach()) - want) <= 1e-9 * abs(want), (k, float(losses[k].detach()), want)
    for l, per in enumerate(indices):
        for b, (s, t) in enumerate(per):
            assert np.array_equal(s.numpy(), g["src_%d_%d" % (l, b)]) and np.array_equal(t.numpy(), g["tgt_%d_%d" % (l, b)]), (l, b)
    total = sum(v * crit.weight_dict[k] for k, v in losses.items())
    grads = torch.autograd.grad(total, [v for _, _, v in leaves])
    for (l, k, _), got in zip(leaves, grads):
        want = torch.from_numpy(g["grad_%d_%s" % (l, k)])
        assert float(want.abs().max()) > 0 and float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()), (l, k)


@pytest.mark.parametrize("config", [None, "inference_mp3d.yaml"])
def test_from_cfg_yields_the_reference_weights(config):
    c = _criterion(config)
    assert c.weights == dict(cost_class=1, cost_mask=20.0, cost_dice=1.0, cost_center=0.5, cost_param=0.5, cost_offset=0.01, cost_angle=0.0028,
                             eos_coef=0.1)
    base = {"loss_ce": 1, "loss_param_l1": 0.5, "loss_param_cos": 10.0, "loss_q": 1.0, "loss_center_ins": 0.5, "loss_center_pixel": 1.0,
            "loss_depth_pixel": 1.0, "loss_mask": 20.0, "loss_dice": 1.0}
    want = dict(base)
    for i in range(5):
        want.update({k + "_%d" % i: v for k, v in base.items()})
    assert c.weight_dict == want and c.num_classes == 1


def _args(**over):
    from nopesac_amd import _lib
    n = (ctypes.c_int32 * 2)(3, 2)
    a = _lib.PlaneCriterionArgs()
    a.L, a.B, a.nq, a.nmax, a.h, a.w, a.H, a.W, a.num_classes = 1, 2, 7, 5, 6, 8, 24, 32, 2
    a.n_host = a.n = ctypes.cast(n, ctypes.c_void_p)
    a.ws, a.ws_floats = 16, 1 << 40                       # never dereferenced: the checks come before any HIP call
    for k, v in over.items():
        setattr(a, k, v)
    return a, n


def test_entry_points_reject_bad_arguments_without_a_device():
    from nopesac_amd import _lib
    lib = _lib.load()
    err = lambda: lib.nopesac_last_error().decode()
    E = _lib.H.NPS_E_ARG
    bad_n0, bad_n9 = (ctypes.c_int32 * 2)(3, 0), (ctypes.c_int32 * 2)(3, 9)
    cases = [(dict(nq=0), "nq"), (dict(nq=129), "nq"), (dict(num_classes=3), "classes"), (dict(H=25), "scale"), (dict(W=64), "scale"),
             (dict(H=0, W=0), "scale"), (dict(ws_floats=3), "workspace"), (dict(n_host=ctypes.cast(bad_n0, ctypes.c_void_p)), "n[b]"),
             (dict(n_host=ctypes.cast(bad_n9, ctypes.c_void_p)), "n[b]"), (dict(nmax=51), "nmax"), (dict(L=9), "L=")]
    for entry in ("nopesac_plane_match_costs", "nopesac_plane_losses", "nopesac_plane_losses_backward"):
        fn = getattr(lib, entry)
        for over, word in cases:
            a, keep = _args(**over)
            assert fn(ctypes.byref(a), None) == E and word in err() and entry[len("nopesac_"):] in err(), (entry, over, err())
        a, keep = _args()
        assert fn(ctypes.byref(a), None) == E and "null" in err(), (entry, err())            # every pointer of a zeroed block is null
    n_ok, n_zero, n_big = (ctypes.c_int32 * 1)(3), (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(51)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    assert lib.nopesac_plane_assign(16, p(n_ok), 16, 1, 1, 129, 50, 16, 16, None) == E and "nq" in err()
    assert lib.nopesac_plane_assign(16, p(n_zero), 16, 1, 1, 7, 50, 16, 16, None) == E and "n[b]" in err()
    assert lib.nopesac_plane_assign(16, p(n_big), 16, 1, 1, 128, 50, 16, 16, None) == E and "n[b]" in err()
    assert lib.nopesac_plane_assign(16, p(n_ok), 16, 1, 1, 7, 50, None, 16, None) == E and "null output" in err()
    assert lib.nopesac_plane_targets(16, p(n_zero), 16, 1, 5, 8, 8, 16, 16, None) == E and "n[0]" in err()
    assert lib.nopesac_plane_targets(16, p(n_ok), 16, 1, 5, 8, 8, None, 16, None) == E and "null output" in err()
    assert lib.nopesac_plane_corr_matrix(16, 3, 16, 16, 2, 129, 50, 16, None) == E and "nq" in err()
    assert lib.nopesac_plane_corr_matrix(16, 3, 16, 16, 2, 50, 50, None, None) == E and "null output" in err()
    assert lib.nopesac_plane_criterion_workspace_floats(3, 32, 50, 50, 120, 160) > 0


@pytest.mark.parametrize("name", list(PI.CASES))
def test_the_optimum_of_every_gpu_case_is_unique(name):
    """scipy's assignment on the float64 cost matrix is unchanged under five draws of +-1e-4 uniform noise: no index comparison on the GPU
    hinges on a tie"""
    from scipy.optimize import linear_sum_assignment
    outputs, targets = PI.make(name)
    crit = _criterion()
    centers, _ = R.prepare_targets(targets["masks"], targets["n"], torch.float64)
    rng = np.random.default_rng(0)
    for o in [outputs] + list(outputs.get("aux_outputs", [])):
        for C in R.layer_costs(o, targets, centers, crit.weights):
            C = C.numpy()
            base = linear_sum_assignment(C)
            for _ in range(5):
                got = linear_sum_assignment(C + rng.uniform(-1e-4, 1e-4, C.shape))
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
