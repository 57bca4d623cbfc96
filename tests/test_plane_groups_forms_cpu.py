"""CPU half of the view-group sweeps (tests/train_step_forms.py): the numpy restatement of the criterion's group normalisers against the
float64 criterion of tests/plane_criterion_ref.py run on each group alone, the point of the groups on numbers (the per-view mean differs
from the pooled 2B value once the views' plane counts differ), the cases' coverage, and the launchers' refusals, which need no GPU: the
C library checks its arguments before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import plane_criterion_forms as P
from tests import train_step_forms as T

# The restatement and the float64 criterion differ by the order of a handful of float64 operations per loss (a mean against a sum and
# a division): a few ulp of float64.  2^-40 relative is twelve bits of slack over that, and 2^-17 below float32's resolution.
REL = 2.0 ** -40


@pytest.mark.parametrize("name", list(T.CRITERION_CASES))
@pytest.mark.parametrize("kind", T.NUM_MASKS)
def test_group_normalisers_are_the_criterion_run_per_group(name, kind):
    case, G = T.CRITERION_CASES[name]
    x = T.criterion_inputs(name)
    _, per_group = T.num_masks_of(kind, G)
    img, last = T.image_sums(x, case)
    got = T.group_losses(img, last, case.n, G, per_group)
    for grp in range(G):
        sub, sub_case = T.group_slice(x, case, G, grp)
        want = T.reference_losses(sub, sub_case, T.F64, per_group[grp])
        err = np.abs(got[grp] - want) / np.maximum(np.abs(want), 1e-300)
        print("group-normalisers %s %s group %d: worst relative error %.3g" % (name, kind, grp, float(np.where(want == 0, np.abs(got[grp]), err).max())))
        assert np.all(np.where(want == 0, got[grp] == 0, err <= REL)), (name, kind, grp, got[grp], want)


def test_groups_are_not_the_pooled_batch():
    """The reason for the groups: with n1 != n2 matched planes in the two views, the pooled 2B value of loss_param_l1 is
    (n1 m1 + n2 m2) / (n1 + n2), the reference's per-view mean is (m1 + m2) / 2, and they differ."""
    case, G = T.CRITERION_CASES["g2_L1"]
    x = T.criterion_inputs("g2_L1")
    k = P.R.LOSS_NAMES.index("loss_param_l1")
    pooled = T.reference_losses(x, case)[k]
    m = [T.reference_losses(*T.group_slice(x, case, G, grp))[k] for grp in range(G)]
    n = [sum(case.n[:2]), sum(case.n[2:])]
    assert n[0] != n[1]
    assert abs(pooled - (n[0] * m[0] + n[1] * m[1]) / (n[0] + n[1])) <= REL * pooled
    assert abs(pooled - (m[0] + m[1]) / 2) > 1e-3 * pooled
    img, last = T.image_sums(x, case)
    assert abs(T.group_losses(img, last, case.n, G)[:, k].mean() - (m[0] + m[1]) / 2) <= REL * pooled
    assert abs(T.group_losses(img, last, case.n, 1)[0, k] - pooled) <= REL * pooled


def test_cases_cover_what_they_claim():
    for name, (case, G) in T.CRITERION_CASES.items():
        assert (case.nq, case.nmax, case.h, case.w, case.s) == (20, 8, 6, 8, 4) and case.B % G == 0 and case.L in (1, 3)
        Bg = case.B // G
        groups = [case.n[g * Bg:(g + 1) * Bg] for g in range(G)]
        assert any(all(v == 1 for v in grp) for grp in groups), name                       # a group of one-plane images
        assert any(all(v == case.nmax for v in grp) for grp in groups), name               # a group at the maximum
        assert len({sum(grp) for grp in groups}) == G, name                                # every group its own count
        empty = [all(g * Bg + b in case.no_valid for b in range(Bg)) for g in range(G)]
        assert sum(empty) == 1, name                                                        # one group without a valid loss_q pixel
        x = T.criterion_inputs(name)
        for grp in range(G):
            sub, sub_case = T.group_slice(x, case, G, grp)
            st = P.stats({**{k: sub[k].double() for k in P.FLOAT_INPUTS}, "masks": sub["masks"]}, sub_case, sub["match_q"])
            assert bool((st["q_stats"][:, 1] == 0).all()) == empty[grp], (name, grp)
    assert {(c.B, G) for c, G in T.CRITERION_CASES.values()} == {(4, 2), (6, 3)}
    keys = T.bn_cases()
    assert len(set(keys)) == len(keys)
    plain = {(C, G, rows) for form, G, rows, C, _, _, _ in keys if form == "plain"}
    assert plain == {(C, G, rows) for C in T.BN_CHANNELS for G in T.BN_GROUPS for rows in T.BN_ROWS}
    assert T.BN_ROWS == (2, T.RPS - 1, T.RPS, T.RPS + 1)
    for form in ("nhwc", "up"):
        assert {(C, G) for f, G, _, C, _, _, _ in keys if f == form} == {(C, G) for C in T.BN_CHANNELS for G in T.BN_GROUPS}
        assert {(relu, add) for f, _, _, C, relu, add, _ in keys if f == form and C == 64} == {(a, b) for a in (True, False) for b in (True, False)}
        assert {tag for f, _, _, _, _, _, tag in keys if f == form} == {"base", "slice"}


# ---- refusals: argument errors come before any HIP call ---------------------------------------------------------------------------------
def _criterion_args(B, groups, per_group=None):
    from nopesac_amd import _lib
    a = _lib.PlaneCriterionArgs()
    L, nq, nmax, h, w = 1, 4, 2, 2, 2
    keep = [torch.zeros(4096) for _ in range(2)]
    n_host = torch.ones(B, dtype=torch.int32)
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name != "num_masks_groups":
            setattr(a, name, keep[0].data_ptr())                                         # never dereferenced: the call is refused first
    a.L, a.B, a.nq, a.nmax, a.h, a.w, a.H, a.W, a.num_classes, a.groups = L, B, nq, nmax, h, w, 2 * h, 2 * w, 2, groups
    a.n_host = n_host.data_ptr()
    a.ws_floats = 1 << 30
    if per_group is not None:
        arr = (ctypes.c_float * len(per_group))(*per_group)
        keep.append(arr)
        a.num_masks_groups = ctypes.addressof(arr)
    return a, keep + [n_host]


@pytest.mark.parametrize("B,groups", [(4, 3), (6, 4), (2, 9), (16, 16), (4, -1)])
def test_criterion_entries_refuse_groups_that_do_not_divide_the_batch(B, groups):
    from nopesac_amd import _lib
    lib = _lib.load()
    a, keep = _criterion_args(B, groups)
    for entry in (lib.nopesac_plane_losses, lib.nopesac_plane_losses_backward):
        assert entry(ctypes.byref(a), None) == _lib.H.NPS_E_ARG
        assert b"groups" in lib.nopesac_last_error()


def test_bn_group_entries_refuse_before_any_launch():
    from nopesac_amd import _lib
    lib = _lib.load()
    E = _lib.H.NPS_E_ARG
    t = torch.zeros(4096)
    p = t.data_ptr()
    assert p % 16 == 0
    stats = lambda B, G, ws: lib.nopesac_bn_train_groups_stats_f32(p, 0, B, 1, 1, 4, 4, G, 1e-5, 0.1, p, p, p, None, None, p, ws, None)
    assert stats(6, 4, 1 << 20) == E and b"groups" in lib.nopesac_last_error()            # G does not divide the rows
    assert stats(6, 9, 1 << 20) == E and stats(6, -2, 1 << 20) == E                       # beyond NPS_BN_TRAIN_MAX_GROUPS, negative
    assert stats(6, 6, 1 << 20) == E and b"more than one value" in lib.nopesac_last_error()       # one row per group
    assert stats(600, 2, 2 * 2 * 2 * 4 - 1) == E and b"workspace" in lib.nopesac_last_error()     # 2 groups x 2 blocks x 2 x C, one short
    apply_ = lambda B, G: lib.nopesac_bn_train_groups_apply_f32(p, 1, B, 2, 2, 4, 4, G, p, p, p, p, 0, None, p, None)
    assert apply_(4, 3) == E and b"groups" in lib.nopesac_last_error()
    bwd = lambda B, G, sums: lib.nopesac_bn_train_groups_backward_f32(p, p, 0, B, 1, 1, 4, 4, G, p, p, p, p, 0, 1, p, p, p, sums, p, 1 << 20, None)
    assert bwd(6, 4, p) == E and b"groups" in lib.nopesac_last_error()
    assert bwd(6, 2, None) == E and b"null" in lib.nopesac_last_error()                    # G > 1 needs group_sums
    out = ctypes.c_int64(-1)
    size = lambda G, n, C: (lib.nopesac_bn_train_groups_workspace_floats(G, n, C, ctypes.addressof(out)), out.value)
    assert size(2, 514, 8) == (0, 2 * 2 * 2 * 8) and size(3, 768, 4) == (0, 3 * 1 * 2 * 4) and size(0, 257, 4) == size(1, 257, 4) == (0, 2 * 2 * 4)
    for n in (2, 255, 256, 257, 100000):                                                  # G <= 1: the ungrouped entry's size
        assert size(1, n, 12) == (0, lib.nopesac_bn_train_workspace_floats(n, 12))
    assert size(2, 513, 8) == (E, 0) and size(9, 18, 4) == (E, 0) and size(2, 0, 4) == (E, 0) and size(2, 4, 0) == (E, 0)
    assert lib.nopesac_bn_train_groups_workspace_floats(2, 4, 4, None) == E


def test_every_plane_trainer_takes_groups():
    """groups, default 1, on the criterion, the pyramid's forward and the four `losses` methods of the plane head's trainers"""
    import inspect

    from nopesac_amd import training as TR
    for fn in (TR.PlaneCriterion.__call__, TR.PlanePyramidTrainer.forward, TR.PlaneInstanceHeadsTrainer.losses, TR.PlaneDecoderTrainer.losses,
               TR.PlanePyramidTrainer.losses, TR.PlaneEncoderTrainer.losses):
        assert inspect.signature(fn).parameters["groups"].default == 1, fn.__qualname__


def test_wrappers_refuse_bad_groups_without_a_gpu():
    """ops checks groups against the batch before it looks at the device"""
    from nopesac_amd import ops
    from nopesac_amd.training import PlaneCriterion
    crit = PlaneCriterion()
    out = {"pred_logits": torch.zeros(4, 5, 2)}
    with pytest.raises(ops.OpsArgumentError, match="groups=3"):
        crit(out, {}, groups=3)
