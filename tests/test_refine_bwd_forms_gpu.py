"""GPU half of the camera head's backward sweep (tests/refine_bwd_forms.py): the four geometry kernels of csrc/refine_bwd.hip through the
raw library, every element of every output against the float64 VJP within limit x (2^-24 S + C) - nothing normalised by a tensor
maximum - at nq = 1 .. 128 (B = 1, 64, 65 for the two loss kernels).  Outputs are NaN-prefilled with a guard tail: every element must be
written, the tail must stay; exact zeros where the header promises them; two launches give the same bits; the pair with m = 0 does not
change what the other pairs get."""
import pytest
import torch

from tests import refine_bwd_forms as R

pytestmark = pytest.mark.gpu
WORST = {}           # (kernel, output) -> (worst error / (limit x A), case)
TAIL = 64


def _note(family, w, case):
    for k, (q, i) in w.items():
        q /= R.limit(family)
        if q > WORST.get((family, k), (-1.0, ""))[0]:
            WORST[(family, k)] = (q, "%s [%d]" % (case, i))


def _raw(name, *args):
    from nopesac_amd import ops
    lib = ops._L()
    rc = getattr(lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._stream())
    assert rc == 0, (name, rc, lib.nopesac_last_error())


def _launch(name, args, shapes, device):
    """One call on NaN-prefilled outputs with a guard tail -> the outputs (device tensors); the tails must still be NaN."""
    bufs = [torch.full((int(torch.Size(s).numel()) + TAIL,), float("nan"), device=device, dtype=torch.float32) for s in shapes]
    outs = [b[:b.numel() - TAIL].view(*s) for b, s in zip(bufs, shapes)]
    _raw(name, *args, *outs)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[-TAIL:]).all()), name + ": wrote past the end of an output"
    return outs


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(family, key, names, outs, rows, case):
    got = {k: (o if rows is None else o[rows]).cpu() for k, o in zip(names, outs)}
    for k, v in got.items():
        assert not bool(torch.isnan(v).any()), (case, k, "an element was not written")
    w = R.worst_ratio(family, key, got)
    with_limit = {k: (q / R.limit(family), i) for k, (q, i) in w.items()}
    print("%s %s: error / (limit x A) %s" % (family, case, {k: "%.3f" % q for k, (q, _) in with_limit.items()}))
    _note(family, w, case)
    assert all(q <= R.limit(family) for q, _ in w.values()), (case, w, R.limit(family))
    return got


@pytest.mark.parametrize("nq", R.NQS)
def test_score_maps_backward_against_f64(nq, device):
    c = R.geometry_inputs(nq)
    B = len(c["ms"])
    d = lambda *ks: [c[k].to(device) for k in ks]
    args = d("geo_local", "rot_raw", "trans_raw", "init_rot", "init_trans", "m") + [B, nq] + d(*R.FAMILIES["score_maps"]["cots"])
    shapes = [(B, nq, 4), (B, nq, 3), (B, 4), (B, 3)]
    outs = _launch("nopesac_refine_score_maps_backward", args, shapes, device)
    again = _launch("nopesac_refine_score_maps_backward", args, shapes, device)
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    got = _judge("score_maps", nq, R.FAMILIES["score_maps"]["out"], outs, None, "nq%d" % nq)      # (the m = 0 pair is judged like any other)
    for b, h in c["no_cotangent"]:                                                                  # no cotangent: exactly zero
        rot, tr = (got["g_init_rot"][b], got["g_init_trans"][b]) if h == 0 else (got["g_rot_raw"][b, h - 1], got["g_trans_raw"][b, h - 1])
        assert float(rot.abs().sum() + tr.abs().sum()) == 0, (nq, b, h)


VOTE_IN = ("sf_rot", "sf_trans", "reg_rot_w", "reg_rot_b", "reg_trans_w", "reg_trans_b", "init_rot_feat", "init_trans_feat", "fused_rot", "fused_trans",
           "rots_w", "rots_b", "trans_w", "trans_b")
PER_PAIR = ("sf_rot", "sf_trans", "init_rot_feat", "init_trans_feat", "fused_rot", "fused_trans", "m") + R.FAMILIES["vote"]["cots"]


@pytest.mark.parametrize("nq", R.NQS)
def test_vote_backward_against_f64(nq, device):
    c = R.geometry_inputs(nq)
    B, NH = len(c["ms"]), nq + 1
    n = B - 1                                                                                       # the pair with m = 0 is the last one

    def run(pairs):
        d = lambda *ks: [(c[k][:pairs].contiguous() if k in PER_PAIR else c[k]).to(device) for k in ks]
        shapes = [(pairs, NH, 64), (pairs, NH, 64), (pairs, 256), (pairs, 256), (pairs, nq, 256), (pairs, nq, 256), (pairs, 4, 256), (pairs, 4),
                  (pairs, 3, 256), (pairs, 3), (pairs, 64), (pairs, 1), (pairs, 64), (pairs, 1)]
        return _launch("nopesac_refine_vote_backward", d(*VOTE_IN) + d("m") + [pairs, nq] + d(*R.FAMILIES["vote"]["cots"]), shapes, device)
    outs, again, without = run(B), run(B), run(n)
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    assert all(_same_bits(a[:n], b) for a, b in zip(outs, without)), "the pair with m = 0 changed what the other pairs get"
    got = _judge("vote", nq, R.VOTE_OUT, outs, slice(0, n), "nq%d" % nq)
    for b, m in enumerate(c["ms"][:n]):
        for k in ("g_fused_rot", "g_fused_trans"):
            assert float(got[k][b, m:].abs().sum()) == 0, (nq, m, k)
        for k in ("g_sf_rot", "g_sf_trans"):
            assert float(got[k][b, m + 1:].abs().sum()) == 0, (nq, m, k)


@pytest.mark.parametrize("B", R.LOSS_BS)
@pytest.mark.parametrize("nq", R.NQS)
def test_losses_backward_against_f64(nq, B, device):
    c = R.loss_inputs(nq, B)
    NH = nq + 1
    d = lambda *ks: [c[k].to(device) for k in ks]
    head = d("pred_rot", "pred_trans", "avg_rot", "avg_trans", "rots_all", "trans_all", "score_rot", "score_trans")
    tail = d("gt_pose", "g_loss") + [B, nq, c["weight"]]
    shapes = [(B, 4), (B, 3), (B, 4), (B, 3), (B, NH), (B, NH), (B, NH, nq)]
    run = lambda m: _launch("nopesac_refine_losses_backward", head + [m.to(device)] + tail, shapes, device)
    outs, again = run(c["m"]), run(c["m"])
    live = c["live"].to(device)
    assert all(_same_bits(a[live], b[live]) for a, b in zip(outs, again))
    if B > 1:                                                       # the same launch with a live pair in the place of the empty one
        m1 = c["m"].clone()
        m1[1] = 1
        assert all(_same_bits(a[live], b[live]) for a, b in zip(outs, run(m1))), "the pair with m = 0 changed what the other pairs get"
    got = _judge("losses", (nq, B), R.FAMILIES["losses"]["out"], outs, live, "nq%d B%d" % (nq, B))
    rows = torch.arange(len(c["live"]))
    for k, pick in (("g_score_rot", c["hr"]), ("g_score_trans", c["ht"])):
        off = got[k].clone()
        off[rows, pick] = 0.0
        assert float(off.abs().sum()) == 0, (nq, B, k)
    off = got["g_l2_dist"].clone()
    off[:, torch.arange(1, NH), torch.arange(nq)] = 0.0
    assert float(off.abs().sum()) == 0, (nq, B)


@pytest.mark.parametrize("layout", ["views_of_pose", "dense"])
@pytest.mark.parametrize("eps", R.TRANS_EPS)
@pytest.mark.parametrize("B", R.LOSS_BS)
def test_camera_pose_loss_backward_against_f64(B, eps, layout, device):
    c = R.pose_inputs(B, eps)
    pose = c["pose"].to(device)
    gt_t, gt_q = pose[:, 0:3], pose[:, 3:7]
    if layout == "dense":
        gt_t, gt_q = (t.clone(memory_format=torch.contiguous_format) for t in (gt_t, gt_q))
    assert (gt_t.stride(0), gt_q.stride(0)) == ((7, 7) if layout == "views_of_pose" else (3, 4))
    args = [c["est_trans"].to(device), c["est_rot"].to(device), gt_t, gt_t.stride(0), gt_q, gt_q.stride(0), B, eps, c["weight"], c["g_out"].to(device)]
    shapes = [(B, 3), (B, 4), (B, 3), (B, 4)]
    outs = _launch("nopesac_camera_pose_loss_backward", args, shapes, device)
    again = _launch("nopesac_camera_pose_loss_backward", args, shapes, device)
    assert all(_same_bits(a, b) for a, b in zip(outs, again))
    got = _judge("pose_loss", (B, eps), R.FAMILIES["pose_loss"]["out"], outs, None, "B%d eps%g %s" % (B, eps, layout))
    if B > 2 and eps == 0.0:                                        # the estimate equals its target: every gradient exactly zero
        assert all(float(v[2].abs().sum()) == 0 for v in got.values())


def test_zz_worst_ratio_per_kernel_and_output(capsys):
    with capsys.disabled():
        print("\ncamera head backward sweep: worst |kernel - f64 VJP| / (limit x (2^-24 S + C)) per kernel and output")
        for fam, k in sorted(WORST):
            q, case = WORST[(fam, k)]
            print("  %-11s %-18s %.3f  %s   (limit %.3g)" % (fam, k, q, case, R.limit(fam)))
    assert len({f for f, _ in WORST}) == len(R.FAMILIES) and all(q <= 1.0 for q, _ in WORST.values())
