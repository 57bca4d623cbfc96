"""The ops wrappers of the training path (nopesac_amd/ops.py: the backward kernels of csrc/refine_bwd.hip and csrc/matcher_bwd.hip, the
optimiser and the gradient clip) at the smallest shapes at which their plumbing can go wrong:
 (a) each wrapper gives, bit for bit, what the same entry point gives when it is called through the raw library with the same buffers
     (the kernels are deterministic and use no atomics);
 (b) each wrapper refuses, with OpsArgumentError and before the library is reached, a tensor of another dtype, int64 lengths, a gt_corr
     without the dustbin row / column, a strided tensor, a tensor one element short and a moment buffer of another size."""
from collections import namedtuple

import pytest
import torch

from nopesac_amd import _lib, ops

pytestmark = pytest.mark.gpu

# fn(*args): the wrapper (through an adapter where it takes dicts / keywords); raw(*args): the same entry point through ops._L() -> the same
# tensors, in the same order; free: the positions of tensors whose element count nothing else fixes (they may be any size); run(*args):
# what (a) compares with raw where that is more than one call of fn (in-place updates run on copies, twice)
Case = namedtuple("Case", "fn args raw free run", defaults=((), None))


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _raw(name, *args):
    """The entry point `name` of the raw library on the current stream; tensors go in as their device address."""
    lib = ops._L()
    rc = getattr(lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._stream())
    assert rc == 0, (name, rc, lib.nopesac_last_error())


def _f32(dev, *shape):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def _tensors(out):
    if torch.is_tensor(out):
        return [out]
    return list(out.values()) if isinstance(out, dict) else list(out)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
AB, ALQ, ALK, HEADS, SCALE = 2, 3, 5, 8, 32 ** -0.5
AW = HEADS * 32


def _attention_lengths(dev):
    return _i32([3, 1], dev), _i32([5, 2], dev)


def case_attention_dense(dev):
    g = torch.Generator().manual_seed(1)
    q, k, v, d_out = (_rand(g, rows, AW).to(dev) for rows in (AB * ALQ, AB * ALK, AB * ALK, AB * ALQ))
    ql, kl = _attention_lengths(dev)

    def raw(q, k, v, d_out, ql, kl):
        dq, dk, dv = _f32(dev, AB * ALQ, AW), _f32(dev, AB * ALK, AW), _f32(dev, AB * ALK, AW)
        _raw("nopesac_attention_small_backward", q, q.stride(0), k, k.stride(0), v, v.stride(0), d_out, d_out.stride(0), AB, ALQ, ALK, HEADS, SCALE,
             ql, kl, dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0))
        return dq, dk, dv
    return Case(lambda q, k, v, d_out, ql, kl: ops.attention_backward(q, k, v, d_out, AB, ALQ, ALK, HEADS, SCALE, ql, kl), (q, k, v, d_out, ql, kl), raw)


def case_attention_sliced(dev):
    """q | k | v as column slices of one [rows, 768] buffer, d_out a column slice too, the gradients into slices of one [rows, 768] buffer
    (returned whole: what lies outside the slices must stay as it was)."""
    g = torch.Generator().manual_seed(2)
    packed = _rand(g, AB * ALK, 3 * AW).to(dev)
    d_out = _rand(g, AB * ALQ, AW + 44).to(dev)[:, :AW]
    q, k, v = packed[:AB * ALQ, :AW], packed[:, AW:2 * AW], packed[:, 2 * AW:]
    ql, kl = _attention_lengths(dev)
    slices = lambda buf: (buf[:AB * ALQ, :AW], buf[:, AW:2 * AW], buf[:, 2 * AW:])
    grads = torch.zeros_like(packed)

    def fn(q, k, v, d_out, ql, kl, dq, dk, dv):
        got = ops.attention_backward(q, k, v, d_out, AB, ALQ, ALK, HEADS, SCALE, ql, kl, out=(dq, dk, dv))
        assert got[0] is dq and got[1] is dk and got[2] is dv
        return grads

    def raw(q, k, v, d_out, ql, kl, *_):
        buf = torch.zeros_like(packed)
        dq, dk, dv = slices(buf)
        _raw("nopesac_attention_small_backward", q, q.stride(0), k, k.stride(0), v, v.stride(0), d_out, d_out.stride(0), AB, ALQ, ALK, HEADS, SCALE,
             ql, kl, dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0))
        return buf
    return Case(fn, (q, k, v, d_out, ql, kl) + slices(grads), raw)


def case_layernorm(dev, rows):
    g = torch.Generator().manual_seed(3)
    x, gamma, dy = _rand(g, rows, 256).to(dev), _rand(g, 256).to(dev), _rand(g, rows, 256).to(dev)

    def raw(x, gamma, dy):
        dx, dg, db = _f32(dev, rows, 256), _f32(dev, 256), _f32(dev, 256)
        n_ws = ops._L().nopesac_layernorm_backward_workspace_floats(rows)
        _raw("nopesac_layernorm_backward", x, gamma, dy, rows, 256, 1e-5, dx, dg, db, _f32(dev, n_ws), n_ws)
        return dx, dg, db
    return Case(lambda x, gamma, dy: ops.layernorm_backward(x, gamma, dy, 1e-5), (x, gamma, dy), raw)


RB, RNQ = 2, 3
RNH = RNQ + 1


def case_score_maps(dev):
    g = torch.Generator().manual_seed(4)
    args = tuple(_rand(g, *s).to(dev) for s in ((RB, RNQ, 6), (RB, RNQ, 4), (RB, RNQ, 3), (RB, 4), (RB, 3)))
    args += (_i32([3, 0], dev),) + tuple(_rand(g, RB, RNH, RNQ).to(dev) for _ in range(3))

    def raw(geo, rot, tr, ir, it, m, g_ns, g_ps, g_l2):
        out = (_f32(dev, RB, RNQ, 4), _f32(dev, RB, RNQ, 3), _f32(dev, RB, 4), _f32(dev, RB, 3))
        _raw("nopesac_refine_score_maps_backward", geo, rot, tr, ir, it, m, RB, RNQ, g_ns, g_ps, g_l2, *out)
        return out
    return Case(ops.ransac_score_maps_backward, args, raw)


def case_vote(dev):
    g = torch.Generator().manual_seed(5)
    shapes = ((RB, RNH, 64), (RB, RNH, 64), (64,), (1,), (64,), (1,), (RB, 256), (RB, 256), (RB, RNQ, 256), (RB, RNQ, 256), (4, 256), (4,), (3, 256),
              (3,))
    grads = ((RB, 4), (RB, 3), (RB, 4), (RB, 3), (RB, RNH), (RB, RNH))
    args = tuple(_rand(g, *s).to(dev) for s in shapes) + (_i32([3, 0], dev),) + tuple(_rand(g, *s).to(dev) for s in grads)

    def raw(*a):
        out = [_f32(dev, *s) for s in ((RB, RNH, 64), (RB, RNH, 64), (RB, 256), (RB, 256), (RB, RNQ, 256), (RB, RNQ, 256), (RB, 1024), (RB, 4),
                                       (RB, 768), (RB, 3), (RB, 64), (RB, 1), (RB, 64), (RB, 1))]
        _raw("nopesac_refine_vote_backward", *a[:15], RB, RNQ, *a[15:], *out)
        return out
    return Case(ops.ransac_soft_vote_backward, args, raw)


def case_losses(dev):
    g = torch.Generator().manual_seed(6)
    shapes = ((RB, 4), (RB, 3), (RB, 4), (RB, 3), (RB, RNH), (RB, RNH), (RB, RNH, 4), (RB, RNH, 3))
    args = tuple(_rand(g, *s).to(dev) for s in shapes) + (_i32([3, 0], dev), _rand(g, RB, 7).to(dev), _rand(g, 7).to(dev))

    def fn(pr, pt, ar, at, sr, st, rots_all, trans_all, m, gt, g_losses):
        vote = {"pred_rot": pr, "pred_trans": pt, "avg_rot": ar, "avg_trans": at, "score_rot": sr, "score_trans": st}
        return ops.plane_cam_ref_losses_backward(vote, {"rots_all": rots_all, "trans_all": trans_all}, m, gt, g_losses, 0.75)

    def raw(pr, pt, ar, at, sr, st, rots_all, trans_all, m, gt, g_losses):
        out = [_f32(dev, *s) for s in ((RB, 4), (RB, 3), (RB, 4), (RB, 3), (RB, RNH), (RB, RNH), (RB, RNH, RNQ))]
        _raw("nopesac_refine_losses_backward", pr, pt, ar, at, rots_all, trans_all, sr, st, m, gt, g_losses, RB, RNQ, 0.75, *out)
        return out
    return Case(fn, args, raw)


def case_normalize(dev):
    g = torch.Generator().manual_seed(7)
    x, gr = _rand(g, 3, 4).to(dev), _rand(g, 3, 4).to(dev)

    def raw(x, gr):
        out = _f32(dev, 3, 4)
        _raw("nopesac_normalize_rows_backward", x, gr, 3, 4, 1, out)
        return out
    return Case(lambda x, gr: ops.normalize_rows_backward(x, gr, True), (x, gr), raw)


def case_pose_loss(dev):
    """B = 3; the ground truth as the column views of one [B, 7] pose tensor (row stride 7), as the trainer's forward passes it."""
    g = torch.Generator().manual_seed(8)
    B = 3
    pose = _rand(g, B, 7).to(dev)
    args = (_rand(g, B, 3).to(dev), _rand(g, B, 4).to(dev), pose[:, 0:3], pose[:, 3:7], _rand(g, 2).to(dev))

    def raw(et, eq, gt_t, gt_q, g_out):
        out = (_f32(dev, B, 3), _f32(dev, B, 4), _f32(dev, B, 3), _f32(dev, B, 4))
        _raw("nopesac_camera_pose_loss_backward", et, eq, gt_t, gt_t.stride(0), gt_q, gt_q.stride(0), B, 1e-3, 0.5, g_out, *out)
        return out
    return Case(lambda et, eq, gt_t, gt_q, g_out: ops.camera_pose_loss_backward(et, eq, gt_t, gt_q, g_out, 0.5, 1e-3), args, raw)


MB, MNQ, MITERS = 2, 4, 3
MR = MNQ + 1


def case_desc_dot(dev):
    g = torch.Generator().manual_seed(9)
    args = (_rand(g, MB, MNQ, MNQ).to(dev), _rand(g, MB, MNQ, 256).to(dev), _rand(g, MB, MNQ, 256).to(dev), _i32([4, 0], dev), _i32([2, 3], dev))

    def raw(gr, d0, d1, n1, n2):
        dd0, dd1 = _f32(dev, MB, MNQ, 256), _f32(dev, MB, MNQ, 256)
        _raw("nopesac_desc_dot_backward", gr, d0, d1, n1, n2, MB, MNQ, 256, dd0, dd1)
        return dd0, dd1
    return Case(ops.desc_dot_backward, args, raw)


# (n1, n2, the pairs whose gt_corr selects something): one pair with n1 = 0; one live pair whose gt_corr selects nothing
SINKHORN_CONFIGS = {"empty_pair": ([0, 3], [2, 4], (1,)), "nothing_selected": ([3, 4], [2, 3], (1,))}


def _sinkhorn_inputs(dev, config):
    n1, n2, selecting = SINKHORN_CONFIGS[config]
    g = torch.Generator().manual_seed(10)
    cam7 = _rand(g, MB, 7)
    cam7[:, 3:] = torch.nn.functional.normalize(cam7[:, 3:], dim=1)
    gt = torch.zeros(MB, MR, MR, dtype=torch.uint8)
    for b in selecting:                                   # one match, every other live row / column to the dustbin
        gt[b, 0, 1] = 1
        gt[b, 1:n1[b], MNQ] = 1
        gt[b, MNQ, [j for j in range(n2[b]) if j != 1]] = 1
    f = (_rand(g, MB, MNQ, MNQ), torch.nn.functional.normalize(_rand(g, MB, MNQ, 3), dim=2), torch.nn.functional.normalize(_rand(g, MB, MNQ, 3), dim=2),
         cam7)
    return tuple(t.to(dev) for t in f) + (_i32(n1, dev), _i32(n2, dev), torch.ones(1, device=dev), gt.to(dev))


def _live_uv(uv, n1, n2):
    """uv with everything the kernel leaves unwritten set to zero: a pair with n1 = 0 or n2 = 0 writes nothing, a live one the first
    n1 + 1 row potentials and n2 + 1 column potentials of every iteration (the workspace is read back at exactly these places)."""
    out = torch.zeros_like(uv)
    for b, (a, c) in enumerate(zip(n1.tolist(), n2.tolist())):
        if a > 0 and c > 0:
            out[b, :, 0, :a + 1] = uv[b, :, 0, :a + 1]
            out[b, :, 1, :c + 1] = uv[b, :, 1, :c + 1]
    return out


def case_sinkhorn_train(dev, config):
    dots, p1, p2, cam7, n1, n2, bin_score, gt = _sinkhorn_inputs(dev, config)

    def fn(dots, p1, p2, cam7, n1, n2, bin_score, gt):
        scores, uv, stats, loss = ops.matcher_sinkhorn_train(dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, gt)
        assert uv.shape == (MB, MITERS, 2, MR)
        return scores, _live_uv(uv, n1, n2), stats, loss

    def raw(dots, p1, p2, cam7, n1, n2, bin_score, gt):
        scores, uv, stats, loss = _f32(dev, MB, MR, MR), _f32(dev, MB, MITERS, 2, MR), _f32(dev, MB, 2), _f32(dev, 2)
        _raw("nopesac_matcher_sinkhorn_train", dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, gt, MB, MNQ, scores, uv, stats, loss)
        return scores, _live_uv(uv, n1, n2), stats, loss
    return Case(fn, (dots, p1, p2, cam7, n1, n2, bin_score, gt), raw)


def case_sinkhorn_backward(dev, config):
    dots, p1, p2, cam7, n1, n2, bin_score, gt = _sinkhorn_inputs(dev, config)
    _scores, uv, _stats, loss = ops.matcher_sinkhorn_train(dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, gt)
    g_loss = torch.full((1,), 0.5, device=dev)

    def raw(dots, p1, p2, cam7, n1, n2, bin_score, gt, uv, loss, g_loss):
        d_dots, d_bin = _f32(dev, MB, MNQ, MNQ), _f32(dev, MB)
        _raw("nopesac_matcher_sinkhorn_train_backward", dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, gt, uv, loss, g_loss, MB, MNQ,
             d_dots, d_bin)
        return d_dots, d_bin
    fn = lambda dots, p1, p2, cam7, n1, n2, bin_score, gt, uv, loss, g_loss: ops.matcher_sinkhorn_train_backward(
        dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, gt, uv, loss, g_loss)
    return Case(fn, (dots, p1, p2, cam7, n1, n2, bin_score, gt, uv, loss, g_loss), raw)


def case_emb_loss(dev, config):
    dots, p1, p2, cam7, n1, n2, bin_score, gt = _sinkhorn_inputs(dev, config)
    scores, _assignment = ops.matcher_sinkhorn(dots, p1, p2, cam7, n1, n2, bin_score, 4.0, 8.0, MITERS, 0.0)

    def raw(scores, gt, n1, n2):
        stats, loss = _f32(dev, MB, 2), _f32(dev, 2)
        _raw("nopesac_matcher_emb_loss", scores, gt, n1, n2, MB, MNQ, stats, loss)
        return stats, loss
    return Case(ops.matcher_emb_loss, (scores, gt, n1, n2), raw)


def _row_slice(dev, seed):
    """[5, 7] as a slice of a [5, 16] buffer: row stride 16."""
    return _rand(torch.Generator().manual_seed(seed), 5, 16).to(dev)[:, :7]


def case_transpose(dev):
    def raw(x):
        y = _f32(dev, 7, 5)
        _raw("nopesac_transpose_f32", x, 5, 7, x.stride(0), y)
        return y
    return Case(ops.transpose_rows, (_row_slice(dev, 11),), raw)


def case_col_sum(dev):
    def raw(x):
        out = _f32(dev, 7)
        _raw("nopesac_col_sum_f32", x, 5, 7, x.stride(0), out)
        return out
    return Case(ops.col_sum, (_row_slice(dev, 12),), raw)


def case_relu(dev):
    """The entry point takes flat arrays: the wrapper asks for contiguous tensors (the slice itself is refused, test_refusals), so the
    slice goes in as the copy the autograd Functions make."""
    def raw(gr, y):
        out = _f32(dev, 5, 7)
        _raw("nopesac_relu_backward_f32", gr, y, 35, out)
        return out
    return Case(ops.relu_backward, (_row_slice(dev, 13).contiguous(), _row_slice(dev, 14).contiguous()), raw)


def _optimiser_state(dev, buffers):
    g = torch.Generator().manual_seed(15)
    return tuple(_rand(g, 5).to(dev) for _ in range(2)) + tuple(_rand(g, 5).abs().to(dev) for _ in range(buffers))


def case_adamw(dev):
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.01)

    def run(p, gr, m1, m2):
        p, m1, m2 = p.clone(), m1.clone(), m2.clone()
        for step in (1, 2):                               # two consecutive steps on the same state
            ops.adamw_step(p, gr, m1, m2, *hyper, step)
        return p, m1, m2

    def raw(p, gr, m1, m2):
        p, m1, m2 = p.clone(), m1.clone(), m2.clone()
        for step in (1, 2):
            _raw("nopesac_adamw_step", p, gr, m1, m2, 5, *hyper, step)
        return p, m1, m2
    return Case(lambda p, gr, m1, m2: ops.adamw_step(p, gr, m1, m2, *hyper, 1), _optimiser_state(dev, 2), raw, run=run)


def case_sgd(dev):
    def run(p, gr, mom):
        p, mom = p.clone(), mom.clone()
        for first in (True, False):
            ops.sgd_step(p, gr, mom, 1e-2, 0.9, 0.01, first)
        return p, mom

    def raw(p, gr, mom):
        p, mom = p.clone(), mom.clone()
        for first in (1, 0):
            _raw("nopesac_sgd_step", p, gr, mom, 5, 1e-2, 0.9, 0.01, first)
        return p, mom
    return Case(lambda p, gr, mom: ops.sgd_step(p, gr, mom, 1e-2, 0.9, 0.01, True), _optimiser_state(dev, 1), raw, run=run)


def case_clip(dev, n):
    """sumsq (a fresh accumulator, then a second tensor onto it) -> clip coefficient -> scaled copy."""
    x = _rand(torch.Generator().manual_seed(16), n).to(dev)

    def fn(x):
        acc = ops.sumsq_accumulate(x)
        assert ops.sumsq_accumulate(x[:n // 2 + 1], acc) is acc
        coef = ops.clip_coefficient(acc, 1.0)
        y = x.clone()
        assert ops.scale_by(y, coef) is y
        return acc, coef, y

    def raw(x):
        acc, coef, y, ws = torch.zeros(1, device=dev), _f32(dev, 1), x.clone(), _f32(dev, 256)
        _raw("nopesac_sumsq_accumulate_f32", x, n, acc, ws, 256)
        _raw("nopesac_sumsq_accumulate_f32", x, n // 2 + 1, acc, ws, 256)
        _raw("nopesac_clip_coefficient", acc, 1.0, coef)
        _raw("nopesac_scale_by_f32", y, n, coef)
        return acc, coef, y
    return Case(fn, (x,), raw, free=(0,))


CASES = {
    "attention_dense": case_attention_dense, "attention_sliced": case_attention_sliced,
    "layernorm_5": lambda dev: case_layernorm(dev, 5), "layernorm_300": lambda dev: case_layernorm(dev, 300),
    "score_maps": case_score_maps, "vote": case_vote, "losses": case_losses, "normalize": case_normalize, "pose_loss": case_pose_loss,
    "desc_dot": case_desc_dot, "transpose": case_transpose, "col_sum": case_col_sum, "relu": case_relu, "adamw": case_adamw, "sgd": case_sgd,
    "clip_16384": lambda dev: case_clip(dev, 16384), "clip_16385": lambda dev: case_clip(dev, 16385), "clip_70001": lambda dev: case_clip(dev, 70001),
}
for _config in SINKHORN_CONFIGS:
    CASES["sinkhorn_train_" + _config] = lambda dev, c=_config: case_sinkhorn_train(dev, c)
    CASES["sinkhorn_backward_" + _config] = lambda dev, c=_config: case_sinkhorn_backward(dev, c)
    CASES["emb_loss_" + _config] = lambda dev, c=_config: case_emb_loss(dev, c)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper_equals_raw_call(device, name):
    case = CASES[name](device)
    mine, ref = _tensors((case.run or case.fn)(*case.args)), _tensors(case.raw(*case.args))
    torch.cuda.synchronize()
    assert len(mine) == len(ref)
    for i, (a, b) in enumerate(zip(mine, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, (name, i, a.shape, b.shape)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, i, (a - b).abs().max().item())        # the same bits


def test_sinkhorn_configs_are_what_they_say(device):
    """One pair with n1 = 0; one live pair whose gt_corr selects nothing, next to a pair that selects."""
    for config, (n1, n2, selecting) in SINKHORN_CONFIGS.items():
        *inputs, gt = _sinkhorn_inputs(device, config)
        _scores, _uv, stats, loss = ops.matcher_sinkhorn_train(*inputs, 4.0, 8.0, MITERS, gt)
        counts = stats[:, 1].tolist()
        assert [c > 0 for c in counts] == [b in selecting for b in range(MB)], (config, counts)
        assert loss[1].item() == sum(counts) and loss[0].item() > 0
    assert SINKHORN_CONFIGS["empty_pair"][0][0] == 0 and min(SINKHORN_CONFIGS["nothing_selected"][0] + SINKHORN_CONFIGS["nothing_selected"][1]) > 0


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def _strided(t):
    """The same shape and values with stride 2 in the last dimension: neither contiguous nor of unit column stride."""
    return torch.stack([t, t], dim=-1)[..., 0]


def _refused(monkeypatch):
    def reached(*args):
        raise AssertionError("a refused argument reached the library")
    for entry in _lib.STATUS:
        monkeypatch.setattr(_lib.C, entry, reached)


def _expect_refusal(case, name, what, i, bad):
    args = list(case.args)
    args[i] = bad
    with pytest.raises(ops.OpsArgumentError):
        case.fn(*args)
        pytest.fail("%s accepted %s as argument %d" % (name, what, i))


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusals(device, monkeypatch, name):
    """Every tensor argument in turn as float64 and bf16 (int64 for the int32 lengths), strided, and one element short."""
    case = CASES[name](device)
    torch.cuda.synchronize()
    _refused(monkeypatch)
    tried = 0
    for i, t in enumerate(case.args):
        if not torch.is_tensor(t):
            continue
        others = {torch.float32: (torch.float64, torch.bfloat16), torch.int32: (torch.int64,), torch.uint8: (torch.bool, torch.int32)}[t.dtype]
        for dtype in others:
            _expect_refusal(case, name, str(dtype), i, t.to(dtype))
        if t.numel() > 1:
            assert not _strided(t).is_contiguous()
            _expect_refusal(case, name, "a strided tensor", i, _strided(t))
        if i not in case.free:
            _expect_refusal(case, name, "a tensor one element short", i, t.flatten()[:-1])
        tried += 1
    assert tried > 0


@pytest.mark.parametrize("wrapper", ["matcher_emb_loss", "matcher_sinkhorn_train", "matcher_sinkhorn_train_backward"])
def test_gt_corr_without_dustbin_is_refused(device, monkeypatch, wrapper):
    build = {"matcher_emb_loss": case_emb_loss, "matcher_sinkhorn_train": case_sinkhorn_train,
             "matcher_sinkhorn_train_backward": case_sinkhorn_backward}[wrapper]
    case = build(device, "nothing_selected")
    torch.cuda.synchronize()
    _refused(monkeypatch)
    (i,) = [i for i, t in enumerate(case.args) if torch.is_tensor(t) and t.dtype == torch.uint8]
    _expect_refusal(case, wrapper, "gt_corr [B, nq, nq]", i, case.args[i][:, :MNQ, :MNQ].contiguous())


def test_moment_buffers_of_another_size_are_refused(device, monkeypatch):
    _refused(monkeypatch)
    p, gr, m1, m2 = _optimiser_state(device, 2)
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.01, 1)
    for longer in (False, True):
        bad = torch.zeros(6, device=device) if longer else torch.zeros(4, device=device)
        for args in ((p, gr, bad, m2), (p, gr, m1, bad), (p, bad, m1, m2)):
            with pytest.raises(ops.OpsArgumentError):
                ops.adamw_step(*args, *hyper)
        with pytest.raises(ops.OpsArgumentError):
            ops.sgd_step(p, gr, bad, 1e-2, 0.9, 0.01, True)


def test_accumulator_and_coefficient_hold_one_element(device, monkeypatch):
    _refused(monkeypatch)
    x, one = torch.ones(5, device=device), torch.ones(1, device=device)
    for bad in (torch.ones(2, device=device), one.double(), one.bfloat16(), torch.ones(0, device=device)):
        for call in (lambda: ops.sumsq_accumulate(x, bad), lambda: ops.clip_coefficient(bad, 1.0), lambda: ops.scale_by(x, bad)):
            with pytest.raises(ops.OpsArgumentError):
                call()


def test_attention_lengths_are_checked_in_both_directions(device, monkeypatch):
    """ops.attention takes qlen / klen through the helper of its backward twin: int32, B elements, on the device (or None)."""
    case = case_attention_dense(device)
    q, k, v, d_out, ql, kl = case.args
    torch.cuda.synchronize()
    _refused(monkeypatch)
    for bad in (ql.long(), ql[:1], torch.cat([ql, ql])):
        for lens in ((bad, kl), (ql, bad)):
            with pytest.raises(ops.OpsArgumentError):
                ops.attention(q, k, v, AB, ALQ, ALK, HEADS, SCALE, *lens)
            with pytest.raises(ops.OpsArgumentError):
                ops.attention_backward(q, k, v, d_out, AB, ALQ, ALK, HEADS, SCALE, *lens)
    with pytest.raises(ops.OpsArgumentError, match="no CPU path"):
        ops.attention(q, k, v, AB, ALQ, ALK, HEADS, SCALE, ql.cpu(), kl)
    with pytest.raises(ops.OpsArgumentError):                  # the [5, 7] row slice of a [5, 16] buffer is not a flat array
        ops.relu_backward(_row_slice(device, 13), _row_slice(device, 14))
