"""The f32 conv kernel (csrc/conv_igemm.hip, all six builds) and the stride-1 dgrad (csrc/conv_bwd.hip: dgrad_weight_kernel + the same
kernel) against tests/conv_f32_forms.py: every element of every case within its allowance, sentinels and padding untouched, the weight
rotation bit for bit, two runs the same bits, and argument errors refused before any launch."""
import pytest
import torch

from tests import conv_f32_forms as CF

pytestmark = pytest.mark.gpu


@pytest.fixture
def ops(monkeypatch):
    """nopesac_amd.ops with an empty tuner (a routing another test loaded must not pick a kernel here) and no forced tile."""
    from nopesac_amd import ops
    monkeypatch.setattr(ops, "TUNER", ops.ConvTuner())
    monkeypatch.delenv("NOPESAC_CONV_FORCE", raising=False)
    return ops


def _untouched(buf, before, pad, C):
    """the columns of `buf` outside [pad[0], pad[0] + C) hold the bits they held"""
    return CF.same_bits(buf[..., :pad[0]], before[..., :pad[0]]) and CF.same_bits(buf[..., pad[0] + C:], before[..., pad[0] + C:])


def _forward(ops, device, name, out_fill=float("nan")):
    c, call = CF.FORWARD[name], CF.call_of(CF.FORWARD[name])
    b = CF.forward_buffers(name, device, out_fill)
    # the pointers are what generic_form and epilogue_vector assumed
    assert b["x"].data_ptr() % 16 == call.x_align and b["w"].data_ptr() % 16 == call.w_align and b["x"].stride(-2) == call.x_cs
    assert b["y"].data_ptr() % 16 == 4 * c.yp[0] % 16 and (b["r"] is None or b["r"].data_ptr() % 16 == 4 * c.rp[0] % 16)
    before = {k: b[k].clone() for k in ("x_buf", "y_buf", "r_buf") if b[k] is not None}
    y = CF.run_forward(ops, name, b)
    assert CF.same_bits(b["x_buf"], before["x_buf"]) and (b["r_buf"] is None or CF.same_bits(b["r_buf"], before["r_buf"])), name
    assert _untouched(b["y_buf"], before["y_buf"], c.yp, c.Cout), name
    return y


@pytest.mark.parametrize("name", [c.name for c in CF.FORWARD_CASES])
def test_forward_within_its_allowance(ops, device, monkeypatch, name):
    c = CF.FORWARD[name]
    if c.force:
        monkeypatch.setenv("NOPESAC_CONV_FORCE", c.force)          # read per call by the C side
    y = _forward(ops, device, name)
    fam = CF.family(c)
    worst, at = CF.forward_worst(name, y, str(device) if name in CF.DEVICE_REFERENCE else "cpu")
    print("conv_f32 %s %s %r: worst error / A = %.3g at %d (limit %.3g)" % (fam, name, CF.generic_form(CF.call_of(c)), worst, at, CF.limit(fam)))
    assert not bool(torch.isnan(y).any()), name
    assert worst <= CF.limit(fam), (name, worst, at)
    assert CF.same_bits(_forward(ops, device, name, out_fill=0.0), y), name      # a second run into a buffer of zeros: the same bits


def _dgrad(ops, device, key, out_fill=float("nan")):
    c, call, tag = CF.dgrad_inputs(key), CF.dgrad_call(key), key[-1]
    b = CF.dgrad_buffers(key, device, out_fill)
    assert b["dy"].data_ptr() % 16 == call.x_align and b["dy"].stride(-2) == call.x_cs
    before = {k: b[k].clone() for k in ("dy_buf", "dx_buf")}
    dx = ops.conv2d_dgrad(b["dy"], b["w"], (c["H"], c["W"]), stride=1, pad=c["pad"], out=b["dx"])
    assert dx.data_ptr() == b["dx"].data_ptr()
    assert CF.same_bits(b["dy_buf"], before["dy_buf"]) and _untouched(b["dx_buf"], before["dx_buf"], CF.DX_PAD[tag], c["Cin"]), key
    return dx


def _check_dgrad(ops, device, key, ref_device="cpu"):
    dx = _dgrad(ops, device, key)
    worst, at = CF.dgrad_worst(key, dx, ref_device)
    print("conv_f32 dgrad %r %r: worst error / A = %.3g at %d (limit %.3g)" % (key, CF.generic_form(CF.dgrad_call(key)), worst, at, CF.limit("dgrad")))
    assert not bool(torch.isnan(dx).any()), key
    assert worst <= CF.limit("dgrad"), (key, worst, at)


@pytest.mark.parametrize("cc", CF.DGRAD_CC, ids=lambda cc: "%d_%d" % cc)
@pytest.mark.parametrize("k", CF.DGRAD_K)
def test_dgrad_within_its_allowance(ops, device, k, cc):
    keys = [key for key in CF.GRID_CASES if key[0] == k and key[4:6] == cc]
    assert len(keys) == len(CF.DGRAD_HW) * len(CF.DGRAD_B)
    for key in keys:
        _check_dgrad(ops, device, key)


@pytest.mark.parametrize("key", CF.SLICE_CASES, ids=lambda k: "k%d_b%d_%dx%d_%d_%d_%s" % k)
def test_dgrad_on_channel_slices(ops, device, key):
    _check_dgrad(ops, device, key)


@pytest.mark.parametrize("key", CF.PRODUCTION_CASES, ids=lambda k: "k%d_b%d_%dx%d_%d_%d_%s" % k)
def test_dgrad_at_the_pose_nets_layers(ops, device, key):
    """the longest inner K, the 300-in-304 layer and a 1x1 at B = 1; the float64 reference and its draws are evaluated on the device"""
    _check_dgrad(ops, device, key, ref_device=str(device))


@pytest.mark.parametrize("shape", CF.ROTATION_SHAPES, ids=lambda s: "k%d_%dx%d_%d_%d" % s)
def test_the_rotation_is_bit_exact(ops, device, shape):
    """dy one-hot: every element of dx is a weight or +0.0, exactly - for an interior pixel (all nine taps) and the four corners"""
    k, H, W, Cin, Cout = shape
    w = CF.dgrad_inputs((k, 1, 5, 9, Cin, Cout, "base"))["w"]
    wd = w.to(device)
    for n, (ph, pw) in enumerate(CF.ROTATION_PIXELS):
        co = (3 * n + 1) % Cout
        dy = torch.zeros(1, H, W, Cout, device=device)
        dy[0, ph, pw, co] = 1.0
        out = torch.full((1, H, W, Cin), float("nan"), device=device)
        ops.conv2d_dgrad(dy, wd, (H, W), stride=1, pad=(k - 1) // 2, out=out)
        assert CF.same_bits(out[0].cpu(), CF.one_hot_expected(w, H, W, ph, pw, co)), (shape, ph, pw)


@pytest.mark.parametrize("key", CF.IDENTITY_CASES, ids=lambda k: "k%d_b%d_%dx%d_%d_%d_%s" % k)
def test_dgrad_repeats_bit_for_bit(ops, device, key):
    a = _dgrad(ops, device, key).clone()
    assert CF.same_bits(_dgrad(ops, device, key, out_fill=0.0), a)


def test_argument_errors_are_refused_before_any_launch(ops, device):
    from nopesac_amd._lib import HipKernelError
    C, p, st, F32 = ops._C, ops._p, ops._stream, ops.F32
    nan = float("nan")
    # dgrad of a stride-1 conv that is not same-size (3x3 without padding): nothing is written, the rotated weights included
    dy, w, out = torch.ones(1, 3, 3, 8, device=device), torch.ones(8, 4, 3, 3, device=device), torch.full((1, 5, 5, 4), nan, device=device)
    ws = ops.scratch(device, 4 * w.numel())
    ws.fill_(nan)
    with pytest.raises(HipKernelError, match="same-size"):
        ops.conv2d_dgrad(dy, w, (5, 5), stride=1, pad=0, out=out)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws[:w.numel()]).all())
    # a workspace one float short
    dy = torch.ones(1, 5, 5, 8, device=device)
    with pytest.raises(HipKernelError, match="workspace too small"):
        C.nopesac_conv2d_dgrad_f32(p(dy), p(w), p(out), p(ws), 4 * w.numel() - 4, 1, 5, 5, 4, 8, 3, 3, 1, 1, 8, 4, st())
    with pytest.raises(HipKernelError, match="workspace too small"):
        C.nopesac_conv2d_dgrad_f32(p(dy), p(w), p(out), None, 0, 1, 5, 5, 4, 8, 3, 3, 1, 1, 8, 4, st())
    # a channel stride below the channel count: dy, dx, and the forward's x, y and residual
    for dy_cs, dx_cs in ((7, 4), (8, 3)):
        with pytest.raises(HipKernelError, match="channel stride"):
            C.nopesac_conv2d_dgrad_f32(p(dy), p(w), p(out), p(ws), 4 * w.numel(), 1, 5, 5, 4, 8, 3, 3, 1, 1, dy_cs, dx_cs, st())
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws[:w.numel()]).all())
    x, wf, y = torch.ones(1, 5, 5, 8, device=device), torch.ones(4, 3, 3, 8, device=device), torch.full((1, 5, 5, 4), nan, device=device)
    res = torch.ones(1, 5, 5, 4, device=device)

    def ex(x_cs=8, y_cs=4, r_cs=4, cfg=0, residual=res):
        C.nopesac_conv2d_nhwc_ex(p(x), p(wf), None, None, p(residual), p(y), 1, 5, 5, 8, 4, 3, 3, 1, 1, x_cs, y_cs, r_cs, 0, ops.ACT_NONE, F32, F32,
                                 cfg, st())
    for kw, what in ((dict(x_cs=7), "channel stride"), (dict(y_cs=3), "channel stride"), (dict(r_cs=3), "residual stride"),
                     (dict(cfg=5), "bad kernel_cfg"), (dict(cfg=-1), "bad kernel_cfg")):
        with pytest.raises(HipKernelError, match=what):
            ex(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    ex()                                                                     # the same call with good arguments runs
    assert float((y - (CF.conv_torch(x.cpu(), wf.cpu(), 1, 1) + 1).to(device)).abs().max()) == 0.0
