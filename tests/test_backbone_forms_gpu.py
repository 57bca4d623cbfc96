"""The backbone's backward kernels (csrc/backbone_bwd.hip) against tests/backbone_forms.py: the strided dgrad per element within its
allowance at every boundary of its tile, the max-pool backward exact on integer gradients, the FrozenBN gate bit for bit."""
import pytest
import torch

from tests import backbone_forms as BF

pytestmark = pytest.mark.gpu


def _dgrad(device, key, fill_out=float("nan")):
    """ops.conv2d_dgrad_strided on a case -> (dx, out buffer, dy buffer); out starts as `fill_out` (a slice case: buffers of FILL)."""
    from nopesac_amd import ops
    c = BF.dgrad_inputs(key)
    sliced = key[-1] == "slice"
    p = BF.SLICE_PAD if sliced else 0
    dy_buf = torch.full((c["B"], c["OH"], c["OW"], c["Cout"] + 2 * p), BF.FILL, device=device)
    dy = dy_buf[..., p:p + c["Cout"]]
    dy.copy_(c["dy"])
    out_buf = torch.full((c["B"], c["H"], c["W"], c["Cin"] + 2 * p), BF.FILL if sliced else fill_out, device=device)
    out = out_buf[..., p:p + c["Cin"]]
    dx = ops.conv2d_dgrad_strided(dy, c["w"].to(device), (c["H"], c["W"]), stride=2, pad=c["pad"], out=out)
    assert dx.data_ptr() == out.data_ptr()
    return dx, out_buf, dy_buf


def _check(device, key, ref_device="cpu"):
    c = BF.dgrad_inputs(key)
    dx, out_buf, dy_buf = _dgrad(device, key)
    worst, at = BF.dgrad_worst(key, dx, ref_device)
    print("dgrad %r: worst error / A = %.3g at %d (limit %.3g)" % (key, worst, at, BF.limit()))
    assert worst <= BF.limit(), (key, worst, at)
    if c["k"] == 1:                                        # odd rows / columns: exact zeros over the NaN (or FILL) the buffer held
        odd = torch.ones(c["H"], c["W"], dtype=torch.bool, device=device)
        odd[::2, ::2] = False
        z = dx[:, odd]
        assert z.numel() == 0 or bool((z.view(torch.int32) == 0).all()), key
    if key[-1] == "slice":
        p = BF.SLICE_PAD
        assert bool((out_buf[..., :p] == BF.FILL).all()) and bool((out_buf[..., p + c["Cin"]:] == BF.FILL).all())
        assert bool((dy_buf[..., :p] == BF.FILL).all()) and bool((dy_buf[..., p + c["Cout"]:] == BF.FILL).all())
        assert torch.equal(dy_buf[..., p:p + c["Cout"]].cpu(), c["dy"])


@pytest.mark.parametrize("key", BF.DGRAD_CASES, ids=lambda k: "k%d_b%d_%dx%d_%d_%d_%s" % k)
def test_strided_dgrad_within_its_allowance(device, key):
    _check(device, key)


@pytest.mark.parametrize("key", BF.PRODUCTION_CASES, ids=lambda k: "k%d_b%d_%dx%d_%d_%d_%s" % k)
def test_strided_dgrad_at_the_production_layers(device, key):
    """res3.0 / res4.0 / res5.0 conv2 and shortcut at B = 1; the float64 reference and its draws are evaluated on the device"""
    _check(device, key, ref_device=str(device))


def test_strided_dgrad_is_the_parents_route_and_repeats_bit_for_bit(device):
    from nopesac_amd import ops
    c = BF.dgrad_inputs(BF.IDENTITY_CASE)
    a = _dgrad(device, BF.IDENTITY_CASE)[0].clone()
    b = _dgrad(device, BF.IDENTITY_CASE, fill_out=0.0)[0]
    assert torch.equal(a, b)
    gather = ops.conv2d_dgrad(c["dy"].to(device), c["w"].to(device), (c["H"], c["W"]), stride=2, pad=c["pad"])     # the scalar gather
    assert BF.dgrad_worst(BF.IDENTITY_CASE, gather)[0] <= BF.limit()


def test_strided_dgrad_refuses_what_it_does_not_take(device):
    from nopesac_amd import ops
    from nopesac_amd._lib import HipKernelError
    dy = torch.zeros(1, 2, 2, 8, device=device)
    with pytest.raises(HipKernelError):
        ops.conv2d_dgrad_strided(dy, torch.zeros(8, 6, 3, 3, device=device), (3, 3), pad=1)          # Cin % 4
    with pytest.raises(HipKernelError):
        ops.conv2d_dgrad_strided(dy, torch.zeros(8, 8, 3, 3, device=device), (5, 5), pad=0)          # pad != (k - 1) / 2
    with pytest.raises(ops.OpsArgumentError):
        ops.conv2d_dgrad_strided(dy, torch.zeros(8, 8, 3, 3, device=device), (8, 8), pad=1)          # dy does not match


@pytest.mark.parametrize("variant", BF.POOL_VARIANTS)
@pytest.mark.parametrize("hw", BF.POOL_HW, ids=lambda hw: "%dx%d" % hw)
def test_maxpool_backward_is_autograds(device, hw, variant):
    from nopesac_amd import ops
    for key in (k for k in BF.POOL_CASES if (k[1], k[2]) == hw and k[4] == variant):
        c = BF.pool_inputs(key)
        x = c["x"].to(device)
        assert torch.equal(ops.maxpool(x, 3, 2, 1).cpu(), BF.F.max_pool2d(c["x"].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)), key
        got = ops.maxpool3x3s2_backward(x, c["dy_int"].to(device)).cpu()
        assert torch.equal(got.double(), BF.pool_backward(c["x"], c["dy_int"])), key
        got = ops.maxpool3x3s2_backward(x, c["dy"].to(device)).cpu()
        ref, S = BF.pool_backward(c["x"], c["dy"]), BF.pool_backward(c["x"], c["dy"].abs())
        assert bool(((got.double() - ref).abs() <= BF.POOL_ROUNDINGS * BF.EPS24 * S).all()), key


def test_maxpool_backward_at_the_production_shape(device):
    from nopesac_amd import ops
    c = BF.pool_inputs(BF.POOL_PRODUCTION)
    got = ops.maxpool3x3s2_backward(c["x"].to(device), c["dy_int"].to(device)).cpu()
    assert torch.equal(got.double(), BF.pool_backward(c["x"], c["dy_int"]))


@pytest.mark.parametrize("rows", BF.GATE_ROWS)
def test_frozen_bn_gate_bit_for_bit(device, rows):
    from nopesac_amd import ops
    for key in (k for k in BF.GATE_CASES if k[0] == rows):
        _, C, relu, want_dz, strided = key
        c = BF.gate_inputs(key)
        gb, yb = c["g_buf"].to(device), c["y_buf"].to(device)
        g, y = gb[:, c["off"]:c["off"] + C], yb[:, c["off"]:c["off"] + C]
        assert g.is_contiguous() != strided
        r = ops.frozen_bn_act_backward(g, y, c["scale"].to(device), ops.ACT_RELU if relu else ops.ACT_NONE, want_dz)
        dc, dz = r if want_dz else (r, None)
        ref_dc, ref_dz = BF.gate_reference(c)
        assert BF.same_bits(dc.cpu(), ref_dc), key
        assert dz is None or BF.same_bits(dz.cpu(), ref_dz), key
        if relu:
            assert bool((dc[y == 0] == 0).all()) and bool(((c["y"] == 0) & (c["g"] != 0)).any())      # both zeros gate
