"""The conv-stack backward kernels of csrc/conv_bwd.hip (nopesac_amd.ops.conv2d_dgrad / conv2d_wgrad / bn_act_backward /
groupnorm_backward / maxpool_backward / upsample2x_nearest_add_backward / corr_softmax_backward) against float64 torch.autograd, at every
conv shape of the pixel pose net at 480 x 640, and bit-for-bit run-to-run determinism."""
import pytest
import torch
import torch.nn.functional as F

from nopesac_amd.synth import state_dict_spec

pytestmark = pytest.mark.gpu
PFX = "camera_head_list.0."
# input spatial size of every conv of the pixel pose net at 480 x 640, (pad, stride)
_HW = {"pixel_decoder.layer_3": (15, 20), "pixel_decoder.adapter_2": (30, 40), "pixel_decoder.layer_2": (30, 40),
       "pixel_decoder.adapter_1": (60, 80), "pixel_decoder.layer_1": (60, 80), "pixel_decoder.mask_features": (60, 80),
       "convs_backbone.0.0": (60, 80), "convs_backbone.1.0": (60, 80), "convs_backbone.3.0": (30, 40), "convs_backbone.4.0": (30, 40),
       "convs_backbone.6.0": (15, 20), "convs_backbone.7.0": (15, 20)}
for _br in ("convs_trans", "convs_rots"):
    for _i, _hw in enumerate([(15, 20), (15, 20), (8, 10), (8, 10), (4, 5), (4, 5)]):
        _HW[f"{_br}.{_i}.0"] = _hw


def _layers():
    spec = state_dict_spec(50)
    out = []
    for name, hw in _HW.items():
        cout, cin, k, _ = spec[PFX + name + ".weight"]
        stride = 2 if name.startswith("convs_") and name.split(".")[0] != "convs_backbone" and int(name.split(".")[1]) % 2 == 1 else 1
        out.append((name, cin, cout, k, stride, (k - 1) // 2, hw))
    return out


LAYERS = _layers()
assert len(LAYERS) == 24


def _nerr(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _conv_case(B, cin, cout, k, stride, pad, hw, seed, cx=None):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(B, cout, OH, OW, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, pad).backward(dy)
    x_nhwc = x.permute(0, 2, 3, 1).float()
    if cx and cx > cin:                                    # channel-padded input (the 300 -> 304 correlation volume)
        x_nhwc = F.pad(x_nhwc, (0, cx - cin))
    return x_nhwc.contiguous(), w.float(), dy.permute(0, 2, 3, 1).float().contiguous(), xr.grad, wr.grad


@pytest.mark.parametrize("name,cin,cout,k,stride,pad,hw", LAYERS, ids=[l[0] for l in LAYERS])
def test_dgrad_wgrad_at_every_pixel_pose_net_layer(device, name, cin, cout, k, stride, pad, hw):
    from nopesac_amd import ops
    B = 1 if cin >= 1024 or hw[0] == 60 else 2
    cx = 304 if cin == 300 else None
    x, w, dy, gx, gw = _conv_case(B, cin, cout, k, stride, pad, hw, sum(map(ord, name)), cx)
    x, w, dy = x.to(device), w.to(device), dy.to(device)
    dx = ops.conv2d_dgrad(dy, w, hw, stride=stride, pad=pad)
    dw = ops.conv2d_wgrad(x, dy, k, stride=stride, pad=pad, cin=cin)
    assert _nerr(dx.permute(0, 3, 1, 2), gx) < 2e-5, name
    assert _nerr(dw, gw) < 2e-5, name


def test_padded_input_dgrad_into_a_channel_slice(device):
    """The branches' first conv reads the 304-wide affinity volume: dgrad into its first 300 channels, the padding left untouched."""
    from nopesac_amd import ops
    x, w, dy, gx, gw = _conv_case(2, 300, 128, 3, 1, 1, (15, 20), 5, cx=304)
    out = torch.full((2, 15, 20, 304), 7.0, device=device)
    ops.conv2d_dgrad(dy.to(device), w.to(device), (15, 20), pad=1, out=out[..., :300])
    assert _nerr(out[..., :300].permute(0, 3, 1, 2), gx) < 2e-5
    assert bool((out[..., 300:] == 7.0).all())


@pytest.mark.parametrize("cin", [512, 1024])
def test_1x1_wide_input(device, cin):
    from nopesac_amd import ops
    x, w, dy, gx, gw = _conv_case(2, cin, 128, 1, 1, 0, (9, 13), cin)
    assert _nerr(ops.conv2d_dgrad(dy.to(device), w.to(device), (9, 13)).permute(0, 3, 1, 2), gx) < 2e-5
    assert _nerr(ops.conv2d_wgrad(x.to(device), dy.to(device), 1), gw) < 2e-5


@pytest.mark.parametrize("splits", [1, 3, 7, 64])
def test_wgrad_split_k_with_ragged_pixel_ranges(device, splits):
    """2 x 7 x 11 = 154 pixels: not a multiple of the split size (nor of the 16-pixel stage); splits beyond the pixels write zeros."""
    from nopesac_amd import ops
    x, w, dy, gx, gw = _conv_case(2, 64, 132, 3, 1, 1, (7, 11), 11 + splits)
    dw = ops.conv2d_wgrad(x.to(device), dy.to(device), 3, pad=1, splits=splits)
    assert _nerr(dw, gw) < 2e-5


@pytest.mark.parametrize("act", ["leaky", "relu"])
def test_bn_act_backward(device, act):
    from nopesac_amd import ops
    g = torch.Generator().manual_seed(3)
    rows, C = 1000, 96
    c = torch.randn(rows, C, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    gamma[:4] = 1e-4                                       # small gamma: the backward reads the raw conv output, not the post-BN value
    mean, var = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.1
    dy = torch.randn(rows, C, generator=g, dtype=torch.float64)
    cr, gr, br = c.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.batch_norm(cr.view(rows, C, 1, 1), mean, var, gr, br, False, 0.0, 1e-3).view(rows, C)
    (F.leaky_relu(z, 0.01) if act == "leaky" else F.relu(z)).backward(dy)
    d = lambda t: t.float().to(device)
    A = ops.ACT_LEAKY if act == "leaky" else ops.ACT_RELU
    y = ops.bn_act_forward(d(c), d(gamma), d(beta), d(mean), d(var), 1e-3, A)
    with torch.no_grad():
        ref_y = F.batch_norm(c.view(rows, C, 1, 1), mean, var, gamma, beta, False, 0.0, 1e-3).view(rows, C)
        ref_y = F.leaky_relu(ref_y, 0.01) if act == "leaky" else F.relu(ref_y)
    assert _nerr(y, ref_y) < 1e-5
    dc, dg, db = ops.bn_act_backward(d(dy), d(c), d(gamma), d(beta), d(mean), d(var), 1e-3, A)
    assert _nerr(dc, cr.grad) < 1e-5 and _nerr(dg, gr.grad) < 1e-5 and _nerr(db, br.grad) < 1e-5


@pytest.mark.parametrize("relu", [False, True])
def test_groupnorm_backward(device, relu):
    from nopesac_amd import ops
    g = torch.Generator().manual_seed(4)
    B, C, H, W = 2, 128, 15, 20
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.group_norm(xr, 32, gr, br, 1e-5)
    (F.relu(y) if relu else y).backward(dy)
    nh = lambda t: t.permute(0, 2, 3, 1).float().contiguous().to(device)
    dx, dg, db = ops.groupnorm_backward(nh(x), nh(dy), gamma.float().to(device), beta.float().to(device), 32, 1e-5,
                                        ops.ACT_RELU if relu else ops.ACT_NONE)
    assert _nerr(dx.permute(0, 3, 1, 2), xr.grad) < 1e-4
    assert _nerr(dg, gr.grad) < 1e-5 and _nerr(db, br.grad) < 1e-5


def test_maxpool_backward_with_ties(device):
    from nopesac_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 6, 10, generator=g, dtype=torch.float64)
    x[:, :, 0:2, 0:2] = 1.5                                # a whole window tied: the first element (row-major) takes the gradient
    x[:, :, 2, 3] = x[:, :, 3, 2] = 9.0                    # two maxima in one window: (2, 3) comes first
    dy = torch.randn(2, 8, 3, 5, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy)
    nh = lambda t: t.permute(0, 2, 3, 1).float().contiguous().to(device)
    dx = ops.maxpool_backward(nh(x), nh(dy))
    assert torch.equal(dx.permute(0, 3, 1, 2).cpu().double(), xr.grad.float().double())


def test_upsample_add_backward(device):
    from nopesac_amd import ops
    g = torch.Generator().manual_seed(6)
    c = torch.randn(2, 16, 15, 20, generator=g, dtype=torch.float64)
    lat = torch.randn(2, 16, 30, 40, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 16, 30, 40, generator=g, dtype=torch.float64)
    cr, lr = c.clone().requires_grad_(True), lat.clone().requires_grad_(True)
    (lr + F.interpolate(cr, size=(30, 40), mode="nearest")).backward(dy)
    nh = lambda t: t.permute(0, 2, 3, 1).float().contiguous().to(device)
    dc, dl = ops.upsample2x_nearest_add_backward(nh(dy))
    assert _nerr(dc.permute(0, 3, 1, 2), cr.grad) < 1e-6 and _nerr(dl.permute(0, 3, 1, 2), lr.grad) < 1e-7


def test_corr_softmax_backward(device):
    from nopesac_amd import ops
    from oracle import nopesac_oracle as O
    g = torch.Generator().manual_seed(7)
    B, C, h, w = 2, 256, 15, 20
    x1 = torch.randn(B, C, h, w, generator=g, dtype=torch.float64) * 0.1
    x2 = torch.randn(B, C, h, w, generator=g, dtype=torch.float64) * 0.1
    da = torch.randn(B, h * w, h, w, generator=g, dtype=torch.float64)
    r1, r2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    a_ref = O.corr_softmax(r1, r2)                         # [B, w2 h2, h1, w1]
    a_ref.backward(da)
    nh = lambda t: t.permute(0, 2, 3, 1).float().contiguous().to(device)
    a = ops.corr_softmax(nh(x1), nh(x2), 304)
    assert _nerr(a[..., :300].permute(0, 3, 1, 2), a_ref.detach()) < 1e-5 and bool((a[..., 300:] == 0).all())
    da_p = torch.cat([nh(da), torch.randn(B, h, w, 4, generator=g).to(device)], -1)   # padded channels: no gradient flows
    dx1, dx2 = ops.corr_softmax_backward(a, da_p, nh(x1), nh(x2))
    assert _nerr(dx1.permute(0, 3, 1, 2), r1.grad) < 1e-4 and _nerr(dx2.permute(0, 3, 1, 2), r2.grad) < 1e-4


def test_two_runs_are_bit_identical(device):
    from nopesac_amd import ops
    x, w, dy, _, _ = _conv_case(4, 256, 256, 3, 1, 1, (30, 40), 8)
    x, w, dy = x.to(device), w.to(device), dy.to(device)
    gam, bet = torch.rand(256, device=device) + 0.5, torch.randn(256, device=device)
    mu, var = torch.randn(256, device=device), torch.rand(256, device=device) + 0.1

    def run():
        dc, dg, db = ops.bn_act_backward(dy, x[..., :256].contiguous(), gam, bet, mu, var, 1e-3, ops.ACT_LEAKY)
        gx, gg, gb = ops.groupnorm_backward(x, dy, gam, bet, 32, 1e-5, ops.ACT_RELU)
        return [ops.conv2d_dgrad(dy, w, (30, 40), pad=1), ops.conv2d_wgrad(x, dy, 3, pad=1), dc, dg, db, gx, gg, gb]

    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
