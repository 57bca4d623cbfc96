"""Shared helpers of the fused sweep (tests/test_fused_forms_*.py): the fused stem (three builds), the pose-net branch tail, the chained
MLP kernel and the fused mask head - their inputs, float64 references with a first-order per-element error bound, and CPU float32
emulations of the kernels' algorithms (negative controls).  Conventions are tests/head_forms.py's: references take the exact operand
values each kernel reads and round to bf16 where the kernel rounds; a GEMM or conv adds 2^-20 A (A = the absolute-value sum) to the bound,
a bf16 rounding point one unit in the last place on the elements within the bound of a rounding midpoint, ReLU / LeakyReLU / max-pool
carry the bound (1-Lipschitz; a pool window's bound is the window's maximum), a folded BatchNorm multiplies it by |scale| and adds its
two f32 roundings.  A stored output is judged with out_tol, every element, nothing normalised by a tensor maximum.

Inputs keep every ReLU / LeakyReLU pre-activation and the top-two gap of every pool window further than MARGIN from 0 in float64 (settled
by moving the inputs that feed an offending element), so that no sign or tie decision lies on its edge; the bound does not depend on it
(the three operations are 1-Lipschitz), the assertion documents that no test measures such a decision."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests.head_forms import BF, GEMM, bf, error_ratio, gemm, out_tol, ulp16

F64, F32 = torch.float64, torch.float32
MARGIN = 5e-5                # no pre-activation / pool gap of a case lies closer to 0 than this (float64); inputs are settled to twice this
R32 = 2.0 ** -24             # one f32 rounding, relative
LEAK = float(torch.tensor(0.01, dtype=F32))            # the kernels' 0.01f
INF = float("inf")


def round_point(v, E):
    """head_forms.round_point with the distance to the rounding midpoint measured in v's OWN binade: ulp16 gives the larger binade's unit
    within a unit of a power of two (right for the allowance), and half of THAT unit never comes within E of |v - bf16(v)| there - a
    midpoint in the top 1 / 128 of a binade went unflagged (found by the f32 emulation of the mask head at 2 x 120 x 160: one of 9.8 M
    lateral values).  Same allowance: one unit where the kernel's value may round to the other neighbour, else 0."""
    r = bf(v)
    own = torch.where(v != 0, torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-38))) - 7), torch.zeros_like(v))
    near = (own / 2 - (v - r).abs()) <= E
    return r, torch.where(near, ulp16(v), torch.zeros_like(v))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def mm32(a, w, chunk):
    """a [R,K] @ w [N,K]^T in float32, K in chunks summed in f32 (the emulations' summation order: neither the kernels' nor BLAS's)."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + a[:, k0:k0 + chunk] @ w[:, k0:k0 + chunk].T
    return acc


def bn(acc, E, scale, bias):
    """Folded BatchNorm as the kernels apply it - a multiply, then an add, both rounded to f32: (value, bound)."""
    t = acc * scale
    return t + bias, E * scale.abs() + 2 * R32 * (t.abs() + bias.abs())


def sigmoid_tol(v, E):
    """(s, tolerance) of s = 1 / (1 + exp(-v)) evaluated in f32 on a logit v with bound E: s (1 - s) (E + 2^-23 |v|) + 2^-22 s.
    ds/dv = s (1 - s) carries E.  e = exp(-v) is evaluated as 2^(-v log2 e): the rounded product and the f32 constant each move the
    exponent by up to 2^-24 |v| log2 e, that is e by 2^-23 |v| relative in all, and a relative error of e reaches s through
    ds / s = -(1 - s) de / e - the same factor s (1 - s).  What is left are relative errors of s itself: the exponential's and the
    reciprocal's own (v_exp_f32 and v_rcp_f32, about 1 ulp = 2^-23 each by the kernel's comment; expf and an IEEE division are tighter)
    and the rounded sum 1 + e: 2^-22 s."""
    s = torch.sigmoid(v)
    return s, s * (1 - s) * (E + 2.0 ** -23 * v.abs()) + 2.0 ** -22 * s + 1e-30


# ============================================================================================================================== 1. stem
# conv 7x7 / s2 / p3 (3 -> 64) + folded BN + ReLU + max-pool 3x3 / s2 / p1; a workgroup owns 4 x 20 pooled pixels = 9 x 41 conv pixels.
STEM_TILE_PH, STEM_TILE_PW = 4, 20
STEM_SIZES = ((7, 7), (8, 9), (13, 157), (13, 161), (17, 33), (100, 172), (480, 640))
PIXEL_MEAN, PIXEL_STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)


def stem_cases():
    """(H, W, B, shift sign, fractional pixels): every size with B = 1 and alternating BN shift signs, B = 3 at one small size, and one
    case with non-integer pixel values for the build that subtracts 128 while staging."""
    cases = [(H, W, 1, 1 if i % 2 == 0 else -1, False) for i, (H, W) in enumerate(STEM_SIZES)]
    cases += [(13, 161, 1, 1, False), (17, 33, 1, -1, False)]          # both seams with both signs
    cases += [(17, 33, 3, 1, False), (8, 9, 1, 1, True)]
    return cases


def stem_dims(H, W):
    CH, CW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return CH, CW, (CH - 1) // 2 + 1, (CW - 1) // 2 + 1


def _stem_pad(X, pad, t, l, b, r):
    """X [B,3,H,W] inside a frame of per-channel value pad[3]."""
    B, C, H, W = X.shape
    out = pad.to(X.dtype).view(1, 3, 1, 1).expand(B, 3, H + t + b, W + l + r).clone()
    out[:, :, t:t + H, l:l + W] = X
    return out


def stem_operand(c, build, x4=None):
    """The staged input of a build in float64: (X [B,3,H,W], allowance, pad value [3]).  Build 0 reads bf16 NHWC x4 as it is; build 1
    rounds (v - mean) / std, an f32 subtraction and division, to bf16: one unit where the quotient lies within its two f32 roundings of
    a midpoint; build 2 rounds v - 128 (exact for 8-bit values, one f32 rounding otherwise) and pads with bf16(mean - 128)."""
    raw = c.raw.double()
    Z3 = torch.zeros(3, dtype=F64)
    if build == 0:
        X = (c.x4 if x4 is None else x4).double()[..., :3].permute(0, 3, 1, 2)
        return X, torch.zeros_like(X), Z3
    if build == 1:
        v = (raw - c.mean.double().view(1, 3, 1, 1)) / c.std.double().view(1, 3, 1, 1)
        X, U = round_point(v, 2 * R32 * v.abs())
        return X, U, Z3
    v = raw - 128.0
    X, U = round_point(v, R32 * v.abs() * (raw != raw.round()))
    return X, U, bf(c.pad3.double())


def stem_reference(c, build, x4=None):
    """float64 stem of one build: z (conv + BN, before the ReLU) [B,64,CH,CW] with bound Ez, and the pooled value v [B,PH,PW,64] with
    bound E - the kernel stores bf16(v) (rounding is monotone: the maximum of the rounded tile is the rounded maximum)."""
    X, U, pad = stem_operand(c, build, x4)
    wk = (c.w224f if build == 2 else c.w224).double().view(64, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()   # [64,3,7,7]
    scale, bias = c.scale.double().view(1, 64, 1, 1), (c.biasf if build == 2 else c.bias).double().view(1, 64, 1, 1)
    Xp = _stem_pad(X, pad, 3, 3, 3, 3)
    acc = F.conv2d(Xp, wk, stride=2)
    E = GEMM * F.conv2d(Xp.abs(), wk.abs(), stride=2)
    if bool((U > 0).any()):
        E = E + F.conv2d(_stem_pad(U, torch.zeros(3, dtype=F64), 3, 3, 3, 3), wk.abs(), stride=2)
    z, Ez = bn(acc, E, scale, bias)
    a = z.clamp_min(0)
    v = F.max_pool2d(a, 3, 2, 1)
    Ev = F.max_pool2d(Ez, 3, 2, 1)
    return SimpleNamespace(z=z, Ez=Ez, a=a, v=v.permute(0, 2, 3, 1).contiguous(), E=Ev.permute(0, 2, 3, 1).contiguous())


def stem_gaps(a):
    """Top-two gap of every pool window of a [B,64,CH,CW] (>= 0): (gap, top) [B,64,PH,PW]; padding never wins."""
    B, C, CH, CW = a.shape
    PH, PW = (CH - 1) // 2 + 1, (CW - 1) // 2 + 1
    ap = F.pad(a, (1, 1, 1, 1), value=-1.0)
    win = F.unfold(ap, 3, stride=2).view(B, C, 9, PH, PW)
    top = win.topk(2, dim=2).values
    return top[:, :, 0] - top[:, :, 1], top[:, :, 0]


def stem_margin(c):
    """Smallest |pre-activation| and smallest decided pool gap (windows whose maximum is a clamped 0 decide nothing) over builds 1 and 2."""
    zmin, gmin = INF, INF
    for build in (1, 2):
        r = stem_reference(c, build)
        gap, top = stem_gaps(r.a)
        zmin = min(zmin, float(r.z.abs().min()))
        gmin = min(gmin, float(torch.where(top > 0, gap, torch.full_like(gap, INF)).min()))
    return zmin, gmin


@functools.lru_cache(maxsize=None)
def stem_case(H, W, B, sign, frac):
    """raw [B,3,H,W] f32 pixel values (8-bit integers; `frac`: with a fractional part), f32 master weights [64,7,7,3], folded BN with a
    shift of sign * (1.5 .. 2) (conv output std ~ 1.3: mostly live, or mostly clamped with pooled zeros), one negative scale; the operands of
    all three builds.  Settled: where a pre-activation or a pool gap of build 1 or 2 is within 2 MARGIN of 0, the input pixel under the
    centre tap of that conv pixel is moved."""
    from nopesac_amd import ops
    g = gen(7000 + 131 * H + 17 * W + B + (3 if sign > 0 else 0) + (11 if frac else 0))
    raw = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
    if frac:
        raw = (raw + torch.rand(B, 3, H, W, generator=g)).clamp(0, 255)
    w = torch.randn(64, 7, 7, 3, generator=g) / math.sqrt(147)
    scale = 1 + 0.1 * torch.randn(64, generator=g)
    scale[5] = -scale[5]
    bias = sign * (1.5 + 0.5 * torch.rand(64, generator=g))
    mean, std = torch.tensor(PIXEL_MEAN), torch.tensor(PIXEL_STD)
    w8 = torch.zeros(64, 7, 8, 4)
    w8[:, :, :7, :3] = w
    pad3, w224f, biasf = ops.fold_stem_normalisation(w, scale, bias, mean, std)
    c = SimpleNamespace(H=H, W=W, B=B, raw=raw, mean=mean, std=std, scale=scale, bias=bias, w224=w8.reshape(64, 224).to(BF), pad3=pad3,
                        w224f=w224f, biasf=biasf)
    CH, CW, PH, PW = stem_dims(H, W)
    for it in range(60):
        c.x4 = stem_preprocess(c)
        bad = torch.zeros(B, CH, CW, dtype=torch.bool)
        for build in (1, 2):
            r = stem_reference(c, build)
            bad |= (r.z.abs() <= 2 * MARGIN).any(1)
            gap, top = stem_gaps(r.a)
            pb = ((gap <= 2 * MARGIN) & (top > 0)).any(1)                       # [B,PH,PW] -> the conv pixel in the window's middle
            bad[:, ::2, ::2] |= pb[:, :(CH + 1) // 2, :(CW + 1) // 2]
        if not bad.any():
            break
        b, cy, cx = bad.nonzero(as_tuple=True)
        iy, ix = (2 * cy).clamp_max(H - 1), (2 * cx).clamp_max(W - 1)
        ch = (cy + cx + it) % 3
        c.raw[b, ch, iy, ix] = (c.raw[b, ch, iy, ix] + 64 + 17 * it) % 256
    c.x4 = stem_preprocess(c)
    return c


def stem_preprocess(c):
    """The documented preprocess in float32 torch: bf16((v - mean) / std) NHWC, channel 3 zero."""
    B, _, H, W = c.raw.shape
    x4 = torch.zeros(B, H, W, 4, dtype=BF)
    x4[..., :3] = ((c.raw - c.mean.view(1, 3, 1, 1)) / c.std.view(1, 3, 1, 1)).permute(0, 2, 3, 1).to(BF)
    return x4


STEM_FAULTS = ("outside_conv_in_pool", "pad_zero", "kw7_tap_nonzero", "seam_col_20", "seam_row_4")


def stem_emulate(c, build, fault=None):
    """The kernel's algorithm in float32: the staged bf16 patch values (pad value outside the image), the conv as a GEMM over
    K = (c, kh, kw padded to 8) in chunks, BN as multiply then add, ReLU, the conv tile rounded to bf16, 3x3 / s2 maximum with the pool
    padding excluded -> bf16 [B,PH,PW,64]."""
    H, W, B = c.H, c.W, c.B
    CH, CW, PH, PW = stem_dims(H, W)
    if build == 0:
        X, pad = c.x4.float()[..., :3].permute(0, 3, 1, 2), torch.zeros(3)
    elif build == 1:
        X, pad = bf((c.raw - c.mean.view(1, 3, 1, 1)) / c.std.view(1, 3, 1, 1)), torch.zeros(3)
    else:
        X, pad = bf(c.raw - 128.0), bf(c.pad3)
        if fault == "pad_zero":
            pad = torch.zeros(3)
    wk = (c.w224f if build == 2 else c.w224).float().view(64, 7, 8, 4)[..., :3].clone()
    if fault == "kw7_tap_nonzero":
        wk[:, :, 7] = wk[:, :, 6]
    wm = wk.permute(0, 3, 1, 2).reshape(64, 168)                                # K = (c, kh, kw), as unfold orders it
    ext = 2 if fault == "outside_conv_in_pool" else 0                           # conv pixels one ring outside the map are computed too
    Xp = _stem_pad(X, pad, 3 + ext, 3 + ext, 3 + ext, 4 + ext)
    cols = F.unfold(Xp, (7, 8), stride=2)                                       # [B,168,L]
    nH, nW = (Xp.shape[2] - 7) // 2 + 1, (Xp.shape[3] - 8) // 2 + 1
    scale, bias = c.scale.view(1, 64), (c.biasf if build == 2 else c.bias).view(1, 64)
    tiles = []
    for b in range(B):
        acc = mm32(cols[b].T.contiguous(), wm, 24)
        t = acc * scale
        tiles.append(bf((t + bias).clamp_min(0)).T.reshape(64, nH, nW))
    a = torch.stack(tiles)
    if ext:
        y = F.max_pool2d(a[:, :, :CH + 2, :CW + 2], 3, 2, 0)                    # the ring takes the place of the pool padding
    else:
        a = a[:, :, :CH, :CW]
        y = F.max_pool2d(a, 3, 2, 1)
        if fault in ("seam_col_20", "seam_row_4"):                              # tiles behind the first read the conv tile one pixel late
            neg = -torch.ones_like(a[..., :1, :] if fault == "seam_row_4" else a[..., :1])
            if fault == "seam_col_20":
                y[..., STEM_TILE_PW:] = F.max_pool2d(torch.cat([a[..., 1:], neg], 3), 3, 2, 1)[..., STEM_TILE_PW:]
            else:
                y[..., STEM_TILE_PH:, :] = F.max_pool2d(torch.cat([a[..., 1:, :], neg], 2), 3, 2, 1)[..., STEM_TILE_PH:, :]
    return y[:, :, :PH, :PW].permute(0, 2, 3, 1).to(BF)


def stem_ratio(y, ref):
    """Worst |y - v| / out_tol over every element of a stem output y [B,PH,PW,64] bf16."""
    return error_ratio(y.float().cpu(), ref.v, out_tol(ref.v, ref.E, BF))[0]


# ============================================================================================================================== 2. pose-net branch tail
# layers 1..5 of convs_trans / convs_rots: Conv3x3 (128 -> 128, pad 1) + folded BN + LeakyReLU(0.01), strides 2, 1, 2, 1, 2 on 15 x 20.
PB_STRIDES = (2, 1, 2, 1, 2)
PB_CASES = ((1, "random"), (2, "random"), (5, "random"), (2, "ring"), (2, "corner"))
# One layer at a time: kind "iso<k>_<routing>" keeps the real weights of layer k only; the other four layers are exact pass-throughs
# (output channel n = input channel n at ONE tap, scale 1, shift 0: the sum has one non-zero term, and bf16(0.01f x) of a bf16 x is a
# function the reference evaluates exactly), so layer k is held to its own 2^-20 A plus one rounding point.  Routing "near": the centre
# tap (the first pixel of every map reaches the output), "far": the tap that sends the LAST pixel of every map to the last output pixel,
# "mixed": a random tap per channel and layer (halo reads included).
PB_ROUTINGS = ("near", "far", "mixed")
PB_FAR_TAPS = ((0, 1), (0, 0), (1, 1), (0, 0), (1, 0))         # (dy, dx) per layer: I - 1 - 2 (O - 1) for the stride-2 layers, 0 for stride 1
PB_ISO_CASES = tuple((1, "iso%d_%s" % (k, r)) for k in range(5) for r in PB_ROUTINGS)


def _pb_live(kind):
    m = torch.zeros(15, 20, dtype=torch.bool)
    if kind == "ring":
        m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    elif kind == "corner":
        m[-1], m[:, -1] = True, True
    else:
        m[:] = True
    return m


def pb_branch(c, br, x, dtype=F64, fault=None, bounds=True):
    """One branch over the images x [n,15,20,128] bf16 through the five layers.  float64: the pre-activations z of every layer and the
    f32 output (value, bound) - F.conv2d on the bf16 weights, activations rounded to bf16 between the layers.  float32 (emulation of
    the kernel): the input parked in a zero halo tile, every layer a sum over the nine taps of (strided window of the tile) x (the tap's
    128 x 128 weights), BN as multiply then add, LeakyReLU, bf16 into the next halo tile; returns the output."""
    wbr = 1 - br if fault == "branches_swapped" else br
    a = x.to(dtype).permute(0, 3, 1, 2)                                        # NCHW
    Ea = torch.zeros_like(a)
    zs = []
    real = getattr(c, "real", None)                                            # iso cases: the one layer with real weights
    for i, s in enumerate(PB_STRIDES):
        w, sc, bi = c.w[wbr][i].to(dtype), c.scale[wbr][i].to(dtype).view(1, -1, 1, 1), c.bias[wbr][i].to(dtype).view(1, -1, 1, 1)
        if dtype == F64 and real is not None and i != real:
            # an exact pass-through: the value as the kernel computes it, and as allowance what a one-unit move of a flagged input does
            def through(av):
                zz = F.conv2d(av, w, stride=s, padding=1)
                vf = torch.where(zz > 0, zz, (zz.float() * torch.tensor(0.01)).double())
                return bf(vf) if i < 4 else vf
            v = through(a)
            Ev = torch.maximum((through(a + Ea) - v).abs(), (through(a - Ea) - v).abs()) if bool((Ea > 0).any()) else torch.zeros_like(v)
            a, Ea = v, Ev
            continue
        if dtype == F64:
            acc = F.conv2d(a, w, stride=s, padding=1)
            E = GEMM * F.conv2d(a.abs(), w.abs(), stride=s, padding=1) + F.conv2d(Ea, w.abs(), stride=s, padding=1) if bounds else 0 * acc
            z, Ez = bn(acc, E, sc, bi)
            v = torch.where(z > 0, z, LEAK * z)
            Ev = Ez + R32 * v.abs()
            zs.append(z)
            if i < 4:
                a, Ea = round_point(v, Ev) if bounds else (bf(v), Ea)
            continue
        B, _, IH, IW = a.shape
        OH, OW = (IH - 1) // s + 1, (IW - 1) // s + 1
        stale = fault == "halo_not_zero" and i == 1
        halo = torch.full((B, IH + 3, IW + 3, 128), 0.5 if stale else 0.0)     # (one spare row / column for the shifted-window fault)
        halo[:, 1:IH + 1, 1:IW + 1] = a.permute(0, 2, 3, 1)
        if i == real and fault in PB_ISO_FAULTS:                               # small errors at the layer under test
            if fault == "corner_channel_zeroed":
                halo[:, IH, IW, int(halo[0, IH, IW].abs().argmax())] = 0       # (the corner pixel's largest channel)
            elif fault == "corner_pixel_dropped":
                halo[:, IH, IW, :] = 0
            elif fault == "input_scaled_by_1.02":
                halo *= 1.02
            else:
                halo[:, 0, :, 3] = 0.25                                        # one channel of the top halo row is not zero
        d = 1 if (fault == "stride2_window_shifted" and s == 2) else 0
        acc = torch.zeros(B * OH * OW, 128)
        for kh in range(3):
            for kw in range(3):
                win = halo[:, kh + d:kh + d + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s]
                acc = acc + win.reshape(-1, 128) @ w[:, :, kh, kw].T
        t = acc * sc.view(1, -1)
        z = t + bi.view(1, -1)
        v = torch.where(z > 0, z, torch.tensor(0.01) * z).view(B, OH, OW, 128)
        if fault == "layer1_last_row_tile_dropped" and i == 0:
            v.view(B, OH * OW, 128)[:, 64:] = 0
        a = (bf(v) if i < 4 else v).permute(0, 3, 1, 2)
    if dtype == F64:
        return SimpleNamespace(z=zs, v=v.permute(0, 2, 3, 1).contiguous(), E=Ev.permute(0, 2, 3, 1).contiguous())
    return a.permute(0, 2, 3, 1).contiguous()


def pb_forward(c, dtype=F64, fault=None):
    return [pb_branch(c, br, c.x[br], dtype, fault) for br in range(2)]


PB_FAULTS = ("halo_not_zero", "stride2_window_shifted", "branches_swapped", "layer1_last_row_tile_dropped")
# at the layer under test of an iso case -> the routing that shows it (the far corner, or the first row's halo taps)
PB_ISO_FAULTS = {"corner_channel_zeroed": "far", "corner_pixel_dropped": "far", "input_scaled_by_1.02": None, "halo_top_row_channel_not_zero": "near"}


@functools.lru_cache(maxsize=None)
def pb_case(B, kind):
    """x[2] bf16 [B,15,20,128] (layer-0 outputs: N(0, 1) on the live positions of `kind`, 0 elsewhere), per branch five conv weights
    bf16 [128,128,3,3] and folded BN (no shift near 0: where the input is 0 the first pre-activation IS the shift).  The branches differ in gain (1 / 1.25), BN scale (about 1 / about -0.8) and shift spread, so that
    a swap cannot hide; both keep the activations at unit scale through the five layers.  Kind "iso<k>_<routing>": see PB_ISO_CASES.
    Settled per (branch, image): one with a pre-activation within 2 MARGIN of 0 in any layer with real weights gets a new draw of its
    live positions."""
    g = gen(9000 + 10 * B + sum(map(ord, kind)))
    live = _pb_live(kind)
    c = SimpleNamespace(B=B, kind=kind, w=[], scale=[], bias=[])
    for br in range(2):
        gain = (1.0, 1.25)[br] * math.sqrt(2.0 / (9 * 128))
        c.w.append([(gain * torch.randn(128, 128, 3, 3, generator=g)).to(BF) for _ in range(5)])
        c.scale.append([(1.0, -0.8)[br] * (1 + 0.1 * torch.randn(128, generator=g)) for _ in range(5)])
        c.bias.append([(0.1, 0.3)[br] * (lambda t: t + 0.1 * t.sign())(torch.randn(128, generator=g)) for _ in range(5)])
    if kind.startswith("iso"):
        c.real, routing = int(kind[3]), kind[5:]
        n = torch.arange(128)
        for br in range(2):
            for i in range(5):
                if i == c.real:
                    continue
                dy, dx = {"near": (0, 0), "far": PB_FAR_TAPS[i]}.get(routing, (None, None))
                kh = torch.randint(0, 3, (128,), generator=g) if dy is None else torch.full((128,), 1 + dy)
                kw = torch.randint(0, 3, (128,), generator=g) if dx is None else torch.full((128,), 1 + dx)
                w = torch.zeros(128, 128, 3, 3)
                w[n, n, kh, kw] = 1.0
                c.w[br][i], c.scale[br][i], c.bias[br][i] = w.to(BF), torch.ones(128), torch.zeros(128)
    draw = lambda: (torch.randn(15, 20, 128, generator=g) * live[:, :, None]).to(BF)
    c.x = [torch.stack([draw() for _ in range(B)]) for _ in range(2)]
    for br in range(2):
        todo = torch.arange(B)
        for it in range(200):
            r = pb_branch(c, br, c.x[br][todo], bounds=False)
            bad = torch.zeros(len(todo), dtype=torch.bool)
            for z in r.z:
                bad |= (z.abs() <= 2 * MARGIN).flatten(1).any(1)
            todo = todo[bad]
            if not len(todo):
                break
            for b in todo.tolist():
                c.x[br][b] = draw()
    return c


def pb_margin(c):
    return min(float(z.abs().min()) for r in pb_forward(c) for z in r.z)


def pb_ratio(ys, ref):
    """Worst |y - v| / out_tol over every element of both branches' f32 outputs [B,2,3,128]."""
    return max(error_ratio(y.float().cpu(), r.v, out_tol(r.v, r.E, F32))[0] for y, r in zip(ys, ref))


# ============================================================================================================================== 3. MLP chain
# y_l = act(bf16(y_{l-1}) W_l^T + b_l), 32 rows per workgroup, f32 taps.  Width classes: N <= 256 (four K ranges per tile), <= 512 (two),
# wider (none); K is padded to 512 / 256 / 128 accordingly; 8 tiles x (1 | 2 | 4) per pass (N = 288, 800: idle tiles in the last pass).
MLP_GUARD = 3                # spare NaN rows behind every tapped buffer


def L(N, act="relu", tap=None, restart=False, bias=True):
    """One layer of a case: width, activation, column offset of its tapped slice (None: not tapped), restart flag, bias present."""
    return (N, act, tap, restart, bias)


def _mlp(rows, kx, layers, kb=0, rows_per=1, x_off=0):
    return SimpleNamespace(rows=rows, kx=kx, kb=kb, rows_per=rows_per, x_off=x_off, layers=layers)


MLP_CASES = {
    # every width class at its edges, K = 50 in; 513 -> 257 and 257 -> 33 cross a padding step of the narrower classes
    "n_edges_k50": _mlp(33, 50, [L(1024), L(513, tap=1), L(257, "leaky", tap=4), L(33, "none", tap=2), L(1, "sigmoid", tap=3)], x_off=1),
    "n_edges_k3": _mlp(31, 3, [L(512, tap=4), L(256, tap=3), L(32, "none", tap=1), L(288, tap=4), L(800, "leaky", tap=2), L(1, "none", tap=1)], x_off=1),
    "k1_one_row": _mlp(1, 1, [L(32, "sigmoid", tap=1), L(1024, "relu", tap=4), L(256, "none", tap=4, bias=False)]),
    # K at and one past the padding step of each class
    "k512_n256": _mlp(32, 512, [L(256, tap=4), L(64, "none", tap=1)]),
    "k513_n256": _mlp(33, 513, [L(256, tap=3), L(64, "none", tap=4)], x_off=3),
    "k256_n512": _mlp(32, 256, [L(512, tap=4), L(40, "none", tap=1)]),
    "k257_n512": _mlp(33, 257, [L(512, "leaky", tap=1), L(40, "none", tap=4)], x_off=2),
    "k128_n1024": _mlp(65, 128, [L(1024, tap=4), L(8, "none", tap=4)]),
    "k129_n1024": _mlp(31, 129, [L(1024, tap=2), L(7, "sigmoid", tap=1)], x_off=1),
    "k1280_n1024": _mlp(65, 1280, [L(1024, tap=4), L(1024, "none", tap=1)]),
    # the maximum depth, a tap every second or third layer, every activation
    "twelve_layers": _mlp(65, 64, [L(256), L(512, tap=4), L(1024), L(288, "leaky", tap=1), L(800), L(40, "none", tap=2), L(512),
                                   L(512, "leaky", tap=4), L(96, "sigmoid"), L(1024, tap=3), L(33), L(4, "none", tap=4)]),
    # wide, narrow, wide: the narrow layer leaves the columns 64 .. 255 of its region as two layers back wrote them (the chain input /
    # layer 0's output); the packer's zero weights must meet them.  Once on each LDS region
    "wide_narrow_wide_r0": _mlp(33, 1280, [L(1024), L(40, tap=1), L(512, "none", tap=4)]),
    "wide_narrow_wide_r1": _mlp(32, 300, [L(256), L(1024), L(40, tap=4), L(512, "none", tap=2)]),
    # broadcast prefix: rows_per 1, 7 and more than rows; aligned (vector staging) and odd widths (scalar staging)
    "bcast_rows_per_1": _mlp(33, 19, [L(96, tap=1), L(40, "none", tap=4)], kb=5, rows_per=1, x_off=1),
    "bcast_rows_per_7": _mlp(65, 256, [L(512, tap=4), L(256, tap=4), L(4, "none", tap=4)], kb=256, rows_per=7),
    "bcast_rows_per_100": _mlp(65, 36, [L(128, "leaky", tap=2), L(3, "none", tap=1)], kb=12, rows_per=100),
    # parallel stacks over the same rows: two and three stacks of different depth; restarts at odd and even layers
    "restart_two_stacks": _mlp(33, 256, [L(512), L(256, "none", tap=4), L(128, restart=True), L(128), L(6, "none", tap=1)]),
    "restart_three_stacks": _mlp(65, 50, [L(128), L(4, "none", tap=4), L(1024, restart=True, tap=4), L(64), L(3, "sigmoid", tap=2),
                                          L(33, "leaky", restart=True, tap=1)], kb=14, rows_per=7, x_off=1),
}


def mlp_tpw(N):
    return 1 if N <= 256 else 2 if N <= 512 else 4


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    """x [rows, kx] f32 ~ N(0, 1) (a column slice at x_off of a wider buffer), the broadcast prefix, f32 master weights ~ N(0, 1.6^2 / K)
    and biases 0.2 N per layer.  Settled per row (rows are independent): a row with a ReLU / LeakyReLU pre-activation within 2 MARGIN of
    0 anywhere in the float64 chain gets a new draw."""
    s = MLP_CASES[name]
    g = gen(11000 + sum(map(ord, name)))
    c = SimpleNamespace(name=name, **vars(s))
    c.xbuf = torch.randn(s.rows, s.kx + s.x_off + (4 - (s.kx + s.x_off) % 4 if s.x_off else 0), generator=g)
    c.xb = torch.randn(-(-s.rows // s.rows_per), s.kb, generator=g) if s.kb else None
    c.w, c.b, K0 = [], [], s.kx + s.kb
    k = K0
    for (N, act, tap, restart, bias) in s.layers:
        k = K0 if restart else k
        c.w.append(torch.randn(N, k, generator=g) * (1.6 / math.sqrt(k)))
        c.b.append(0.2 * torch.randn(N, generator=g) if bias else None)
        k = N
    for it in range(400):
        bad = torch.zeros(s.rows, dtype=torch.bool)
        for z in mlp_preacts(c):
            bad |= (z.abs() <= 2 * MARGIN).any(1)
        if not bad.any():
            break
        c.xbuf[bad] = torch.randn(int(bad.sum()), c.xbuf.shape[1], generator=g)
    return c


def mlp_x(c):
    return c.xbuf[:, c.x_off:c.x_off + c.kx]


def mlp_input(c, dtype=F64, fault=None):
    """The staged chain input: bf16([x_bcast[r // rows_per] | x[r]]), exact (the f32 operands are given)."""
    x = mlp_x(c)
    if c.xb is None:
        return bf(x.to(dtype))
    r = torch.arange(c.rows)
    idx = (r % c.rows_per) % c.xb.shape[0] if fault == "bcast_row_modulo" else r // c.rows_per
    return bf(torch.cat([c.xb[idx], x], 1).to(dtype))


def _act64(z, E, act):
    """(value, bound carried to the next layer, tolerance of the f32 tap) of an activation on z with bound E."""
    if act == "sigmoid":
        s, tol = sigmoid_tol(z, E)
        return s, tol, tol
    v = z.clamp_min(0) if act == "relu" else torch.where(z > 0, z, LEAK * z) if act == "leaky" else z
    Ev = E + (R32 * v.abs() if act == "leaky" else 0)
    return v, Ev, out_tol(v, Ev, F32)


def mlp_preacts(c):
    """Pre-activations of the ReLU / LeakyReLU layers in the float64 chain."""
    a0 = mlp_input(c)
    a, zs = a0, []
    for (N, act, tap, restart, bias), w, b in zip(c.layers, c.w, c.b):
        a = a0 if restart else a
        z = a @ w.to(BF).double().T + (b.double() if b is not None else 0)
        if act in ("relu", "leaky"):
            zs.append(z)
        a = bf(_act64(z, 0 * z, act)[0])
    return zs


def mlp_buffers(c, device="cpu"):
    """Per layer None or (buffer [rows + MLP_GUARD, off + N + 5 .. 8] of NaN, its slice [:rows, off:off + N])."""
    out = []
    for (N, act, tap, restart, bias) in c.layers:
        if tap is None:
            out.append(None)
            continue
        width = -(-(tap + N + 5) // 4) * 4
        buf = torch.full((c.rows + MLP_GUARD, width), float("nan"), device=device)
        out.append((buf, buf[:c.rows, tap:tap + N]))
    return out


MLP_FAULTS = ("ksplit_partial_dropped", "bcast_row_modulo", "restart_reads_previous", "rows_beyond_rows_leak", "tap_columns_past_n")


def mlp_emulate(c, fault=None):
    """The kernel's algorithm in float32 into NaN-filled tap buffers: the staged bf16 input tile (rows beyond `rows` zero), every layer a
    GEMM over K in chunks of 64, bias, activation, the f32 tap (rows < rows, columns < N), bf16 into the next layer."""
    bufs = mlp_buffers(c)
    R = -(-c.rows // 32) * 32
    a0 = torch.zeros(R, c.kx + c.kb)
    a0[:c.rows] = mlp_input(c, F32, fault)
    a, dropped = a0, False
    for l, ((N, act, tap, restart, bias), w, b) in enumerate(zip(c.layers, c.w, c.b)):
        if restart:
            if fault == "restart_reads_previous":
                a = torch.cat([a, torch.zeros(R, max(0, a0.shape[1] - a.shape[1]))], 1)[:, :a0.shape[1]]
            else:
                a = a0
        w16 = w.to(BF).float()
        ks = 4 // mlp_tpw(N)
        if fault == "ksplit_partial_dropped" and not dropped and ks > 1 and w16.shape[1] > 64:
            part = (torch.arange(w16.shape[1]) // 64) % ks                     # K range p of a tile: the 64-channel blocks with index = p mod ksplit
            w16 = w16 * (part != 1)
            dropped = True
        z = mm32(a, w16, 64) + (b if b is not None else 0)
        v = z.clamp_min(0) if act == "relu" else torch.where(z > 0, z, torch.tensor(0.01) * z) if act == "leaky" else \
            1 / (1 + torch.exp(-z)) if act == "sigmoid" else z
        if tap is not None:
            buf, view = bufs[l]
            view.copy_(v[:c.rows])
            if fault == "rows_beyond_rows_leak" and c.rows % 32:
                buf[c.rows, tap:tap + N] = v[c.rows]
            if fault == "tap_columns_past_n" and N % 32:
                buf[:c.rows, tap + N:tap + N + 1] = 0.0                        # (the padded channel's value: bias 0, weights 0)
        a = bf(v)
    return bufs


def mlp_ratio(c, bufs):
    """Worst |tap - reference| / tolerance over every element of every tapped layer; infinite if anything outside a slice (the columns
    around it, the guard rows) is no longer NaN.  Behind a tap the reference goes on from the kernel's OWN tapped values (their bf16
    rounding is what the kernel fed to the next layer), so every tap is judged on the layers since the previous tap alone."""
    a0 = mlp_input(c)
    a, Ea, worst = a0, torch.zeros_like(a0), 0.0
    per_layer = []
    for l, ((N, act, tap, restart, bias), w, b) in enumerate(zip(c.layers, c.w, c.b)):
        if restart:
            a, Ea = a0, torch.zeros_like(a0)
        z, E = gemm(a, Ea, w.to(BF).double(), None if b is None else b.double())
        v, Ev, tol = _act64(z, E, act)
        if tap is None:
            a, Ea = round_point(v, Ev)
            continue
        buf, view = bufs[l]
        got = view.detach().cpu()
        q = error_ratio(got, v, tol)[0]
        whole = buf.detach().cpu()
        outside = torch.ones_like(whole, dtype=torch.bool)
        outside[:c.rows, tap:tap + N] = False
        if not bool(torch.isnan(whole[outside]).all()):
            q = INF
        per_layer.append((l, q))
        worst = max(worst, q)
        a = bf(got.double().nan_to_num(0.0, 0.0, 0.0))
        Ea = torch.zeros_like(a)
    return worst, per_layer


# ============================================================================================================================== 4. mask head
# p1 = bf16(bf16(relu(bn(W c1))) + relu(bilinear_2x(t1)));  mask = sigmoid(M_b p1 + m_b);  128 pixels per workgroup, builds for <= 64 and
# <= 128 planes.  (B, H, W, nq): one tile with a one-row t1; a one-column t1 (W % 4 != 0: the per-pixel bilinear form); W = 6 (groups of
# four would straddle rows); tiles that start mid-row; whole-row tiles; three images with their own mask operands; the real size; two images
# of the real size.
MH_CASES = ((1, 2, 64, 2), (1, 64, 2, 50), (1, 64, 6, 64), (1, 8, 48, 66), (1, 16, 32, 128), (3, 16, 32, 50), (3, 8, 48, 128), (1, 120, 160, 50),
            (2, 120, 160, 20))          # 300 tiles: more than the CUs of the part, so the persistent form's workgroups walk to a second tile
MH_FOLD_LD = 260             # the folded plane embeddings are [B * nq, >= 257]: columns 0..255 weights, 256 bias, the rest not read


def _up2(t):
    """F.interpolate(scale 2, bilinear, align_corners=False) of NHWC t."""
    return F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def mh_case(B, H, W, nq):
    """c1 [B,H,W,256] / t1 [B,H/2,W/2,256] bf16 ~ 0.5 N(0, 1), lateral weights bf16 ~ N(0, 1/256) with folded BN (one negative scale),
    per-image mask weights f32 ~ N(0, 1/256) and biases N(0, 1), also as the folded embeddings [B * nq, MH_FOLD_LD] with noise in the
    columns behind the bias.  Settled: a pixel with a lateral pre-activation within 2 MARGIN of 0 gets a new c1 row; where an
    interpolated value is, its dominant tap (source pixel dst // 2, weight >= 9/16) is moved."""
    g = gen(13000 + 1000 * B + 131 * H + 17 * W + nq)
    r = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(B=B, H=H, W=W, nq=nq)
    c.c1, c.t1 = (0.5 * r(B, H, W, 256)).to(BF), (0.5 * r(B, H // 2, W // 2, 256)).to(BF)
    c.wl = (r(256, 256) / 16).to(BF)
    c.sc, c.bi = 1 + 0.1 * r(256), 0.1 * r(256)
    c.sc[7] = -c.sc[7]
    c.mask_w, c.mask_b = r(B, nq, 256) / 16, r(B, nq)
    c.fold = torch.cat([c.mask_w, c.mask_b[..., None], r(B, nq, MH_FOLD_LD - 257)], 2).reshape(B * nq, MH_FOLD_LD).contiguous()
    wl, sc, bi = c.wl.double(), c.sc.double(), c.bi.double()
    for it in range(100):
        rows = c.c1.view(-1, 256)
        bad = (((rows.double() @ wl.T) * sc + bi).abs() <= 2 * MARGIN).any(1)
        if not bad.any():
            break
        rows[bad] = (0.5 * r(int(bad.sum()), 256)).to(BF)
    for it in range(40):
        bad = _up2(c.t1.double()).abs() <= 2 * MARGIN
        if not bad.any():
            break
        hit = bad.view(B, H // 2, 2, W // 2, 2, 256).any(4).any(2)
        t = c.t1.double()
        c.t1 = torch.where(hit, t + 0.03 * (it + 1) * torch.where(t >= 0, 1.0, -1.0), t).to(BF)
    return c


def mh_margin(c):
    z = (c.c1.view(-1, 256).double() @ c.wl.double().T) * c.sc.double() + c.bi.double()
    return min(float(z.abs().min()), float(_up2(c.t1.double()).abs().min()))


def mh_reference(c):
    """float64 mask head: p1 (value before its bf16 rounding, bound), logits (value, bound), probabilities (value, tolerance), all NHWC
    / [B,H,W,nq].  The bilinear blend is three dependent f32 operations on exact products of bf16 values and the weights 1/4, 3/4:
    4 x 2^-24 of its absolute-value blend."""
    B, H, W, nq = c.B, c.H, c.W, c.nq
    rows = c.c1.view(-1, 256).double()
    acc, E = gemm(rows, torch.zeros_like(rows), c.wl.double())
    z, Ez = bn(acc, E, c.sc.double(), c.bi.double())
    l16, ul = round_point(z.clamp_min(0), Ez)
    t = c.t1.double()
    up, Eup = _up2(t).reshape(-1, 256), 4 * R32 * _up2(t.abs()).reshape(-1, 256)
    s = l16 + up.clamp_min(0)
    Es = ul + Eup + R32 * s.abs()
    p16, up1 = round_point(s, Es)
    mw = c.mask_w.to(BF).double()
    lg, El = [], []
    for b in range(B):
        sl = slice(b * H * W, (b + 1) * H * W)
        v, Ev = gemm(p16[sl], up1[sl], mw[b], c.mask_b[b].double())
        lg.append(v)
        El.append(Ev)
    lg, El = torch.stack(lg).view(B, H, W, nq), torch.stack(El).view(B, H, W, nq)
    prob, ptol = sigmoid_tol(lg, El)
    return SimpleNamespace(p1=s.view(B, H, W, 256), Ep1=Es.view(B, H, W, 256), logit=lg, Elogit=El, prob=prob, prob_tol=ptol)


MH_FAULTS = ("clamp_last_row", "clamp_last_col", "bias_of_image_0", "planes_64_up_dropped", "planes_64_up_duplicated", "p1_not_rounded")


def mh_emulate(c, fault=None, sigmoid=True):
    """The kernel's algorithm in float32: lateral GEMM over K in chunks of 32, BN as multiply then add, ReLU, bf16; the four taps of
    every output pixel by the kernel's index formulas (sy = max(0.5 (oh + 0.5) - 0.5, 0), y1 = min(y0 + 1, H/2 - 1)), blended in f32,
    ReLU, added, bf16 = p1; mask GEMM in chunks, bias, 1 / (1 + exp(-v)) -> (prob or logits [B,H,W,nq] f32, p1 bf16)."""
    B, H, W, nq = c.B, c.H, c.W, c.nq
    H2, W2 = H // 2, W // 2
    z = mm32(c.c1.view(-1, 256).float(), c.wl.float(), 32) * c.sc + c.bi
    l16 = bf(z.clamp_min(0)).view(B, H, W, 256)

    def taps(n, n2, wrap):
        s = (0.5 * (torch.arange(n, dtype=F32) + 0.5) - 0.5).clamp_min(0)
        i0 = s.floor().long()
        i1 = (i0 + 1) % n2 if wrap else (i0 + 1).clamp_max(n2 - 1)
        return i0, i1, s - i0
    y0, y1, ly = taps(H, H2, fault == "clamp_last_row")
    x0, x1, lx = taps(W, W2, fault == "clamp_last_col")
    t = c.t1.float()
    lx, ly = lx.view(1, 1, W, 1), ly.view(1, H, 1, 1)
    top = (1 - lx) * t[:, y0][:, :, x0] + lx * t[:, y0][:, :, x1]
    bot = (1 - lx) * t[:, y1][:, :, x0] + lx * t[:, y1][:, :, x1]
    s = ((1 - ly) * top + ly * bot).clamp_min(0) + l16
    p16 = bf(s)
    a = s if fault == "p1_not_rounded" else p16
    mw = c.mask_w.to(BF).float()
    out = []
    for b in range(B):
        w = mw[b]
        if fault == "planes_64_up_dropped":
            w = torch.cat([w[:64], 0 * w[64:]])
        if fault == "planes_64_up_duplicated":
            w = torch.cat([w[:64], w[:max(nq - 64, 0)]])
        out.append(mm32(a[b].reshape(-1, 256), w, 32) + c.mask_b[0 if fault == "bias_of_image_0" else b])
    v = torch.stack(out).view(B, H, W, nq)
    return (1 / (1 + torch.exp(-v)) if sigmoid else v), p16.to(BF)


def mh_ratio(ref, prob=None, logit=None, p1=None):
    """Worst |kernel - reference| / tolerance over every element of the outputs given: probabilities and logits [B,H,W,nq] as f32, p1 as
    a bf16 store."""
    q = 0.0
    if prob is not None:
        q = max(q, error_ratio(prob.float().cpu(), ref.prob, ref.prob_tol)[0])
    if logit is not None:
        q = max(q, error_ratio(logit.float().cpu(), ref.logit, out_tol(ref.logit, ref.Elogit, F32))[0])
    if p1 is not None:
        q = max(q, error_ratio(p1.float().cpu(), ref.p1, out_tol(ref.p1, ref.Ep1, BF))[0])
    return q


def mh_own_p1_ratio(c, p1, prob=None, logit=None):
    """The mask GEMM alone: the probabilities / logits of a launch against float64 on the bf16 p1 the SAME launch stored - the tile its
    GEMM read - so the bound is the accumulation's 2^-20 A with no rounding point in between."""
    B, H, W, nq = c.B, c.H, c.W, c.nq
    a = p1.float().cpu().double().view(B, H * W, 256)
    mw, q = c.mask_w.to(BF).double(), 0.0
    for b in range(B):
        v, E = gemm(a[b], torch.zeros_like(a[b]), mw[b], c.mask_b[b].double())
        if logit is not None:
            q = max(q, error_ratio(logit[b].float().cpu().reshape(H * W, nq), v, out_tol(v, E, F32))[0])
        if prob is not None:
            s, tol = sigmoid_tol(v, E)
            q = max(q, error_ratio(prob[b].float().cpu().reshape(H * W, nq), s, tol)[0])
    return q
