"""The f32 implicit-GEMM conv (csrc/conv_igemm.hip: conv_igemm_kernel<float, float, ...>, behind every f32 ops.conv2d / ops.linear) and
the stride-1 input gradient that is the same kernel again (csrc/conv_bwd.hip: dgrad_weight_kernel + nopesac_conv2d_nhwc_ex) as data:
the host's choice among the kernel's six builds restated, seeded cases, float64 references, allowances, and a float32 restatement of
the kernel's summation in which errors can be planted.  tests/test_conv_f32_forms_gpu.py holds the kernels to it;
tests/test_conv_f32_forms_cpu.py proves the case lists, the constants, the references, the committed figures and the sharpness of the
bound.  Imports without a GPU.

The rule is the backbone sweep's (tests/backbone_forms.py): per element an allowance A_k = 2^-24 S_k + C_k and the limit
LIMIT_FACTOR x max(F32_WORST[family], 1).
  S_k    |scale| sum |x w| + |bias| + |residual|: the magnitudes of the terms that make y_k, taken before the activation for ReLU and
         LeakyReLU (1-Lipschitz).  Sigmoid (1/4-Lipschitz): a quarter of the pre-activation sum plus 2 |sigmoid| - that is, 2^-23 |y|
         in A for the exponential's and the division's own rounding; a residual added after the activation enters with its magnitude.
  C_k    the largest change of the float64 result at k over DRAWS seeded draws that multiply every f32 input by 1 +- 2^-23
  F32_WORST  the worst error / A of the float32 restatement of the kernel's summation per family (measured on the CPU, never from the
         kernel): K in tap-major-then-channel order, in blocks of BK = 16 terms, and for the two-level build a flush into a second
         accumulator every FLUSH x BK = 128 terms.
The float64 reference is F.conv2d (its autograd for the dgrad) on the f32 inputs; on a device it is the same sum stated tap by tap as
matrix products (conv_taps / dgrad_taps, which the CPU test holds to F.conv2d), so that the large cases are evaluated where the test
runs.  No element is left out of any comparison."""
from __future__ import annotations

import functools
import itertools
import zlib
from collections import namedtuple

import torch
from torch.nn import functional as F

from nopesac_amd import _lib
from nopesac_amd.synth import _g
from tests.refine_bwd_forms import DRAWS, EPS23, EPS24, F32, F64, LIMIT_FACTOR, _cot, jiggle, ratios

_H = _lib.H
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = _H.NPS_ACT_NONE, _H.NPS_ACT_RELU, _H.NPS_ACT_LEAKY, _H.NPS_ACT_SIGMOID
ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID)
ACT_RES_AFTER, ACT_BIAS_BATCHED = _H.NPS_ACT_RES_AFTER, _H.NPS_ACT_BIAS_BATCHED

# ---- the constants of the kernel and of its launcher (tests/test_conv_f32_forms_cpu.py reads them out of the source)
BK, VECW = 16, 4              # Cfg<float>: floats per K-tile, floats per 16-byte vector
FLUSH = 8                     # two-level build: K-tiles per first-level chain
TWO_LEVEL_K = 512             # launch_cfg: the two-level build from this K on (VEC 4 only)
AUTO_TILES = 192              # launch_dtype: 128x128 tiles when there are at least this many of them ...
SMALL_N = 64                  # ... N is above this ...
STREAM_K = 256                # ... and the call is not a 1x1 with K up to this
XCDS = 8                      # the block-index remap walks 8 contiguous runs of tiles
LEAKY_SLOPE = float(torch.tensor(0.01, dtype=F32))     # apply_act's 0.01f

# worst error / A of the float32 restatement per family.  Printed by
#   python -c "from tests import conv_f32_forms as C; C.print_f32_worst()"
# and re-measured by tests/test_conv_f32_forms_cpu.py (a figure off by more than 2x fails).
F32_WORST = {"fwd_single": 1.23, "fwd_two_level": 0.466, "fwd_vec1": 0.994, "dgrad": 1.09}
FAMILIES = tuple(F32_WORST)

FILL = 7.0                    # what every wider buffer holds outside the slice


def limit(family):
    return LIMIT_FACTOR * max(F32_WORST[family], 1.0)


# ===================================================================================================================== dispatch, restated
# what launch_dtype / launch_cfg see of one f32 / f32 call.  M: rows per grid.y slice; x_align / w_align: the pointers modulo 16 bytes;
# force: NOPESAC_CONV_FORCE ("t128", "t64") or None
Call = namedtuple("Call", "B M N K Cin taps x_cs w_bs x_align w_align batched force")


def generic_form(call):
    """(BM, VEC, two_level) of conv_igemm_kernel<float, float, BM, BM, VEC, 1, two_level> as the host picks it for `call`."""
    vec_ok = (call.Cin % VECW == 0 and call.K % VECW == 0 and call.x_cs % VECW == 0 and call.w_bs % VECW == 0
              and call.x_align % (4 * VECW) == 0 and call.w_align % (4 * VECW) == 0)
    vec = VECW if vec_ok else 1
    two_level = vec == VECW and call.K >= TWO_LEVEL_K
    if call.force in ("t128", "t64"):
        return (128 if call.force == "t128" else 64), vec, two_level
    tiles128 = -(-call.M // 128) * -(-call.N // 128) * (call.B if call.batched else 1)
    small_k_stream = call.taps == 1 and call.K <= STREAM_K
    return (128 if (call.N > SMALL_N and tiles128 >= AUTO_TILES and not small_k_stream) else 64), vec, two_level


def family_of_form(form):
    return "fwd_vec1" if form[1] == 1 else ("fwd_two_level" if form[2] else "fwd_single")


def tile_count(call, form):
    """Workgroups per grid.y slice: what the XCD remap permutes."""
    return -(-call.M // form[0]) * -(-call.N // form[0])


def xcd_remap(bid, nwg):
    """The kernel's block id -> tile id map."""
    q, r, xcd, within = nwg // XCDS, nwg % XCDS, bid % XCDS, bid // XCDS
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + within


# ===================================================================================================================== forward cases
# xp / yp / rp: (columns before, columns after) the slice in the wider x / y / residual buffer; rp None: no residual.  bbias: bias is
# [B, Cout] (batched weights).  linear: through ops.linear on row buffers (B = H = 1, W = rows)
Case = namedtuple("Case", "name B H W Cin Cout k s p force xp yp rp scale bias act res_after batched bbias linear")


def fc(name, B, H, W, Cin, Cout, k=1, s=1, p=0, force="t64", xp=(0, 0), yp=(0, 0), rp=None, scale=True, bias=True, act=ACT_RELU,
       res_after=False, batched=False, bbias=False, linear=False):
    return Case(name, B, H, W, Cin, Cout, k, s, p, force, xp, yp, rp, scale, bias, act, res_after, batched, bbias, linear)


def _forward_cases():
    c = []
    # K tails at VEC 4 (dense 1x1, H = 1, M = 70 < 128, M % 64 = 6): below one tile, K % 16 in {0, 4, 12}
    for K in (4, 12, 16, 20, 28, 32):
        c.append(fc("k%d" % K, 1, 1, 70, K, 24))
    c += [fc("k20_t128", 1, 1, 70, 20, 24, force="t128"), fc("k28_t128", 1, 1, 70, 28, 24, force="t128")]
    # VEC 1, four ways: Cin % 4 (the stem's 7x7 / stride 2 / pad 3 on 3 channels: K = 147; 5 channels at 3x3: K = 45; 3 at 3x3: K = 27),
    # an x slice 4 bytes off a 16-byte boundary, a channel stride that is no multiple of 4
    for force in ("t64", "t128"):
        t = "" if force == "t64" else "_t128"
        c += [fc("c3_k7_s2" + t, 2, 9, 11, 3, 8, k=7, s=2, p=3, force=force), fc("c5_k3" + t, 1, 5, 9, 5, 12, k=3, p=1, force=force),
              fc("c3_k3" + t, 1, 5, 9, 3, 12, k=3, p=1, force=force), fc("x_off4" + t, 1, 1, 70, 32, 24, xp=(1, 3), force=force),
              fc("x_cs_odd" + t, 1, 1, 70, 32, 24, xp=(0, 1), force=force)]
    # two-level flush boundaries: nk = ceil(K / 16) in {32, 33, 39, 40, 41}; a 3x3 with K = 576; one long chain at five rows
    for K in (512, 516, 624, 640, 644):
        c.append(fc("tl%d" % K, 1, 1, 70, K, 24))
    c += [fc("tl512_t128", 1, 1, 70, 512, 24, force="t128"), fc("tl644_t128", 1, 1, 130, 644, 72, force="t128"),
          fc("tl_k3", 2, 5, 9, 64, 24, k=3, p=1), fc("tl_k3_t128", 2, 5, 9, 64, 24, k=3, p=1, force="t128"),
          fc("tl4608", 1, 1, 5, 4608, 8), fc("tl4608_t128", 1, 1, 5, 4608, 8, force="t128")]
    # VEC 1 gives up the two-level accumulation: a misaligned slice with K >= 512 runs one chain (recorded in docs/kernels.md)
    c += [fc("chain644_vec1", 1, 1, 70, 644, 24, xp=(1, 3)), fc("chain4608_vec1", 1, 1, 5, 4608, 8, xp=(1, 3)),
          fc("chain4608_vec1_t128", 1, 1, 5, 4608, 8, xp=(1, 3), force="t128")]
    # M: M % BM in {1, BM - 1, 0}, one row, a tile across two (three) images
    for M in (1, 65, 127, 128):
        c.append(fc("m%d" % M, 1, 1, M, 20, 8))
    for M in (129, 255, 256):
        c.append(fc("m%d_t128" % M, 1, 1, M, 20, 8, force="t128"))
    c += [fc("straddle", 3, 5, 9, 8, 8, k=3, p=1), fc("straddle_t128", 4, 5, 9, 8, 8, k=3, p=1, force="t128")]
    # N, dense (Cout % 4 != 0: the scalar epilogue), N = 300 in a 304-wide buffer, a residual out of a wider buffer
    for N in (1, 3, 31, 33, 64, 65):
        c.append(fc("n%d" % N, 1, 1, 70, 20, N, rp=(0, 0)))
    c += [fc("n65_t128", 1, 1, 70, 20, 65, rp=(0, 0), force="t128"), fc("n300_in_304", 1, 1, 70, 20, 300, yp=(0, 4)),
          fc("n300_res_wide", 1, 1, 70, 20, 300, yp=(0, 4), rp=(4, 4)),
          fc("n300_res_wide_t128", 1, 1, 300, 20, 300, yp=(0, 4), rp=(4, 4), force="t128")]
    # the XCD remap: 7, 8 (4 x 2), 9 (3 x 3) and 17 tiles (1: most cases; 9 at 128x128: n300_res_wide_t128)
    c += [fc("tiles7", 1, 1, 7 * 64 - 3, 8, 8), fc("tiles8", 1, 1, 256, 8, 100), fc("tiles9", 1, 1, 150, 8, 150),
          fc("tiles17", 1, 1, 17 * 64 - 10, 8, 8)]
    # general addressing
    c += [fc("s2_1x1", 2, 5, 9, 8, 8, s=2), fc("k3_s1", 2, 5, 9, 8, 12, k=3, p=1), fc("k3_s2", 2, 5, 9, 8, 12, k=3, s=2, p=1),
          fc("k7_s2_c4", 1, 9, 11, 4, 8, k=7, s=2, p=3), fc("h1_k3", 1, 1, 9, 8, 8, k=3, p=1), fc("w1_k3", 1, 9, 1, 8, 8, k=3, p=1),
          fc("k3_p0", 1, 5, 9, 8, 8, k=3, p=0), fc("k3_s1_t128", 2, 9, 10, 8, 12, k=3, p=1, force="t128")]
    # the epilogue: activation x residual (absent, before, after) with scale / bias cycling through present / absent; vector (N = 24)
    # at 64x64 and scalar (N = 6) at 128x128, then the other way round for the residual forms
    sb = ((True, True), (True, False), (False, True), (False, False))
    for i, (act, res) in enumerate(itertools.product(ACTS, ("none", "before", "after"))):
        for N, force in ((24, "t64"), (6, "t128")) + (((24, "t128"), (6, "t64")) if res != "none" else ()):
            c.append(fc("epi_a%d_%s_n%d_%s" % (act, res, N, force), 1, 1, 70, 20, N, force=force, rp=None if res == "none" else (0, 0),
                        scale=sb[(i + N) % 4][0], bias=sb[(i + N) % 4][1], act=act, res_after=res == "after"))
    # y / residual 4 bytes off a 16-byte boundary: the scalar epilogue at Cout % 4 == 0
    c += [fc("y_off4", 1, 1, 70, 20, 24, yp=(1, 3), rp=(0, 0)), fc("r_off4", 1, 1, 70, 20, 24, rp=(1, 3), res_after=True),
          fc("r_cs_odd", 1, 1, 70, 20, 24, rp=(0, 1))]
    # batched weights (grid.y = image, M = rows per image): no bias, one bias row, a bias row per image (vector and scalar epilogue),
    # B = 1 (the wrapper does not set the flag), general addressing, the two-level build, more than one tile per image
    c += [fc("bat_plain", 3, 1, 70, 20, 24, batched=True, scale=False, bias=False, act=ACT_NONE),
          fc("bat_bias_shared", 3, 1, 70, 20, 24, batched=True), fc("bat_bias_image", 3, 1, 70, 20, 24, batched=True, bbias=True, act=ACT_SIGMOID),
          fc("bat_bias_image_n6", 3, 1, 70, 20, 6, batched=True, bbias=True, scale=False), fc("bat_b1", 1, 1, 70, 20, 24, batched=True),
          fc("bat_k3", 2, 5, 9, 8, 12, k=3, p=1, batched=True, bbias=True, rp=(0, 0)),
          fc("bat_tl", 2, 1, 70, 512, 24, batched=True, bbias=True),
          fc("bat_t128", 3, 1, 130, 20, 72, batched=True, bbias=True, force="t128", rp=(0, 4), res_after=True)]
    # ops.linear on column slices of wider row buffers
    c += [fc("lin_dense", 1, 1, 70, 20, 24, linear=True, act=ACT_NONE, scale=False),
          fc("lin_slices", 1, 1, 70, 20, 24, linear=True, xp=(4, 4), yp=(4, 4), rp=(8, 0), act=ACT_LEAKY),
          fc("lin_slices_odd", 1, 1, 70, 20, 24, linear=True, xp=(1, 2), yp=(3, 2), rp=(1, 0), scale=False),
          fc("lin_tl", 1, 1, 70, 516, 24, linear=True, xp=(4, 0), yp=(0, 4))]
    # the host's own choice: 64x64, and 128x128 at 192 tiles of 128x128 (M = 12288, N = 256, K = 36)
    c += [fc("auto64", 1, 5, 9, 8, 12, k=3, p=1, force=None), fc("auto128", 1, 96, 128, 4, 256, k=3, p=1, force=None, rp=(0, 0))]
    return tuple(c)


FORWARD_CASES = _forward_cases()
FORWARD = {c.name: c for c in FORWARD_CASES}
DEVICE_REFERENCE = ("auto128",)                    # float64 reference and draws evaluated where the test runs


def out_hw(c):
    return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1


def call_of(c):
    OH, OW = out_hw(c)
    K = c.k * c.k * c.Cin
    return Call(c.B, OH * OW if c.batched else c.B * OH * OW, c.Cout, K, c.Cin, c.k * c.k, c.Cin + sum(c.xp), c.Cout * K if c.batched else 0,
                4 * c.xp[0] % 16, 0, c.batched, c.force)


def family(c):
    return family_of_form(generic_form(call_of(c)))


def epilogue_vector(c):
    """conv_epi_vec and the batched-bias condition: whether the epilogue takes its 8-channel vector path."""
    ok = (c.Cout + sum(c.yp)) % 4 == 0 and c.yp[0] % 4 == 0
    if c.rp is not None:
        ok = ok and (c.Cout + sum(c.rp)) % 4 == 0 and c.rp[0] % 4 == 0
    return ok and not (c.bbias and c.B > 1 and c.Cout % 4 != 0)


@functools.lru_cache(maxsize=None)
def forward_inputs(name):
    """x [B, H, W, Cin], w [Cout, k, k, Cin] ([B, ...] batched), scale / bias [Cout] (bias [B, Cout] per image), residual: f32, CPU."""
    c = FORWARD[name]
    g = _g(81000 + zlib.crc32(name.encode()) % 100000)
    OH, OW = out_hw(c)
    K = c.k * c.k * c.Cin
    lead = (c.B,) if c.batched else ()
    t = dict(x=_cot(g, c.B, c.H, c.W, c.Cin), w=torch.randn(*lead, c.Cout, c.k, c.k, c.Cin, generator=g) * K ** -0.5)
    t["scale"] = 0.3 + 0.7 * torch.randn(c.Cout, generator=g) if c.scale else None
    t["bias"] = 0.5 * torch.randn(*((c.B,) if c.bbias else ()), c.Cout, generator=g) if c.bias else None
    t["residual"] = torch.randn(c.B, OH, OW, c.Cout, generator=g) if c.rp is not None else None
    return t


def _widen(t, pad, fill, device):
    """t [..., C] as the slice [pad[0] : pad[0] + C] of a buffer of `fill` -> (buffer, view)."""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + sum(pad),), fill, dtype=F32, device=device)
    view = buf[..., pad[0]:pad[0] + t.shape[-1]]
    view.copy_(t)
    return buf, view


def forward_buffers(name, device, out_fill=float("nan")):
    """The case's tensors on `device` as the wrapper takes them: x / residual / out as slices of buffers of FILL, out filled with
    `out_fill`.  A linear case: row buffers [2, rows / 2, width] (rows even) or [rows, width]."""
    c, t = FORWARD[name], forward_inputs(name)
    OH, OW = out_hw(c)
    b = dict(w=t["w"].to(device), scale=None if t["scale"] is None else t["scale"].to(device),
             bias=None if t["bias"] is None else t["bias"].to(device))
    b["x_buf"], b["x"] = _widen(t["x"], c.xp, FILL, device)
    b["y_buf"], b["y"] = _widen(torch.full((c.B, OH, OW, c.Cout), out_fill), c.yp, FILL, device)
    b["r_buf"], b["r"] = _widen(t["residual"], c.rp, FILL, device) if c.rp is not None else (None, None)
    if c.linear:
        rows = c.W
        lead = (2, rows // 2) if rows % 2 == 0 else (rows,)
        for k in ("x", "y", "r"):
            if b[k] is not None:
                C = b[k].shape[-1]
                b[k + "_buf"] = b[k + "_buf"].view(*lead, -1)
                pad = {"x": c.xp, "y": c.yp, "r": c.rp}[k]
                b[k] = b[k + "_buf"][..., pad[0]:pad[0] + C]
        b["w"] = b["w"].view(c.Cout, c.Cin)
    return b


def act_word(c):
    return c.act | (ACT_RES_AFTER if c.res_after else 0)


def run_forward(ops, name, b):
    """The call, through ops.conv2d or ops.linear -> y as [B, OH, OW, Cout] (a view of b["y"])."""
    c = FORWARD[name]
    if c.linear:
        ops.linear(b["x"], b["w"], b["bias"], act=act_word(c), residual=b["r"], out=b["y"], scale=b["scale"])
    else:
        ops.conv2d(b["x"], b["w"], b["scale"], b["bias"], b["r"], stride=c.s, pad=c.p, act=act_word(c), out=b["y"], batched_weights=c.batched)
    return b["y"].reshape(c.B, *out_hw(c), c.Cout)


# ---- float64
def conv_torch(x, w, s, p):
    """F.conv2d, NHWC in and out; w [N, k, k, C] or one [N, k, k, C] per image."""
    if w.dim() == 5:
        return torch.cat([conv_torch(x[i:i + 1], w[i], s, p) for i in range(x.shape[0])])
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def conv_taps(x, w, s, p):
    """The same sum tap by tap as matrix products (any device): the tap's strided window of the zero-padded input times its [N, C]."""
    B, H, W, C = x.shape
    k = w.shape[-2]
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(x, (0, 0, p, p, p, p))
    out = torch.zeros(B, OH, OW, w.shape[-4], dtype=x.dtype, device=x.device)
    for kh in range(k):
        for kw in range(k):
            win = xp[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s]
            wt = w[..., kh, kw, :]
            out += win @ wt.t() if w.dim() == 4 else torch.einsum("bhwc,bnc->bhwn", win, wt)
    return out


def _conv(device):
    return conv_torch if str(device) == "cpu" else conv_taps


def activation(v, act):
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, LEAKY_SLOPE * v)
    return torch.sigmoid(v) if act == ACT_SIGMOID else v


def _per_image(bias, c):
    return bias.view(c.B, 1, 1, c.Cout) if c.bbias else bias


def forward_eval(c, t, conv):
    """y of the case at tensors t (any dtype / device)."""
    v = conv(t["x"], t["w"], c.s, c.p)
    if t["scale"] is not None:
        v = v * t["scale"]
    if t["bias"] is not None:
        v = v + _per_image(t["bias"], c)
    if t["residual"] is not None and not c.res_after:
        v = v + t["residual"]
    v = activation(v, c.act)
    return v + t["residual"] if (t["residual"] is not None and c.res_after) else v


def forward_magnitudes(c, t, conv, y):
    """S of the module docstring."""
    S = conv(t["x"].abs(), t["w"].abs(), c.s, c.p)
    if t["scale"] is not None:
        S = S * t["scale"].abs()
    if t["bias"] is not None:
        S = S + _per_image(t["bias"], c).abs()
    r = t["residual"]
    if r is not None and not c.res_after:
        S = S + r.abs()
    if c.act == ACT_SIGMOID:
        S = S / 4 + 2 * (y - r if (r is not None and c.res_after) else y).abs()
    return S + r.abs() if (r is not None and c.res_after) else S


@functools.lru_cache(maxsize=None)
def forward_reference(name, device="cpu"):
    """-> (ref, A) on the CPU, [B, OH, OW, Cout] float64, evaluated on `device`."""
    c, t32 = FORWARD[name], forward_inputs(name)
    conv = _conv(device)
    t = {k: None if v is None else v.to(device=device, dtype=F64) for k, v in t32.items()}
    ref = forward_eval(c, t, conv)
    S = forward_magnitudes(c, t, conv, ref)
    g = _g(88)
    C = torch.zeros_like(ref)
    for _ in range(DRAWS):
        tj = {k: None if v is None else jiggle(v, g).to(device) for k, v in t32.items()}
        C = torch.maximum(C, (forward_eval(c, tj, conv) - ref).abs())
    return ref.cpu(), (EPS24 * S + C).cpu()


def _worst(got, ref, A):
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    q = ratios(got.detach().cpu(), ref, A).reshape(-1)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max()), int(q.argmax())


def forward_worst(name, got, device="cpu"):
    """(worst error / A, flat index) of `got` [B, OH, OW, Cout]; a NaN counts as inf."""
    return _worst(got, *forward_reference(name, device))


# ---- float32: the kernel's summation
def im2col(x, k, s, p):
    """[B, H, W, C] -> [B, OH * OW, k * k * C], K in the kernel's order: tap-major, then channel."""
    B, H, W, C = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(x, (0, 0, p, p, p, p))
    cols = [xp[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s] for kh in range(k) for kw in range(k)]
    return torch.cat(cols, -1).reshape(B, OH * OW, k * k * C)


ACCUMULATE_PLANTS = ("no_hi", "flush_last", "k_tail")


def accumulate(A, Wm, two_level, plant=None):
    """A [G, M, K] x Wm [N, K] or [G, N, K] in float32 as the kernel sums: one K-tile of BK terms after another into one accumulator;
    two_level: after every FLUSH tiles but the last the accumulator is added into a second one and cleared, and the second is added at
    the end.  Plants: "no_hi" - the second accumulator is not added at the end; "flush_last" - the flush is also taken on the last tile
    (without the clear that the loop's end never needs), so its terms are counted twice; "k_tail" - the last, partial tile is dropped."""
    K = A.shape[-1]
    nk = K // BK if plant == "k_tail" else -(-K // BK)
    acc = torch.zeros(A.shape[0], A.shape[1], Wm.shape[-2], dtype=A.dtype)
    hi = torch.zeros_like(acc)
    for kt in range(nk):
        sl = slice(kt * BK, min(K, (kt + 1) * BK))
        acc = acc + A[..., sl] @ Wm[..., sl].transpose(-1, -2)
        if two_level and kt % FLUSH == FLUSH - 1:
            if kt + 1 < nk:
                hi, acc = hi + acc, torch.zeros_like(acc)
            elif plant == "flush_last":
                hi = hi + acc
    return acc + hi if (two_level and plant != "no_hi") else acc


FORWARD_PLANTS = ACCUMULATE_PLANTS + ("res_side", "bias_image0")


def emulate_forward(name, plant=None):
    """The forward call in float32 as the kernel computes it (accumulate, then scale, bias, residual and activation in the epilogue's
    order).  Plants: those of accumulate; "res_side" - the residual is added on the other side of the activation; "bias_image0" - the
    batched form reads image 0's bias row for every image."""
    c, t = FORWARD[name], forward_inputs(name)
    OH, OW = out_hw(c)
    A = im2col(t["x"], c.k, c.s, c.p)
    Wm = t["w"].reshape(*t["w"].shape[:-4], c.Cout, -1)
    if not c.batched:
        A = A.reshape(1, -1, A.shape[-1])
    v = accumulate(A, Wm, generic_form(call_of(c))[2], plant if plant in ACCUMULATE_PLANTS else None).reshape(c.B, OH, OW, c.Cout)
    if t["scale"] is not None:
        v = v * t["scale"]
    if t["bias"] is not None:
        v = v + (t["bias"][0] if (plant == "bias_image0" and c.bbias) else _per_image(t["bias"], c))
    after = c.res_after != (plant == "res_side")
    r = t["residual"]
    if r is not None and not after:
        v = v + r
    v = activation(v, c.act)
    return v + r if (r is not None and after) else v


def plant_applies(name, plant):
    """Whether `plant` changes the arithmetic of the case at all."""
    c = FORWARD[name]
    call = call_of(c)
    two_level, nk = generic_form(call)[2], -(-call.K // BK)
    # (the last partial tile of a 3x3 on a one-row image is padding only: dropping it drops zeros)
    tail = call.K % BK != 0 and bool(im2col(forward_inputs(name)["x"], c.k, c.s, c.p)[..., call.K // BK * BK:].any())
    return {"no_hi": two_level and nk > FLUSH, "flush_last": two_level and nk % FLUSH == 0, "k_tail": tail,
            "res_side": c.rp is not None and c.act != ACT_NONE, "bias_image0": c.bbias and c.B > 1}[plant]


# ===================================================================================================================== stride-1 dgrad
DGRAD_K = (1, 3)
DGRAD_HW = ((1, 1), (2, 3), (5, 9), (7, 10))
DGRAD_B = (1, 2)
# (Cin, Cout); the inner conv has Cin and Cout swapped and K = k k Cout: (5, 7) makes it VEC 1; Cout = 64 at k = 3 is K = 576, the
# two-level build (Cout = 132: K = 1188)
DGRAD_CC = ((4, 4), (12, 8), (64, 132), (132, 64), (5, 7))
# (k, B, H, W, Cin, Cout, tag).  base: dense dy and dx.  dy_slice: dy is channels [4, 4 + Cout) of a wider buffer; dy_off1: channels
# [1, 1 + Cout) (the inner conv's x 4 bytes off: VEC 1); dx304: dx is channels [0, Cin) of a buffer of FILL 4 channels wider
GRID_CASES = tuple((k, b, h, w, ci, co, "base") for k in DGRAD_K for h, w in DGRAD_HW for b in DGRAD_B for ci, co in DGRAD_CC)
SLICE_CASES = tuple((k, 2, 5, 9, ci, co, tag) for k in DGRAD_K for ci, co, tag in
                    ((12, 8, "dy_slice"), (132, 64, "dy_slice"), (12, 8, "dy_off1"), (132, 64, "dy_off1"), (300, 8, "dx304"), (5, 7, "dx304")))
DGRAD_CASES = GRID_CASES + SLICE_CASES
# the pixel pose net at 480 x 640, B = 1: the longest inner K (convs_backbone.*: 9 x 256 = 2304), the 300-in-304 layer (the branches' first
# conv) and a 1x1 (pixel_decoder.adapter_2).  Their float64 references are evaluated on the device; not part of F32_WORST
PRODUCTION_CASES = ((3, 1, 60, 80, 256, 256, "base"), (3, 1, 15, 20, 300, 128, "dx304"), (1, 1, 30, 40, 1024, 128, "base"))
IDENTITY_CASES = ((3, 2, 7, 10, 132, 64, "base"), (3, 2, 5, 9, 5, 7, "dx304"))
DY_PAD = {"base": (0, 0), "dx304": (0, 0), "dy_slice": (4, 4), "dy_off1": (1, 3)}
DX_PAD = {"base": (0, 0), "dx304": (0, 4), "dy_slice": (0, 0), "dy_off1": (0, 0)}
# one-hot rotation statement: (k, H, W, Cin, Cout) x pixels (an interior one - all nine taps land inside - and the four corners)
ROTATION_SHAPES = ((3, 5, 6, 12, 8), (3, 5, 6, 5, 7), (3, 5, 6, 132, 64), (1, 5, 6, 12, 8))
ROTATION_PIXELS = ((2, 3), (0, 0), (0, 5), (4, 0), (4, 5))


def dgrad_call(key):
    """The inner forward call of nopesac_conv2d_dgrad_f32: Cin and Cout swapped, dy as x, the rotated weights in scratch (aligned)."""
    k, B, H, W, Cin, Cout, tag = key
    return Call(B, B * H * W, Cin, k * k * Cout, Cout, k * k, Cout + sum(DY_PAD[tag]), 0, 4 * DY_PAD[tag][0] % 16, 0, False, None)


@functools.lru_cache(maxsize=None)
def dgrad_inputs(key):
    k, B, H, W, Cin, Cout, tag = key
    g = _g(82000 + zlib.crc32(repr(key).encode()) % 100000)
    return dict(key=key, k=k, pad=(k - 1) // 2, B=B, H=H, W=W, Cin=Cin, Cout=Cout, dy=_cot(g, B, H, W, Cout),
                w=torch.randn(Cout, Cin, k, k, generator=g) * (Cout * k * k) ** -0.5)


def dgrad_autograd(dy, w, pad):
    """The input gradient of the same-size stride-1 conv from F.conv2d's autograd; dy NHWC, w [Cout, Cin, k, k] -> NHWC."""
    x = torch.zeros(dy.shape[0], w.shape[1], dy.shape[1], dy.shape[2], dtype=dy.dtype, requires_grad=True)
    y = F.conv2d(x, w, padding=pad)
    return torch.autograd.grad(y, x, dy.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1).contiguous()


def dgrad_taps(dy, w, pad):
    """The same gradient tap by tap (any device): dy [pixels, Cout] @ w[:, :, kh, kw] lands on the padded input at offset (kh, kw)."""
    B, H, W, _ = dy.shape
    k = w.shape[2]
    dxp = torch.zeros(B, H + 2 * pad, W + 2 * pad, w.shape[1], dtype=dy.dtype, device=dy.device)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + H, kw:kw + W] += dy @ w[:, :, kh, kw]
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


@functools.lru_cache(maxsize=None)
def dgrad_reference(key, device="cpu"):
    """-> (ref, A) on the CPU: the float64 gradient [B, H, W, Cin] and 2^-24 S + C per element, evaluated on `device`."""
    c = dgrad_inputs(key)
    run = dgrad_autograd if str(device) == "cpu" else dgrad_taps
    to = lambda t: t.to(device=device, dtype=F64)
    ref = run(to(c["dy"]), to(c["w"]), c["pad"])
    S = run(to(c["dy"]).abs(), to(c["w"]).abs(), c["pad"])
    g = _g(89)
    C = torch.zeros_like(ref)
    for _ in range(DRAWS):
        C = torch.maximum(C, (run(jiggle(c["dy"], g).to(device), jiggle(c["w"], g).to(device), c["pad"]) - ref).abs())
    return ref.cpu(), (EPS24 * S + C).cpu()


def dgrad_worst(key, got, device="cpu"):
    return _worst(got, *dgrad_reference(key, device))


def rotate(w, plant=None):
    """dgrad_weight_kernel in plain torch: w [Cout, Cin, KH, KW] -> [Cin, KH, KW, Cout], taps rotated by 180 degrees.  Plants:
    "no_kw_flip" / "no_kh_flip" - transposed, but that axis is not flipped."""
    wf = w.permute(1, 2, 3, 0)
    return wf.flip(*((1,) if plant != "no_kh_flip" else ()), *((2,) if plant != "no_kw_flip" else ())).contiguous()


DGRAD_PLANTS = ("no_kw_flip", "no_kh_flip")


def emulate_dgrad(key, plant=None):
    """The stride-1 dgrad in float32 as the library computes it: the rotated weights, then the forward summation of the inner call."""
    c = dgrad_inputs(key)
    k = c["k"]
    A = im2col(c["dy"], k, 1, k - 1 - c["pad"]).reshape(1, -1, k * k * c["Cout"])
    return accumulate(A, rotate(c["w"], plant).reshape(c["Cin"], -1), generic_form(dgrad_call(key))[2]).reshape(c["B"], c["H"], c["W"], c["Cin"])


def dgrad_buffers(key, device, out_fill=float("nan")):
    """dy and dx on `device` as slices of buffers of FILL (dense for "base") -> dict(dy_buf, dy, dx_buf, dx, w)."""
    c = dgrad_inputs(key)
    tag = key[-1]
    b = dict(w=c["w"].to(device))
    b["dy_buf"], b["dy"] = _widen(c["dy"], DY_PAD[tag], FILL, device)
    b["dx_buf"], b["dx"] = _widen(torch.full((c["B"], c["H"], c["W"], c["Cin"]), out_fill), DX_PAD[tag], FILL, device)
    return b


def one_hot_expected(w, H, W, ph, pw, co):
    """dx [H, W, Cin] of dy = 1.0 at (ph, pw, co), zero elsewhere: output pixel (ph, pw) read input pixel (ih, iw) through the tap
    (ih - ph + pad, iw - pw + pad), so dx[ih, iw, ci] = w[co, ci, ih - ph + pad, iw - pw + pad] where that tap exists and +0.0
    elsewhere - exactly, since every product is with 1.0 or 0.0."""
    k = w.shape[2]
    pad = (k - 1) // 2
    dx = torch.zeros(H, W, w.shape[1])
    for ih in range(H):
        for iw in range(W):
            kh, kw = ih - ph + pad, iw - pw + pad
            if 0 <= kh < k and 0 <= kw < k:
                dx[ih, iw] = w[co, :, kh, kw]
    return dx


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ===================================================================================================================== the committed figures
def f32_worst():
    """{family: the worst error / A of the float32 restatement over the family's cases}."""
    out = dict.fromkeys(FAMILIES, 0.0)
    for c in FORWARD_CASES:
        out[family(c)] = max(out[family(c)], forward_worst(c.name, emulate_forward(c.name))[0])
    out["dgrad"] = max(dgrad_worst(key, emulate_dgrad(key))[0] for key in DGRAD_CASES)
    return out


def print_f32_worst():
    print("F32_WORST = {%s}" % ", ".join('"%s": %.3g' % kv for kv in f32_worst().items()))
