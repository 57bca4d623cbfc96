"""The streaming, norm and optimiser kernels around the GEMMs (csrc/elementwise.hip, the utility / optimiser tail of csrc/refine_bwd.hip)
as data: which BUILD or PATH each entry point picks for its arguments (a restatement of the host dispatch, so a test can name what it
reaches), float64 references of every operation in plain torch on the f32- / bf16-rounded inputs the kernel gets, with the per-element
magnitude S = sum |terms| an error is judged against, plain f32 formulations of the documented algorithms (their error against the
float64 reference is the FLOOR a bound is derived from), input generators that keep every activation decision off its margin, and the
case lists of tests/test_stream_forms_gpu.py.  tests/test_stream_forms_cpu.py proves the tables complete and the references right.
Imports without a GPU."""
from __future__ import annotations

import functools

import torch
from torch.nn import functional as F

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2       # include/nopesac_hip.h NPS_ACT_*
REFUSED = "refused"
MARGIN = 1e-3                                 # no ReLU pre-activation of a case lies closer to 0 than this (float64)
# A bound is FLOOR_FACTOR x the floor of its family: the kernels sum in another order and depth than torch does.  A floor is never below
# EPS32 = 2^-24: every f32 result carries half an ulp of its own rounding, and the floor of a reduction to ONE number is a single random
# draw that can come out as 0.
FLOOR_FACTOR = 8.0
EPS32 = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126
DT_NAME = {F32: "f32", BF16: "bf16"}


def gen(seed):
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def bf16_ulp(ref):
    """The bf16 unit in the last place at |ref| (float64 tensor): 2^(floor(log2 |ref|) - 7); the smallest denormal at 0."""
    _, e = torch.frexp(ref.abs())
    u = torch.ldexp(torch.ones_like(ref), (e - 8).clamp_min(-133))
    return torch.where(ref == 0, torch.full_like(ref, 2.0 ** -133), u)


def quotient(got, ref, S):
    """max over EVERY element of |got - ref| / S (S = 0 only where the result is exact by construction: then the error must be 0)."""
    got, ref = got.double().cpu().reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    return float(((got - ref).abs() / S.reshape(-1).clamp_min(1e-300)).max())


def quotient_bf16(got, ref, S, bound):
    """A bf16 result: the f32 arithmetic within bound x S, plus one bf16 ulp of the reference for the final rounding (half an ulp, a
    whole one where the f32 error moves the value across a rounding boundary).  Returns the worst |got - ref| / allowed."""
    got, ref = got.double().cpu().reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (bound * S.reshape(-1) + bf16_ulp(ref))).max())


def misaligned(t):
    """A contiguous copy of t that starts at element 1 of a flat buffer: 4 (f32) or 2 (bf16) bytes off every 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# ===================================================================================================================== 1. pool / upsample
POOL_FORMS = ("f32x4", "f32x1", "bf16x8", "bf16x1")
POOL_OPS = ("maxpool", "bilinear", "nearest_add")
GRID_LIMIT = 16384 * 256                      # grid_for(): at most 16384 workgroups of 256 threads, the rest by grid stride


def pool_form(dtype, C, aligned):
    """The build nopesac_maxpool_nhwc / nopesac_upsample2x_bilinear_nhwc / nopesac_upsample2x_nearest_add_nhwc launch: 16-byte channel
    vectors when the channel count allows it and EVERY pointer (x, y and the addend / lateral) is 16-byte aligned."""
    if dtype == BF16:
        return "bf16x8" if C % 8 == 0 and aligned else "bf16x1"
    assert dtype == F32
    return "f32x4" if C % 4 == 0 and aligned else "f32x1"


# (dtype, C, the operand that is misaligned: None, "x" or "other" = addend / lateral)
POOL_CASES = [(F32, 8, None), (BF16, 16, None), (F32, 6, None), (BF16, 12, None), (F32, 8, "x"), (BF16, 16, "x"), (F32, 8, "other"),
              (BF16, 16, "other")]
POOL_B = 2
POOL_HW = ((1, 1), (1, 5), (5, 1), (7, 9))
POOL_KSP = ((3, 2, 1), (2, 2, 0), (3, 1, 1))
POOL_GRID_CASE = (F32, 9, 300, 400)           # B = 1, the scalar f32 build: 4 H W C = 4.32 M items, just above GRID_LIMIT


def pool_case_id(c):
    return "%s_C%d_%s" % (DT_NAME[c[0]], c[1], "aligned" if c[2] is None else "mis-" + c[2])


def pool_out(H, k, s, p):
    """Output size of the max-pool, or None where the window does not fit the padded input (refused by the entry point)."""
    return (H + 2 * p - k) // s + 1 if H + 2 * p >= k else None


def maxpool_ref(x, k, s, p):
    """[B,H,W,C] -> float64 [B,OH,OW,C]: max over the k x k window, positions outside the image never win."""
    B, H, W, C = x.shape
    OH, OW = pool_out(H, k, s, p), pool_out(W, k, s, p)
    xp = F.pad(x.double(), (0, 0, p, p, p, p), value=float("-inf"))
    out = torch.full((B, OH, OW, C), float("-inf"), dtype=F64)
    for kh in range(k):
        for kw in range(k):
            out = torch.maximum(out, xp[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s])
    return out


def _lin2x(n):
    """[2n, n] float64 interpolation matrix of one axis: src = max(0.5 (dst + 0.5) - 0.5, 0), i1 = min(i0 + 1, n - 1)."""
    o = torch.arange(2 * n, dtype=F64)
    s = (0.5 * (o + 0.5) - 0.5).clamp_min(0)
    i0 = s.floor().long()
    i1 = (i0 + 1).clamp_max(n - 1)
    lam = s - i0
    M = torch.zeros(2 * n, n, dtype=F64)
    r = torch.arange(2 * n)
    M[r, i0] += 1 - lam
    M[r, i1] += lam
    return M


def act64(z, act):
    return z if act == ACT_NONE else (z.clamp_min(0) if act == ACT_RELU else torch.where(z > 0, z, 0.01 * z))


def bilinear_ref(x, addend, act):
    """-> (y, S, z): y = act(z) + addend with z the x2 bilinear interpolation (align_corners = False), S = interpolation of |x| + |addend|."""
    My, Mx = _lin2x(x.shape[1]), _lin2x(x.shape[2])
    z = torch.einsum("oh,bhwc,pw->bopc", My, x.double(), Mx)
    S = torch.einsum("oh,bhwc,pw->bopc", My, x.double().abs(), Mx)
    y = act64(z, act)
    if addend is not None:
        y, S = y + addend.double(), S + addend.double().abs()
    return y, S, z


def bilinear_f32(x, addend, act):
    """The plain f32 formulation: torch's own bilinear resize in f32, the activation, the addend."""
    z = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    y = act64(z, act)
    return y if addend is None else y + addend.float()


def up2(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def nearest_add_ref(x, lat):
    return up2(x.double()) + lat.double(), up2(x.double().abs()) + lat.double().abs()


@functools.lru_cache(maxsize=None)
def pool_inputs(dtype, C, H, W, B=POOL_B, settle=True):
    """x [B,H,W,C], addend [B,2H,2W,C] (both rounded to dtype; the addend doubles as the lateral).  Settled: no interpolated value lies
    within MARGIN of 0 - where one does, its dominant tap (the source pixel dst // 2, weight >= 9/16) is moved."""
    g = gen(1000 + 131 * H + 17 * W + C + (7 if dtype == BF16 else 0))
    x = randn(g, B, H, W, C).to(dtype)
    addend = randn(g, B, 2 * H, 2 * W, C).to(dtype)
    for it in range(40 if settle else 0):
        z = bilinear_ref(x, None, ACT_NONE)[2]
        bad = z.abs() <= 2 * MARGIN
        if not bad.any():
            break
        hit = bad.view(B, H, 2, W, 2, C).any(4).any(2)
        x = torch.where(hit, x.double() + 0.03 * (it + 1) * torch.where(x >= 0, 1.0, -1.0), x.double()).to(dtype)
    return x, addend


def bilinear_variants():
    return [(act, add) for act in (ACT_NONE, ACT_RELU) for add in (False, True)]


# ===================================================================================================================== 2. GroupNorm
GN_SPLITS = 16
GN_EPS = 1e-5
GN_SPLIT_CG = ((8, 1), (8, 8), (128, 32), (256, 32), (2048, 256))
GN_GENERIC_CG = ((12, 3), (96, 6), (48, 3), (24, 6))
GN_REFUSED_CG = ((24, 1), (12, 2), (48, 1), (20, 2), (1032, 2))          # generic path, channels / group does not divide 256
GN_HW = (1, 5, 63, 300)
GN_B = (1, 3)
GN_RATIOS = (0.0, 2.5, 30.0)                  # |group mean| / group std
GN_MISALIGNED = (128, 32, 5, 3)               # a split-path shape whose x is misaligned: the generic path (C, G, HW, B)


def groupnorm_form(C, G, aligned=True, workspace=True):
    """What nopesac_groupnorm_nhwc does with (C, G): "split" (statistics over GN_SPLITS pixel ranges as E[x^2] - mean^2, then apply),
    "generic(gpb)" (two-pass, gpb groups per workgroup, grid G / gpb: gpb is the largest value <= 256 / cpg / 16 that divides G with
    cpg gpb dividing 256), or REFUSED."""
    if C <= 0 or G <= 0 or C % G:
        return REFUSED
    if workspace and C % 8 == 0 and 256 % (C // 8) == 0 and C <= 2048 and G <= 256 and aligned:
        return "split"
    cpg = C // G
    if cpg > 256 or 256 % cpg:
        return REFUSED
    gpb = max(256 // cpg // 16, 1)
    while gpb > 1 and (G % gpb or 256 % (cpg * gpb)):
        gpb -= 1
    return "generic(%d)" % gpb


def gn_cases():
    """(C, G, HW, B, aligned)"""
    out = [(C, G, HW, B, True) for C, G in GN_SPLIT_CG + GN_GENERIC_CG for HW in GN_HW for B in GN_B]
    return out + [GN_MISALIGNED + (False,)]


def gn_case_id(c):
    return "C%d_G%d_HW%d_B%d%s" % (c[0], c[1], c[2], c[3], "" if c[4] else "_mis-x")


def groupnorm_ref(x, gamma, beta, G, act, eps=GN_EPS):
    """x [B,HW,C] -> (y, S, z) in float64: z = (x - mean) rstd gamma + beta, S = (|x| + |mean|) rstd |gamma| + |beta| - the terms before
    any of them cancel."""
    B, HW, C = x.shape
    x4 = x.double().view(B, HW, G, C // G)
    mean = x4.mean((1, 3), keepdim=True)
    var = ((x4 - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1 / (var + eps).sqrt()
    xh = ((x4 - mean) * rstd).view(B, HW, C)
    z = xh * gamma.double() + beta.double()
    return act64(z, act), ((x4.abs() + mean.abs()) * rstd).view(B, HW, C) * gamma.double().abs() + beta.double().abs(), z


def groupnorm_f32(x, gamma, beta, G, act, split, eps=GN_EPS):
    """The documented algorithm of either path in plain f32 torch: two-pass statistics (generic), or mean(x^2) - mean(x)^2 and one
    multiply-add per element y = x a + d (split)."""
    B, HW, C = x.shape
    x4 = x.float().view(B, HW, G, C // G)
    mean = x4.mean((1, 3), keepdim=True)
    if split:
        var = ((x4 * x4).mean((1, 3), keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = ((x4 - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = torch.rsqrt(var + eps)
    a = (rstd.expand(B, 1, G, C // G).reshape(B, 1, C)) * gamma
    d = beta - mean.expand(B, 1, G, C // G).reshape(B, 1, C) * a
    return act64(x.float() * a + d, act)


@functools.lru_cache(maxsize=None)          # (every case is walked twice: by the floors, then by its test; ~100 MB in all)
def gn_inputs(C, G, HW, B, dtype, ratio):
    """(x [B,HW,C] rounded to dtype, gamma, beta f32): group g of image b has std in [0.5, 2] and mean +-ratio x std; |gamma| >= 0.5,
    |beta| >= 0.05.  No pre-activation within MARGIN of 0: where one is, its x is moved (and rounded again) until none is."""
    g = gen(2000 + 7 * C + 3 * G + 11 * HW + B + int(10 * ratio) + (5 if dtype == BF16 else 0))
    cpg = C // G
    std = (0.5 + 1.5 * torch.rand(B, 1, G, 1, generator=g, dtype=F64))
    sgn = torch.where(torch.rand(B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0).double()
    x = ((randn(g, B, HW, G, cpg) + ratio * sgn) * std).view(B, HW, C).to(dtype)
    pm = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    gamma = (pm(C) * (0.5 + torch.rand(C, generator=g, dtype=F64))).float()
    beta = (pm(C) * (0.05 + 0.3 * torch.rand(C, generator=g, dtype=F64))).float()
    step = std.expand(B, HW, G, cpg).reshape(B, HW, C)
    for it in range(60):
        z = groupnorm_ref(x, gamma, beta, G, ACT_NONE)[2]
        bad = z.abs() <= 2 * MARGIN
        if not bad.any():
            break
        d = torch.maximum(0.05 * (it + 1) * step, x.double().abs() * 2.0 ** -7)
        x = torch.where(bad, x.double() + d, x.double()).to(dtype)
    return x, gamma, beta


# ===================================================================================================================== 3. LayerNorm
LN_D = (64, 256, 1024)
LN_ROWS = (1, 3, 5, 77)
LN_ADDEND_ROWS = (None, 1, 11)
LN_EPS = 1e-5
LN_WANTS_PLAIN = (("y",), ("y16",), ("y", "y16"))
LN_WANTS_ADDEND = (("y",), ("y16",), ("y2",), ("y2_16",), ("y", "y16", "y2", "y2_16"))
LN_REFUSED_D = (65, 1088)


def layernorm_ref(x, res, gamma, beta, addend, eps=LN_EPS):
    """-> (y, S, y2, S2) float64 (y2 / S2 None without an addend; its row is row % addend rows)."""
    t = x.double() + (0 if res is None else res.double())
    mean = t.mean(-1, keepdim=True)
    var = ((t - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1 / (var + eps).sqrt()
    y, S = (t - mean) * rstd * gamma.double() + beta.double(), (t.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()
    if addend is None:
        return y, S, None, None
    a = addend.double()[torch.arange(x.shape[0]) % addend.shape[0]]
    return y, S, y + a, S + a.abs()


def layernorm_f32(x, res, gamma, beta, addend, eps=LN_EPS):
    t = x if res is None else x + res
    mean = t.mean(-1, keepdim=True)
    var = ((t - mean) ** 2).mean(-1, keepdim=True)
    y = (t - mean) * torch.rsqrt(var + eps) * gamma + beta
    return y, (None if addend is None else y + addend[torch.arange(x.shape[0]) % addend.shape[0]])


@functools.lru_cache(maxsize=None)
def ln_inputs(D, rows):
    g = gen(3000 + D + rows)
    f = lambda *s: randn(g, *s).float()
    return {"x": f(rows, D) * 2 + 1.5, "res": f(rows, D), "gamma": 1 + 0.3 * f(D), "beta": 0.3 * f(D), 1: f(1, D), 11: f(11, D)}


# ===================================================================================================================== 4. row softmax
SM_D = (1, 63, 64, 65, 300, 1023, 1024)
SM_ROWS = (1, 5)
SM_SCALE = 30.0


def softmax_lds(D):
    """Leading dimensions of the padded form at D: D itself, the next multiple of 16 of the 300-wide affinity, and 1024 where the output
    row spans many more 64-lane trips than the input row."""
    return (D,) + ((304,) if D == 300 else ()) + ((1024,) if D in (64, 65) else ())


def softmax_form(D, ld, out_dtype):
    """ops.softmax_rows: the plain kernel for an f32 result without padding, the padding kernel <f32> / <bf16> otherwise."""
    return "plain" if out_dtype == F32 and ld <= D else "pad<%s>" % DT_NAME[out_dtype]


SM_CASES = [(D, ld, dt) for D in SM_D for ld in softmax_lds(D) for dt in (F32, BF16)]


def sm_case_id(c):
    return "D%d_ld%d_%s" % (c[0], c[1], DT_NAME[c[2]])


@functools.lru_cache(maxsize=None)
def sm_inputs(D, rows):
    """x [rows, D] f32, N(0, 30^2); the last row holds -inf at its first and last element and both sides of the first wave boundary
    (never in every column)."""
    x = (SM_SCALE * randn(gen(4000 + D + rows), rows, D)).float()
    idx = sorted({0, D - 1, 63, 64} & set(range(D)))[:D - 1]
    if idx:
        x[rows - 1, idx] = float("-inf")
    return x


def softmax_ref(x):
    """-> (p, S): S = max(p, smallest normal f32): the unit an f32 result near or below the normal range can be held to."""
    p = torch.softmax(x.double(), -1)
    return p, p.clamp_min(F32_MIN_NORMAL)


# ===================================================================================================================== 5. re-layout / exact
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 65), (257, 3))
TRANSPOSE_B = (1, 3)
ADD_ROWS_CASES = ((1, 1, 1), (7, 5, 3), (300, 256, 11))            # (rows, D, b_rows)
CONCAT_CASES = ((1, 1, 1), (5, 3, 4), (300, 7, 64))                # (rows, Da, Db)
HW_ROWS_CASES = ((2, 3, 5, 1), (2, 3, 5, 8), (1, 5, 2, 8))         # (B, H, W, C)
U8_N = (1, 15, 16, 17, 4099)
ADD_ROWS_BF16_CASES = ((7, 4, 3), (5, 256, 2))                     # (rows, D, b_rows)
NONFINITE_N = (1, 63, 65, 1024 * 256 + 3)
NONFINITE_SINGLE_LIMIT, NONFINITE_BATCH_LIMIT = 1024 * 256, 256 * 256
NORMALIZE_D = (3, 4)
NORMALIZE_ROWS = 70


def transpose_hw_rows_ref(x, H, W):
    """[B, H W, C] rows in (h, w) order -> rows in (w, h) order."""
    B, _, C = x.shape
    return x.view(B, H, W, C).permute(0, 2, 1, 3).reshape(B, H * W, C)


def nonfinite_input(n, seed=0):
    """(x f32 [n], number of NaN / Inf in it): NaN, +-Inf, the largest finite value and a denormal at the first and last element and
    on both sides of the wave (64) and workgroup (256) boundaries."""
    x = randn(gen(5000 + n + seed), n).float()
    kinds = [float("nan"), float("inf"), float("-inf"), 3.4028234663852886e38, 1e-45, -float("nan"), -3.4028234663852886e38]
    pos = sorted({0, n - 1, 63, 64, 255, 256, n - 2} & set(range(n)))
    for i, p in enumerate(pos):
        x[p] = kinds[(i + n) % len(kinds)]
    return x, int((~torch.isfinite(x)).sum())


def normalize_rows_f32(x, canon):
    """The kernel's own f32 operation order (every step correctly rounded, so the result is reproducible bit for bit): the squares
    summed front to back, n = max(sqrt(s), 1e-12), y = sign (x / n) with sign = -1 where canon and x[0] / n < 0.
    Every operation is done in float64 on f32 values and rounded to f32 at once: for + x / sqrt that IS the correctly rounded f32
    result (53 >= 2 x 24 + 2 bits, so the second rounding changes nothing), on any host - a CPU library's own f32 sqrt or divide need
    not be correctly rounded (torch's vectorised f32 sqrt is not, on some hosts)."""
    r = lambda t: t.float().double()
    xd = x.double()
    s = torch.zeros(x.shape[0], dtype=F64)
    for d in range(x.shape[1]):
        s = r(s + r(xd[:, d] * xd[:, d]))
    n = r(s.sqrt()).clamp_min(float(torch.tensor(1e-12, dtype=F32)))
    sign = torch.where((r(xd[:, 0] / n) < 0) & bool(canon), -1.0, 1.0).double()
    return (sign[:, None] * r(xd / n[:, None])).float()


def normalize_rows_ref(x, canon):
    x = x.double()
    n = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    sign = torch.where((x[:, :1] < 0) & bool(canon), -1.0, 1.0)
    return sign * x / n


def normalize_rows_bwd_ref(x, g, canon, dtype=F64):
    """-> (dx, S) by autograd in `dtype`; S = |g| / n + |x| sum |x g| / n^3."""
    xx = x.to(dtype).clone().requires_grad_(True)
    n = xx.norm(dim=-1, keepdim=True)
    sign = torch.where((xx[:, :1] < 0) & bool(canon), -1.0, 1.0).to(dtype)
    (sign * xx / n * g.to(dtype)).sum().backward()
    xd, gd = x.double(), g.double()
    nd = xd.norm(dim=-1, keepdim=True)
    return xx.grad, gd.abs() / nd + xd.abs() * (xd * gd).abs().sum(-1, keepdim=True) / nd ** 3


@functools.lru_cache(maxsize=None)
def normalize_inputs(D):
    """x [rows, D] with |x[0]| > MARGIN in every row (the canonical sign is decided there) and one all-zero row at the end for the forward."""
    g = gen(5500 + D)
    x = randn(g, NORMALIZE_ROWS, D).float()
    x[3] *= 1e-3
    x[:, 0] = torch.where(x[:, 0].abs() <= 2 * MARGIN, torch.full_like(x[:, 0], 0.5), x[:, 0])
    return x, randn(g, NORMALIZE_ROWS, D).float()


# ===================================================================================================================== 6. reductions / optimiser
SUMSQ_ONE_WG_MAX = 16384
CLIP_N = (1, 255, 257, 16384, 16385, 1048576, 1048577)
STEP_N = (1, 255, 257, 1048577)
STEPS = 3
STEP_CONFIGS = [("ADAMW", 0.0, 0.0), ("ADAMW", 0.01, 0.0), ("SGD", 0.0, 0.0), ("SGD", 0.01, 0.0), ("SGD", 0.0, 0.9), ("SGD", 0.01, 0.9)]
STEP_LR = {"ADAMW": 1e-2, "SGD": 1e-1}
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def sumsq_form(n):
    """nopesac_sumsq_accumulate_f32: one workgroup up to 16384 elements; above, up to 256 slices of a multiple of 4096 elements (one
    workgroup each) and a final workgroup: ("two_stage", slice length, number of slices)."""
    if n <= SUMSQ_ONE_WG_MAX:
        return "one_wg"
    chunk = ((n + 255) // 256 + 4095) // 4096 * 4096
    return ("two_stage", chunk, (n + chunk - 1) // chunk)


@functools.lru_cache(maxsize=None)
def grad_input(n, k=0):
    return randn(gen(6000 + n + 97 * k), n).float()


def clip_ref(g, max_norm):
    """-> (sum of squares, norm, coefficient, scaled gradient) in float64: torch.nn.utils.clip_grad_norm_."""
    ss = (g.double() ** 2).sum()
    norm = ss.sqrt()
    coef = (max_norm / (norm + 1e-6)).clamp_max(1.0)
    return ss, norm, coef, g.double() * coef


def optimiser_steps(p0, grads, name, wd, momentum, dtype=F64):
    """STEPS steps of AdamW (decoupled decay, bias-corrected moments) or SGD (decay added to the gradient, momentum buffer = the gradient
    on its first step) in `dtype` -> (p, S): S = |p0| + the magnitudes of every term added to p since."""
    p = p0.to(dtype).clone()
    S = p0.double().abs().clone()
    lr = STEP_LR[name]
    m1 = m2 = mom = None
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        if name == "ADAMW":
            b1, b2 = ADAM_BETAS
            m1 = (1 - b1) * g if m1 is None else b1 * m1 + (1 - b1) * g
            m2 = (1 - b2) * g * g if m2 is None else b2 * m2 + (1 - b2) * g * g
            d = (lr / (1 - b1 ** t)) * m1 / (m2.sqrt() / (1 - b2 ** t) ** 0.5 + ADAM_EPS)
            S += (lr * wd * p).double().abs() + d.double().abs()
            p = p * (1 - lr * wd) - d
        else:
            gi = g + wd * p
            if momentum:
                mom = gi if mom is None else momentum * mom + gi
                gi = mom
            S += (lr * gi).double().abs()
            p = p - lr * gi
    return p, S


def torch_optimiser_steps(p0, grads, name, wd, momentum, dtype):
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = (torch.optim.AdamW([p], lr=STEP_LR[name], betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=wd) if name == "ADAMW" else
           torch.optim.SGD([p], lr=STEP_LR[name], momentum=momentum, weight_decay=wd))
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
    return p.detach()


def col_sum_cases():
    """(rows, cols, leading dimension): the transpose shapes, dense and as a column slice of a wider buffer."""
    return [(r, c, ld) for r, c in TRANSPOSE_SHAPES for ld in (c, c + 5)]


@functools.lru_cache(maxsize=None)
def matrix_input(rows, ld, B=1):
    return randn(gen(6500 + rows + 3 * ld + B), B, rows, ld).float()


# ===================================================================================================================== floors
def _q(a, ref, S):
    return float(((a.double() - ref).abs() / S.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def floor_bilinear():
    worst = 0.0
    for dtype, C, _ in POOL_CASES[:4]:
        for H, W in POOL_HW:
            x, addend = pool_inputs(dtype, C, H, W)
            for act, add in bilinear_variants():
                y, S, _ = bilinear_ref(x, addend if add else None, act)
                worst = max(worst, _q(bilinear_f32(x, addend if add else None, act), y, S))
    return max(worst, EPS32)


def gn_floor_key(form, ratio):
    return ("split" if form == "split" else "generic", ratio)


@functools.lru_cache(maxsize=None)
def floors_groupnorm():
    """{(path, ratio): floor} over every case of the family (both dtypes' inputs, both activations), in f32 arithmetic."""
    out = {}
    for C, G, HW, B, aligned in gn_cases():
        form = groupnorm_form(C, G, aligned)
        for dtype in (F32, BF16):
            for ratio in GN_RATIOS:
                x, gamma, beta = gn_inputs(C, G, HW, B, dtype, ratio)
                for act in (ACT_NONE, ACT_RELU):
                    y, S, _ = groupnorm_ref(x, gamma, beta, G, act)
                    k = gn_floor_key(form, ratio)
                    out[k] = max(out.get(k, EPS32), _q(groupnorm_f32(x, gamma, beta, G, act, form == "split"), y, S))
    return out


@functools.lru_cache(maxsize=None)
def floor_layernorm():
    worst = EPS32
    for D in LN_D:
        for rows in LN_ROWS:
            c = ln_inputs(D, rows)
            for res in (None, c["res"]):
                for ar in LN_ADDEND_ROWS:
                    add = None if ar is None else c[ar]
                    y, S, y2, S2 = layernorm_ref(c["x"], res, c["gamma"], c["beta"], add)
                    a, a2 = layernorm_f32(c["x"], res, c["gamma"], c["beta"], add)
                    worst = max(worst, _q(a, y, S), 0.0 if add is None else _q(a2, y2, S2))
    return worst


@functools.lru_cache(maxsize=None)
def floor_softmax():
    worst = EPS32
    for D in SM_D:
        for rows in SM_ROWS:
            x = sm_inputs(D, rows)
            p, S = softmax_ref(x)
            worst = max(worst, _q(torch.softmax(x, -1), p, S))
    return worst


@functools.lru_cache(maxsize=None)
def floor_normalize_bwd():
    worst = EPS32
    for D in NORMALIZE_D:
        x, g = normalize_inputs(D)
        for canon in (False, True):
            ref, S = normalize_rows_bwd_ref(x, g, canon)
            worst = max(worst, _q(normalize_rows_bwd_ref(x, g, canon, F32)[0], ref, S))
    return worst


@functools.lru_cache(maxsize=None)
def floor_sumsq():
    worst = EPS32
    for n in CLIP_N:
        g = grad_input(n)
        ss = clip_ref(g, 1.0)[0]
        worst = max(worst, float(((g * g).sum().double() - ss).abs() / ss))
    return worst


@functools.lru_cache(maxsize=None)
def floor_optimiser(name):
    worst = EPS32
    for n in STEP_N:
        grads = [grad_input(n, k + 1) for k in range(STEPS)]
        for nm, wd, mom in STEP_CONFIGS:
            if nm == name:
                ref, S = optimiser_steps(grad_input(n), grads, nm, wd, mom)
                worst = max(worst, _q(torch_optimiser_steps(grad_input(n), grads, nm, wd, mom, F32), ref, S))
    return worst


@functools.lru_cache(maxsize=None)
def floor_col_sum():
    worst = EPS32
    for r, c, ld in col_sum_cases():
        x = matrix_input(r, ld)[0, :, ld - c:]
        worst = max(worst, _q(x.sum(0), x.double().sum(0), x.double().abs().sum(0)))
    return worst


@functools.lru_cache(maxsize=None)
def floor_clipped_gradient():
    """The scaled gradient in plain f32: the f32 coefficient times the f32 gradient (the multiply's own rounding is part of the floor)."""
    worst = EPS32
    for n in CLIP_N:
        g = grad_input(n)
        for k in (0.25, 4.0):
            max_norm = k * float(clip_ref(g, 1.0)[1])
            coef32 = (max_norm / ((g * g).sum().sqrt() + 1e-6)).clamp_max(1.0)
            scaled = clip_ref(g, max_norm)[3]
            worst = max(worst, _q(g * coef32, scaled, scaled.abs()))
    return worst


# ===================================================================================================================== 4b. correlation softmax
CORR_HW = ((3, 5), (8, 8), (5, 13))           # P = h w = 15, 64, 65: below, at and one past the 64 lanes of a row's wave
CORR_B, CORR_C = 2, 8


def corr_pad(P):
    return (P + 15) // 16 * 16 + 16           # a padded leading dimension, always > P


def corr_ref(x1, x2, dtype=F64):
    """x1, x2 [B,h,w,C] -> (A [B,h,w,P], S): A[b,h1,w1, w2 h + h2] = softmax over the view-2 positions of x1[b,h1,w1,:] . x2[b,h2,w2,:]."""
    B, h, w, C = x1.shape
    x2t = x2.to(dtype).permute(0, 2, 1, 3).reshape(B, h * w, C)                  # rows in (w, h) order
    p = torch.softmax(torch.einsum("bhwc,bqc->bhwq", x1.to(dtype), x2t), -1)
    return p, p.double().clamp_min(F32_MIN_NORMAL)


@functools.lru_cache(maxsize=None)
def corr_inputs(h, w):
    g = gen(4500 + 31 * h + w)
    P = h * w
    return {"x1": randn(g, CORR_B, h, w, CORR_C).float(), "x2": randn(g, CORR_B, h, w, CORR_C).float(),
            "da": randn(g, CORR_B, h, w, P).float(), "noise": randn(g, CORR_B, h, w, corr_pad(P) - P).float()}


def corr_bwd_ref(a, da, x1, x2, dtype=F64):
    """Backward of the correlation softmax FROM the probabilities a [B,h,w,P] the kernel is given: dS = a (dA - sum dA a), dx1 = dS x2t,
    dx2t = dS^T x1, dx2 back in (h, w) order -> (dx1, dx2, S1, S2); S from the same sums on absolute values."""
    B, h, w, C = x1.shape
    P = h * w
    a, da, x1, x2 = (t.to(dtype) for t in (a, da, x1, x2))
    x2t = x2.permute(0, 2, 1, 3).reshape(B, P, C)
    dot = (da * a).sum(-1, keepdim=True)
    ds = (a * (da - dot)).view(B, P, P)
    Sds = (a.abs() * (da.abs() + (da * a).abs().sum(-1, keepdim=True))).view(B, P, P).double()
    back = lambda t: t.view(B, w, h, C).permute(0, 2, 1, 3)
    dx1, dx2 = (ds @ x2t).view(B, h, w, C), back(ds.transpose(1, 2) @ x1.reshape(B, P, C))
    S1 = (Sds @ x2t.double().abs()).view(B, h, w, C)
    S2 = back(Sds.transpose(1, 2) @ x1.reshape(B, P, C).double().abs())
    return dx1, dx2, S1, S2


@functools.lru_cache(maxsize=None)
def floors_corr():
    """(forward, backward)"""
    f = b = EPS32
    for h, w in CORR_HW:
        c = corr_inputs(h, w)
        p, S = corr_ref(c["x1"], c["x2"])
        f = max(f, _q(corr_ref(c["x1"], c["x2"], F32)[0], p, S))
        a = p.float()
        r = corr_bwd_ref(a, c["da"], c["x1"], c["x2"])
        q = corr_bwd_ref(a, c["da"], c["x1"], c["x2"], F32)
        b = max(b, _q(q[0], r[0], r[2]), _q(q[1], r[1], r[3]))
    return f, b


# ===================================================================================================================== 7. norm / pool backward
BN_ROWS = (1, 255, 256, 257, 1000)
BN_C = (4, 64, 65, 96)
BN_ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY)
BN_EPS = 1e-3
BN_RPS, BN_CBLOCK = 256, 64                   # bn_act_bwd_kernel: 256 rows per split, 64 channels per workgroup


def bn_grid(rows, C):
    """(channel blocks, row splits) of nopesac_bn_act_backward_f32."""
    return (C + BN_CBLOCK - 1) // BN_CBLOCK, (rows + BN_RPS - 1) // BN_RPS


@functools.lru_cache(maxsize=None)
def bn_inputs(rows, C):
    """c, dy [rows, C], gamma (|gamma| >= 0.5, the first with 1e-4: the backward reads the raw conv output), beta, mean, var f32; no
    pre-activation within MARGIN of 0 (where one is, its c is moved)."""
    g = gen(7000 + 3 * rows + C)
    c, dy = randn(g, rows, C).float(), randn(g, rows, C).float()
    pm = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    gamma = (pm * (0.5 + torch.rand(C, generator=g, dtype=F64))).float()
    gamma[0] = 1e-4
    beta, mean = (0.5 * randn(g, C)).float(), randn(g, C).float()
    var = (0.1 + torch.rand(C, generator=g, dtype=F64)).float()
    beta[0] = 0.3
    for it in range(40):
        z = bn_ref(c, dy, gamma, beta, mean, var, ACT_NONE)["z"]
        bad = z.abs() <= 2 * MARGIN
        if not bad.any():
            break
        c = torch.where(bad & (gamma.abs() > 1e-2), c + 0.05 * (it + 1), c)
    return c, dy, gamma, beta, mean, var


def bn_ref(c, dy, gamma, beta, mean, var, act, dtype=F64, eps=BN_EPS):
    """Inference BatchNorm + activation and its backward in `dtype`, with S (float64) of every output."""
    c, dy, gamma, beta, mean, var = (t.to(dtype) for t in (c, dy, gamma, beta, mean, var))
    rstd = 1 / (var + eps).sqrt()
    s = gamma * rstd
    z = c * s + (beta - mean * s)
    slope = torch.ones_like(z) if act == ACT_NONE else torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.0 if act == ACT_RELU else 0.01))
    dz = dy * slope
    d = lambda t: t.double().abs()
    return {"z": z, "y": z * slope, "Sy": (d(c * s) + d(beta) + d(mean * s)) * d(slope), "dc": dz * s, "Sdc": d(dz * s),
            "dgamma": (dz * ((c - mean) * rstd)).sum(0), "Sdgamma": (d(dz) * (d(c) + d(mean)) * d(rstd)).sum(0),
            "dbeta": dz.sum(0), "Sdbeta": d(dz).sum(0)}


BN_KEYS = ("y", "dc", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def floors_bn():
    out = dict.fromkeys(BN_KEYS, EPS32)
    for rows in BN_ROWS:
        for C in BN_C:
            a = bn_inputs(rows, C)
            for act in BN_ACTS:
                r, q = bn_ref(*a, act), bn_ref(*a, act, F32)
                for k in BN_KEYS:
                    out[k] = max(out[k], _q(q[k], r[k], r["S" + k]))
    return out


GNB_CG = ((32, 32), (128, 32), (256, 32), (256, 1))          # channels per group 1, 4, 8, 256: every lane split of the 256 threads
GNB_HW = (1, 5, 300)
GNB_B = (1, 3)
GNB_RATIO = 2.5


def gnb_cases():
    return [(C, G, HW, B) for C, G in GNB_CG for HW in GNB_HW for B in GNB_B]


def gnb_ref(x, dy, gamma, beta, G, relu, dtype=F64, eps=GN_EPS):
    """GroupNorm (+ ReLU) backward in `dtype` by the formula of the kernel's comment (checked against autograd in the CPU half):
    dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dz gamma; dgamma = sum dz xh; dbeta = sum dz.  S: the same sums on absolute
    values with |xh| taken before the mean cancels, (|x| + |mean|) rstd."""
    B, HW, C = x.shape
    cpg = C // G
    x4, dy4 = x.to(dtype).view(B, HW, G, cpg), dy.to(dtype).view(B, HW, G, cpg)
    ga, be = gamma.to(dtype).view(1, 1, G, cpg), beta.to(dtype).view(1, 1, G, cpg)
    mu = x4.mean((1, 3), keepdim=True)
    rstd = 1 / (((x4 - mu) ** 2).mean((1, 3), keepdim=True) + eps).sqrt()
    xh = (x4 - mu) * rstd
    dz = dy4 * ((xh * ga + be > 0).to(dtype) if relu else 1.0)
    dxh = dz * ga
    m1, m2 = dxh.mean((1, 3), keepdim=True), (dxh * xh).mean((1, 3), keepdim=True)
    d = lambda t: t.double().abs()
    XH = (d(x4) + d(mu)) * d(rstd)
    Sdx = d(rstd) * (d(dxh) + d(dxh).mean((1, 3), keepdim=True) + XH * (d(dxh) * XH).mean((1, 3), keepdim=True))
    v = lambda t: t.reshape(B, HW, C)
    return {"dx": v(rstd * (dxh - m1 - xh * m2)), "Sdx": v(Sdx), "dgamma": v(dz * xh).sum((0, 1)), "Sdgamma": v(d(dz) * XH).sum((0, 1)),
            "dbeta": v(dz).sum((0, 1)), "Sdbeta": v(d(dz)).sum((0, 1))}


GNB_KEYS = ("dx", "dgamma", "dbeta")


def gnb_inputs(C, G, HW, B):
    x, gamma, beta = gn_inputs(C, G, HW, B, F32, GNB_RATIO)
    return x, randn(gen(7500 + C + G + HW + B), B, HW, C).float(), gamma, beta


@functools.lru_cache(maxsize=None)
def floors_gnb():
    out = dict.fromkeys(GNB_KEYS, EPS32)
    for C, G, HW, B in gnb_cases():
        x, dy, gamma, beta = gnb_inputs(C, G, HW, B)
        for relu in (False, True):
            r, q = gnb_ref(x, dy, gamma, beta, G, relu), gnb_ref(x, dy, gamma, beta, G, relu, F32)
            for k in GNB_KEYS:
                out[k] = max(out[k], _q(q[k], r[k], r["S" + k]))
    return out


MPB_HW = ((2, 2), (5, 7), (6, 10))
MPB_B, MPB_C = 2, 5


@functools.lru_cache(maxsize=None)
def mpb_inputs(H, W, ties):
    """x [B,H,W,C], dy [B,H/2,W/2,C] f32.  Every 2 x 2 window has a unique maximum; with `ties` a whole window is tied (its first element
    takes the gradient) and, where the map is large enough, two maxima share a window (the first in row-major order wins)."""
    g = gen(7700 + 13 * H + W)
    x, dy = randn(g, MPB_B, H, W, MPB_C).float(), randn(g, MPB_B, H // 2, W // 2, MPB_C).float()
    if ties:
        x[:, 0:2, 0:2] = 1.5
        if H >= 4 and W >= 4:
            x[:, 2, 3] = x[:, 3, 2] = 9.0
    return x, dy


def mpb_unique(x):
    """True where the 2 x 2 window's maximum is attained once -> [B,H/2,W/2,C]."""
    B, H, W, C = x.shape
    win = x[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C)
    m = win.amax((2, 4), keepdim=True)
    return (win == m).sum((2, 4)) == 1


def mpb_ref(x, dy):
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy.double().permute(0, 3, 1, 2))
    return xr.grad.permute(0, 2, 3, 1).float().contiguous()


UPB_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7))                    # (B, H, W, C) of the coarse map


def upb_f32(dy):
    """The kernel's order in f32, every add exact IEEE: (top-left + top-right) + (bottom-left + bottom-right)."""
    return (dy[:, 0::2, 0::2] + dy[:, 0::2, 1::2]) + (dy[:, 1::2, 0::2] + dy[:, 1::2, 1::2])


# ===================================================================================================================== 8. conv gradients
DGRAD_KP = ((3, 1), (1, 0))
DGRAD_HW = ((1, 1), (2, 3), (7, 9), (8, 10))
DGRAD_CIN, DGRAD_COUT, DGRAD_B = (1, 5), (1, 7), 2
DGRAD_DY_EXTRA, DGRAD_DX_EXTRA = 3, 2                         # channels of the wider buffers dy is read from / dx is written into


def conv_out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def dgrad_cases():
    return [(k, p, hw, cin, cout) for k, p in DGRAD_KP for hw in DGRAD_HW for cin in DGRAD_CIN for cout in DGRAD_COUT]


def _conv_grads(x, w, dy, stride, pad, dtype):
    """x [B,H,W,Cin], w [Cout,Cin,k,k], dy [B,OH,OW,Cout] -> (dx NHWC, dw) in `dtype`, written out as the two GEMMs over the unfolded
    input (im2col): dw = dY^T X_col, dx = fold(dY W).  (No library conv backward: the f32 one of some CPU builds is not usable here.)"""
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    xcol = F.unfold(x.to(dtype).permute(0, 3, 1, 2), k, padding=pad, stride=stride)              # [B, Cin k k, L]
    dyf = dy.to(dtype).permute(0, 3, 1, 2).reshape(B, Cout, -1)                                  # [B, Cout, L]
    dw = torch.einsum("bol,bnl->on", dyf, xcol).view(Cout, Cin, k, k)
    dcol = torch.einsum("on,bol->bnl", w.to(dtype).reshape(Cout, -1), dyf)
    return F.fold(dcol, (H, W), k, padding=pad, stride=stride).permute(0, 2, 3, 1), dw


def conv_grad_ref(x, w, dy, stride, pad):
    """-> (dx, Sdx, dw, Sdw): float64 gradients and the same convs on absolute values."""
    dx, dw = _conv_grads(x, w, dy, stride, pad, F64)
    Sdx, Sdw = _conv_grads(x.abs(), w.abs(), dy.abs(), stride, pad, F64)
    return dx, Sdx, dw, Sdw


@functools.lru_cache(maxsize=None)
def dgrad_inputs(k, pad, hw, cin, cout):
    g = gen(8000 + 100 * k + 10 * hw[0] + hw[1] + 7 * cin + cout)
    H, W = hw
    OH, OW = conv_out(H, k, 2, pad), conv_out(W, k, 2, pad)
    return (randn(g, DGRAD_B, H, W, cin).float(), (randn(g, cout, cin, k, k) / (cin * k * k) ** 0.5).float(),
            randn(g, DGRAD_B, OH, OW, cout + DGRAD_DY_EXTRA).float())


# (Cin, channels of the x buffer, Cout)
WGRAD_CH = ((4, 4, 4), (36, 36, 132), (300, 304, 8))
WGRAD_KS = ((1, 1), (1, 2), (3, 1), (3, 2))
WGRAD_P = {1: (1, 1, 1), 17: (1, 1, 17), 154: (2, 7, 11)}      # P -> (B, OH, OW)
WG_BM = WG_BN = 128
WG_BK = 16


def wgrad_splits(P):
    return (1, 2, P + 3)


def wgrad_grid(Cin, Cout, k, P, splits):
    """nopesac_conv2d_wgrad_f32's launch: 128 x 128 tiles over N = k k Cin columns and Cout rows, blockIdx.z = split; a split covers
    `chunk` pixels, a multiple of the 16-pixel LDS stage -> dict(grid, chunk, empty splits, and whether the last tile of either
    dimension, the last stage of a split and the last split are partial)."""
    N = k * k * Cin
    chunk = ((P + splits - 1) // splits + WG_BK - 1) // WG_BK * WG_BK
    used = (P + chunk - 1) // chunk
    return {"grid": ((N + WG_BN - 1) // WG_BN, (Cout + WG_BM - 1) // WG_BM, splits), "chunk": chunk, "empty_splits": splits - used,
            "n_tail": N % WG_BN != 0, "m_tail": Cout % WG_BM != 0, "stage_tail": P % WG_BK != 0, "split_tail": P % chunk != 0 and used > 1}


def wgrad_cases():
    return [(ch, ks, P) for ch in WGRAD_CH for ks in WGRAD_KS for P in WGRAD_P]


def wgrad_case_id(c):
    return "cin%d_cout%d_k%d_s%d_P%d" % (c[0][0], c[0][2], c[1][0], c[1][1], c[2])


@functools.lru_cache(maxsize=None)
def wgrad_inputs(ch, ks, P):
    """x [B,H,W,Cx] (channels beyond Cin hold noise that must not count), dy [B,OH,OW,Cout] f32."""
    cin, cx, cout = ch
    k, stride = ks
    B, OH, OW = WGRAD_P[P]
    H, W = (OH, OW) if stride == 1 else (2 * OH - 1, 2 * OW - 1)
    pad = (k - 1) // 2
    assert conv_out(H, k, stride, pad) == OH and conv_out(W, k, stride, pad) == OW
    g = gen(8500 + cin + cout + 10 * k + stride + P)
    return randn(g, B, H, W, cx).float(), randn(g, B, OH, OW, cout).float(), pad


@functools.lru_cache(maxsize=None)
def floors_conv_grad():
    """(dgrad, wgrad): plain f32 autograd of torch's conv against float64."""
    fd = fw = EPS32
    for c in dgrad_cases():
        k, pad, hw, cin, cout = c
        x, w, dyw = dgrad_inputs(*c)
        dy = dyw[..., :cout]
        dx, Sdx, _, _ = conv_grad_ref(x, w, dy, 2, pad)
        fd = max(fd, _q(_conv_grads(x, w, dy, 2, pad, F32)[0], dx, Sdx))
    for ch, ks, P in wgrad_cases():
        x, dy, pad = wgrad_inputs(ch, ks, P)
        xs = x[..., :ch[0]]
        w0 = torch.zeros(ch[2], ch[0], ks[0], ks[0])
        _, _, dw, Sdw = conv_grad_ref(xs, w0, dy, ks[1], pad)
        fw = max(fw, _q(_conv_grads(xs, w0, dy, ks[1], pad, F32)[1], dw, Sdw))
    return fd, fw
