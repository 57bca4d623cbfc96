"""Shared helpers of the head sweep (tests/test_head_forms_*.py): the transformer-tail, attention and GNN-layer calls of the bf16 model, their
inputs at production statistics with edge rows, and float64 references with a first-order per-element error bound.

References take the exact operand values each kernel reads (bf16 weights as packed, Wq * 32^-0.5 rounded after the scaling) and round to
bf16 where the kernel rounds.  The bound of a value is propagated to first order: a GEMM adds 2^-20 A (A = the absolute-value sum), a
LayerNorm carries the incoming bound through its derivative and adds an f32 term for its statistics, and a bf16 rounding point adds one
unit in the last place, but only on elements whose f64 value lies within the propagated bound of a rounding midpoint (elsewhere the kernel
rounds to the same bf16 value and the rounding absorbs the error).  error_ratio keeps tests/conv_routing.py's contract."""
import math
from types import SimpleNamespace

import torch

BF = torch.bfloat16
LN_EPS = 1e-5
GEMM = 2.0 ** -20            # f32 accumulation, per unit of the absolute-value sum
STATS = 2.0 ** -18           # LayerNorm mean / variance / rsqrtf in f32, relative
LOG2E = 1.4426950408889634

# ------------------------------------------------------------------------------------------------------------------------- inventory
# (images, L) of one forward: 480 x 640 inputs give 15 x 20 = 300 encoder tokens; 32 pairs = 64 images, one pair = 2
L_ENC = 300
LEG_NQ = {"headline_mp3d_k32": 50, "scannet_k64": 64, "bf16_k128": 128}
ONE_PAIR_NQ = 50


def tail_key(entry, M, pre_norm, skip_ffn, want, n_pos, n_proj, pos_rows, prefetch):
    return ("tail", entry, M, bool(pre_norm), bool(skip_ffn), tuple(sorted(want)), n_pos, n_proj, pos_rows, bool(prefetch))


def attention_key(B, Lq, Lk, q_ld, k_ld, v_ld, io16, lens):
    return ("attention", B, Lq, Lk, q_ld, k_ld, v_ld, bool(io16), bool(lens))


def gnn_key(n_sets, nq, x_off, src_off, out_off, self_layer, aliased, prefetch):
    return ("gnn", n_sets, nq, x_off, src_off, out_off, bool(self_layer), bool(aliased), bool(prefetch))


def _production():
    """key -> pinned default tail form name (None for attention / GNN calls)."""
    calls = {}
    for pairs in (32, 1):
        for nq in (sorted(set(LEG_NQ.values())) if pairs == 32 else [ONE_PAIR_NQ]):
            B = 2 * pairs
            Me, Md = B * L_ENC, B * nq
            pf = Me <= 2048                                      # ops.transformer_tail prefetches only for M <= 64 * 32
            big = "t96" if Me == 19200 else "t32"
            calls[tail_key("transformer_tail", Me, 0, 0, ("y",), 512, 256, L_ENC, pf)] = big                 # encoder layers 0-4
            calls[tail_key("transformer_tail", Me, 0, 0, ("y",), 0, 0, L_ENC, pf)] = big                     # encoder layer 5
            calls[tail_key("transformer_tail", Md, 1, 1, ("y",), 256, 0, nq, Md <= 2048)] = "t32"            # decoder self half
            calls[tail_key("transformer_tail", Md, 1, 0, ("y",), 512, 256, nq, Md <= 2048)] = "t32"          # decoder layers 0-4
            calls[tail_key("decoder_tail", Md, 1, 0, ("yn",), 0, 0, nq, False)] = "t32"                      # decoder layer 5
            calls[attention_key(B, L_ENC, L_ENC, 512, 512, 256, True, False)] = None
            calls[attention_key(B, nq, nq, 512, 512, 256, True, False)] = None
            calls[attention_key(B, nq, L_ENC, 256, 1536, 1536, True, False)] = None
            P = pairs
            pf = 2 * P <= 16
            calls[gnn_key(2 * P, nq, 0, 0, 0, True, False, pf)] = None
            calls[gnn_key(P, nq, 0, P, 0, False, False, False)] = None
            calls[gnn_key(P, nq, P, 0, P, False, True, pf)] = None
            calls[gnn_key(P, nq, P, 0, P, False, True, False)] = None         # the last layer: no next weights to prefetch
    return calls


PRODUCTION = _production()


def production_tails():
    return sorted(k for k in PRODUCTION if k[0] == "tail")


def forms_of(mask):
    return [f for f in range(32) if (mask >> f) & 1]


# ------------------------------------------------------------------------------------------------------------------------- rounding
def bf(t):
    """t rounded to bf16 (round to nearest even), same dtype."""
    return t.to(BF).to(t.dtype)


def ulp16(v):
    """One bf16 unit in the last place at |v| (the larger binade's when |v| is within a unit of a power of two)."""
    a = v.abs() * (1 + 2.0 ** -7)
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-38))) - 7), torch.zeros_like(a))


def round_point(v, E):
    """A bf16 rounding point of the kernel: (bf16(v), allowance).  The allowance is one unit where v lies within E of a rounding
    midpoint (the kernel's value, off by up to E, may round to the other neighbour), else 0."""
    r = bf(v)
    u = ulp16(v)
    near = (u / 2 - (v - r).abs()) <= E
    return r, torch.where(near, u, torch.zeros_like(u))


def layernorm(s, Es, g, b):
    """LayerNorm of rows s [R, 256] with bound Es: (n, bound).  The derivative of the normalisation (rstd (I - 11'/N - x x'/N)) carries Es,
    plus the statistics in f32 and the f32 affine step."""
    mean = s.mean(1, keepdim=True)
    var = (s - mean).square().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xh = (s - mean) * rstd
    n = xh * g + b
    dx = rstd * (Es + Es.mean(1, keepdim=True) + xh.abs() * (xh.abs() * Es).mean(1, keepdim=True))
    stat = rstd * STATS * s.abs().mean(1, keepdim=True) + xh.abs() * STATS
    return n, g.abs() * (dx + stat) + 2.0 ** -22 * (n.abs() + b.abs())


def gemm(a, Ea, w, bias=None):
    """a [R, K] (bound Ea) @ w[N, K]^T + bias: (value, bound)."""
    v = a @ w.T
    A = a.abs() @ w.abs().T
    E = GEMM * A + Ea @ w.abs().T
    if bias is not None:
        v = v + bias
        E = E + GEMM * bias.abs()
    return v, E


def error_ratio(y, r, tol):
    """(worst |y - r| / tol, flat index); a non-finite y counts as infinite."""
    q = (y.double() - r).abs() / tol
    q = torch.where(torch.isfinite(y.double()), q, torch.full_like(q, math.inf))
    i = int(q.argmax())
    return float(q.flatten()[i]), i


def out_tol(r, E, dtype):
    """Bound of a stored output: f32 adds its own rounding, bf16 one half unit of the output (2^-8 relative) on top of twice E."""
    if dtype == torch.float32:
        return E + 2.0 ** -22 * r.abs() + 1e-30
    return 2.0 ** -8 * r.abs() + 2 * E + 1e-30


# ------------------------------------------------------------------------------------------------------------------------- tails
TAIL_TILES = (32, 64, 96, 128)
GUARD_ROWS = 128


def edge_rows(M):
    """Rows that get edge inputs: a large-mean / small-variance row and a near-constant row near the start, at a 96 / 128 tile edge and at
    the end."""
    big = [r for r in (1, 95, 127, M - 1) if 0 <= r < M]
    const = [r for r in (2, 96, 128, M - 2) if 0 <= r < M]
    return sorted(set(big)), sorted(set(const) - set(big))


def sample_tail_rows(M, pos_rows, seed, n_rand=96):
    g = torch.Generator().manual_seed(seed)
    rows = set(range(min(4, M))) | set(range(max(0, M - 4), M))
    for t in TAIL_TILES:
        nb = (M - 1) // t
        for j in {1, 2, nb} | {1 + int(v) for v in torch.randint(0, max(nb, 1), (2,), generator=g)}:
            rows |= {j * t - 1, j * t}
        rows |= {nb * t, nb * t + 1}                          # the ragged last tile
    if pos_rows:
        nw = (M - 1) // pos_rows
        for j in {1, 2, nw} | {1 + int(v) for v in torch.randint(0, max(nw, 1), (2,), generator=g)}:
            rows |= {j * pos_rows - 1, j * pos_rows}
    for r_list in edge_rows(M):
        rows |= set(r_list)
    rows |= {int(v) for v in torch.randint(0, M, (n_rand,), generator=g)}
    return torch.tensor(sorted(r for r in rows if 0 <= r < M), dtype=torch.long)


def build_tail(M, pre_norm, skip_ffn, n_pos, n_proj, pos_rows, device, seed):
    """Inputs of one tail call at production statistics (attention rows ~ N(0, 1) bf16, residual ~ N(0, 1), weights ~ N(0, 1 / K) bf16,
    norms 1 + 0.1 N / 0.1 N, out-proj bias 1e-3 N) with edge rows: |mean| = 40 with std 0.05, and a constant row (variance of s ~ 1e-6 < eps).
    Plain [N, K] weights; *_f fragment-major (on a GPU, as the kernels read them)."""
    from nopesac_amd import ops
    device = torch.device(device)
    g = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(shape, generator=g)

    c = SimpleNamespace(M=M, pre_norm=bool(pre_norm), skip_ffn=bool(skip_ffn), n_pos=n_pos, n_proj=n_proj, pos_rows=pos_rows, device=device)
    attn, src = randn(M, 256), randn(M, 256)
    big, const = edge_rows(M)
    for r in big:
        attn[r], src[r] = 0, 40 + 0.05 * randn(256)
    for r in const:
        attn[r], src[r] = 0, 3.0
    W = {"wo": (randn(256, 256) / 16).to(BF), "bo": 1e-3 * randn(256), "ga": 1 + 0.1 * randn(256), "bea": 0.1 * randn(256)}
    if not skip_ffn:
        W.update(w1=(randn(1024, 256) / 16).to(BF), b1=0.1 * randn(1024), w2=(randn(256, 1024) / 32).to(BF), b2=0.1 * randn(256),
                 gb=1 + 0.1 * randn(256), beb=0.1 * randn(256))
    c.pos = randn(pos_rows, 256) if pos_rows else None
    c.wpa = (randn(n_pos, 256) / 16).to(BF) if n_pos else None
    c.bpa = 0.1 * randn(n_pos) if n_pos else None
    c.wpb = (randn(n_proj, 256) / 16).to(BF) if n_proj else None
    c.bpb = 0.1 * randn(n_proj) if n_proj else None
    c.attn, c.src, c.W = attn.to(BF), src, W
    if device.type == "cuda":
        fm = ops.mfma_fragment_major
        c.attn_d, c.src_d = c.attn.to(device), c.src.to(device)
        c.W_d = {k: (fm(v.to(device)) if v.dtype == BF else v.to(device)) for k, v in W.items()}
        c.pos_d = c.pos.to(device) if pos_rows else None
        c.wpa_d = fm(c.wpa.to(device)) if n_pos else None
        c.bpa_d = c.bpa.to(device) if n_pos else None
        c.wpb_d = fm(c.wpb.to(device)) if n_proj else None
        c.bpb_d = c.bpb.to(device) if n_proj else None
    return c


def tail_reference(c, rows, fault=None, dtype=torch.float64):
    """Reference of the tail at `rows`: dict of (value, bound) for "s" (first residual sum), "n" (the normalised result), "u" (the
    residual stream y of a pre-norm call).  With dtype = float32 and a `fault` the same arithmetic is a CPU float32 emulation of a kernel
    (negative controls); faults act on the whole tail, so rows must then be all rows."""
    f = lambda t: t.to(dtype) if t is not None else None
    W = {k: f(v.float()) for k, v in c.W.items()}
    attn, src = f(c.attn.float())[rows], f(c.src)[rows]
    if fault == "ragged_tile_reads_last_row":                 # the 96-token form's last partial tile reads row M - 1's attention rows
        last = (c.M - 1) // 96 * 96
        attn = torch.where((rows >= last)[:, None], f(c.attn.float())[c.M - 1], attn)
    Z = torch.zeros_like(src)
    s, Es = gemm(attn, Z, W["wo"], W["bo"])
    s, Es = s + src, Es + GEMM * src.abs()
    ga, bea = W["ga"].clone(), W["bea"].clone()
    if fault == "ln_a_uses_ln_b_params_for_one_wave":
        ga[64:96], bea[64:96] = W["gb"][64:96], W["beb"][64:96]
    na, Ena = layernorm(s, Es, ga, bea)
    out = {"s": (s, Es)}
    if c.skip_ffn:
        out["n"], out["u"] = (na, Ena), (s, Es)
        return out
    x16, ux = round_point(na, Ena)                            # bf16 copy of y1 / LN_a(s): the FFN operand
    b1 = W["b1"].clone()
    if fault == "b1_missing_on_one_hidden_tile":
        b1[320:352] = 0
    h, Eh = gemm(x16, ux, W["w1"], b1)
    h16, uh = round_point(h.clamp_min(0), Eh)
    w2 = W["w2"].clone()
    if fault == "linear2_last_k_step_skipped":
        w2[:, 1008:] = 0
    z, Ez = gemm(h16, uh, w2, W["b2"])
    res, Eres = (s, Es) if c.pre_norm else (na, Ena)
    z, Ez = z + res, Ez + Eres
    n, En = layernorm(z, Ez, W["gb"], W["beb"])
    out["n"], out["u"] = (n, En), (z, Ez)
    return out


def tail_outputs_reference(c, rows, n_kernel, fault=None, dtype=torch.float64):
    """References of the bf16 outputs at `rows` from the kernel's own normalised rows n_kernel (f32 [len(rows), 256]): y16 = bf16(n),
    ypos16 = bf16(n + pos[row % pos_rows]) exactly, and f64 proj_pos / proj = (value, A) over the rounded tiles."""
    f = lambda t: t.to(dtype)
    n32 = n_kernel.float()
    prow = rows % c.pos_rows if c.pos_rows else None
    if fault == "pos_row_off_by_one_at_tile_edge" and c.pos_rows:
        prow = torch.where(rows % 32 == 31, (rows + 1) % c.pos_rows, prow)
    y16 = n32.to(BF)
    ypos16 = (n32 + c.pos[prow]).to(BF) if c.pos_rows else None
    out = {"y16": y16, "ypos16": ypos16}
    if c.n_pos:
        a = f(ypos16.float())
        if fault == "proj_pos_from_n_for_one_tile":
            a_t = f(y16.float())
            v = a @ f(c.wpa.float()).T
            v[:, 32:64] = (a_t @ f(c.wpa.float())[32:64].T)
            v = v + f(c.bpa)
        else:
            v = a @ f(c.wpa.float()).T + f(c.bpa)
        out["proj_pos"] = (v, a.abs() @ f(c.wpa.float()).abs().T + f(c.bpa).abs())
    if c.n_proj:
        a = f(y16.float())
        out["proj"] = (a @ f(c.wpb.float()).T + f(c.bpb), a.abs() @ f(c.wpb.float()).abs().T + f(c.bpb).abs())
    return out


def run_tail(c, form, want, prefetch=False, entry="transformer_tail"):
    """One launch of the call into NaN-filled buffers with GUARD_ROWS spare rows: (outputs [M, *] views, buffers)."""
    from nopesac_amd import ops
    M, dev = c.M, c.device
    bufs, out = {}, {}
    widths = {k: 256 for k in want}
    if c.n_pos:
        widths["proj_pos"] = c.n_pos
    if c.n_proj:
        widths["proj"] = c.n_proj
    for k, w in widths.items():
        dt = torch.float32 if k in ("y", "yn") else BF
        bufs[k] = torch.full((M + GUARD_ROWS, w), float("nan"), device=dev).to(dt)
        out[k] = bufs[k][:M]
    pf = None
    if prefetch:                                             # the next launch's weights: these very tensors (any valid ranges do)
        pf = ([c.W_d["wo"], c.W_d.get("w1"), c.W_d.get("w2")], 2)
    if entry == "decoder_tail":
        Wd = {"wo": c.W_d["wo"], "bo": c.W_d["bo"], "w1": c.W_d["w1"], "b1": c.W_d["b1"], "w2": c.W_d["w2"], "b2": c.W_d["b2"],
              "g3": c.W_d["ga"], "be3": c.W_d["bea"], "gn": c.W_d["gb"], "ben": c.W_d["beb"]}
        r = ops.decoder_tail(c.attn_d, c.src_d, Wd, pos=c.pos_d, want=tuple(want))
        for k in want:
            bufs[k][:M].copy_(r[k])
        return out, bufs
    if entry == "encoder_tail":
        We = {"wo": c.W_d["wo"], "bo": c.W_d["bo"], "w1": c.W_d["w1"], "b1": c.W_d["b1"], "w2": c.W_d["w2"], "b2": c.W_d["b2"],
              "g1": c.W_d["ga"], "be1": c.W_d["bea"], "g2": c.W_d["gb"], "be2": c.W_d["beb"]}
        r = ops.encoder_tail(c.attn_d, c.src_d, We, pos=c.pos_d, want=tuple(want))
        for k in want:
            bufs[k][:M].copy_(r[k])
        return out, bufs
    ops.transformer_tail(c.attn_d, c.src_d, c.W_d, pre_norm=c.pre_norm, skip_ffn=c.skip_ffn, pos=c.pos_d, want=tuple(want),
                         proj_pos=(c.wpa_d, c.bpa_d, c.n_pos) if c.n_pos else None, proj=(c.wpb_d, c.bpb_d, c.n_proj) if c.n_proj else None,
                         prefetch=pf, form=form, out=out)
    return out, bufs


# ------------------------------------------------------------------------------------------------------------------------- attention
def build_attention(B, Lq, Lk, ld, io16, seed, device, heads=8, scale=32 ** -0.5):
    """q [B*Lq, ld[0]], k / v [B*Lk, ld[1] / ld[2]] (the kernel reads columns 0..255 of each) at production statistics (q / k entries
    ~ N(0, 1): scores of std ~ 1 after the scale, v ~ N(0, 1)), with edge rows in image 0: queries whose score grows with the key index
    (the running max rises in every tile) and queries with one dominant key at the last live key."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(B * Lq, ld[0], generator=g), torch.randn(B * Lk, ld[1], generator=g), torch.randn(B * Lk, ld[2], generator=g)
    # image 0, every head: key j's first channel grows with j, and queries 0..3 align with it -> late maxima
    k[:Lk, 0:256:32] = torch.linspace(-3, 3, Lk)[:, None]
    q[0:min(4, Lq), 0:256:32] = 4.0
    # image B - 1: key Lk - 1 dominant for queries 4..7 (or the last rows when Lq is small)
    kb = (B - 1) * Lk
    k[kb + Lk - 1, 0:256] = 0.5 * torch.sign(q[(B - 1) * Lq + min(4, Lq - 1), 0:256]) * 3
    c = SimpleNamespace(B=B, Lq=Lq, Lk=Lk, heads=heads, scale=scale, io16=io16)
    if io16:
        q, k, v = q.to(BF), k.to(BF), v.to(BF)
    c.q, c.k, c.v = q, k, v
    c.qlen = c.klen = None
    if device is not None and torch.device(device).type == "cuda":
        c.q_d, c.k_d, c.v_d = q.to(device), k.to(device), v.to(device)
    return c


def attention_reference(c, b, qlen=None, klen=None, mfma=True, fault=None, dtype=torch.float64):
    """Attention of image b, all heads: (o [Lq, 256], bound).  mfma: the bf16 MFMA kernel (q * scale * log2 e rounded to bf16 once, k / v
    bf16; unnormalised probabilities rounded to bf16 before the PV product, their sum in f32); else the scalar f32 kernel.  Rows >= qlen
    and every row when klen = 0 are 0.  With dtype = float32 and a fault: a CPU float32 emulation of the MFMA kernel's tile loop."""
    Lq, Lk = c.Lq, c.Lk
    nq = Lq if qlen is None else min(qlen, Lq)
    nk = Lk if klen is None else min(klen, Lk)
    q = c.q[b * Lq:(b + 1) * Lq, :256].float()
    k = c.k[b * Lk:(b + 1) * Lk, :256].float()
    v = c.v[b * Lk:(b + 1) * Lk, :256].float()
    o = torch.zeros(Lq, 256, dtype=dtype)
    E = torch.zeros(Lq, 256, dtype=dtype)
    if nk == 0 or nq == 0:
        return o, E
    if mfma:
        sc2 = torch.tensor(c.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        qs, k, v = (q * sc2).to(BF).to(dtype), k.to(BF).to(dtype), v.to(BF).to(dtype)
    else:
        qs = (q * torch.tensor(c.scale, dtype=torch.float32)).to(dtype)
        k, v = k.to(dtype), v.to(dtype)
    for h in range(c.heads):
        cs = slice(32 * h, 32 * h + 32)
        qh = qs[:nq, cs]
        if fault == "scale_applied_twice_in_one_head" and h == 3:
            qh = (qh.float() * sc2).to(BF).to(dtype)
        kh, vh = k[:nk, cs], v[:nk, cs]
        if fault == "v_rows_shifted_in_second_tile" and nk > 33:
            vh = vh.clone()
            vh[32:min(64, nk) - 1] = v[33:min(64, nk), cs]
        S = qh @ kh.T
        ES = GEMM * (qh.abs() @ kh.abs().T)
        if fault == "key_mask_at_nk_minus_1":
            S[:, nk - 1] = -math.inf
        if dtype == torch.float32 and mfma:
            oh = _online_softmax_f32(S, vh, 32, skip_rescale=fault == "running_max_rescale_skipped")
            o[:nq, cs] = oh
            continue
        m = S.max(1, keepdim=True).values
        base = 2.0 if mfma else math.e
        p = torch.pow(torch.tensor(base, dtype=dtype), S - m)
        ps = p.sum(1, keepdim=True)
        oh = (p @ vh) / ps
        o[:nq, cs] = oh
        # bounds: scores (f32 GEMM) through the exponent, the probabilities' bf16 rounding, the PV accumulation and rescales, the division
        lnb = math.log(base)
        Em = ES.gather(1, S.argmax(1, keepdim=True))
        dp = lnb * (ES + Em + 2.0 ** -23 * (S.abs() + m.abs())) + 2.0 ** -21
        pv = (p @ vh.abs()) / ps
        Eh = ((p * dp) @ vh.abs() + (p * dp).sum(1, keepdim=True) * oh.abs()) / ps
        Eh = Eh + 2.0 ** -18 * pv + 2.0 ** -22 * oh.abs()
        if mfma:
            Eh = Eh + 2.0 ** -9 * pv
        E[:nq, cs] = Eh
    return o, E


def _online_softmax_f32(S, V, tile, skip_rescale=False):
    """The MFMA kernel's loop in float32: per key tile a running max, exp2, bf16 probabilities into the PV product, f32 sum."""
    R = S.shape[0]
    m_run = torch.full((R, 1), -math.inf)
    l_run = torch.zeros(R, 1)
    o = torch.zeros(R, V.shape[1])
    for t0 in range(0, S.shape[1], tile):
        s = S[:, t0:t0 + tile].float()
        m_new = torch.maximum(m_run, s.max(1, keepdim=True).values)
        alpha = torch.exp2(m_run - m_new)
        p = torch.exp2(s - m_new)
        l_run = l_run * alpha + p.sum(1, keepdim=True)
        if not (skip_rescale and t0 == tile):
            o = o * alpha
        o = o + p.to(BF).float() @ V[t0:t0 + tile].float()
        m_run = m_new
    return o / l_run


# ------------------------------------------------------------------------------------------------------------------------- GNN
def gnn_lengths(nq, n_sets, seed):
    """Set lengths: {0, 1, 31, 32, 33, 63, 64, 65, nq - 1, nq} (those <= nq) first, then random, so that the two halves of a cross pair
    differ."""
    base = [n for n in (0, 1, 31, 32, 33, 63, 64, 65, nq - 1, nq) if n <= nq]
    g = torch.Generator().manual_seed(seed)
    lens = [base[i % len(base)] if i < len(base) else int(torch.randint(0, nq + 1, (1,), generator=g)) for i in range(n_sets)]
    if n_sets >= 2:                                          # rotate the second half: n1 != n2 per pair
        h = n_sets // 2
        lens[h:] = lens[h + 1:] + lens[h:h + 1] if n_sets - h > 1 else lens[h:]
    return torch.tensor(lens, dtype=torch.int32)


def build_gnn_weights(seed):
    """One layer's weights as the packer makes them: plain bf16 [N, K] (wq = bf16(Wq * 32^-0.5)) and f32 norms."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)
    W = {"wq": (r(256, 256) / 16 * (32 ** -0.5)).to(BF), "wk": (r(256, 256) / 16).to(BF), "wv": (r(256, 256) / 16).to(BF),
         "wm": (r(256, 256) / 16).to(BF), "w0": (r(512, 512) / math.sqrt(512)).to(BF), "w2": (r(256, 512) / math.sqrt(512)).to(BF),
         "g1": 1 + 0.1 * r(256), "b1": 0.1 * r(256), "g2": 1 + 0.1 * r(256), "b2": 0.1 * r(256)}
    return W


def gnn_weights_device(W, device):
    from nopesac_amd import ops
    return {k: (ops.mfma_fragment_major(v.to(device)) if v.dtype == BF else v.to(device).contiguous()) for k, v in W.items()}


def gnn_features(n_sets, nq, seed):
    """x [n_sets, nq, 256] f32 at production statistics: N(0, 1) descriptors, with set rows of growing norm so that the score maxima
    of the second key chunk exceed the first's."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_sets, nq, 256, generator=g)
    x = x * (1 + 0.5 * torch.arange(nq, dtype=torch.float32) / nq)[None, :, None]
    return x


def gnn_reference(W, x, s, nrow, nkey, fault=None, dtype=torch.float64):
    """One GNN layer for one set: x / s f32 [nq, 256] (query / source set), nrow query rows live, nkey keys -> (out [nq, 256], bound).
    Rows >= nrow get a zero message (the kernel's `live` flag), as does every row when nkey = 0; the merge then sees zeros."""
    f = lambda t: t.float().to(dtype)
    nq = x.shape[0]
    Wd = {k: f(v) for k, v in W.items()}
    x16, s16 = f(x.to(BF)), f(s.to(BF))
    Z = torch.zeros(nq, 256, dtype=dtype)
    q, Eq = gemm(x16, Z, Wd["wq"])
    q, uq = round_point(q, Eq)
    if fault == "second_query_block_reuses_block_0_q" and nq > 64:
        q = q.clone()
        q[64:] = q[:nq - 64]
    k, Ek = gemm(s16, Z, Wd["wk"])
    k, uk = round_point(k, Ek)
    v, Ev = gemm(s16, Z, Wd["wv"])
    v, uv = round_point(v, Ev)
    msg = torch.zeros(nq, 256, dtype=dtype)
    Emsg = torch.zeros(nq, 256, dtype=dtype)
    nk = nkey
    if nk > 0:
        for h in range(8):
            cs = slice(32 * h, 32 * h + 32)
            S = q[:, cs] @ k[:nk, cs].T
            ES = GEMM * (q[:, cs].abs() @ k[:nk, cs].abs().T) + uq[:, cs] @ k[:nk, cs].abs().T + q[:, cs].abs() @ uk[:nk, cs].T
            if dtype == torch.float32:
                msg[:, cs] = _gnn_online_f32(S, v[:nk, cs], skip_chunk2=fault == "chunk2_rescale_skipped")
                continue
            m = S.max(1, keepdim=True).values
            p = torch.exp(S - m)
            ps = p.sum(1, keepdim=True)
            oh = (p @ v[:nk, cs]) / ps
            Em = ES.gather(1, S.argmax(1, keepdim=True))
            dp = ES + Em + 2.0 ** -23 * (S.abs() + m.abs()) + 2.0 ** -21
            pv = (p @ v[:nk, cs].abs()) / ps
            Eh = ((p * dp) @ v[:nk, cs].abs() + (p * dp).sum(1, keepdim=True) * oh.abs()) / ps
            Eh = Eh + (p @ uv[:nk, cs]) / ps + 2.0 ** -18 * pv + 2.0 ** -9 * pv + 2.0 ** -22 * oh.abs()
            msg[:, cs], Emsg[:, cs] = oh, Eh
    live = (torch.arange(nq) < nrow)[:, None] & (nkey > 0)
    msg = torch.where(live, msg, torch.zeros_like(msg))
    Emsg = torch.where(live, Emsg, torch.zeros_like(Emsg))
    msg, umsg = round_point(msg, Emsg)
    mm, Emm = gemm(msg, umsg, Wd["wm"])
    m1, Em1 = layernorm(mm, Emm, Wd["g1"], Wd["b1"])
    m16, um = round_point(m1, Em1)
    hx, Ehx = gemm(x16, Z, Wd["w0"][:, :256])
    hm, Ehm = gemm(m16, um, Wd["w0"][:, 256:])
    h16, uh = round_point((hx + hm).clamp_min(0), Ehx + Ehm)
    z, Ez = gemm(h16, uh, Wd["w2"])
    xr = f(x)
    if fault == "residual_added_before_ln2":
        n, En = layernorm(z + xr, Ez, Wd["g2"], Wd["b2"])
        return n, En
    n, En = layernorm(z, Ez, Wd["g2"], Wd["b2"])
    return xr + n, En + 2.0 ** -23 * (xr + n).abs()


def _gnn_online_f32(S, V, skip_chunk2=False):
    """The GNN kernel's per-chunk loop in float32: 64 keys per chunk, natural exp, bf16 probabilities, f32 running sum."""
    R = S.shape[0]
    m_run = torch.full((R, 1), -math.inf)
    l_run = torch.zeros(R, 1)
    o = torch.zeros(R, V.shape[1])
    for c, t0 in enumerate(range(0, S.shape[1], 64)):
        s = S[:, t0:t0 + 64].float()
        mx = torch.maximum(m_run, s.max(1, keepdim=True).values)
        sc = torch.ones_like(mx) if c == 0 else torch.exp(m_run - mx)
        p = torch.exp(s - mx)
        l_run = l_run * sc + p.sum(1, keepdim=True)
        if c > 0 and not (skip_chunk2 and c == 1):
            o = o * sc
        o = o + p.to(BF).float() @ V[t0:t0 + 64].float()
        m_run = mx
    return o / l_run
