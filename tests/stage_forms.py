"""The non-GEMM stage kernels behind the heads - the matcher tail (matcher.hip), post-selection (postselect.hip) and the wavefront parts of
the one-plane RANSAC (ransac.hip) - as data: which BUILD each entry point picks for a shape (a restatement of the host dispatch, so a test
can name the build it reaches), float64 references of every operation in plain torch (written from the kernels' comments and the oracle's
formulas; no library call and no oracle call on the float64 path), seeded input generators whose decisions are not trivial, and the case
lists of tests/test_stage_forms_gpu.py.  tests/test_stage_forms_cpu.py proves the tables complete and the references and inputs fit.
Imports without a GPU."""
from __future__ import annotations

import functools
import math

import torch
from torch.nn import functional as F

from nopesac_amd.synth import _g, consistent_planes, rand_planes, rand_unit_quat
from tests import golden_inputs as GI

F64 = torch.float64
NQS = (50, 64, 100, 128)                     # the three bench legs' plane counts (head_forms.LEG_NQ) and the 100 in between

# ===================================================================================================================== forms: Sinkhorn
SINK_BUILDS = ("w4<13>", "w4<16>", "wg<2,17>", "wg<2,26>", "wg<2,32>", "wg<3,33>", "k1024<16>", "k1024<36>")
SINK_SWITCHES = ("NOPESAC_SINKHORN_NO_W4", "NOPESAC_SINKHORN_NO_WG")


def sinkhorn_build(nq, no_w4=False, no_wg=False):
    """The build nopesac_matcher_sinkhorn launches (matcher.hip, the dispatch at the end of the file)."""
    if not 1 <= nq <= 128:
        raise ValueError("sinkhorn: nq in 1..128")
    R = nq + 1
    if R <= 64 and not no_w4:
        return "w4<13>" if R <= 52 else "w4<16>"
    if not no_wg:
        return "wg<2,17>" if R <= 4 * 17 else ("wg<2,26>" if R <= 4 * 26 else ("wg<2,32>" if R <= 128 else "wg<3,33>"))
    return "k1024<16>" if R <= 128 else "k1024<36>"


# (nq, build): every build at the first and the last size it serves; the 1024-thread builds behind both switches
SINK_GPU_CASES = ([(n, "w4<13>") for n in (1, 7, 50, 51)] + [(n, "w4<16>") for n in (52, 63)] + [(n, "wg<2,17>") for n in (64, 67)] +
                  [(n, "wg<2,26>") for n in (68, 103)] + [(n, "wg<2,32>") for n in (104, 127)] + [(128, "wg<3,33>")] +
                  [(n, "k1024<16>") for n in (50, 64, 100, 127)] + [(128, "k1024<36>")])
SINK_ITERS = (200, 0, 1)


def sinkhorn_switches(nq, build):
    """The environment a case needs so that `build` is what runs at nq."""
    env = dict.fromkeys(SINK_SWITCHES, "1") if build.startswith("k1024") else {}
    assert sinkhorn_build(nq, *(k in env for k in SINK_SWITCHES)) == build, (nq, build)
    return env


def sinkhorn_pairs(nq):
    """(n1, n2) of one launch (<= 12 pairs): full, single, an empty side, both empty, thin on either side, and 63 / 64 / 65 rows or
    columns (a row group of the wg builds exactly full / one into the next) where nq allows."""
    k = max(nq // 2, 1)
    pairs = [(nq, nq), (1, 1), (0, k), (k, 0), (nq, min(2, nq)), (min(3, nq), nq), (0, 0)]
    pairs += [p for p in ((63, 64), (64, 63), (65, nq), (nq, 65)) if max(p) <= nq]
    if nq > 3:
        pairs.append((nq - 1, nq // 3 + 1))
    out = []
    for p in pairs:
        if p not in out:
            out.append(p)
    assert len(out) <= 12
    return out


# Floors: rel_err of the oracle's float32 evaluation (f32 geometric priors, f32 scores, oracle.log_sinkhorn, 200 iterations) against the
# float64 reference below, worst pair of the launch sinkhorn_inputs(nq) - the cost of f32 arithmetic over 200 iterations at that size.
# The kernels' bound is SINK_FLOOR_FACTOR times the floor (another summation order; the 1-ulp hardware exp / log of the w4 / wg builds),
# for every iteration count, and at nq = 50 never above the 5e-5 that test_matcher_ragged_batch holds.  Printed by
#   python -c "from tests import stage_forms as S; S.print_sinkhorn_floors()"
# and re-measured by tests/test_stage_forms_cpu.py (a floor off by more than 2x fails).
SINK_FLOOR = {1: 6.56e-06, 7: 7.24e-07, 50: 1.14e-06, 51: 1.68e-06, 52: 1.08e-06, 63: 9.34e-07, 64: 3.24e-06, 67: 6.18e-06, 68: 2.79e-06,
              100: 3.62e-06, 103: 1.74e-06, 104: 1.18e-06, 127: 1.93e-06, 128: 4.86e-06}
SINK_FLOOR_FACTOR = 4.0
SINK_NQ50_BOUND = 5e-5


def sinkhorn_bound(nq):
    b = SINK_FLOOR_FACTOR * SINK_FLOOR[nq]
    return min(b, SINK_NQ50_BOUND) if nq == 50 else b


# ===================================================================================================================== forms: post-selection
PS_TW = 64
PS_LDS_LIMIT = 64 * 1024
PS_BUILDS = ((1, False), (2, False), (4, True), (4, False), (8, False))
REFUSED = "refused"


def ps_pad4(n):
    return (n + 3) & ~3


def ps_head_words(nq):
    return ((9 * nq + 3) & ~3) + 2 * ps_pad4(nq) + 4


def postselect_form(nq, h, w, H, W, ps_th=None):
    """(th, ROWS, X4) of the pixel kernel nopesac_postselect_planes_ex launches, or REFUSED (postselect.hip: the tile height is 16 rows, or
    what NOPESAC_PS_TH asks for, halved until the source tile of all nq queries fits 64 KB of LDS)."""
    th = 16
    if ps_th is not None:
        v = int(ps_th)
        th = 32 if v >= 32 else (16 if v >= 16 else (8 if v >= 8 else 4))
    src_cols = (PS_TW * w + W - 1) // W + 2
    while True:
        src_rows = (th * h + H - 1) // H + 2
        lds = 4 * ps_head_words(nq) + 4 * src_rows * src_cols * ps_pad4(nq)
        if lds <= PS_LDS_LIMIT or th == 4:
            break
        th >>= 1
    if lds > PS_LDS_LIMIT:
        return REFUSED
    return th, th // 4, th == 16 and H == 4 * h


# geometry name -> (h, w, H, W, NOPESAC_PS_TH)
PS_GEOMETRIES = {
    "8x32_x4": (8, 32, 32, 128, None),        # <4, X4>: two tiles each way, top and bottom border rows
    "8x25_x4": (8, 25, 32, 100, None),        # W no multiple of 64
    "7x20_x4": (7, 20, 28, 80, None),         # H no multiple of 16
    "10x20_x3": (10, 20, 30, 60, None),       # H = 3 h: <4, false>
    "12x24_x2": (12, 24, 24, 48, None),       # the host loop halves to th = 8 at nq = 50: <2, false>; refused at nq = 128
    "8x32_th4": (8, 32, 32, 128, 4),          # <1, false>
    "8x32_th32": (8, 32, 32, 128, 32),        # <8, false> (where the 32-row tile fits: nq <= 64)
    "6x12_x5": (6, 12, 30, 60, None),         # 5x: the 16-row tile of all 128 queries fits, <4, false> with both count registers
    "4x8_x8_th32": (4, 8, 32, 64, 32),        # 8x: the 32-row tile fits at nq = 128, <8, false> with both count registers
}
PS_NV = (0, 1, 3, 5, 63, 64, 65, 127, 128)


def _ps_cases():
    """(nq, geometry, (valid queries of image 0, of image 1)).  Every count of PS_NV that nq allows runs on the plain 4x geometry;
    the other geometries take the pairs that straddle a count register (63 / 64 / 65) or fill the list (nq), and the fallback."""
    nv = {50: [(0, 1), (3, 5), (50, 47)], 64: [(0, 1), (3, 5), (63, 64)], 100: [(0, 5), (1, 3), (63, 64), (65, 100), (99, 98)],
          128: [(0, 3), (1, 5), (63, 64), (65, 127), (128, 126)]}
    cases = []
    for nq in NQS:
        for pair in nv[nq] + [(-5, 5)]:
            cases.append((nq, "8x32_x4", pair))
        big = nv[nq][-1]
        for geom in ("8x25_x4", "7x20_x4", "10x20_x3", "8x32_th4", "8x32_th32"):
            cases.append((nq, geom, big))
            cases.append((nq, geom, nv[nq][1]))
        cases.append((nq, "6x12_x5", big))
        if nq >= 100:
            cases.append((nq, "4x8_x8_th32", big))
        cases.append((nq, "12x24_x2", big if postselect_form(nq, 12, 24, 24, 48) != REFUSED else (3, 5)))
    return cases


PS_SEEDS = {(100, "10x20_x3", (99, 98)): 1, (128, "10x20_x3", (128, 126)): 2}                                 # (nq, geometry, pair) -> seed offset where the first seed does not meet the input conditions
PS_GPU_CASES = _ps_cases()                   # (defined after PS_SEEDS' keys: the cases themselves)
PS_MARGIN = 2e-5       # per-pixel decision margin.  The kernel forms the tap position scale * (X + 0.5) - 0.5 in f32: with w <= 32 source
#                        columns that is an absolute error <= 4e-6 in the blend weight, so <= 4e-6 in a probability (taps differ by <= 1),
#                        plus ~5e-7 from the three roundings of the blend and one of the score product; twice that, rounded up
PS_PIXEL_CAP = 5e-4    # share of pixels of an image that may sit inside the margin
PS_OVERLAP_MARGIN = 1e-3


def ps_case_id(c):
    return "nq%d_%s_nv%d-%d" % (c[0], c[1], c[2][0], c[2][1])


# ===================================================================================================================== float64 geometry
_FLIP = torch.tensor([1.0, -1.0, -1.0], dtype=F64)


def quat_to_rot(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                        2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], dim=-1).reshape(*q.shape[:-1], 3, 3)


def warp(p, q, t):
    """common.h warp_plane: end = R flip(p) + t, b = end - t, out = (end . b) / (|b| + 1e-5)^2 b.  p [..., n, 3], q [..., 4], t [..., 3]."""
    end = torch.einsum("...ij,...nj->...ni", quat_to_rot(q), p * _FLIP) + t.unsqueeze(-2)
    b = end - t.unsqueeze(-2)
    return ((end * b).sum(-1) / (b.norm(dim=-1) + 1e-5) ** 2).unsqueeze(-1) * b


def unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def pair_geometry(p1, p2, q, t):
    """normal angle [deg], raw offset distance and the sign-deciding dot product n1_rt . n2 for every (view-1, view-2) plane pair."""
    f2 = p2 * _FLIP
    n2, o2 = unit(f2), f2.norm(dim=-1)
    ang = torch.acos((unit(warp(p1, q, torch.zeros_like(t))) @ n2.T).clamp(-1, 1)) / math.pi * 180.0
    w_rt = warp(p1, q, t)
    o1 = w_rt.norm(dim=-1)
    ntn = unit(w_rt) @ n2.T
    off = torch.where(ntn < 0, (o1[:, None] + o2[None]).abs(), (o1[:, None] - o2[None]).abs())
    return ang, off, ntn


# ===================================================================================================================== matcher tail
MATCH_THR, OFFSET_MULT, NORMAL_MULT, BIN_SCORE = 0.2, 4.0, 8.0, 0.7
NTN_MARGIN, ANGLE_MARGIN = 1e-3, 1.0          # pairs left out of the log-score comparison: the offset sign branch may flip; acos amplifies
PAIR_CAP, ROW_CAP = 5e-3, 1e-2


def log_sinkhorn64(scores, bin_score, iters):
    """[n1, n2] f64 couplings -> ([n1+1, n2+1] log scores, norm); dustbin row / column, `iters` log-space iterations, Z + u + v - norm."""
    n1, n2 = scores.shape
    b = torch.tensor(float(bin_score), dtype=F64)
    Z = torch.cat([torch.cat([scores, b.expand(n1, 1)], 1), b.expand(1, n2 + 1)], 0)
    lg = lambda n: torch.log(torch.tensor(float(n), dtype=F64))
    norm = -lg(n1 + n2)
    log_mu = torch.cat([norm.expand(n1), (lg(n2) + norm).view(1)])
    log_nu = torch.cat([norm.expand(n2), (lg(n1) + norm).view(1)])
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return Z + u[:, None] + v[None] - norm, norm


def matcher_scores64(dot, p1, p2, cam7, offset_mult=OFFSET_MULT, normal_mult=NORMAL_MULT):
    """dot [n1,n2], planes [n,3], cam7 = (t, q), all f64 -> (scores, mask of the pairs whose f32 evaluation may take the other branch)."""
    ang, off, ntn = pair_geometry(p1, p2, cam7[3:], cam7[:3])
    scores = dot - off.clamp(1e-10, 5.0) / offset_mult - ang / normal_mult
    return scores, (ntn.abs() < NTN_MARGIN) | (ang < ANGLE_MARGIN)


def top2_gap(x, dim):
    if x.shape[dim] < 2:
        return torch.full(x.max(dim).values.shape, float("inf"), dtype=x.dtype)
    t = x.topk(2, dim=dim).values
    return t.select(dim, 0) - t.select(dim, 1)


def matcher_reference(c, b, iters, margin):
    """Pair b of a sinkhorn_inputs case -> dict: `ls` the padded [nq+1, nq+1] f64 log scores (-1e30 outside; None when n1 = n2 = 0),
    `A` [nq, nq], `pair_out` [nq+1, nq+1] (entries left out of the log-score comparison), `a_keep` [nq, nq] (assignment entries that are
    compared), `n_out_rows`.  `margin`: absolute log-score distance under which a row / column decision is left out."""
    nq, n1, n2 = c["nq"], int(c["n1"][b]), int(c["n2"][b])
    A = torch.zeros(nq, nq, dtype=F64)
    out = {"n1": n1, "n2": n2, "A": A, "ls": None, "a_keep": torch.ones(nq, nq, dtype=torch.bool), "n_out_rows": 0, "n_out_pairs": 0}
    if n1 + n2 == 0:
        return out
    sc, risky = matcher_scores64(c["dot"][b, :n1, :n2].double(), c["p1"][b, :n1].double(), c["p2"][b, :n2].double(), c["cam7"][b].double())
    ls, _ = log_sinkhorn64(sc, BIN_SCORE, iters)
    pad = torch.full((nq + 1, nq + 1), -1e30, dtype=F64)
    rows = list(range(n1)) + [nq]
    cols = list(range(n2)) + [nq]
    pad[torch.tensor(rows)[:, None], torch.tensor(cols)[None]] = ls
    out["ls"], out["block"] = pad, ls
    po = torch.zeros(nq + 1, nq + 1, dtype=torch.bool)
    po[:n1, :n2] = risky
    out["pair_out"], out["n_out_pairs"] = po, int(risky.sum())
    if n1 and n2:
        s = ls[:n1, :n2]
        v0, i0 = s.max(1)
        i1 = s.max(0).indices
        ok = (i1[i0] == torch.arange(n1)) & (v0.exp() > MATCH_THR)
        A[torch.arange(n1)[ok], i0[ok]] = 1.0
        row_out = (top2_gap(s, 1) < margin) | ((v0.exp() - MATCH_THR).abs() < margin)
        col_out = top2_gap(s, 0) < margin
        out["a_keep"][:n1, :n2] = ~row_out[:, None] & ~col_out[None]
        out["n_out_rows"] = int(row_out.sum() + col_out.sum())
    return out


SINK_SEED_STEP = {7: 1}           # nq -> seed step where the first seed leaves more pairs or rows inside the margins than the caps allow


@functools.lru_cache(maxsize=None)
def sinkhorn_inputs(nq):
    """One launch at nq (f32 CPU tensors): per pair consistent matched planes seen under a perturbed pose (as golden_inputs.matcher_case),
    dot products built directly - matched pairs well above the dustbin score, the rest N(0, 2) - and random planes / dots in the padding."""
    g = _g(7000 + nq + 1000 * SINK_SEED_STEP.get(nq, 0))
    pairs = sinkhorn_pairs(nq)
    B = len(pairs)
    dot = 2.0 * torch.randn(B, nq, nq, generator=g)
    p1 = torch.stack([rand_planes(nq, g) for _ in range(B)])
    p2 = torch.stack([rand_planes(nq, g) for _ in range(B)])
    cam7 = torch.zeros(B, 7)
    for b, (n1, n2) in enumerate(pairs):
        lo = min(n1, n2)
        nc = (max(lo - lo // 4, 1) if lo > 1 else 1) if lo > 0 else 0
        if lo > 0:
            a1, a2, perm, (t, q) = consistent_planes(n1, n2, nc, g)
            p1[b, :n1], p2[b, :n2] = a1, a2
            for i in range(n1):
                if perm[i] >= 0:
                    dot[b, i, perm[i]] = BIN_SCORE + 6.0 + 3.0 * torch.rand(1, generator=g).item()
        else:
            t, q = 0.4 * torch.randn(3, generator=g), rand_unit_quat(g)
        cam7[b] = torch.cat([t + 0.05 * torch.randn(3, generator=g), F.normalize(q + 0.03 * torch.randn(4, generator=g), dim=0)])
    return {"nq": nq, "pairs": pairs, "dot": dot, "p1": p1, "p2": p2, "cam7": cam7,
            "n1": torch.tensor([p[0] for p in pairs], dtype=torch.int32), "n2": torch.tensor([p[1] for p in pairs], dtype=torch.int32)}


def block_rel_err(got, ref, leave_out=None):
    """rel_err (max |a - b| / max |b|) over the finite entries of ref that are not left out; infinities must coincide."""
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf] > 0, ref[inf] > 0), "infinite entries differ"
    keep = ~inf if leave_out is None else ~inf & ~leave_out
    if not keep.any():
        return 0.0
    return float((got.double() - ref)[keep].abs().max() / (ref[~inf].abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def matcher_references(nq, iters):
    c = sinkhorn_inputs(nq)
    peak = max((float(r["block"][torch.isfinite(r["block"])].abs().max()) for r in
                (matcher_reference(c, b, iters, 0.0) for b in range(len(c["pairs"]))) if r["ls"] is not None), default=1.0)
    # a decision is compared where twice the allowed log-score error cannot change it
    return [matcher_reference(c, b, iters, 2.0 * sinkhorn_bound(nq) * peak + 1e-9) for b in range(len(c["pairs"]))]


def oracle_f32_sinkhorn_floor(nq, iters=200):
    """Worst pair rel_err of the oracle's f32 matcher tail against the f64 reference on sinkhorn_inputs(nq) (pairs with a plane on both
    sides: the oracle's log_sinkhorn takes log(n) of both counts)."""
    from oracle import nopesac_oracle as O
    c = sinkhorn_inputs(nq)
    worst = 0.0
    for b, r in enumerate(matcher_references(nq, iters)):
        n1, n2 = r["n1"], r["n2"]
        if not (n1 and n2):
            continue
        ang, off = O._geometric_dists(c["p1"][b, :n1], c["p2"][b, :n2], c["cam7"][b, 3:], c["cam7"][b, :3], 1e-10, 5.0)
        s32 = c["dot"][b, :n1, :n2] - off / OFFSET_MULT - ang / NORMAL_MULT
        ls32 = O.log_sinkhorn(s32, torch.tensor(BIN_SCORE), iters)
        lo = torch.zeros_like(r["block"], dtype=torch.bool)
        lo[:n1, :n2] = r["pair_out"][:n1, :n2]
        worst = max(worst, block_rel_err(ls32.double(), r["block"], lo))
    return worst


def print_sinkhorn_floors():
    for nq in sorted({n for n, _ in SINK_GPU_CASES} | set(NQS)):
        print("%d: %.2e," % (nq, oracle_f32_sinkhorn_floor(nq)))


# ---- assignment re-filter (matcher.hip refilter_kernel)
REFILTER_ANGLE_MARGIN, REFILTER_OFFSET_MARGIN = 1e-3, 1e-4


def refilter_reference(A, p1, p2, n1, n2, rot, trans):
    """One pair, f64 -> (filtered assignment [nq, nq], entries that are compared)."""
    nq = A.shape[0]
    q = rot.double()
    q = -q if q[0] < 0 else q
    ang, off, _ = pair_geometry(p1[:n1].double(), p2[:n2].double(), q, trans.double())
    off = off.clamp(1e-4, 10.0)
    out = torch.zeros(nq, nq, dtype=F64)
    out[:n1, :n2] = A[:n1, :n2].double() * ((ang < 45.0) & (off < 1.0)).double()
    keep = torch.ones(nq, nq, dtype=torch.bool)
    keep[:n1, :n2] = ~(((ang - 45.0).abs() < REFILTER_ANGLE_MARGIN) | ((off - 1.0).abs() < REFILTER_OFFSET_MARGIN))
    return out, keep


# ===================================================================================================================== RANSAC
def ransac_ms(nq):
    return [0, 1, 2, nq - 1, nq, nq // 2]


@functools.lru_cache(maxsize=None)
def ransac_inputs(nq):
    """<= 6 pairs, one per m of ransac_ms(nq): a 0/1 assignment with exactly m ones inside [:n1, :n2] - one row holds two of them - and
    ones OUTSIDE the valid block that must not count; ragged (n1, n2); raw hypothesis quaternions with one of norm < 1e-12; random
    score features, fused features and regression weights."""
    g = _g(9000 + nq)
    ms = ransac_ms(nq)
    B = len(ms)
    A = torch.zeros(B, nq, nq)
    p1, p2 = torch.zeros(B, nq, 3), torch.zeros(B, nq, 3)
    n1s, n2s, rots, trs = [], [], [], []
    for b, m in enumerate(ms):
        n1 = min(max(m, 1) + (3 if b % 2 else 0), nq)
        n2 = min(max(m, 1) + (0 if b % 2 else 2), nq)
        a1, a2, perm, (t, q) = consistent_planes(n1, n2, min(m, n1, n2), g, noise=0.05) if m else (
            rand_planes(n1, g), rand_planes(n2, g), torch.full((n1,), -1, dtype=torch.long), (0.4 * torch.randn(3, generator=g), rand_unit_quat(g)))
        ones = [(i, int(perm[i])) for i in range(n1) if perm[i] >= 0][:m]
        if m >= 2:                                   # move the last one into the first one's row, at a free column
            i0 = ones[0][0]
            free = [j for j in range(n2) if j not in {o[1] for o in ones[:-1]}]
            ones[-1] = (i0, free[-1])
        for i, j in ones:
            A[b, i, j] = 1.0
        assert int(A[b].sum()) == m
        A[b, n1:, :] = 1.0                            # outside the valid block: never counted
        A[b, :, n2:] = 1.0
        p1[b], p2[b] = rand_planes(nq, g), rand_planes(nq, g)
        p1[b, :n1], p2[b, :n2] = a1, a2
        n1s.append(n1); n2s.append(n2)
        r0 = F.normalize(q + 0.05 * torch.randn(4, generator=g), dim=0)
        rots.append(-r0 if r0[0] < 0 else r0)
        trs.append(t + 0.1 * torch.randn(3, generator=g))
    rot_raw = torch.randn(B, nq, 4, generator=g) * (0.2 + 2.0 * torch.rand(B, nq, 1, generator=g))
    rot_raw[0, 0] = 1e-20 * torch.randn(4, generator=g)
    rot_raw[B - 1, nq - 1] = 1e-20 * torch.randn(4, generator=g)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"nq": nq, "ms": ms, "A": A, "p1": p1, "p2": p2, "n1": torch.tensor(n1s, dtype=torch.int32), "n2": torch.tensor(n2s, dtype=torch.int32),
            "init_rot": torch.stack(rots), "init_trans": torch.stack(trs), "rot_raw": rot_raw, "trans_raw": 0.5 * r(B, nq, 3),
            "sf_rot": r(B, nq + 1, 64), "sf_trans": r(B, nq + 1, 64), "reg_rot_w": r(64) / 4, "reg_rot_b": r(1), "reg_trans_w": r(64) / 4,
            "reg_trans_b": r(1), "init_rot_feat": F.relu(r(B, 256)), "init_trans_feat": F.relu(r(B, 256)), "fused_rot": F.relu(r(B, nq, 256)),
            "fused_trans": F.relu(r(B, nq, 256)), "rots_w": r(4, 256) / 16, "rots_b": r(4) / 4, "trans_w": r(3, 256) / 16, "trans_b": r(3) / 4,
            "refilter_A": (torch.rand(B, nq, nq, generator=g) < 0.6).float() * (0.5 + 0.5 * (torch.rand(B, nq, nq, generator=g) < 0.8).float())}


SIG_MARGIN = 1e-6


def geo_sequence_reference(c, b, warp_in_ref):
    """ransac.hip geo_sequence_kernel in f64 -> dict(m, geo_local, geo_global [nq,6], sig [nq], geo_enc [nq,8], sig_margin)."""
    nq, n1, n2 = c["nq"], int(c["n1"][b]), int(c["n2"][b])
    idx = torch.nonzero(c["A"][b, :n1, :n2])[:nq]                     # row-major order
    m = idx.shape[0]
    P1, P2 = c["p1"][b].double()[idx[:, 0]], c["p2"][b].double()[idx[:, 1]]
    q, t = c["init_rot"][b].double(), c["init_trans"][b].double()
    g1, ga, f2 = warp(P1, q, t), warp(P1, q, torch.zeros(3, dtype=F64)), P2 * _FLIP
    prod = g1[:, 0] * ga[:, 0]
    sg = torch.where(prod >= 0, 1.0, -1.0).double()
    s0, s1 = (g1, f2) if warp_in_ref else (P1, P2)
    o0, o1 = s0.norm(dim=-1, keepdim=True), s1.norm(dim=-1, keepdim=True)
    e = torch.cat([s0 / (o0 + 1e-10), o0, s1 / (o1 + 1e-10), o1], -1)
    if warp_in_ref:
        e[:, :4] *= sg[:, None]
    z = lambda k, fill=0.0: torch.full((nq, k), fill, dtype=F64)
    out = {"m": m, "geo_local": z(6), "geo_global": z(6), "geo_enc": z(8), "sig": z(1, 1.0)[:, 0],
           "sig_margin": float(prod.abs().min()) if m else float("inf")}
    out["geo_local"][:m], out["geo_global"][:m], out["geo_enc"][:m], out["sig"][:m] = torch.cat([P1, P2], -1), torch.cat([g1, f2], -1), e, sg
    return out


def score_maps_reference(geo_local, rot_raw, trans_raw, init_rot, init_trans, m):
    """ransac.hip ransac_score_maps_kernel for one pair in f64 (inputs: the f32 tensors the kernel reads).  `offset_out`: the entries of
    offset_dist whose sign branch an f32 evaluation may take the other way."""
    nq = geo_local.shape[0]
    gl = geo_local.double()
    rr = rot_raw.double()
    rots = torch.cat([init_rot.double()[None], rr / rr.norm(dim=-1, keepdim=True).clamp_min(1e-12)], 0)       # [NH,4]
    trans = torch.cat([init_trans.double()[None], trans_raw.double()], 0)
    p0 = gl[:, :3][None].expand(nq + 1, -1, -1)
    p1 = (gl[:, 3:] * _FLIP)[None].expand(nq + 1, -1, -1)
    w_r, w_rt = warp(p0, rots, torch.zeros(nq + 1, 3, dtype=F64)), warp(p0, rots, trans)
    n0, n1v, n0t = unit(w_r), unit(p1), unit(w_rt)
    ang = torch.acos((n0 * n1v).sum(-1).clamp(-1, 1)) / math.pi * 180.0
    dn = (n0 - n1v).norm(dim=-1)
    off0, off1 = w_rt.norm(dim=-1), p1.norm(dim=-1)
    ntn = (n0t * n1v).sum(-1)
    doff = torch.where(ntn < 0, (off0 + off1).abs(), (off0 - off1).abs())
    dl2 = (w_rt - p1).norm(dim=-1)
    mask = torch.zeros(nq + 1, nq, dtype=F64)
    mask[:m + 1, :m] = 1.0
    return {"rots_all": rots, "trans_all": trans, "normal_score": torch.exp(-dn * mask) * mask, "param_score": torch.exp(-dl2 * mask) * mask,
            "l2_dist": dl2, "normal_angle": ang, "offset_dist": doff, "dn_sum": (dn * mask).sum(-1), "dl2_sum": (dl2 * mask).sum(-1),
            "offset_out": (ntn.abs() < NTN_MARGIN) & (ntn != 0)}


VOTE_MODES = (0, 1, 2, 3)
VOTE_TRAIN = 16


def soft_vote_reference(c, b, maps, mode):
    """ransac.hip ransac_soft_vote_kernel for pair b in f64.  `maps`: rots_all / trans_all / dn_sum / dl2_sum of that pair (what the
    kernel is given).  Returns the six outputs and `select_gap`, the top-two margin of the selection a mode 2 / 3 launch makes."""
    nq, m = c["nq"], c["ms"][b]
    train, mode = bool(mode & VOTE_TRAIN), mode & 15
    d = lambda k: c[k].double()
    init_rot, init_trans = d("init_rot")[b], d("init_trans")[b]
    z = torch.zeros(nq + 1, dtype=F64)
    out = {"score_rot": z.clone(), "score_trans": z.clone(), "select_gap": float("inf")}
    if m == 0 and not train:
        out.update(pred_rot=init_rot, avg_rot=init_rot, pred_trans=init_trans, avg_trans=init_trans)
        return out

    def scores(sf, w, bias):
        s = torch.softmax(sf[b, :m + 1] @ w + bias, 0)
        if train:
            s = s.clamp(0.01, 0.9) * (1.0 if m >= 1 else 0.0)
            s = s / (s.sum() + 1e-10)
        return s
    s_r, s_t = scores(d("sf_rot"), d("reg_rot_w"), d("reg_rot_b")), scores(d("sf_trans"), d("reg_trans_w"), d("reg_trans_b"))
    out["score_rot"][:m + 1], out["score_trans"][:m + 1] = s_r, s_t
    FR, FT, ir, it = d("fused_rot")[b, :m], d("fused_trans")[b, :m], d("init_rot_feat")[b], d("init_trans_feat")[b]
    avg_w = 1.0 / ((m + 1) + 1e-10)
    soft = lambda F0, FF, s: F0 * s[0] + (FF * s[1:, None]).sum(0)
    fr_soft, ft_soft = torch.zeros(256, dtype=F64), torch.zeros(256, dtype=F64)
    if train:
        fr_soft, ft_soft = soft(ir, FR, s_r), soft(it, FT, s_t)
        if m == 0:                                  # 0 / 0: the kernel's (and the reference model's) result for an empty sequence
            fr_avg = ft_avg = torch.full((256,), float("nan"), dtype=F64)
        else:
            fr_avg, ft_avg = FR.sum(0) / m, FT.sum(0) / m
    elif m > 1:
        fr_avg, ft_avg = (ir + FR.sum(0)) * avg_w, (it + FT.sum(0)) * avg_w
        fr_soft, ft_soft = soft(ir, FR, s_r), soft(it, FT, s_t)
    else:
        fr_avg, ft_avg = FR[0], FT[0]
    nrm = lambda v: v / v.norm().clamp_min(1e-12)
    ra, ta = nrm(d("rots_w") @ fr_avg + d("rots_b")), d("trans_w") @ ft_avg + d("trans_b")
    rs, ts = nrm(d("rots_w") @ fr_soft + d("rots_b")), d("trans_w") @ ft_soft + d("trans_b")
    pr, pt = ra, ta
    if train:
        pr, pt = rs, ts
    elif m > 1:
        if mode == 0:
            pr, pt = rs, ts
        elif mode in (2, 3):
            kr, kt = (-maps["dn_sum"][:m + 1].double(), -maps["dl2_sum"][:m + 1].double()) if mode == 2 else (s_r, s_t)
            pr, pt = maps["rots_all"][int(kr.argmax())].double(), maps["trans_all"][int(kt.argmax())].double()
            out["select_gap"] = float(min(top2_gap(kr, 0) / kr.abs().max(), top2_gap(kt, 0) / kt.abs().max()))
    out.update(pred_rot=pr, pred_trans=pt, avg_rot=ra, avg_trans=ta)
    return out


SELECT_MARGIN = 1e-3         # relative top-two gap a mode 2 / 3 selection needs (the scores are held to 2e-4, the row sums to 1e-4)


# ===================================================================================================================== post-selection
SCORE_THR, MASK_THR, OVERLAP_THR = 0.6, 0.5, 0.6


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def postselect_inputs(nq, h, w, n_valid, seed):
    """(logits [nq,2], params [nq,3], prob [nq,h,w] f32 = sigmoid(mask logits), feat [nq,256]) with exactly n_valid queries passing the
    score test (0: the arg-max fallback; -n: n queries that all fail the overlap rule - the max-overlap fallback)."""
    kind = "none_pass" if n_valid == 0 else ("multi" if n_valid > 0 else "all_overlap_rejected")
    logits, params, mask, feat = GI.postselect_case(kind, seed, nq, h, w, n_valid=abs(n_valid) if n_valid else None)
    return logits, params, torch.sigmoid(mask), feat


def postselect_reference(logits, prob, params, feat, H, W, score_thr=SCORE_THR, mask_thr=MASK_THR, overlap_thr=OVERLAP_THR):
    """One image in f64 from the f32 tensors the kernels read -> what ops.postselect_planes returns for it (n_kept, kept_idx, planes, feats,
    scores, areas, centers, winner, flags) plus `margin` [H,W] (per pixel: the smallest of the top-two weighted gap, |p - mask_thr| over
    the valid queries and |best - mask_thr|), `n_valid`, and `overlap_gap` (the smallest |overlap - threshold| of a decision taken).  The
    thresholds are compared as the f32 values the kernels receive."""
    nq, D = logits.shape[0], feat.shape[1]
    score_thr, mask_thr, overlap_thr = _f32(score_thr), _f32(mask_thr), _f32(overlap_thr)
    cls = torch.softmax(logits.double(), -1)
    label = (cls[:, 1] > cls[:, 0]).long()
    score = torch.where(label == 1, cls[:, 1], cls[:, 0])
    valid = (label == 0) & (score > score_thr)
    zero_flag = not bool(valid.any())
    if zero_flag:
        i = int(cls[:, 0].argmax())
        valid[i], score[i] = True, cls[i, 0]
    ori = torch.arange(nq)[valid]
    up = F.interpolate(prob.double()[valid][None], size=(H, W), mode="bilinear", align_corners=False)[0]        # [nv,H,W]
    wgt = score[valid].view(-1, 1, 1) * up
    best, ids = wgt.max(0)
    passed = best > mask_thr
    margin = torch.minimum(top2_gap(wgt, 0), torch.minimum((up - mask_thr).abs().min(0).values, (best - mask_thr).abs()))
    winner = (ori[ids] | torch.where(passed, 0x80, 0)).to(torch.uint8)
    xs, ys = torch.arange(W, dtype=F64).view(1, W), torch.arange(H, dtype=F64).view(H, 1)
    keep, max_ov, max_ov_k, gap = [], 0.0, -1, float("inf")
    area_pass = [int(((ids == k) & passed).sum()) for k in range(len(ori))]
    for k in range(len(ori)):
        area, orig = area_pass[k], int((up[k] >= mask_thr).sum())
        if not zero_flag:
            if area < 1 or orig < 1:
                continue
            ov = area / orig
            gap = min(gap, abs(ov - overlap_thr))
            if ov > max_ov:
                max_ov, max_ov_k = ov, k
            if ov < overlap_thr:
                continue
        keep.append(k)
    fb = not keep
    if fb:
        keep = [max_ov_k if max_ov_k >= 0 else 0]
    n = len(keep)
    out = {"n_kept": n, "kept_idx": torch.full((nq,), -1, dtype=torch.int64), "planes": torch.zeros(nq, 3), "feats": torch.zeros(nq, D),
           "scores": torch.zeros(nq, dtype=F64), "areas": torch.zeros(nq, dtype=torch.int64), "centers": torch.zeros(nq, 2, dtype=F64),
           "flags": int(zero_flag) | (2 if fb else 0), "margin": margin, "n_valid": int(valid.sum()), "overlap_gap": gap}
    for i, k in enumerate(keep):
        msk = (ids == k) if fb else ((ids == k) & passed)
        area = int(msk.sum())
        sx, sy = float((xs * msk).sum()), float((ys * msk).sum())
        if not fb and zero_flag and area == 0:
            area, sx, sy = 1, 0.0, 0.0
            winner[0, 0] = int(ori[k]) | 0x80
        eps = 0.0 if fb else 1e-10
        out["kept_idx"][i], out["areas"][i], out["scores"][i] = ori[k], area, score[valid][k]
        out["centers"][i] = torch.tensor([(sx / W) / (area + eps), (sy / H) / (area + eps)], dtype=F64)
        out["planes"][i], out["feats"][i] = params[ori[k]], feat[ori[k]]
    out["winner"] = winner
    return out


@functools.lru_cache(maxsize=None)
def postselect_case(case):
    """case of PS_GPU_CASES -> (inputs of the two images, their references)."""
    nq, geom, pair = case
    h, w, H, W, _ = PS_GEOMETRIES[geom]
    seed = 4000 + 7 * nq + sum(map(ord, geom)) + 3 * pair[0] + PS_SEEDS.get(case, 0)
    ins = [postselect_inputs(nq, h, w, nv, seed + 1000 * i) for i, nv in enumerate(pair)]
    return ins, [postselect_reference(i[0], i[2], i[1], i[3], H, W) for i in ins]


def postselect_case_ok(case):
    """The input conditions of a post-selection case: the valid counts asked for, at most PS_PIXEL_CAP of the pixels of an image inside the
    decision margin, and no overlap ratio within PS_OVERLAP_MARGIN of the threshold (widened by what the left-out pixels could move)."""
    nq, geom, pair = case
    _, refs = postselect_case(case)
    H, W = PS_GEOMETRIES[geom][2:4]
    for nv, r in zip(pair, refs):
        n_out = int((r["margin"] < PS_MARGIN).sum())
        if r["n_valid"] != max(abs(nv), 1) or r["flags"] != (1 if nv == 0 else (2 if nv < 0 else 0)) or n_out > PS_PIXEL_CAP * H * W:
            return False
        if r["overlap_gap"] < PS_OVERLAP_MARGIN + 0.25 * n_out:
            return False
    return True
