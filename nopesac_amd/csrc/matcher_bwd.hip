// Backward (gradient) kernels of the matching head (reference: matching_net/matching_head.py:43-139, transformer/gnn.py): what
// nopesac_amd/training.py::MatchingHeadTrainer needs beyond the Linear layers' dgrad / wgrad.
//   (1) ragged multi-head attention backward (forward twin: attention_small_kernel, attention.hip) - softmax recomputed from q and k;
//   (2) LayerNorm backward over D = 256 - per-block partials of dgamma / dbeta into a workspace, then a fixed-order reduce;
//   (3) the training twin of matcher_sinkhorn (matcher.hip): the same couplings and log-space Sinkhorn with a dustbin, no assignment,
//       every iteration's potentials (u, v) saved, plus the embedding loss 2 * mean(-min(log_scores, 0)) over the entries gt_corr selects
//       in the whole batch; and its backward - the gradient of the UNROLLED iterations, walked back from the saved potentials.  The
//       trainer's forward launches the inference kernel itself and takes the loss from its scores (emb_loss_pairs_kernel); the twin
//       runs as a replay when the backward pass starts;
//   (4) descriptor dot backward (dots = D0 D1^T / 16 per pair).
// Everything is f32 and deterministic: no atomics, every reduction has a fixed order (wave shuffles, LDS partials summed by index, per-pair
// partials reduced by nopesac_col_sum_f32).  Gated per element against float64 VJPs (tests/matcher_bwd_forms.py, docs/kernels.md) and, as a
// whole head, against float64 torch.autograd on the oracle (tests/test_matcher_training_gpu.py).
#include "common.h"

namespace nps {

constexpr int MB_HD = 32;            // head dimension
constexpr int MB_LS = MB_HD + 1;     // LDS row stride of the attention tiles (odd: a column of rows walks distinct banks)
constexpr float MB_NEG_PAD = -1e30f;

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) attention backward.  One workgroup per (set, head), 256 threads; L, S <= 128.  q (pre-scaled), k, v, dO of the (set, head) are staged
// in LDS once.  Phase 1: threads (2 i, 2 i + 1) own query row i and split the keys by parity - row max, row sum and
// delta_i = sum_j P_ij (dO_i . v_j), then dq_i = scale * sum_j dS_ij k_j with dS_ij = P_ij (dO_i . v_j - delta_i); the two halves meet in
// one shuffle.  (delta_i is formed from the same dO_i . v_j that dS_ij subtracts it from, not as dO_i . O_i: on a peaked row
// dS_ij = P_ij (dp_ij - delta_i) cancels, and the rounding of dO_i . O_i - two sums of 32 products that need not be small where their
// difference is - was up to 1.9 x the sweep's per-element bound on dq; a single live key gives dS = 0 exactly.)  Phase 2: threads (2 j, 2 j + 1) own key j and split the queries by parity: dv_j = sum_i P_ij dO_i, dk_j = sum_i dS_ij
// (scale q_i), P_ij recomputed from the row statistics of phase 1 (same operations in the same order: the same bits).  The sums over
// queries run inside this one workgroup in index order.
__global__ __launch_bounds__(256) void attention_small_bwd_kernel(
    const float* __restrict__ q, long long q_stride, const float* __restrict__ k, long long k_stride, const float* __restrict__ v,
    long long v_stride, const float* __restrict__ dout, long long do_stride, int Lq, int Lk, float scale, const int* __restrict__ qlen,
    const int* __restrict__ klen, float* __restrict__ dq, long long dq_stride, float* __restrict__ dk, long long dk_stride,
    float* __restrict__ dv, long long dv_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.y, h = blockIdx.x, tid = threadIdx.x;
    float* Qs = smem;                         // [Lq][33] scale * q
    float* Ds = Qs + Lq * MB_LS;              // [Lq][33] dO
    float* Ks = Ds + Lq * MB_LS;              // [Lk][33]
    float* Vs = Ks + Lk * MB_LS;              // [Lk][33]
    float* st_m = Vs + Lk * MB_LS;            // [Lq] row max
    float* st_il = st_m + Lq;                 // [Lq] 1 / row sum
    float* st_dl = st_il + Lq;                // [Lq] delta
    const int nq = qlen ? min(max(qlen[b], 0), Lq) : Lq;
    const int nk = klen ? min(max(klen[b], 0), Lk) : Lk;
    for (int e = tid; e < Lq * MB_HD; e += 256) {
        const int i = e >> 5, d = e & 31;
        const bool ok = i < nq;
        const long long r = (long long)b * Lq + (ok ? i : 0);          // clamped address + select
        const float qv = q[r * q_stride + h * MB_HD + d], gv = dout[r * do_stride + h * MB_HD + d];
        Qs[i * MB_LS + d] = ok ? qv * scale : 0.f;
        Ds[i * MB_LS + d] = ok ? gv : 0.f;
    }
    for (int e = tid; e < Lk * MB_HD; e += 256) {
        const int j = e >> 5, d = e & 31;
        const bool ok = j < nk;
        const long long r = (long long)b * Lk + (ok ? j : 0);
        const float kv = k[r * k_stride + h * MB_HD + d], vv = v[r * v_stride + h * MB_HD + d];
        Ks[j * MB_LS + d] = ok ? kv : 0.f;
        Vs[j * MB_LS + d] = ok ? vv : 0.f;
    }
    __syncthreads();
    const int half = tid & 1;
    // ---- phase 1: query rows (two passes of 128 rows would be needed beyond 128 rows; the entry point caps Lq at 128)
    {
        const int i = tid >> 1;
        const bool ok = i < nq && nk > 0;
        const int ic = i < Lq ? i : 0;
        float qr[MB_HD], gr[MB_HD], acc[MB_HD];
#pragma unroll
        for (int d = 0; d < MB_HD; ++d) { qr[d] = Qs[ic * MB_LS + d]; gr[d] = Ds[ic * MB_LS + d]; acc[d] = 0.f; }
        float m = -INFINITY;
        for (int j = half; j < nk; j += 2) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) s = fmaf(qr[d], Ks[j * MB_LS + d], s);
            m = fmaxf(m, s);
        }
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        if (!(m > -INFINITY)) m = 0.f;                   // nk == 0 (or one key and the empty half): keep the arithmetic finite
        float l = 0.f, dsum = 0.f;
        for (int j = half; j < nk; j += 2) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) {
                s = fmaf(qr[d], Ks[j * MB_LS + d], s);
                dp = fmaf(gr[d], Vs[j * MB_LS + d], dp);
            }
            const float p = expf(s - m);
            l += p;
            dsum = fmaf(p, dp, dsum);
        }
        l += __shfl_xor(l, 1, 64);
        const float il = l > 0.f ? 1.f / l : 0.f;
        const float delta = (dsum + __shfl_xor(dsum, 1, 64)) * il;
        for (int j = half; j < nk; j += 2) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) {
                s = fmaf(qr[d], Ks[j * MB_LS + d], s);
                dp = fmaf(gr[d], Vs[j * MB_LS + d], dp);
            }
            const float ds = expf(s - m) * il * (dp - delta);
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) acc[d] = fmaf(ds, Ks[j * MB_LS + d], acc[d]);
        }
        if (i < Lq) {
            if (half == 0) { st_m[i] = m; st_il[i] = il; st_dl[i] = delta; }
            float* out = dq + ((long long)b * Lq + i) * dq_stride + h * MB_HD;
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) {
                const float t = (acc[d] + __shfl_xor(acc[d], 1, 64)) * scale;
                if ((d >> 4) == half) out[d] = ok ? t : 0.f;           // each thread of the pair writes 16 of the 32 values
            }
        } else {
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) (void)__shfl_xor(acc[d], 1, 64);
        }
    }
    __syncthreads();
    // ---- phase 2: keys
    {
        const int j = tid >> 1;
        const bool ok = j < nk;
        const int jc = j < Lk ? j : 0;
        float kr[MB_HD], vr[MB_HD], ak[MB_HD], av[MB_HD];
#pragma unroll
        for (int d = 0; d < MB_HD; ++d) { kr[d] = Ks[jc * MB_LS + d]; vr[d] = Vs[jc * MB_LS + d]; ak[d] = 0.f; av[d] = 0.f; }
        for (int i = half; i < nq; i += 2) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) {
                s = fmaf(Qs[i * MB_LS + d], kr[d], s);
                dp = fmaf(Ds[i * MB_LS + d], vr[d], dp);
            }
            const float p = expf(s - st_m[i]) * st_il[i];
            const float ds = p * (dp - st_dl[i]);
#pragma unroll
            for (int d = 0; d < MB_HD; ++d) {
                av[d] = fmaf(p, Ds[i * MB_LS + d], av[d]);
                ak[d] = fmaf(ds, Qs[i * MB_LS + d], ak[d]);
            }
        }
        float* ok_ = dk + ((long long)b * Lk + jc) * dk_stride + h * MB_HD;
        float* ov_ = dv + ((long long)b * Lk + jc) * dv_stride + h * MB_HD;
#pragma unroll
        for (int d = 0; d < MB_HD; ++d) {
            const float tk = ak[d] + __shfl_xor(ak[d], 1, 64), tv = av[d] + __shfl_xor(av[d], 1, 64);
            if (j < Lk && (d >> 4) == half) { ok_[d] = ok ? tk : 0.f; ov_[d] = ok ? tv : 0.f; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) LayerNorm backward, D = 256: one wave per row (4 columns per lane), a workgroup of 4 waves walks LNB_ROWS rows; the per-lane sums
// of dy * xhat and dy over a wave's rows meet in LDS in wave order and land in ws[block][2][256]; layernorm_bwd_reduce_kernel sums the
// blocks in index order.
constexpr int LNB_ROWS = 32;

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, int rows, float eps, float* __restrict__ dx,
                                                            float* __restrict__ ws) {
    __shared__ float part[4][2][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float gm[4], sg[4], sb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { gm[c] = gamma[lane + 64 * c]; sg[c] = 0.f; sb[c] = 0.f; }
    const int r0 = blockIdx.x * LNB_ROWS;
    for (int rr = w; rr < LNB_ROWS; rr += 4) {
        const int row = r0 + rr;
        if (row >= rows) break;                                 // wave-uniform
        float xv[4], gv[4];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xv[c] = x[(long long)row * 256 + lane + 64 * c];
            gv[c] = dy[(long long)row * 256 + lane + 64 * c];
            s += xv[c];
        }
        const float mean = wave_sum(s) / 256.f;
        float s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { xv[c] -= mean; s2 += xv[c] * xv[c]; }
        const float rstd = 1.f / sqrtf(wave_sum(s2) / 256.f + eps);
        float a = 0.f, bsum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xv[c] *= rstd;                                      // xhat
            sg[c] += gv[c] * xv[c];
            sb[c] += gv[c];
            gv[c] *= gm[c];                                     // d xhat
            a += gv[c];
            bsum += gv[c] * xv[c];
        }
        a = wave_sum(a) / 256.f;
        bsum = wave_sum(bsum) / 256.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) dx[(long long)row * 256 + lane + 64 * c] = rstd * (gv[c] - a - xv[c] * bsum);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { part[w][0][lane + 64 * c] = sg[c]; part[w][1][lane + 64 * c] = sb[c]; }
    __syncthreads();
    for (int e = threadIdx.x; e < 512; e += 256) {
        const int which = e >> 8, col = e & 255;
        ws[(long long)blockIdx.x * 512 + e] = ((part[0][which][col] + part[1][which][col]) + part[2][which][col]) + part[3][which][col];
    }
}

__global__ __launch_bounds__(256) void layernorm_bwd_reduce_kernel(const float* __restrict__ ws, int nblocks, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
    const int e = blockIdx.x * 256 + threadIdx.x;               // 2 blocks: dgamma, dbeta
    float s = 0.f;
    for (int i = 0; i < nblocks; ++i) s += ws[(long long)i * 512 + e];
    if (e < 256) dgamma[e] = s; else dbeta[e - 256] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) Sinkhorn + embedding loss, training twin.  One workgroup per pair; the compacted (n1 + 1) x (n2 + 1) coupling matrix Z (dustbin
// row n1 / column n2) lives in LDS with an odd leading dimension, as in matcher.hip; a group of tg lanes (the largest power of two that
// still gives every row / column a group, if possible) owns a row in the row phase and a column in the column phase.
struct SinkT {
    float *Z, *dZ, *u, *v, *vp, *lmu, *lnu, *du, *dv, *geo, *red;
    int R, LD;
};
__host__ __device__ constexpr size_t sinkt_floats(int nq, bool bwd) {
    return (size_t)(nq + 1) * (((nq + 1) & 1) ? (nq + 1) : (nq + 2)) * (bwd ? 2 : 1) + 7 * (size_t)(nq + 1) + 11 * (size_t)nq + 32;
}
__device__ __forceinline__ SinkT sinkt_lds(float* smem, int nq, bool bwd) {
    SinkT L;
    L.R = nq + 1;
    L.LD = (L.R & 1) ? L.R : L.R + 1;
    const int R = L.R;
    L.Z = smem;
    L.dZ = L.Z + R * L.LD;
    L.u = L.dZ + (bwd ? R * L.LD : 0);
    L.v = L.u + R;
    L.vp = L.v + R;
    L.lmu = L.vp + R;
    L.lnu = L.lmu + R;
    L.du = L.lnu + R;
    L.dv = L.du + R;
    L.geo = L.dv + R;            // 11 nq
    L.red = L.geo + 11 * nq;     // 32
    return L;
}

__device__ __forceinline__ float mb_group_max(float v, int tg) {
    for (int o = tg >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float mb_group_sum(float v, int tg) {
    for (int o = tg >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over the workgroup in a fixed order (wave shuffles, then the waves by index); every thread gets the result
template <int NT>
__device__ __forceinline__ float mb_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

// geometric priors (constants of the backward pass: the reference detaches them, matching_head.py:98-99) + couplings + marginals into
// LDS, the same arithmetic as sink_setup of matcher.hip; ends with a workgroup barrier.  Needs n1 > 0 and n2 > 0.
template <int NT>
__device__ __forceinline__ float sinkt_setup(const SinkT& L, int b, int tid, int nq, int n1, int n2, const float* __restrict__ desc_dot,
                                             const float* __restrict__ planes1, const float* __restrict__ planes2, const float* __restrict__ cam7,
                                             const float* __restrict__ bin_score, float offset_mult, float normal_mult) {
    const int R = L.R, LD = L.LD, R1 = n1 + 1, C1 = n2 + 1;
    float *g1r = L.geo, *g1rt = g1r + 3 * nq, *o1 = g1rt + 3 * nq, *g2 = o1 + nq, *o2 = g2 + 3 * nq;
    const float* cam = cam7 + 7 * b;
    for (int i = tid; i < nq; i += NT) {
        if (i < n1) {
            float Rm[9], qq[4] = {cam[3], cam[4], cam[5], cam[6]}, t[3] = {cam[0], cam[1], cam[2]}, z[3] = {0.f, 0.f, 0.f};
            quat_to_rot(qq, Rm);
            const float* pp = planes1 + ((long long)b * nq + i) * 3;
            float p[3] = {pp[0], pp[1], pp[2]};
            float wr[3], wrt[3], nr[3], nrt[3];
            warp_plane(p, Rm, z, wr);
            warp_plane(p, Rm, t, wrt);
            normalize3(wr, nr);
            normalize3(wrt, nrt);
            for (int d = 0; d < 3; ++d) { g1r[3 * i + d] = nr[d]; g1rt[3 * i + d] = nrt[d]; }
            o1[i] = norm3(wrt);
        }
        if (i < n2) {
            const float* pp = planes2 + ((long long)b * nq + i) * 3;
            float p[3] = {pp[0], -pp[1], -pp[2]};
            float nn[3];
            normalize3(p, nn);
            for (int d = 0; d < 3; ++d) g2[3 * i + d] = nn[d];
            o2[i] = norm3(p);
        }
    }
    __syncthreads();
    const float bin = bin_score[0];
    const float* dd = desc_dot + (long long)b * nq * nq;
    for (int e = tid; e < R1 * C1; e += NT) {
        const int i = e / C1, j = e % C1;
        float val = bin;
        if (i < n1 && j < n2) {
            const float* a = g1r + 3 * i;
            const float* c = g2 + 3 * j;
            const float* at = g1rt + 3 * i;
            const float ntn_r = a[0] * c[0] + a[1] * c[1] + a[2] * c[2];
            const float ang = acosf(fminf(fmaxf(ntn_r, -1.f), 1.f)) / 3.14159265358979323846f * 180.f;
            const float ntn_rt = at[0] * c[0] + at[1] * c[1] + at[2] * c[2];
            float off = ntn_rt < 0.f ? fabsf(o1[i] + o2[j]) : fabsf(o1[i] - o2[j]);
            off = fminf(fmaxf(off, 1e-10f), 5.f);
            val = dd[i * nq + j] - off / offset_mult - ang / normal_mult;
        }
        L.Z[i * LD + j] = val;
    }
    const float norm = -logf((float)(n1 + n2));
    for (int i = tid; i < R; i += NT) {
        L.u[i] = 0.f; L.v[i] = 0.f;
        L.lmu[i] = i < n1 ? norm : logf((float)n2) + norm;
        L.lnu[i] = i < n2 ? norm : logf((float)n1) + norm;
    }
    __syncthreads();
    return norm;
}

struct MbGroups { int tg, ngroups, grp, gl; };
template <int NT>
__device__ __forceinline__ MbGroups mb_groups(int big, int tid) {
    MbGroups G;
    G.tg = 64;
    while (G.tg > 1 && (NT / G.tg) < big) G.tg >>= 1;
    G.ngroups = NT / G.tg; G.grp = tid / G.tg; G.gl = tid % G.tg;
    return G;
}

// padded index (dustbin at nq) of a compact row / column index
__device__ __forceinline__ int mb_pad_index(int i, int n, int nq) { return i < n ? i : nq; }

// forward: log_scores [B, nq+1, nq+1] (padded layout of matcher_sinkhorn), uv [B, iters, 2, nq+1] = (u^t, v^t) of iteration t (compact
// indices), stats [B, 2] = (sum of -min(score, 0) over the pair's selected entries, their count)
template <int NT>
__global__ __launch_bounds__(NT) void sinkhorn_train_fwd_kernel(
    const float* __restrict__ desc_dot, const float* __restrict__ planes1, const float* __restrict__ planes2, const float* __restrict__ cam7,
    const int* __restrict__ n1p, const int* __restrict__ n2p, const float* __restrict__ bin_score, float offset_mult, float normal_mult,
    int iters, const unsigned char* __restrict__ gt_corr, int nq, float* __restrict__ log_scores, float* __restrict__ uv,
    float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const SinkT L = sinkt_lds(smem, nq, false);
    const int R = L.R, LD = L.LD;
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    float* out = log_scores + (long long)b * R * R;
    if (n1 == 0 || n2 == 0) {                     // an empty pair: no live entry, nothing selected
        for (int e = tid; e < R * R; e += NT) out[e] = MB_NEG_PAD;
        if (tid == 0) { stats[2 * b] = 0.f; stats[2 * b + 1] = 0.f; }
        return;
    }
    const int R1 = n1 + 1, C1 = n2 + 1;
    const float norm = sinkt_setup<NT>(L, b, tid, nq, n1, n2, desc_dot, planes1, planes2, cam7, bin_score, offset_mult, normal_mult);
    float *Z = L.Z, *u = L.u, *v = L.v;
    const MbGroups G = mb_groups<NT>(max(R1, C1), tid);
    const int tg = G.tg, ngroups = G.ngroups, grp = G.grp, gl = G.gl;
    float* uvb = uv + (long long)b * iters * 2 * R;
    for (int it = 0; it < iters; ++it) {
        for (int i = grp; i < ((R1 + ngroups - 1) / ngroups) * ngroups; i += ngroups) {
            const bool ok = i < R1;
            float m = -INFINITY;
            if (ok) for (int j = gl; j < C1; j += tg) m = fmaxf(m, Z[i * LD + j] + v[j]);
            m = mb_group_max(m, tg);
            float s = 0.f;
            if (ok) for (int j = gl; j < C1; j += tg) s += expf(Z[i * LD + j] + v[j] - m);
            s = mb_group_sum(s, tg);
            if (ok && gl == 0) { const float t = L.lmu[i] - (m + logf(s)); u[i] = t; uvb[((long long)it * 2) * R + i] = t; }
        }
        __syncthreads();
        for (int j = grp; j < ((C1 + ngroups - 1) / ngroups) * ngroups; j += ngroups) {
            const bool ok = j < C1;
            float m = -INFINITY;
            if (ok) for (int i = gl; i < R1; i += tg) m = fmaxf(m, Z[i * LD + j] + u[i]);
            m = mb_group_max(m, tg);
            float s = 0.f;
            if (ok) for (int i = gl; i < R1; i += tg) s += expf(Z[i * LD + j] + u[i] - m);
            s = mb_group_sum(s, tg);
            if (ok && gl == 0) { const float t = L.lnu[j] - (m + logf(s)); v[j] = t; uvb[((long long)it * 2 + 1) * R + j] = t; }
        }
        __syncthreads();
    }
    const unsigned char* gt = gt_corr + (long long)b * R * R;
    float lsum = 0.f, lcnt = 0.f;
    for (int e = tid; e < R1 * C1; e += NT) {
        const int i = e / C1, j = e % C1;
        const float sc = Z[i * LD + j] + u[i] + v[j] - norm;
        Z[i * LD + j] = sc;
        if (gt[mb_pad_index(i, n1, nq) * R + mb_pad_index(j, n2, nq)]) { lsum += -fminf(sc, 0.f); lcnt += 1.f; }
    }
    lsum = mb_block_sum<NT>(lsum, L.red);
    lcnt = mb_block_sum<NT>(lcnt, L.red);             // (its first barrier also orders the Z writes above before the reads below)
    if (tid == 0) { stats[2 * b] = lsum; stats[2 * b + 1] = lcnt; }
    for (int e = tid; e < R * R; e += NT) {
        const int i = e / R, j = e % R;
        const int si = i < n1 ? i : (i == nq ? n1 : -1), sj = j < n2 ? j : (j == nq ? n2 : -1);
        out[e] = (si >= 0 && sj >= 0) ? Z[si * LD + sj] : MB_NEG_PAD;
    }
}

// loss[0] = 2 * sum / count over the whole batch (0 if nothing is selected), loss[1] = count; the pairs in index order
__global__ void emb_loss_finalize_kernel(const float* __restrict__ stats, int B, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.f, c = 0.f;
    for (int b = 0; b < B; ++b) { s += stats[2 * b]; c += stats[2 * b + 1]; }
    loss[0] = c > 0.f ? 2.f * s / c : 0.f;
    loss[1] = c;
}

// the embedding loss alone, on log scores in the padded layout (the inference kernel's output): per pair (sum of -min(score, 0) over the
// selected live entries, their count); emb_loss_finalize_kernel then forms the batch mean.  One workgroup of 256 threads per pair.
__global__ __launch_bounds__(256) void emb_loss_pairs_kernel(const float* __restrict__ log_scores, const unsigned char* __restrict__ gt_corr,
                                                             const int* __restrict__ n1p, const int* __restrict__ n2p, int nq,
                                                             float* __restrict__ stats) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, R = nq + 1;
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    const int R1 = n1 + 1, C1 = n2 + 1;
    const float* ls = log_scores + (long long)b * R * R;
    const unsigned char* gt = gt_corr + (long long)b * R * R;
    float lsum = 0.f, lcnt = 0.f;
    if (n1 > 0 && n2 > 0)
        for (int e = tid; e < R1 * C1; e += 256) {
            const int o = mb_pad_index(e / C1, n1, nq) * R + mb_pad_index(e % C1, n2, nq);
            if (gt[o]) { lsum += -fminf(ls[o], 0.f); lcnt += 1.f; }
        }
    lsum = mb_block_sum<256>(lsum, red);
    lcnt = mb_block_sum<256>(lcnt, red);
    if (tid == 0) { stats[2 * b] = lsum; stats[2 * b + 1] = lcnt; }
}

// backward of the unrolled iterations.  With out = Z + u^T + v^T - norm and d out_ij = -2 g / count on the selected entries with
// out_ij <= 0 (torch's clamp passes the gradient at the bound): dZ = d out, du = row sums, dv = column sums; then for t = T .. 1
//   v^t_j = lnu_j - LSE_i(Z_ij + u^t_i):     W_ij = exp(Z_ij + u^t_i + v^t_j - lnu_j)      dZ_ij -= dv_j W_ij,  du_i -= sum_j dv_j W_ij
//   u^t_i = lmu_i - LSE_j(Z_ij + v^(t-1)_j): P_ij = exp(Z_ij + v^(t-1)_j + u^t_i - lmu_i)  dZ_ij -= du_i P_ij,  dv_j  = -sum_i du_i P_ij
// (one exp pass per half-iteration: the softmax weights follow from the saved potentials).  Z and dZ stay in LDS; the next iteration's
// potentials are fetched into registers while the current one runs.
template <int NT>
__global__ __launch_bounds__(NT) void sinkhorn_train_bwd_kernel(
    const float* __restrict__ desc_dot, const float* __restrict__ planes1, const float* __restrict__ planes2, const float* __restrict__ cam7,
    const int* __restrict__ n1p, const int* __restrict__ n2p, const float* __restrict__ bin_score, float offset_mult, float normal_mult,
    int iters, const unsigned char* __restrict__ gt_corr, const float* __restrict__ uv, const float* __restrict__ loss,
    const float* __restrict__ g_loss, int nq, float* __restrict__ d_desc_dot, float* __restrict__ d_bin) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const SinkT L = sinkt_lds(smem, nq, true);
    const int R = L.R, LD = L.LD;
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    float* gd = d_desc_dot + (long long)b * nq * nq;
    const float count = loss[1];
    if (n1 == 0 || n2 == 0 || !(count > 0.f)) {
        for (int e = tid; e < nq * nq; e += NT) gd[e] = 0.f;
        if (tid == 0) d_bin[b] = 0.f;
        return;
    }
    const int R1 = n1 + 1, C1 = n2 + 1;
    const float norm = sinkt_setup<NT>(L, b, tid, nq, n1, n2, desc_dot, planes1, planes2, cam7, bin_score, offset_mult, normal_mult);
    float *Z = L.Z, *dZ = L.dZ, *u = L.u, *v = L.v, *vp = L.vp, *du = L.du, *dv = L.dv;
    const float* uvb = uv + (long long)b * iters * 2 * R;
    // u^T, v^T (u = v = 0 from the setup when iters == 0)
    if (iters > 0)
        for (int i = tid; i < R; i += NT) {
            const bool ri = i < R1, ci = i < C1;
            const float a = uvb[((long long)(iters - 1) * 2) * R + (ri ? i : 0)], c = uvb[((long long)(iters - 1) * 2 + 1) * R + (ci ? i : 0)];
            u[i] = ri ? a : 0.f;
            v[i] = ci ? c : 0.f;
        }
    __syncthreads();
    const float coef = -2.f * g_loss[0] / count;
    const unsigned char* gt = gt_corr + (long long)b * R * R;
    for (int e = tid; e < R1 * C1; e += NT) {
        const int i = e / C1, j = e % C1;
        const float sc = Z[i * LD + j] + u[i] + v[j] - norm;
        const bool sel = gt[mb_pad_index(i, n1, nq) * R + mb_pad_index(j, n2, nq)] != 0;
        dZ[i * LD + j] = (sel && sc <= 0.f) ? coef : 0.f;
    }
    __syncthreads();
    const MbGroups G = mb_groups<NT>(max(R1, C1), tid);
    const int tg = G.tg, ngroups = G.ngroups, grp = G.grp, gl = G.gl;
    for (int i = grp; i < ((R1 + ngroups - 1) / ngroups) * ngroups; i += ngroups) {
        const bool ok = i < R1;
        float s = 0.f;
        if (ok) for (int j = gl; j < C1; j += tg) s += dZ[i * LD + j];
        s = mb_group_sum(s, tg);
        if (ok && gl == 0) du[i] = s;
    }
    for (int j = grp; j < ((C1 + ngroups - 1) / ngroups) * ngroups; j += ngroups) {
        const bool ok = j < C1;
        float s = 0.f;
        if (ok) for (int i = gl; i < R1; i += tg) s += dZ[i * LD + j];
        s = mb_group_sum(s, tg);
        if (ok && gl == 0) dv[j] = s;
    }
    // registers of thread i < R: u^t_i and v^(t-1)_i of the iteration about to be walked back (NT >= R)
    const bool mine_r = tid < R1, mine_c = tid < C1;
    float nu = 0.f, nvp = 0.f;
    if (iters > 0) {
        const float a = uvb[((long long)(iters - 1) * 2) * R + (mine_r ? tid : 0)];
        nu = mine_r ? a : 0.f;
        if (iters > 1) {
            const float c = uvb[((long long)(iters - 2) * 2 + 1) * R + (mine_c ? tid : 0)];
            nvp = mine_c ? c : 0.f;
        }
    }
    __syncthreads();
    for (int t = iters; t >= 1; --t) {
        // LDS: v = v^t.  Publish u^t and v^(t-1), then start fetching u^(t-1) and v^(t-2)
        if (tid < R) { u[tid] = nu; vp[tid] = nvp; }
        if (t > 1) {
            const float a = uvb[((long long)(t - 2) * 2) * R + (mine_r ? tid : 0)];
            nu = mine_r ? a : 0.f;
            const int tv = t > 2 ? t - 3 : 0;
            const float c = uvb[((long long)tv * 2 + 1) * R + (mine_c ? tid : 0)];
            nvp = (mine_c && t > 2) ? c : 0.f;
        }
        __syncthreads();
        const bool last = t == iters;            // du of u^T starts from the row sums of d out; every earlier u^t from 0
        for (int i = grp; i < ((R1 + ngroups - 1) / ngroups) * ngroups; i += ngroups) {
            const bool ok = i < R1;
            float acc = 0.f;
            if (ok) {
                const float ui = u[i];
                for (int j = gl; j < C1; j += tg) {
                    const float w = expf(Z[i * LD + j] + ui + v[j] - L.lnu[j]) * dv[j];
                    dZ[i * LD + j] -= w;
                    acc += w;
                }
            }
            acc = mb_group_sum(acc, tg);
            if (ok && gl == 0) du[i] = (last ? du[i] : 0.f) - acc;
        }
        __syncthreads();
        for (int j = grp; j < ((C1 + ngroups - 1) / ngroups) * ngroups; j += ngroups) {
            const bool ok = j < C1;
            float acc = 0.f;
            if (ok) {
                const float vj = vp[j];
                for (int i = gl; i < R1; i += tg) {
                    const float p = expf(Z[i * LD + j] + vj + u[i] - L.lmu[i]) * du[i];
                    dZ[i * LD + j] -= p;
                    acc += p;
                }
            }
            acc = mb_group_sum(acc, tg);
            if (ok && gl == 0) dv[j] = -acc;
        }
        __syncthreads();
        float* sw = v; v = vp; vp = sw;
    }
    for (int e = tid; e < nq * nq; e += NT) {
        const int i = e / nq, j = e % nq;
        const bool live = i < n1 && j < n2;
        const float g = dZ[(live ? i : 0) * LD + (live ? j : 0)];
        gd[e] = live ? g : 0.f;
    }
    float sb = 0.f;                               // bin_score fills the dustbin row and column
    for (int e = tid; e < R1 + C1 - 1; e += NT) sb += e < C1 ? dZ[n1 * LD + e] : dZ[(e - C1) * LD + n2];
    sb = mb_block_sum<NT>(sb, L.red);
    if (tid == 0) d_bin[b] = sb;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (4) dots[b] = D0[b] D1[b]^T / 16  ->  dD0[b,i,:] = sum_j G[b,i,j] D1[b,j,:] / 16, dD1[b,j,:] = sum_i G[b,i,j] D0[b,i,:] / 16 over the
// live block (G is zero outside it); rows >= n are written as zeros.  One workgroup per output row, one thread per column (D = 256).
__global__ __launch_bounds__(256) void desc_dot_bwd_kernel(const float* __restrict__ g, const float* __restrict__ d0, const float* __restrict__ d1,
                                                           const int* __restrict__ n1p, const int* __restrict__ n2p, int nq,
                                                           float* __restrict__ dd0, float* __restrict__ dd1) {
    const int r = blockIdx.x, b = blockIdx.y, side = blockIdx.z, c = threadIdx.x;
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    const float* gb = g + (long long)b * nq * nq;
    float acc = 0.f;
    if (side == 0) {
        if (r < n1) for (int j = 0; j < n2; ++j) acc = fmaf(gb[r * nq + j], d1[((long long)b * nq + j) * 256 + c], acc);
        dd0[((long long)b * nq + r) * 256 + c] = acc * 0.0625f;
    } else {
        if (r < n2) for (int i = 0; i < n1; ++i) acc = fmaf(gb[i * nq + r], d0[((long long)b * nq + i) * 256 + c], acc);
        dd1[((long long)b * nq + r) * 256 + c] = acc * 0.0625f;
    }
}

}  // namespace nps

extern "C" int nopesac_attention_small_backward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                                                int64_t v_stride, const float* d_out, int64_t do_stride, int B, int Lq, int Lk, int heads,
                                                float scale, const int32_t* qlen, const int32_t* klen, float* dq, int64_t dq_stride,
                                                float* dk, int64_t dk_stride, float* dv, int64_t dv_stride, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(q && k && v && d_out, "attention_small_backward: null input");
    NPS_CHECK_ARG(dq && dk && dv, "attention_small_backward: null output");
    NPS_CHECK_ARG(B > 0 && heads > 0 && Lq > 0 && Lk > 0 && Lq <= 128 && Lk <= 128, "attention_small_backward: bad dims (Lq=%d, Lk=%d; 1..128)",
                  Lq, Lk);
    const long long width = (long long)heads * MB_HD;
    NPS_CHECK_ARG(q_stride >= width && k_stride >= width && v_stride >= width && do_stride >= width && dq_stride >= width && dk_stride >= width &&
                      dv_stride >= width,
                  "attention_small_backward: heads * 32 = %lld is wider than a row stride", width);
    const size_t lds = sizeof(float) * ((size_t)2 * (Lq + Lk) * MB_LS + 3 * (size_t)Lq);
    if (lds > 64 * 1024) NPS_ENSURE_LDS(160 * 1024 - 256, attention_small_bwd_kernel);
    hipLaunchKernelGGL(attention_small_bwd_kernel, dim3(heads, B), dim3(256), lds, (hipStream_t)stream, q, (long long)q_stride, k,
                       (long long)k_stride, v, (long long)v_stride, d_out, (long long)do_stride, Lq, Lk, scale, qlen, klen, dq,
                       (long long)dq_stride, dk, (long long)dk_stride, dv, (long long)dv_stride);
    NPS_LAUNCH_RET();
}

extern "C" int64_t nopesac_layernorm_backward_workspace_floats(int rows) {
    return rows > 0 ? (int64_t)((rows + nps::LNB_ROWS - 1) / nps::LNB_ROWS) * 512 : 0;
}

extern "C" int nopesac_layernorm_backward(const float* x, const float* gamma, const float* dy, int rows, int D, float eps, float* dx,
                                          float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && gamma && dy, "layernorm_backward: null input");
    NPS_CHECK_ARG(dx && dgamma && dbeta && ws, "layernorm_backward: null output");
    NPS_CHECK_ARG(rows > 0 && D == 256, "layernorm_backward: bad dims (rows=%d, D=%d; D must be 256)", rows, D);
    NPS_CHECK_ARG(ws_floats >= nopesac_layernorm_backward_workspace_floats(rows), "layernorm_backward: workspace too small");
    const int nblocks = (rows + LNB_ROWS - 1) / LNB_ROWS;
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, x, gamma, dy, rows, eps, dx, ws);
    hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3(2), dim3(256), 0, (hipStream_t)stream, ws, nblocks, dgamma, dbeta);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_matcher_sinkhorn_train(const float* desc_dot, const float* planes1, const float* planes2, const float* cam7,
                                              const int32_t* n1, const int32_t* n2, const float* bin_score, float offset_mult,
                                              float normal_mult, int iters, const uint8_t* gt_corr, int B, int nq, float* log_scores,
                                              float* uv, float* pair_stats, float* loss, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(desc_dot && planes1 && planes2 && cam7 && n1 && n2 && bin_score && gt_corr, "sinkhorn_train: null input");
    NPS_CHECK_ARG(log_scores && pair_stats && loss && (uv || iters == 0), "sinkhorn_train: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= 128 && iters >= 0, "sinkhorn_train: bad dims (B=%d, nq=%d in 1..128, iters=%d >= 0)", B, nq, iters);
    const size_t lds = sizeof(float) * sinkt_floats(nq, false);
#define NPS_SINKT_FWD(NT_)                                                                                                               \
    do {                                                                                                                                 \
        if (lds > 64 * 1024) NPS_ENSURE_LDS(160 * 1024 - 256, sinkhorn_train_fwd_kernel<NT_>);                                           \
        hipLaunchKernelGGL(sinkhorn_train_fwd_kernel<NT_>, dim3(B), dim3(NT_), lds, (hipStream_t)stream, desc_dot, planes1, planes2, cam7, \
                           n1, n2, bin_score, offset_mult, normal_mult, iters, gt_corr, nq, log_scores, uv, pair_stats);                  \
    } while (0)
    if (nq + 1 <= 64) NPS_SINKT_FWD(256); else NPS_SINKT_FWD(1024);
#undef NPS_SINKT_FWD
    hipLaunchKernelGGL(emb_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pair_stats, B, loss);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_matcher_emb_loss(const float* log_scores, const uint8_t* gt_corr, const int32_t* n1, const int32_t* n2, int B, int nq,
                                       float* pair_stats, float* loss, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(log_scores && gt_corr && n1 && n2, "emb_loss: null input");
    NPS_CHECK_ARG(pair_stats && loss, "emb_loss: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= 128, "emb_loss: bad dims (B=%d, nq=%d in 1..128)", B, nq);
    hipLaunchKernelGGL(emb_loss_pairs_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, log_scores, gt_corr, n1, n2, nq, pair_stats);
    hipLaunchKernelGGL(emb_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pair_stats, B, loss);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_matcher_sinkhorn_train_backward(const float* desc_dot, const float* planes1, const float* planes2, const float* cam7,
                                                       const int32_t* n1, const int32_t* n2, const float* bin_score, float offset_mult,
                                                       float normal_mult, int iters, const uint8_t* gt_corr, const float* uv,
                                                       const float* loss, const float* g_loss, int B, int nq, float* d_desc_dot,
                                                       float* d_bin_pairs, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(desc_dot && planes1 && planes2 && cam7 && n1 && n2 && bin_score && gt_corr && loss && g_loss && (uv || iters == 0),
                  "sinkhorn_train_backward: null input");
    NPS_CHECK_ARG(d_desc_dot && d_bin_pairs, "sinkhorn_train_backward: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= 128 && iters >= 0, "sinkhorn_train_backward: bad dims (B=%d, nq=%d in 1..128, iters=%d >= 0)", B, nq,
                  iters);
    const size_t lds = sizeof(float) * sinkt_floats(nq, true);
#define NPS_SINKT_BWD(NT_)                                                                                                               \
    do {                                                                                                                                 \
        if (lds > 64 * 1024) NPS_ENSURE_LDS(160 * 1024 - 256, sinkhorn_train_bwd_kernel<NT_>);                                           \
        hipLaunchKernelGGL(sinkhorn_train_bwd_kernel<NT_>, dim3(B), dim3(NT_), lds, (hipStream_t)stream, desc_dot, planes1, planes2, cam7, \
                           n1, n2, bin_score, offset_mult, normal_mult, iters, gt_corr, uv, loss, g_loss, nq, d_desc_dot, d_bin_pairs);   \
    } while (0)
    if (nq + 1 <= 64) NPS_SINKT_BWD(256); else NPS_SINKT_BWD(1024);
#undef NPS_SINKT_BWD
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_desc_dot_backward(const float* d_desc_dot, const float* d0, const float* d1, const int32_t* n1, const int32_t* n2, int B,
                                         int nq, int D, float* dd0, float* dd1, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(d_desc_dot && d0 && d1 && n1 && n2, "desc_dot_backward: null input");
    NPS_CHECK_ARG(dd0 && dd1, "desc_dot_backward: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= 128 && D == 256, "desc_dot_backward: bad dims (B=%d, nq=%d in 1..128, D=%d must be 256)", B, nq, D);
    hipLaunchKernelGGL(desc_dot_bwd_kernel, dim3(nq, B, 2), dim3(256), 0, (hipStream_t)stream, d_desc_dot, d0, d1, n1, n2, nq, dd0, dd1);
    NPS_LAUNCH_RET();
}
