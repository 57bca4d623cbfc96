// Training kernels of the plane head's transformer decoder (reference: transformer/transformer.py:214-322 under dropout = 0.1,
// planeTR_head.py:88): what nopesac_amd/training.py::PlaneDecoderTrainer needs beyond the Linear / LayerNorm kernels it shares with the
// other trainers.
//   (1) multi-head attention forward with dropout on the probabilities, for ANY Lq / Lk: keys come through LDS in tiles of DT_TK, each
//       thread keeps an online softmax (running max, sum, weighted accumulator) over the keys it owns;
//   (2) its backward in three kernels - row statistics (max, 1 / sum, D_i = sum_j P_ij dP_ij), dq per query tile, dk / dv per key tile -
//       that recompute the probabilities from q and k, so nothing a forward kernel saved is read (the p = 0 forward of the trainer is the
//       inference head's own launch, attention_small_kernel);
//   (3) element-wise dropout with an optional residual (its own backward without one) and the materialised keep mask.
// The keep decision is counter based (dropout.h): a pure function of (seed, site, logical element index), recomputed wherever it is
// needed.  Thread layout of every attention kernel here: 256 threads = 64 rows (lane) x 4 splits (wave).  The row of a thread lives in
// registers, the other side's tile in LDS, where the row a wave reads is wave-uniform (an LDS broadcast: no bank conflicts); the four
// splits meet through LDS and are summed in split order.  Everything is f32 scalar FMA and deterministic: no atomics, every reduction has a
// fixed order.  The score s_ij = sum_d (scale q_id) k_jd is formed by the same fmaf chain in all four kernels: the same bits everywhere.
// Every load comes from a clamped address with a select behind it; every store stays inside rows < Lq (Lk), columns < heads * 32.
// Gated per element against float64 (tests/plane_decoder_forms.py, docs/kernels.md).
#include <algorithm>

#include "common.h"
#include "dropout.h"

namespace nps {

constexpr int DT_HD = 32;                  // head dimension
constexpr int DT_LS = DT_HD + 1;           // LDS row stride of a tile (odd: the staging stores walk distinct banks)
constexpr int DT_TQ = NPS_ATT_TRAIN_TQ;    // query rows per workgroup (= lanes)
constexpr int DT_TK = NPS_ATT_TRAIN_TK;    // keys per LDS tile
constexpr int DT_SPLITS = 4;               // waves: each owns the keys (queries) j = split, split + 4, ... of a tile
constexpr int DT_PER = DT_TK / DT_SPLITS;  // keys of a tile per thread
static_assert(DT_TQ == 64 && DT_TK == DT_TQ && DT_TK % DT_SPLITS == 0, "a lane per row, one tile shape for both sides");
static_assert(NPS_ATT_TRAIN_WS_ROW_FLOATS == 3, "the statistics workspace holds (m, 1 / l, D) per (set, head, row)");

struct DropSite {
    uint64_t key;          // dropout_key(seed, stream)
    uint32_t threshold;    // floor(p 2^32); 0 = no dropout (the hash is skipped)
    float inv_keep;        // (float)(1 / (1 - p))
};

__device__ __forceinline__ bool dt_keep(const DropSite& ds, long long index) {
    return ds.threshold == 0u || dropout_keep_keyed(ds.key, index, ds.threshold);
}

__device__ __forceinline__ float dt_dot(const float (&a)[DT_HD], const float* __restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DT_HD; ++d) s = fmaf(a[d], row[d], s);
    return s;
}

// K and V rows kt .. kt + DT_TK of set b, head h -> LDS, zero beyond nk (clamped address + select).
__device__ __forceinline__ void dt_stage_pair(const float* __restrict__ a, long long a_stride, const float* __restrict__ c, long long c_stride,
                                              long long row0, int t0, int n, int h, float a_mul, float* __restrict__ As, float* __restrict__ Cs) {
    for (int e = threadIdx.x; e < DT_TK * DT_HD; e += 256) {
        const int j = e >> 5, d = e & 31;
        const bool ok = t0 + j < n;
        const long long r = row0 + (ok ? t0 + j : 0);
        const float av = a[r * a_stride + h * DT_HD + d], cv = c[r * c_stride + h * DT_HD + d];
        As[j * DT_LS + d] = ok ? av * a_mul : 0.f;
        Cs[j * DT_LS + d] = ok ? cv : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) + (2a).  STATS = false: the forward, o = (keep o softmax(s)) v / (1 - p).  STATS = true: the backward's statistics pass,
// ws[(b, h, i)] = (row max m_i, 1 / l_i, D_i) with D_i = sum_j P_ij dP_ij, dP_ij = keep_ij (dO_i . v_j) / (1 - p).
// Online softmax per thread over its keys, tile by tile: the tile's scores are held in registers, the running (m, l, accumulator) are
// rescaled once per tile; at the end the four splits are brought to the common max.
template <bool STATS>
__global__ __launch_bounds__(256) void attention_train_rows_kernel(
    const float* __restrict__ q, long long q_stride, const float* __restrict__ k, long long k_stride, const float* __restrict__ v,
    long long v_stride, const float* __restrict__ dout, long long do_stride, float* __restrict__ o, long long o_stride, float* __restrict__ ws,
    int Lq, int Lk, int heads, float scale, const int* __restrict__ qlen, const int* __restrict__ klen, DropSite site) {
    __shared__ float Ks[DT_TK * DT_LS];
    __shared__ float Vs[DT_TK * DT_LS];
    __shared__ float sh_m[DT_SPLITS][DT_TQ];
    __shared__ float sh_l[DT_SPLITS][DT_TQ];
    __shared__ float sh_a[STATS ? DT_SPLITS * DT_TQ : DT_SPLITS * DT_HD * (DT_TQ + 1)];      // STATS: [split][row] D sums; else [split][d][row + pad]
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int split = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * DT_TQ + lane;
    const int nq = qlen ? min(max(qlen[b], 0), Lq) : Lq;
    const int nk = klen ? min(max(klen[b], 0), Lk) : Lk;
    const bool row_ok = row < nq;
    const long long qrow = (long long)b * Lq + (row_ok ? row : 0);
    float qr[DT_HD], gr[STATS ? DT_HD : 1], acc[STATS ? 1 : DT_HD];
#pragma unroll
    for (int d = 0; d < DT_HD; ++d) qr[d] = q[qrow * q_stride + h * DT_HD + d] * scale;
    if constexpr (STATS) {
#pragma unroll
        for (int d = 0; d < DT_HD; ++d) {
            const float g = dout[qrow * do_stride + h * DT_HD + d];
            gr[d] = row_ok ? g : 0.f;
        }
        acc[0] = 0.f;
    } else {
#pragma unroll
        for (int d = 0; d < DT_HD; ++d) acc[d] = 0.f;
    }
    const long long idx0 = (((long long)b * heads + h) * Lq + (row_ok ? row : 0)) * Lk;       // index of P[b, h, row, 0] in [B, heads, Lq, Lk]
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < nk; kt += DT_TK) {
        __syncthreads();                                   // the previous tile has been consumed
        dt_stage_pair(k, k_stride, v, v_stride, (long long)b * Lk, kt, nk, h, 1.f, Ks, Vs);
        __syncthreads();
        float s[DT_PER];
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < DT_PER; ++t) {
            const int j = split + DT_SPLITS * t;
            const float sv = dt_dot(qr, Ks + j * DT_LS);
            s[t] = kt + j < nk ? sv : -INFINITY;
            tmax = fmaxf(tmax, s[t]);
        }
        const float m_new = fmaxf(m, tmax);
        if (m_new > -INFINITY) {                           // (a thread without a live key so far keeps m = -inf, l = 0)
            const float corr = expf(m - m_new);            // m = -inf: 0
            l *= corr;
            if constexpr (STATS) acc[0] *= corr;
            else {
#pragma unroll
                for (int d = 0; d < DT_HD; ++d) acc[d] *= corr;
            }
#pragma unroll
            for (int t = 0; t < DT_PER; ++t) {
                const int j = split + DT_SPLITS * t;
                if (kt + j < nk) {                         // wave-uniform
                    const float pj = expf(s[t] - m_new);
                    l += pj;
                    const bool keep = dt_keep(site, idx0 + kt + j);
                    if constexpr (STATS) {
                        const float dp = dt_dot(gr, Vs + j * DT_LS);
                        const float dpm = keep ? dp * site.inv_keep : 0.f;
                        acc[0] = fmaf(pj, dpm, acc[0]);
                    } else {
                        const float w = keep ? pj : 0.f;
#pragma unroll
                        for (int d = 0; d < DT_HD; ++d) acc[d] = fmaf(w, Vs[j * DT_LS + d], acc[d]);
                    }
                }
            }
            m = m_new;
        }
    }
    sh_m[split][lane] = m;
    sh_l[split][lane] = l;
    if constexpr (STATS) sh_a[split * DT_TQ + lane] = acc[0];
    else {
#pragma unroll
        for (int d = 0; d < DT_HD; ++d) sh_a[(split * DT_HD + d) * (DT_TQ + 1) + lane] = acc[d];
    }
    __syncthreads();
    float M = -INFINITY;
#pragma unroll
    for (int sp = 0; sp < DT_SPLITS; ++sp) M = fmaxf(M, sh_m[sp][lane]);
    float wgt[DT_SPLITS], L = 0.f;
#pragma unroll
    for (int sp = 0; sp < DT_SPLITS; ++sp) {
        wgt[sp] = sh_m[sp][lane] > -INFINITY ? expf(sh_m[sp][lane] - M) : 0.f;
        L = fmaf(sh_l[sp][lane], wgt[sp], L);
    }
    const bool live = row_ok && nk > 0;
    if constexpr (STATS) {
        if (split == 0 && row < Lq) {
            float ds = 0.f;
#pragma unroll
            for (int sp = 0; sp < DT_SPLITS; ++sp) ds = fmaf(sh_a[sp * DT_TQ + lane], wgt[sp], ds);
            const float il = L > 0.f ? 1.f / L : 0.f;
            float* st = ws + (((long long)b * heads + h) * Lq + row) * 3;
            st[0] = live ? M : 0.f;
            st[1] = live ? il : 0.f;
            st[2] = live ? ds * il : 0.f;
        }
    } else {
        if (row < Lq) {
            float* op = o + ((long long)b * Lq + row) * o_stride + h * DT_HD;
            const float f = L > 0.f ? site.inv_keep / L : 0.f;
#pragma unroll
            for (int dd = 0; dd < DT_HD / DT_SPLITS; ++dd) {
                const int d = split * (DT_HD / DT_SPLITS) + dd;
                float t = 0.f;
#pragma unroll
                for (int sp = 0; sp < DT_SPLITS; ++sp) t = fmaf(sh_a[(sp * DT_HD + d) * (DT_TQ + 1) + lane], wgt[sp], t);
                op[d] = live ? t * f : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2b) dq_i = scale sum_j dS_ij k_j, dS_ij = P_ij (dP_ij - D_i), P_ij = exp(s_ij - m_i) / l_i from the statistics.  One workgroup per
// (set, head, query tile); the key tiles pass through LDS.
__global__ __launch_bounds__(256) void attention_train_dq_kernel(
    const float* __restrict__ q, long long q_stride, const float* __restrict__ k, long long k_stride, const float* __restrict__ v,
    long long v_stride, const float* __restrict__ dout, long long do_stride, const float* __restrict__ ws, float* __restrict__ dq,
    long long dq_stride, int Lq, int Lk, int heads, float scale, const int* __restrict__ qlen, const int* __restrict__ klen, DropSite site) {
    __shared__ float Ks[DT_TK * DT_LS];
    __shared__ float Vs[DT_TK * DT_LS];
    __shared__ float sh_a[DT_SPLITS * DT_HD * (DT_TQ + 1)];
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int split = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * DT_TQ + lane;
    const int nq = qlen ? min(max(qlen[b], 0), Lq) : Lq;
    const int nk = klen ? min(max(klen[b], 0), Lk) : Lk;
    const bool row_ok = row < nq;
    const int rc = row_ok ? row : 0;
    const long long qrow = (long long)b * Lq + rc;
    float qr[DT_HD], gr[DT_HD], acc[DT_HD];
#pragma unroll
    for (int d = 0; d < DT_HD; ++d) {
        qr[d] = q[qrow * q_stride + h * DT_HD + d] * scale;
        const float g = dout[qrow * do_stride + h * DT_HD + d];
        gr[d] = row_ok ? g : 0.f;
        acc[d] = 0.f;
    }
    const float* st = ws + (((long long)b * heads + h) * Lq + rc) * 3;
    const float m = st[0], il = st[1], delta = st[2];
    const long long idx0 = (((long long)b * heads + h) * Lq + rc) * Lk;
    for (int kt = 0; kt < nk; kt += DT_TK) {
        __syncthreads();
        dt_stage_pair(k, k_stride, v, v_stride, (long long)b * Lk, kt, nk, h, 1.f, Ks, Vs);
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < DT_PER; ++t) {
            const int j = split + DT_SPLITS * t;
            if (kt + j < nk) {                             // wave-uniform
                const float s = dt_dot(qr, Ks + j * DT_LS);
                const float dp = dt_dot(gr, Vs + j * DT_LS);
                const float dpm = dt_keep(site, idx0 + kt + j) ? dp * site.inv_keep : 0.f;
                const float dsv = expf(s - m) * il * (dpm - delta);
#pragma unroll
                for (int d = 0; d < DT_HD; ++d) acc[d] = fmaf(dsv, Ks[j * DT_LS + d], acc[d]);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < DT_HD; ++d) sh_a[(split * DT_HD + d) * (DT_TQ + 1) + lane] = acc[d];
    __syncthreads();
    if (row < Lq) {
        float* op = dq + ((long long)b * Lq + row) * dq_stride + h * DT_HD;
        const bool live = row_ok && nk > 0;
#pragma unroll
        for (int dd = 0; dd < DT_HD / DT_SPLITS; ++dd) {
            const int d = split * (DT_HD / DT_SPLITS) + dd;
            float t = 0.f;
#pragma unroll
            for (int sp = 0; sp < DT_SPLITS; ++sp) t += sh_a[(sp * DT_HD + d) * (DT_TQ + 1) + lane];
            op[d] = live ? t * scale : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2c) dv_j = sum_i keep_ij P_ij dO_i / (1 - p), dk_j = sum_i dS_ij (scale q_i).  One workgroup per (set, head, key tile): lane = key (its k
// and v rows in registers), wave = query split; the query tiles (scale q, dO and the three statistics) pass through LDS.  The sum over
// the queries runs inside this one workgroup: per split in index order, then over the splits in order.
__global__ __launch_bounds__(256) void attention_train_dkv_kernel(
    const float* __restrict__ q, long long q_stride, const float* __restrict__ k, long long k_stride, const float* __restrict__ v,
    long long v_stride, const float* __restrict__ dout, long long do_stride, const float* __restrict__ ws, float* __restrict__ dk,
    long long dk_stride, float* __restrict__ dv, long long dv_stride, int Lq, int Lk, int heads, float scale, const int* __restrict__ qlen,
    const int* __restrict__ klen, DropSite site) {
    __shared__ float Qs[DT_TQ * DT_LS];
    __shared__ float Ds[DT_TQ * DT_LS];
    __shared__ float St[DT_TQ * 3];
    __shared__ float sh_a[DT_SPLITS * DT_HD * (DT_TK + 1)];
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int split = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int key = blockIdx.x * DT_TK + lane;
    const int nq = qlen ? min(max(qlen[b], 0), Lq) : Lq;
    const int nk = klen ? min(max(klen[b], 0), Lk) : Lk;
    const bool key_ok = key < nk;
    const int kc = key_ok ? key : 0;
    const long long krow = (long long)b * Lk + kc;
    float kr[DT_HD], vr[DT_HD], ak[DT_HD], av[DT_HD];
#pragma unroll
    for (int d = 0; d < DT_HD; ++d) {
        const float kv = k[krow * k_stride + h * DT_HD + d], vv = v[krow * v_stride + h * DT_HD + d];
        kr[d] = key_ok ? kv : 0.f;
        vr[d] = key_ok ? vv : 0.f;
        ak[d] = 0.f;
        av[d] = 0.f;
    }
    const float* stb = ws + ((long long)b * heads + h) * Lq * 3;
    const long long idx0 = ((long long)b * heads + h) * Lq * Lk + kc;
    for (int it = 0; it < nq; it += DT_TQ) {
        __syncthreads();
        dt_stage_pair(q, q_stride, dout, do_stride, (long long)b * Lq, it, nq, h, scale, Qs, Ds);
        if (threadIdx.x < DT_TQ * 3) {
            const int i = threadIdx.x / 3, c = threadIdx.x - 3 * i;
            const bool ok = it + i < nq;
            const float sv = stb[(long long)(ok ? it + i : 0) * 3 + c];
            St[threadIdx.x] = ok ? sv : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < DT_PER; ++t) {
            const int i = split + DT_SPLITS * t;
            if (it + i < nq) {                             // wave-uniform
                const float s = dt_dot(kr, Qs + i * DT_LS);             // (the products of dt_dot(qr, Ks) with the factors swapped: the same bits)
                const float dp = dt_dot(vr, Ds + i * DT_LS);
                const bool keep = dt_keep(site, idx0 + (long long)(it + i) * Lk);
                const float pj = expf(s - St[i * 3]) * St[i * 3 + 1];
                const float dpm = keep ? dp * site.inv_keep : 0.f;
                const float dsv = pj * (dpm - St[i * 3 + 2]);
                const float w = keep ? pj * site.inv_keep : 0.f;
#pragma unroll
                for (int d = 0; d < DT_HD; ++d) {
                    av[d] = fmaf(w, Ds[i * DT_LS + d], av[d]);
                    ak[d] = fmaf(dsv, Qs[i * DT_LS + d], ak[d]);
                }
            }
        }
    }
    const bool live = key_ok && nq > 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();                                   // (pass 1: the dk sums have been read)
#pragma unroll
        for (int d = 0; d < DT_HD; ++d) sh_a[(split * DT_HD + d) * (DT_TK + 1) + lane] = pass == 0 ? ak[d] : av[d];
        __syncthreads();
        if (key < Lk) {
            float* op = (pass == 0 ? dk + ((long long)b * Lk + key) * dk_stride : dv + ((long long)b * Lk + key) * dv_stride) + h * DT_HD;
#pragma unroll
            for (int dd = 0; dd < DT_HD / DT_SPLITS; ++dd) {
                const int d = split * (DT_HD / DT_SPLITS) + dd;
                float t = 0.f;
#pragma unroll
                for (int sp = 0; sp < DT_SPLITS; ++sp) t += sh_a[(sp * DT_HD + d) * (DT_TK + 1) + lane];
                op[d] = live ? t : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) element-wise dropout and the materialised mask.  One thread per element; the element's index is the counter.
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const float* __restrict__ residual, float* __restrict__ y,
                                                      long long n, DropSite site) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float xv = x[i];
    float r = dt_keep(site, i) ? xv * site.inv_keep : 0.f;
    if (residual) r += residual[i];
    y[i] = r;
}

__global__ __launch_bounds__(256) void dropout_keep_mask_kernel(uint8_t* __restrict__ out, long long n, DropSite site) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = dt_keep(site, i) ? 1 : 0;
}

static bool make_site(double p, int64_t seed, int64_t stream_id, DropSite* site) {
    if (!(p >= 0.0 && p < 1.0)) return false;
    site->key = dropout_key(seed, stream_id);
    site->threshold = (uint32_t)(uint64_t)(p * 4294967296.0);
    site->inv_keep = (float)(1.0 / (1.0 - p));
    return true;
}

}  // namespace nps

#define NPS_DROP_SITE(who)                                                                                     \
    nps::DropSite site;                                                                                        \
    NPS_CHECK_ARG(nps::make_site(p, seed, stream_id, &site), who ": p = %g is not in [0, 1)", p)

extern "C" int nopesac_dropout_keep_mask(uint8_t* out, int64_t n, double p, int64_t seed, int64_t stream_id, void* stream) {
    using namespace nps;
    NPS_DROP_SITE("dropout_keep_mask");
    NPS_CHECK_ARG(out && n > 0 && n <= (1ll << 38), "dropout_keep_mask: null output or n = %lld not in 1 .. 2^38", (long long)n);
    hipLaunchKernelGGL(dropout_keep_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, (long long)n, site);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_dropout_f32(const float* x, const float* residual, float* y, int64_t n, double p, int64_t seed, int64_t stream_id,
                                   void* stream) {
    using namespace nps;
    NPS_DROP_SITE("dropout");
    NPS_CHECK_ARG(x && y && n > 0 && n <= (1ll << 38), "dropout: null pointer or n = %lld not in 1 .. 2^38", (long long)n);
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, residual, y, (long long)n, site);
    NPS_LAUNCH_RET();
}

static int attention_train_check(const char* who, int B, int Lq, int Lk, int heads, int64_t min_stride) {
    NPS_CHECK_ARG(B > 0 && B <= 65535 && heads > 0 && heads <= 65535 && Lq > 0 && Lk > 0, "%s: bad dims (B=%d, heads=%d in 1..65535, Lq=%d, Lk=%d >= 1)",
                  who, B, heads, Lq, Lk);
    NPS_CHECK_ARG((double)B * heads * Lq * Lk < 4e18, "%s: B heads Lq Lk does not fit the 63-bit element counter", who);
    NPS_CHECK_ARG(min_stride >= (long long)heads * nps::DT_HD, "%s: heads * 32 = %lld is wider than a row stride", who, (long long)heads * nps::DT_HD);
    return 0;
}

extern "C" int nopesac_attention_train_forward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                                               int64_t v_stride, float* o, int64_t o_stride, int B, int Lq, int Lk, int heads, float scale,
                                               const int32_t* qlen, const int32_t* klen, double p, int64_t seed, int64_t stream_id,
                                               void* stream) {
    using namespace nps;
    NPS_DROP_SITE("attention_train_forward");
    NPS_CHECK_ARG(q && k && v && o, "attention_train_forward: null pointer");
    const int64_t ms = std::min(std::min(q_stride, k_stride), std::min(v_stride, o_stride));
    if (int rc = attention_train_check("attention_train_forward", B, Lq, Lk, heads, ms)) return rc;
    hipLaunchKernelGGL(attention_train_rows_kernel<false>, dim3((Lq + DT_TQ - 1) / DT_TQ, heads, B), dim3(256), 0, (hipStream_t)stream, q,
                       (long long)q_stride, k, (long long)k_stride, v, (long long)v_stride, (const float*)nullptr, 0ll, o, (long long)o_stride,
                       (float*)nullptr, Lq, Lk, heads, scale, qlen, klen, site);
    NPS_LAUNCH_RET();
}

extern "C" int64_t nopesac_attention_train_backward_workspace_floats(int B, int heads, int Lq) {
    return B >= 0 && heads >= 0 && Lq >= 0 ? NPS_ATT_TRAIN_BACKWARD_WORKSPACE_FLOATS(B, heads, Lq) : 0;
}

extern "C" int nopesac_attention_train_backward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                                                int64_t v_stride, const float* d_out, int64_t do_stride, int B, int Lq, int Lk, int heads,
                                                float scale, const int32_t* qlen, const int32_t* klen, double p, int64_t seed,
                                                int64_t stream_id, float* dq, int64_t dq_stride, float* dk, int64_t dk_stride, float* dv,
                                                int64_t dv_stride, float* ws, int64_t ws_floats, void* stream) {
    using namespace nps;
    NPS_DROP_SITE("attention_train_backward");
    NPS_CHECK_ARG(q && k && v && d_out, "attention_train_backward: null input");
    NPS_CHECK_ARG(dq && dk && dv && ws, "attention_train_backward: null output or workspace");
    const int64_t ms = std::min(std::min(std::min(q_stride, k_stride), std::min(v_stride, do_stride)),
                                std::min(dq_stride, std::min(dk_stride, dv_stride)));
    if (int rc = attention_train_check("attention_train_backward", B, Lq, Lk, heads, ms)) return rc;
    NPS_CHECK_ARG(ws_floats >= nopesac_attention_train_backward_workspace_floats(B, heads, Lq), "attention_train_backward: workspace too small");
    const dim3 qgrid((Lq + DT_TQ - 1) / DT_TQ, heads, B), kgrid((Lk + DT_TK - 1) / DT_TK, heads, B);
    hipLaunchKernelGGL(attention_train_rows_kernel<true>, qgrid, dim3(256), 0, (hipStream_t)stream, q, (long long)q_stride, k, (long long)k_stride,
                       v, (long long)v_stride, d_out, (long long)do_stride, (float*)nullptr, 0ll, ws, Lq, Lk, heads, scale, qlen, klen, site);
    hipLaunchKernelGGL(attention_train_dq_kernel, qgrid, dim3(256), 0, (hipStream_t)stream, q, (long long)q_stride, k, (long long)k_stride, v,
                       (long long)v_stride, d_out, (long long)do_stride, (const float*)ws, dq, (long long)dq_stride, Lq, Lk, heads, scale, qlen,
                       klen, site);
    hipLaunchKernelGGL(attention_train_dkv_kernel, kgrid, dim3(256), 0, (hipStream_t)stream, q, (long long)q_stride, k, (long long)k_stride, v,
                       (long long)v_stride, d_out, (long long)do_stride, (const float*)ws, dk, (long long)dk_stride, dv, (long long)dv_stride, Lq,
                       Lk, heads, scale, qlen, klen, site);
    NPS_LAUNCH_RET();
}
