// Training kernels of the plane head's top-down pyramid (training.PlanePyramidTrainer; reference top_down, planeTR_head.py:209-252, trained
// unfrozen: nn.BatchNorm2d on BATCH statistics, nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)): the statistics of a
// training-mode BatchNorm with the running-statistics update, its normalisation + ReLU (+ lateral), its backward, and the adjoint of the
// bilinear 2x upsampling.  f32 throughout, NHWC, caller-allocated buffers.
//
// Every BatchNorm kernel takes its input in one of two forms: plain, v = src [n][C] (n = B H W rows, channel stride cs), or upsampled,
// v = up2(src) with src = t [B][H][W][C] and n = B 2H 2W rows: an up stage relu(bn(conv1x1(up2(x)))) is evaluated as relu(bn(up2(t))),
// t = conv1x1(x) (the 1x1 conv commutes with the interpolation), and the statistics are those of up2(t) at the HIGH resolution - the
// clamped borders make them differ from t's.  up2(t) is evaluated on the fly with the expression of upsample_bilinear2x_kernel
// (elementwise.hip), so it has that kernel's bits, and is never written.
//
// A thread works on four consecutive channels (one 16-byte load per tensor and pixel: a wave reads a whole 256-channel row at once), so
// C, the channel stride and every pointer are multiples of 4 floats (checked by the entry points; the pyramid's 256 channels are).
// Deterministic: no atomics; every cross-workgroup sum goes through per-block partials in the caller's workspace and is finished in a
// fixed order.  Every load is unconditional from a clamped address and the value is selected afterwards; stores are guarded by the counts.
//
// View groups: the rows may be cut into G groups of ng = n / G consecutive rows (whole images: the two views of a 2B-image batch), each
// with its own statistics, as G module calls on the groups would have them.  A group's rows are cut into Sg = ceil(ng / BT_RPS) blocks
// from the group's first row - the partition an ungrouped call on those rows makes - and its partials are finished on their own in the
// ungrouped order, so every per-group result has the bits of an ungrouped call on the group's sub-tensor; one launch per stage covers
// all groups.  The upsampling and its adjoint never cross an image, so they never cross a group.
#include "common.h"

#include <cstdint>
#include <initializer_list>

namespace nps {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BT_RPS = NPS_BN_TRAIN_RPS;          // rows per partial block (64 channel quads x 4 row lanes)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// ---- bilinear x2, align_corners=False (PyTorch area_pixel_compute_source_index): the two taps and the weight of the second one for
// output index o of an axis of n inputs.  o = 2i: (i - 1, i, 0.75), at o = 0 (0, min(1, n - 1), 0); o = 2i + 1: (i, min(i + 1, n - 1), 0.25).
__device__ __forceinline__ void up2_taps(int o, int n, int& i0, int& i1, float& l) {
    const float s = fmaxf(0.5f * (o + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    i1 = min(i0 + 1, n - 1);
    l = s - i0;
}

__device__ __forceinline__ f32x4 up2_mix(f32x4 v00, f32x4 v01, f32x4 v10, f32x4 v11, float ly, float lx) {
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

struct Src {                                      // the input form of a BatchNorm kernel
    const float* p;
    int up, H, W;                                 // H, W: the spatial size of p (plain form: only H * W matters)
    long long cs;                                 // channel stride of p
};

// v at row r (plain: pixel r of p; upsampled: pixel r of the [B][2H][2W] map), channels ch .. ch + 3.  r and ch must be in range.
__device__ __forceinline__ f32x4 src_value(const Src& s, long long r, int ch) {
    if (!s.up) return ld4(s.p + r * s.cs + ch);
    const int OW = 2 * s.W, OH = 2 * s.H;
    const int ow = (int)(r % OW);
    const long long q = r / OW;
    const int oh = (int)(q % OH);
    const long long base = (q / OH) * s.H * s.W;
    int y0, y1, x0, x1;
    float ly, lx;
    up2_taps(oh, s.H, y0, y1, ly);
    up2_taps(ow, s.W, x0, x1, lx);
    const float* p = s.p + ch;
    return up2_mix(ld4(p + (base + (long long)y0 * s.W + x0) * s.cs), ld4(p + (base + (long long)y0 * s.W + x1) * s.cs),
                   ld4(p + (base + (long long)y1 * s.W + x0) * s.cs), ld4(p + (base + (long long)y1 * s.W + x1) * s.cs), ly, lx);
}

__device__ __forceinline__ f32x4 sum4(const f32x4 (*sh)[64], int cl) { return (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]); }

// the block's geometry: lane cl of wave rl works on channels ch .. ch + 3 (clamped to chc for the loads) of rows r0 + rl, r0 + rl + 4, ...
// (the wave index is made a scalar, so that the row's index arithmetic runs once per wave); block y = grp * Sg + z is block z of group grp,
// whose rows are [grp ng, (grp + 1) ng)
#define BT_BLOCK_GEOMETRY()                                                                              \
    const int cl = threadIdx.x & 63, rl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);              \
    const int ch = (blockIdx.x * 64 + cl) * 4, chc = min(ch, C - 4);                                     \
    const int grp = blockIdx.y / Sg;                                                                     \
    const long long gbeg = grp * ng, r0 = gbeg + (long long)(blockIdx.y - grp * Sg) * BT_RPS, r1 = min(gbeg + ng, r0 + BT_RPS)

// a wave's rows, BT_ROWS_IN_FLIGHT at a time: the loads of rows r, r + 4, ... are issued together, each from an address clamped to the
// block's last row, and a row beyond it is left out of the sums afterwards (the condition is the same for the whole wave); the sums
// take the rows in increasing order
constexpr int BT_ROWS_IN_FLIGHT = 4;
#define BT_FOR_ROWS(r) for (long long r = r0 + rl; r < r1; r += 4 * BT_ROWS_IN_FLIGHT)
#define BT_ROW(r, u) min(r + 4 * (u), r1 - 1)
#define BT_LIVE(r, u) (r + 4 * (u) < r1)

// ---- statistics, first launch: per block of BT_RPS rows and per channel the block's mean and its sum of squares about that mean (two
// passes over the block's rows; the second one hits the cache) -> part[group][block][2][C].
__global__ __launch_bounds__(256) void bn_train_stats_kernel(Src s, long long ng, int Sg, int C, float* __restrict__ part) {
    __shared__ f32x4 sh[4][64];
    BT_BLOCK_GEOMETRY();
    f32x4 a = 0.f;
    BT_FOR_ROWS(r) {
        f32x4 v[BT_ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u) v[u] = src_value(s, BT_ROW(r, u), chc);
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u)
            if (BT_LIVE(r, u)) a += v[u];
    }
    sh[rl][cl] = a;
    __syncthreads();
    const f32x4 mu = sum4(sh, cl) / (float)(r1 - r0);
    __syncthreads();
    f32x4 q = 0.f;
    BT_FOR_ROWS(r) {
        f32x4 v[BT_ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u) v[u] = src_value(s, BT_ROW(r, u), chc);
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u) {
            const f32x4 d = v[u] - mu;
            if (BT_LIVE(r, u)) q += d * d;
        }
    }
    sh[rl][cl] = q;
    __syncthreads();
    if (rl == 0 && ch < C) {
        float* o = part + (long long)blockIdx.y * 2 * C;
        st4(o + ch, mu);
        st4(o + C + ch, sum4(sh, cl));
    }
}

// ---- ... second launch: the blocks' (mean, M2) merged by Chan et al.'s formula (no E[x^2] - E[x]^2 anywhere) in a fixed order: the S
// blocks are cut into BT_SEGMENTS runs of K = ceil(S / BT_SEGMENTS) consecutive blocks, a thread merges one run in block order, and the
// runs are merged in run order (a chain of K + BT_SEGMENTS dependent steps instead of S: S = 2400 at the workload) -> mean, biased
// variance, rstd = 1 / sqrt(var + eps) and, if given, the running statistics updated in place (the variance with n / (n - 1)).
// Block: 16 channels x BT_SEGMENTS runs.  Groups are finished one after the other by the same block, each from its own Sg partials of
// its ng rows (above: S = Sg, n = ng); the running statistics stay in a register and take the groups' statistics in group order, as G module calls would leave them.
constexpr int BT_SEGMENTS = 16;

struct Moments {
    long long n;
    float mu, m2;
};

__device__ __forceinline__ void chan_merge(Moments& a, long long nb, float mb, float qb) {      // a <- a u b; an empty b changes nothing
    if (nb <= 0) return;
    const long long nt = a.n + nb;
    const float f = (float)nb / (float)nt, d = mb - a.mu;
    a.mu += d * f;
    a.m2 += qb + d * d * ((float)a.n * f);
    a.n = nt;
}

__global__ __launch_bounds__(256) void bn_train_finish_kernel(const float* __restrict__ part, int G, int Sg, long long ng, int C, float eps,
                                                              float mom, float* __restrict__ mean, float* __restrict__ var,
                                                              float* __restrict__ rstd, float* __restrict__ run_mean,
                                                              float* __restrict__ run_var) {
    __shared__ float smu[BT_SEGMENTS][16], sm2[BT_SEGMENTS][16];
    const int c = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int ch = blockIdx.x * 16 + c, chc = min(ch, C - 1);
    const int K = (Sg + BT_SEGMENTS - 1) / BT_SEGMENTS;
    const int z0 = min(seg * K, Sg), z1 = min(z0 + K, Sg);
    const bool owner = seg == 0 && ch < C;
    float rm = run_mean ? run_mean[chc] : 0.f, rv = run_var ? run_var[chc] : 0.f;
    for (int grp = 0; grp < G; ++grp) {
        const float* pg = part + (long long)grp * Sg * 2 * C;
        Moments m{0, 0.f, 0.f};
        for (int z = z0; z < z1; ++z)
            chan_merge(m, min((long long)BT_RPS, ng - (long long)z * BT_RPS), pg[(long long)z * 2 * C + chc], pg[(long long)z * 2 * C + C + chc]);
        smu[seg][c] = m.mu;
        sm2[seg][c] = m.m2;
        __syncthreads();
        if (owner) {
            for (int j = 1; j < BT_SEGMENTS; ++j) {            // run j holds the rows [j K RPS, (j + 1) K RPS) that exist
                const long long lo = min(ng, (long long)j * K * BT_RPS), hi = min(ng, (long long)(j + 1) * K * BT_RPS);
                chan_merge(m, hi - lo, smu[j][c], sm2[j][c]);
            }
            const float v = m.m2 / (float)ng;
            mean[(long long)grp * C + ch] = m.mu;
            var[(long long)grp * C + ch] = v;
            rstd[(long long)grp * C + ch] = 1.f / sqrtf(v + eps);
            rm = (1.f - mom) * rm + mom * m.mu;
            rv = (1.f - mom) * rv + mom * (v * ((float)ng / (float)(ng - 1)));
        }
        __syncthreads();
    }
    if (owner && run_mean) run_mean[ch] = rm;
    if (owner && run_var) run_var[ch] = rv;
}

// z = gamma xhat + beta, xhat = (v - mean) rstd: ONE expression for the forward and for the gate the backward recomputes
__device__ __forceinline__ f32x4 bn_xhat(f32x4 v, f32x4 mu, f32x4 rstd) { return (v - mu) * rstd; }
__device__ __forceinline__ f32x4 bn_z(f32x4 xh, f32x4 ga, f32x4 be) { return ga * xh + be; }

// g where the gate is open (z > 0 under ReLU), else 0
__device__ __forceinline__ f32x4 bn_gate(f32x4 g, f32x4 z, int relu) {
    f32x4 dz;
#pragma unroll
    for (int e = 0; e < 4; ++e) dz[e] = (!relu || z[e] > 0.f) ? g[e] : 0.f;
    return dz;
}

// ---- y = act(z) (+ addend): one thread per channel quad
// the statistics' offset of row r: its group's [C] block of mean / rstd (0 without groups: no division)
__device__ __forceinline__ long long bn_group_offset(long long r, int G, long long ng, int C) { return G > 1 ? (r / ng) * C : 0; }

__global__ __launch_bounds__(256) void bn_train_apply_kernel(Src s, long long n, int G, long long ng, int C, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, int relu, const float* __restrict__ addend,
                                                             float* __restrict__ y) {
    const int CV = C / 4;
    const long long total = n * CV;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        const long long go = bn_group_offset(i / CV, G, ng, C);
        const f32x4 z = bn_z(bn_xhat(src_value(s, i / CV, ch), ld4(mean + go + ch), ld4(rstd + go + ch)), ld4(gamma + ch), ld4(beta + ch));
        f32x4 o = bn_gate(z, z, relu);
        if (addend) o += ld4(addend + i * 4);
        st4(y + i * 4, o);
    }
}

// ---- backward, first launch: dz = g [z > 0]; per block of BT_RPS rows the partials of dgamma = sum dz xhat and dbeta = sum dz
__global__ __launch_bounds__(256) void bn_train_bwd_reduce_kernel(const float* __restrict__ g, Src s, long long ng, int Sg, int C,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd, int relu,
                                                                  float* __restrict__ part) {
    __shared__ f32x4 sg[4][64], sb[4][64];
    BT_BLOCK_GEOMETRY();
    const f32x4 ga = ld4(gamma + chc), be = ld4(beta + chc), mu = ld4(mean + (long long)grp * C + chc), rs = ld4(rstd + (long long)grp * C + chc);
    f32x4 ag = 0.f, ab = 0.f;
    BT_FOR_ROWS(r) {
        f32x4 v[BT_ROWS_IN_FLIGHT], gv[BT_ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u) {
            v[u] = src_value(s, BT_ROW(r, u), chc);
            gv[u] = ld4(g + BT_ROW(r, u) * C + chc);
        }
#pragma unroll
        for (int u = 0; u < BT_ROWS_IN_FLIGHT; ++u) {
            const f32x4 xh = bn_xhat(v[u], mu, rs);
            const f32x4 dz = bn_gate(gv[u], bn_z(xh, ga, be), relu);
            if (BT_LIVE(r, u)) {
                ag += dz * xh;
                ab += dz;
            }
        }
    }
    sg[rl][cl] = ag;
    sb[rl][cl] = ab;
    __syncthreads();
    if (rl == 0 && ch < C) {
        float* o = part + (long long)blockIdx.y * 2 * C;
        st4(o + ch, sum4(sg, cl));
        st4(o + C + ch, sum4(sb, cl));
    }
}

// ---- per-channel partial sums [S][2][C] -> a[C], b[C] in a fixed order: BT_SEGMENTS runs of consecutive blocks summed in block order
// by a thread each, then the runs in run order.  Block: 16 of the 2 C sums x BT_SEGMENTS runs.  Groups: each group's S partials are
// summed on their own -> gsums[group][2][C] (the S2_g = sum dz xhat and S1_g = sum dz the second launch reads; null: G = 1, not written),
// and a, b take the groups' sums in group order.
__global__ __launch_bounds__(256) void bn_train_sum_partials_kernel(const float* __restrict__ part, int G, int Sg, int C, float* __restrict__ a,
                                                                    float* __restrict__ b, float* __restrict__ gsums) {
    __shared__ float sh[BT_SEGMENTS][16];
    const int c = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + c, ic = min(i, 2 * C - 1);
    const int K = (Sg + BT_SEGMENTS - 1) / BT_SEGMENTS;
    const int z0 = min(seg * K, Sg), z1 = min(z0 + K, Sg);
    const bool owner = seg == 0 && i < 2 * C;
    float tot = 0.f;
    for (int grp = 0; grp < G; ++grp) {
        const float* pg = part + (long long)grp * Sg * 2 * C;
        float s = 0.f;
        for (int z = z0; z < z1; ++z) s += pg[(long long)z * 2 * C + ic];
        sh[seg][c] = s;
        __syncthreads();
        if (owner) {
            for (int j = 1; j < BT_SEGMENTS; ++j) s += sh[j][c];
            if (gsums) gsums[(long long)grp * 2 * C + i] = s;
            tot = grp == 0 ? s : tot + s;
        }
        __syncthreads();
    }
    if (!owner) return;
    if (i < C) a[i] = tot;
    else b[i - C] = tot;
}

// the per-channel constants of the second backward launch
struct BnBwd {
    f32x4 ga, be, mu, rs, mb, mg;                 // mb = dbeta / n, mg = dgamma / n (0 with stored statistics)
};

__device__ __forceinline__ BnBwd bn_bwd_consts(const float* gamma, const float* beta, const float* mean, const float* rstd,
                                               const float* dgamma, const float* dbeta, float inv_n, int ch) {
    return BnBwd{ld4(gamma + ch), ld4(beta + ch), ld4(mean + ch), ld4(rstd + ch), ld4(dbeta + ch) * inv_n, ld4(dgamma + ch) * inv_n};
}

// dv = gamma rstd (dz - dbeta / n - xhat dgamma / n)
__device__ __forceinline__ f32x4 bn_dv(f32x4 gv, f32x4 v, const BnBwd& k, int relu) {
    const f32x4 xh = bn_xhat(v, k.mu, k.rs);
    const f32x4 dz = bn_gate(gv, bn_z(xh, k.ga, k.be), relu);
    return (k.ga * k.rs) * ((dz - k.mb) - xh * k.mg);
}

// ---- backward, second launch, plain form: dv per element.  dgamma / dbeta here are the sums of the element's group: [C] each without
// groups, else gsums' [group][2][C] (the caller passes gsums, gsums + C), inv_n = 1 / ng.
__global__ __launch_bounds__(256) void bn_train_bwd_apply_kernel(const float* __restrict__ g, Src s, long long n, int G, long long ng, int C,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ dgamma, const float* __restrict__ dbeta, int relu,
                                                                 float inv_n, float* __restrict__ dv) {
    const int CV = C / 4;
    const long long total = n * CV;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        const long long go = bn_group_offset(i / CV, G, ng, C);
        const BnBwd k = bn_bwd_consts(gamma, beta, mean + go, rstd + go, dgamma + 2 * go, dbeta + 2 * go, inv_n, ch);
        st4(dv + i * 4, bn_dv(ld4(g + i * 4), ld4(s.p + (i / CV) * s.cs + ch), k, relu));
    }
}

// ---- the adjoint of the bilinear 2x upsampling as a gather: low-resolution index i of an axis of n reads the outputs o = 2i - 1 + d,
// d = 0..3, with the weight input i has in output o: 0.25, 0.75, 0.75, 0.25; the clamped border taps fold back in, so that output 0
// weighs input 0 by 1 and output 2n - 1 weighs input n - 1 by 1; outputs outside [0, 2n) get weight 0 and a clamped address.
// l[d]: the interpolation weight of output o (as up2_taps gives it), for the fused form that recomputes up2(t) from t's 3 x 3
// neighbourhood t[i - 1 .. i + 1] (clamped): d < 2 mixes rows (0, 1) of it, d >= 2 rows (1, 2).
struct Gather {
    int o[4];
    float w[4], l[4];
};

__device__ __forceinline__ Gather up2_gather(int i, int n) {
    Gather t;
    const bool first = i == 0, last = i == n - 1;
    t.o[0] = max(2 * i - 1, 0);
    t.o[1] = 2 * i;
    t.o[2] = 2 * i + 1;
    t.o[3] = min(2 * i + 2, 2 * n - 1);
    t.w[0] = first ? 0.f : 0.25f;
    t.w[1] = first ? 1.f : 0.75f;
    t.w[2] = last ? 1.f : 0.75f;
    t.w[3] = last ? 0.f : 0.25f;
    t.l[0] = 0.25f;
    t.l[1] = first ? 0.f : 0.75f;
    t.l[2] = 0.25f;
    t.l[3] = 0.75f;
    return t;
}

__global__ __launch_bounds__(256) void upsample2x_bilinear_bwd_kernel(const float* __restrict__ du, float* __restrict__ dx, int B, int H,
                                                                      int W, int C) {
    const int CV = C / 4;
    const long long total = (long long)B * H * W * CV;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        long long px = i / CV;
        const int ix = (int)(px % W); px /= W;
        const int iy = (int)(px % H);
        const long long base = (px / H) * 4 * H * W;
        const Gather gy = up2_gather(iy, H), gx = up2_gather(ix, W);
        f32x4 acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4 row = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) row += gx.w[b] * ld4(du + (base + (long long)gy.o[a] * 2 * W + gx.o[b]) * C + ch);
            acc += gy.w[a] * row;
        }
        st4(dx + i * 4, acc);
    }
}

// ---- backward, second launch, upsampled form: dt = up2^T(dv) with dv evaluated inside the gather and never written.  One thread per
// channel quad of a pixel of t: its 3 x 3 neighbourhood of t (clamped) gives up2(t) at the 4 x 4 outputs, g is read at those 16 pixels.
__global__ __launch_bounds__(256) void bn_train_bwd_apply_up_kernel(const float* __restrict__ g, Src s, int B, int G, int Bg, int C,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta, int relu,
                                                                    float inv_n, float* __restrict__ dt) {
    const int H = s.H, W = s.W, CV = C / 4;
    const long long total = (long long)B * H * W * CV;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        long long px = i / CV;
        const int ix = (int)(px % W); px /= W;
        const int iy = (int)(px % H);
        const long long b = px / H;
        const Gather gy = up2_gather(iy, H), gx = up2_gather(ix, W);
        const int ys[3] = {max(iy - 1, 0), iy, min(iy + 1, H - 1)}, xs[3] = {max(ix - 1, 0), ix, min(ix + 1, W - 1)};
        f32x4 t[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) t[a][c] = ld4(s.p + ((b * H + ys[a]) * W + xs[c]) * s.cs + ch);
        const long long go = bn_group_offset(b, G, Bg, C);          // the image's group: the gather stays inside the image
        const BnBwd k = bn_bwd_consts(gamma, beta, mean + go, rstd + go, dgamma + 2 * go, dbeta + 2 * go, inv_n, ch);
        const long long gbase = b * 4 * H * W;
        f32x4 acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ra = a < 2 ? 0 : 1;
            f32x4 row = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int rc = c < 2 ? 0 : 1;
                const f32x4 v = up2_mix(t[ra][rc], t[ra][rc + 1], t[ra + 1][rc], t[ra + 1][rc + 1], gy.l[a], gx.l[c]);
                const f32x4 gv = ld4(g + (gbase + (long long)gy.o[a] * 2 * W + gx.o[c]) * C + ch);
                row += gx.w[c] * bn_dv(gv, v, k, relu);
            }
            acc += gy.w[a] * row;
        }
        st4(dt + i * 4, acc);
    }
}

static inline int grid_for(long long total) {
    const long long g = (total + 255) / 256;
    return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

static inline bool quad_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p % 16) return false;
    return true;
}

}  // namespace nps

using namespace nps;

// the argument checks the three BatchNorm entry points share: -> n (rows of v), or 0 with the error set
static long long bn_train_rows(const char* who, const void* src, int up, int B, int H, int W, int C, int64_t cs) {
    if (!(src && B > 0 && H > 0 && W > 0 && C > 0 && (up == 0 || up == 1) && cs >= C)) {
        nps::set_error("%s: bad arguments up=%d B=%d H=%d W=%d C=%d cstride=%lld", who, up, B, H, W, C, (long long)cs);
        return 0;
    }
    if (C % 4 || cs % 4) {
        nps::set_error("%s: C = %d and the channel stride %lld must be multiples of 4", who, C, (long long)cs);
        return 0;
    }
    const long long n = (long long)B * H * W * (up ? 4 : 1);
    if (n >= (1ll << 31) / 2 || (n + BT_RPS - 1) / BT_RPS >= 65536) {
        nps::set_error("%s: %lld rows are more than the kernels index", who, n);
        return 0;
    }
    return n;
}

// the groups of a call: G = 1 for groups 0 or 1; else G must divide the B images (rows of the matrix form) -> rows per group, or 0 with
// the error set
static long long bn_train_group_rows(const char* who, long long n, int B, int groups, int& G) {
    G = groups <= 1 ? 1 : groups;
    if (groups < 0 || G > NPS_BN_TRAIN_MAX_GROUPS || B % G != 0) {
        nps::set_error("%s: groups=%d must be 0..%d and divide B=%d", who, groups, NPS_BN_TRAIN_MAX_GROUPS, B);
        return 0;
    }
    const long long ng = n / G;
    if ((long long)G * ((ng + BT_RPS - 1) / BT_RPS) >= 65536) {
        nps::set_error("%s: %d groups of %lld rows are more blocks than a launch indexes", who, G, ng);
        return 0;
    }
    return ng;
}

extern "C" int64_t nopesac_bn_train_workspace_floats(int64_t n, int C) { return n > 0 && C > 0 ? NPS_BN_TRAIN_WORKSPACE_FLOATS(n, C) : 0; }

extern "C" int nopesac_bn_train_groups_workspace_floats(int groups, int64_t n, int C, int64_t* floats) {
    NPS_CHECK_ARG(floats, "bn_train_groups_workspace_floats: null pointer");
    *floats = 0;
    const int G = groups <= 1 ? 1 : groups;
    NPS_CHECK_ARG(groups >= 0 && G <= NPS_BN_TRAIN_MAX_GROUPS && n > 0 && C > 0 && n % G == 0,
                  "bn_train_groups_workspace_floats: bad arguments groups=%d n=%lld C=%d", groups, (long long)n, C);
    *floats = NPS_BN_TRAIN_GROUPS_WORKSPACE_FLOATS(G, n, C);
    return 0;
}

static int bn_train_stats_launch(const char* who, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups, float eps,
                                 float momentum, float* mean, float* var, float* rstd, float* running_mean, float* running_var, float* ws,
                                 int64_t ws_floats, void* stream) {
    const long long n = bn_train_rows(who, src, up, B, H, W, C, src_cstride);
    if (!n) return NPS_E_ARG;
    int G;
    const long long ng = bn_train_group_rows(who, n, B, groups, G);
    if (!ng) return NPS_E_ARG;
    NPS_CHECK_ARG(mean && var && rstd && ws, "%s: null pointer", who);
    NPS_CHECK_ARG(quad_aligned({src, ws}), "%s: src and ws must be 16-byte aligned", who);
    NPS_CHECK_ARG(ng >= 2, "%s: batch statistics need more than one value per channel (n = %lld)", who, ng);
    NPS_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "%s: eps / momentum out of range", who);
    NPS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "%s: running_mean and running_var come together", who);
    NPS_CHECK_ARG(ws_floats >= NPS_BN_TRAIN_GROUPS_WORKSPACE_FLOATS(G, n, C), "%s: workspace too small", who);
    const int Sg = (int)((ng + BT_RPS - 1) / BT_RPS);
    hipStream_t st = (hipStream_t)stream;
    const Src s{src, up, H, W, (long long)src_cstride};
    bn_train_stats_kernel<<<dim3((C + 255) / 256, G * Sg), 256, 0, st>>>(s, ng, Sg, C, ws);
    bn_train_finish_kernel<<<(C + 15) / 16, 256, 0, st>>>(ws, G, Sg, ng, C, eps, momentum, mean, var, rstd, running_mean, running_var);
    NPS_LAUNCH_RET();
}

static int bn_train_apply_launch(const char* who, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups,
                                 const float* gamma, const float* beta, const float* mean, const float* rstd, int act, const float* addend,
                                 float* y, void* stream) {
    const long long n = bn_train_rows(who, src, up, B, H, W, C, src_cstride);
    if (!n) return NPS_E_ARG;
    int G;
    const long long ng = bn_train_group_rows(who, n, B, groups, G);
    if (!ng) return NPS_E_ARG;
    NPS_CHECK_ARG(gamma && beta && mean && rstd && y, "%s: null pointer", who);
    NPS_CHECK_ARG(quad_aligned({src, gamma, beta, mean, rstd, addend, y}), "%s: every pointer must be 16-byte aligned", who);
    NPS_CHECK_ARG(act == NPS_ACT_NONE || act == NPS_ACT_RELU, "%s: bad act %d", who, act);
    const Src s{src, up, H, W, (long long)src_cstride};
    bn_train_apply_kernel<<<grid_for(n * (C / 4)), 256, 0, (hipStream_t)stream>>>(s, n, G, ng, C, gamma, beta, mean, rstd, act == NPS_ACT_RELU, addend, y);
    NPS_LAUNCH_RET();
}

static int bn_train_backward_launch(const char* who, const float* dy, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride,
                                    int groups, const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                                    int batch_stats, float* dsrc, float* dgamma, float* dbeta, float* group_sums, float* ws, int64_t ws_floats,
                                    void* stream) {
    const long long n = bn_train_rows(who, src, up, B, H, W, C, src_cstride);
    if (!n) return NPS_E_ARG;
    int G;
    const long long ng = bn_train_group_rows(who, n, B, groups, G);
    if (!ng) return NPS_E_ARG;
    NPS_CHECK_ARG(dy && gamma && beta && mean && rstd && dsrc && dgamma && dbeta && ws && (G == 1 || group_sums), "%s: null pointer", who);
    NPS_CHECK_ARG(quad_aligned({dy, src, gamma, beta, mean, rstd, dsrc, dgamma, dbeta, group_sums, ws}), "%s: every pointer must be 16-byte aligned", who);
    NPS_CHECK_ARG(act == NPS_ACT_NONE || act == NPS_ACT_RELU, "%s: bad act %d", who, act);
    NPS_CHECK_ARG(ws_floats >= NPS_BN_TRAIN_GROUPS_WORKSPACE_FLOATS(G, n, C), "%s: workspace too small", who);
    const int Sg = (int)((ng + BT_RPS - 1) / BT_RPS), relu = act == NPS_ACT_RELU;
    const float inv_n = batch_stats ? 1.f / (float)ng : 0.f;     // stored statistics: mean and rstd are constants, dv = gamma rstd dz
    hipStream_t st = (hipStream_t)stream;
    const Src s{src, up, H, W, (long long)src_cstride};
    float* gsums = G > 1 ? group_sums : nullptr;                 // without groups the second launch reads dgamma / dbeta themselves
    const float* k1 = gsums ? gsums : dgamma;
    const float* k2 = gsums ? gsums + C : dbeta;
    bn_train_bwd_reduce_kernel<<<dim3((C + 255) / 256, G * Sg), 256, 0, st>>>(dy, s, ng, Sg, C, gamma, beta, mean, rstd, relu, ws);
    bn_train_sum_partials_kernel<<<(2 * C + 15) / 16, 256, 0, st>>>(ws, G, Sg, C, dgamma, dbeta, gsums);
    if (up)
        bn_train_bwd_apply_up_kernel<<<grid_for((long long)B * H * W * (C / 4)), 256, 0, st>>>(dy, s, B, G, B / G, C, gamma, beta, mean, rstd, k1, k2, relu, inv_n, dsrc);
    else
        bn_train_bwd_apply_kernel<<<grid_for(n * (C / 4)), 256, 0, st>>>(dy, s, n, G, ng, C, gamma, beta, mean, rstd, k1, k2, relu, inv_n, dsrc);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_bn_train_stats_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, float eps, float momentum,
                                          float* mean, float* var, float* rstd, float* running_mean, float* running_var, float* ws,
                                          int64_t ws_floats, void* stream) {
    return bn_train_stats_launch("bn_train_stats", src, up, B, H, W, C, src_cstride, 1, eps, momentum, mean, var, rstd, running_mean, running_var, ws,
                                 ws_floats, stream);
}

extern "C" int nopesac_bn_train_apply_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, const float* gamma,
                                          const float* beta, const float* mean, const float* rstd, int act, const float* addend, float* y,
                                          void* stream) {
    return bn_train_apply_launch("bn_train_apply", src, up, B, H, W, C, src_cstride, 1, gamma, beta, mean, rstd, act, addend, y, stream);
}

extern "C" int nopesac_bn_train_backward_f32(const float* dy, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride,
                                             const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                                             int batch_stats, float* dsrc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats,
                                             void* stream) {
    return bn_train_backward_launch("bn_train_backward", dy, src, up, B, H, W, C, src_cstride, 1, gamma, beta, mean, rstd, act, batch_stats, dsrc,
                                    dgamma, dbeta, nullptr, ws, ws_floats, stream);
}

extern "C" int nopesac_bn_train_groups_stats_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups, float eps,
                                                 float momentum, float* mean, float* var, float* rstd, float* running_mean, float* running_var,
                                                 float* ws, int64_t ws_floats, void* stream) {
    return bn_train_stats_launch("bn_train_groups_stats", src, up, B, H, W, C, src_cstride, groups, eps, momentum, mean, var, rstd, running_mean,
                                 running_var, ws, ws_floats, stream);
}

extern "C" int nopesac_bn_train_groups_apply_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups,
                                                 const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                                                 const float* addend, float* y, void* stream) {
    return bn_train_apply_launch("bn_train_groups_apply", src, up, B, H, W, C, src_cstride, groups, gamma, beta, mean, rstd, act, addend, y, stream);
}

extern "C" int nopesac_bn_train_groups_backward_f32(const float* dy, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride,
                                                    int groups, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                                    int act, int batch_stats, float* dsrc, float* dgamma, float* dbeta, float* group_sums,
                                                    float* ws, int64_t ws_floats, void* stream) {
    return bn_train_backward_launch("bn_train_groups_backward", dy, src, up, B, H, W, C, src_cstride, groups, gamma, beta, mean, rstd, act,
                                    batch_stats, dsrc, dgamma, dbeta, group_sums, ws, ws_floats, stream);
}

extern "C" int nopesac_upsample2x_bilinear_backward_f32(const float* du, float* dx, int B, int H, int W, int C, void* stream) {
    NPS_CHECK_ARG(du && dx, "upsample2x_bilinear_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && (long long)B * H * W * 4 < (1ll << 30), "upsample2x_bilinear_backward: bad dims B=%d H=%d W=%d C=%d", B, H, W, C);
    NPS_CHECK_ARG(C % 4 == 0 && quad_aligned({du, dx}), "upsample2x_bilinear_backward: C = %d must be a multiple of 4 and the pointers 16-byte aligned", C);
    upsample2x_bilinear_bwd_kernel<<<grid_for((long long)B * H * W * (C / 4)), 256, 0, (hipStream_t)stream>>>(du, dx, B, H, W, C);
    NPS_LAUNCH_RET();
}
