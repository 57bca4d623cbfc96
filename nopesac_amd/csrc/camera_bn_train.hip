// Training-mode BatchNorm of the camera head's conv stacks (training.CameraHeadTrainer(batch_stats=True); reference conv + nn.BatchNorm2d(eps
// 0.001, momentum 0.01) + LeakyReLU blocks, camera_modules.py:36-48, trained unfrozen: camera_head.py:78-112) on GROUPED batch statistics:
// the input c [G * n][C] is cut into G groups of n consecutive rows, every group is normalised by its own mean and variance, and the
// running buffers take the groups' statistics one after the other.  The siamese tower runs once per view in the reference
// (camera_head.py:646-647): the trainer runs both views as one batch, view 1 first, with G = 2; the two branches use G = 1.  One entry call
// covers all groups: statistics 2 launches, apply 1, backward 3, whatever G is.  f32 throughout, NHWC, caller-allocated buffers.
//
// A thread works on four consecutive channels (one 16-byte load per tensor and row).  A block of 256 threads is QL channel quads x
// 256 / QL row lanes, QL = the smallest power of two >= min(C / 4, 64): a 128-channel layer keeps every lane busy (32 quads x 8 rows),
// a 4-channel one too (1 quad x 256 rows).  The row lanes of a wave are summed by xor shuffles (distances 32 .. QL), the four waves
// through LDS.  Deterministic: no atomics; every cross-workgroup sum goes through per-block partials in the caller's workspace and is
// finished in a fixed order; QL depends on C alone and a group's blocks on n alone, so G = 2 gives per group the bits of G = 1 on
// that group's rows.  Every load is unconditional from a clamped address and the value is selected afterwards; stores are guarded.
#include "common.h"

#include <cstdint>
#include <initializer_list>

namespace nps {
namespace bng {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RPS = NPS_BN_GROUPED_RPS;              // rows of a group per partial block
constexpr int SEGMENTS = NPS_BN_GROUPED_SEGMENTS;    // the finishing kernels merge a group's blocks in this many runs of consecutive blocks
constexpr int ROWS_IN_FLIGHT = 4;
constexpr float LEAKY_SLOPE = 0.01f;                 // (bn_act_forward's, common.h apply_act)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// the block's geometry.  qsh = log2(QL).  Lane cl of a wave's row lane rs works on channels ch .. ch + 3 (clamped to chc for the loads) of
// the rows r0 + row, r0 + row + RL, ... of group blockIdx.z; r0, r1: the block's rows within the group; base: the group's first row in c
struct Geo {
    int cl, wave, lane, ch, chc, RL;
    long long r0, r1, base, row;
};

__device__ __forceinline__ Geo geometry(int qsh, long long n, int C) {
    Geo g;
    g.lane = threadIdx.x & 63;
    g.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    g.cl = g.lane & ((1 << qsh) - 1);
    const int rpw = 64 >> qsh;                      // row lanes per wave
    g.RL = 4 * rpw;
    g.row = g.wave * rpw + (g.lane >> qsh);
    g.ch = ((blockIdx.x << qsh) + g.cl) * 4;
    g.chc = min(g.ch, C - 4);
    g.r0 = (long long)blockIdx.y * RPS;
    g.r1 = min(n, g.r0 + RPS);
    g.base = (long long)blockIdx.z * n;
    return g;
}

// sum over the row lanes of a wave (lanes that share cl): every lane ends with the total of its cl
__device__ __forceinline__ f32x4 wave_rows_sum(f32x4 v, int qsh) {
    for (int o = 32; o >= (1 << qsh); o >>= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], o);
    }
    return v;
}

// ... and over the four waves: sh[wave][lane] holds the waves' totals (two barriers; every thread of the block calls it)
__device__ __forceinline__ f32x4 block_rows_sum(f32x4 v, int qsh, const Geo& g, f32x4 (*sh)[64]) {
    v = wave_rows_sum(v, qsh);
    __syncthreads();
    sh[g.wave][g.lane] = v;
    __syncthreads();
    return (sh[0][g.lane] + sh[1][g.lane]) + (sh[2][g.lane] + sh[3][g.lane]);
}

// a thread's rows, ROWS_IN_FLIGHT at a time: the loads of rows r, r + RL, ... are issued together, each from an address clamped to the
// block's last row, and a row beyond it is left out of the sums afterwards
#define BNG_FOR_ROWS(r) for (long long r = g.r0 + g.row; r < g.r1; r += (long long)g.RL * ROWS_IN_FLIGHT)
#define BNG_ROW(r, u) (g.base + min(r + (long long)g.RL * (u), g.r1 - 1))
#define BNG_LIVE(r, u) (r + (long long)g.RL * (u) < g.r1)

// ---- statistics, first launch: per group, per block of RPS rows and per channel the block's mean and its sum of squares about that
// mean (two passes over the block's rows; the second one hits the cache) -> part[group][block][2][C].
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ c, long long n, int C, int qsh, float* __restrict__ part) {
    __shared__ f32x4 sh[4][64];
    const Geo g = geometry(qsh, n, C);
    f32x4 a = 0.f;
    BNG_FOR_ROWS(r) {
        f32x4 v[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) v[u] = ld4(c + BNG_ROW(r, u) * C + g.chc);
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u)
            if (BNG_LIVE(r, u)) a += v[u];
    }
    const f32x4 mu = block_rows_sum(a, qsh, g, sh) / (float)(g.r1 - g.r0);
    f32x4 q = 0.f;
    BNG_FOR_ROWS(r) {
        f32x4 v[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) v[u] = ld4(c + BNG_ROW(r, u) * C + g.chc);
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
            const f32x4 d = v[u] - mu;
            if (BNG_LIVE(r, u)) q += d * d;
        }
    }
    const f32x4 m2 = block_rows_sum(q, qsh, g, sh);
    if (g.wave == 0 && g.lane < (1 << qsh) && g.ch < C) {
        float* o = part + ((long long)blockIdx.z * gridDim.y + blockIdx.y) * 2 * C;
        st4(o + g.ch, mu);
        st4(o + C + g.ch, m2);
    }
}

// ---- ... second launch: per group the blocks' (mean, M2) merged by Chan et al.'s formula (no E[x^2] - E[x]^2 anywhere) in a fixed
// order: the S blocks are cut into SEGMENTS runs of K = ceil(S / SEGMENTS) consecutive blocks, a thread merges one run in block order, and
// the runs are merged in run order -> mean, biased variance, rstd = 1 / sqrt(var + eps), [G][C] each.  The running statistics, if given,
// take the groups' statistics in group order (the variance with n / (n - 1)): the value stays in a register between the groups, which
// is what G single-group calls would store and load again.  Block: 16 channels x SEGMENTS runs, the groups one after the other.
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

__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ part, int S, long long n, int C, int G, float eps, float mom,
                                                     float* __restrict__ mean, float* __restrict__ var, float* __restrict__ rstd,
                                                     float* __restrict__ run_mean, float* __restrict__ run_var) {
    __shared__ float smu[SEGMENTS][16], sm2[SEGMENTS][16];
    const int c = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int ch = blockIdx.x * 16 + c, chc = min(ch, C - 1);
    const int K = (S + SEGMENTS - 1) / SEGMENTS;
    const int z0 = min(seg * K, S), z1 = min(z0 + K, S);
    const bool writer = seg == 0 && ch < C;
    float rm = run_mean ? run_mean[chc] : 0.f, rv = run_var ? run_var[chc] : 0.f;
    for (int grp = 0; grp < G; ++grp) {
        const float* pg = part + (long long)grp * S * 2 * C;
        Moments m{0, 0.f, 0.f};
        for (int z = z0; z < z1; ++z)
            chan_merge(m, min((long long)RPS, n - (long long)z * RPS), pg[(long long)z * 2 * C + chc], pg[(long long)z * 2 * C + C + chc]);
        __syncthreads();                                         // (the previous group's runs have been read)
        smu[seg][c] = m.mu;
        sm2[seg][c] = m.m2;
        __syncthreads();
        if (writer) {
            for (int j = 1; j < SEGMENTS; ++j) {                 // run j holds the rows [j K RPS, (j + 1) K RPS) that exist
                const long long lo = min(n, (long long)j * K * RPS), hi = min(n, (long long)(j + 1) * K * RPS);
                chan_merge(m, hi - lo, smu[j][c], sm2[j][c]);
            }
            const float v = m.m2 / (float)n;
            mean[(long long)grp * C + ch] = m.mu;
            var[(long long)grp * C + ch] = v;
            rstd[(long long)grp * C + ch] = 1.f / sqrtf(v + eps);
            rm = (1.f - mom) * rm + mom * m.mu;
            rv = (1.f - mom) * rv + mom * (v * ((float)n / (float)(n - 1)));
        }
    }
    if (writer && run_mean) {
        run_mean[ch] = rm;
        run_var[ch] = rv;
    }
}

// z = gamma xhat + beta, xhat = (c - mean) rstd: ONE expression for the forward and for the gate the backward recomputes
__device__ __forceinline__ f32x4 xhat_of(f32x4 v, f32x4 mu, f32x4 rstd) { return (v - mu) * rstd; }
__device__ __forceinline__ f32x4 z_of(f32x4 xh, f32x4 ga, f32x4 be) { return ga * xh + be; }

// act'(z) g: g where z > 0 (or without activation), else 0 (RELU) or 0.01 g (LEAKY); with g = z it is act(z).  act is uniform.
__device__ __forceinline__ f32x4 gate(f32x4 gv, f32x4 z, int act) {
    f32x4 dz;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float closed = act == NPS_ACT_LEAKY ? LEAKY_SLOPE * gv[e] : 0.f;
        dz[e] = (act == NPS_ACT_NONE || z[e] > 0.f) ? gv[e] : closed;
    }
    return dz;
}

// ---- y = act(z): one thread per channel quad, blockIdx.y = group
__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ c, long long n, int C, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, int act, float* __restrict__ y) {
    const int CV = C / 4;
    const long long total = n * CV, off = (long long)blockIdx.y * total * 4;
    const float *mg = mean + (long long)blockIdx.y * C, *rg = rstd + (long long)blockIdx.y * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        const f32x4 z = z_of(xhat_of(ld4(c + off + i * 4), ld4(mg + ch), ld4(rg + ch)), ld4(gamma + ch), ld4(beta + ch));
        st4(y + off + i * 4, gate(z, z, act));
    }
}

// ---- backward, first launch: dz = dy act'(z); per group and block of RPS rows the partials of S2 = sum dz xhat and S1 = sum dz
// -> part[group][block][2][C]
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ c, long long n, int C, int qsh,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd, int act,
                                                         float* __restrict__ part) {
    __shared__ f32x4 sh[4][64];
    const Geo g = geometry(qsh, n, C);
    const f32x4 ga = ld4(gamma + g.chc), be = ld4(beta + g.chc);
    const f32x4 mu = ld4(mean + (long long)blockIdx.z * C + g.chc), rs = ld4(rstd + (long long)blockIdx.z * C + g.chc);
    f32x4 ag = 0.f, ab = 0.f;
    BNG_FOR_ROWS(r) {
        f32x4 v[ROWS_IN_FLIGHT], gv[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
            v[u] = ld4(c + BNG_ROW(r, u) * C + g.chc);
            gv[u] = ld4(dy + BNG_ROW(r, u) * C + g.chc);
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
            const f32x4 xh = xhat_of(v[u], mu, rs);
            const f32x4 dz = gate(gv[u], z_of(xh, ga, be), act);
            if (BNG_LIVE(r, u)) {
                ag += dz * xh;
                ab += dz;
            }
        }
    }
    const f32x4 s2 = block_rows_sum(ag, qsh, g, sh);
    const f32x4 s1 = block_rows_sum(ab, qsh, g, sh);
    if (g.wave == 0 && g.lane < (1 << qsh) && g.ch < C) {
        float* o = part + ((long long)blockIdx.z * gridDim.y + blockIdx.y) * 2 * C;
        st4(o + g.ch, s2);
        st4(o + C + g.ch, s1);
    }
}

// ---- ... second launch: part[G][S][2][C] -> per group its sums gsum[G][2][C] (S2 | S1; SEGMENTS runs of consecutive blocks summed in
// block order by a thread each, then the runs in run order) and dgamma = sum_g S2_g, dbeta = sum_g S1_g, added in group order.
// Block: 16 of the 2 C sums x SEGMENTS runs, the groups one after the other.
__global__ __launch_bounds__(256) void bwd_sum_kernel(const float* __restrict__ part, int S, int C, int G, float* __restrict__ gsum,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float sh[SEGMENTS][16];
    const int c = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + c, ic = min(i, 2 * C - 1);
    const int K = (S + SEGMENTS - 1) / SEGMENTS;
    const int z0 = min(seg * K, S), z1 = min(z0 + K, S);
    const bool writer = seg == 0 && i < 2 * C;
    float total = 0.f;
    for (int grp = 0; grp < G; ++grp) {
        const float* pg = part + (long long)grp * S * 2 * C;
        float s = 0.f;
        for (int z = z0; z < z1; ++z) s += pg[(long long)z * 2 * C + ic];
        __syncthreads();
        sh[seg][c] = s;
        __syncthreads();
        if (writer) {
            for (int j = 1; j < SEGMENTS; ++j) s += sh[j][c];
            gsum[(long long)grp * 2 * C + i] = s;
            total = grp == 0 ? s : total + s;
        }
    }
    if (writer) {
        if (i < C) dgamma[i] = total;
        else dbeta[i - C] = total;
    }
}

// ---- ... third launch: dc = gamma rstd_g (dz - S1_g / n - xhat S2_g / n) per element (inv_n = 0: the statistics are constants of the
// backward, dc = gamma rstd dz); blockIdx.y = group
__global__ __launch_bounds__(256) void bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ c, long long n, int C,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gsum, int act, float inv_n, float* __restrict__ dc) {
    const int CV = C / 4;
    const long long total = n * CV, off = (long long)blockIdx.y * total * 4;
    const float *mg = mean + (long long)blockIdx.y * C, *rg = rstd + (long long)blockIdx.y * C, *sg = gsum + (long long)blockIdx.y * 2 * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % CV) * 4;
        const f32x4 ga = ld4(gamma + ch), rs = ld4(rg + ch);
        const f32x4 m2 = ld4(sg + ch) * inv_n, m1 = ld4(sg + C + ch) * inv_n;
        const f32x4 xh = xhat_of(ld4(c + off + i * 4), ld4(mg + ch), rs);
        const f32x4 dz = gate(ld4(dy + off + i * 4), z_of(xh, ga, ld4(beta + ch)), act);
        st4(dc + off + i * 4, (ga * rs) * ((dz - m1) - xh * m2));
    }
}

static inline int grid_for(long long total) {
    const long long g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

static inline bool quad_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p % 16) return false;
    return true;
}

static inline int quad_shift(int C) {               // log2 of the smallest power of two >= min(C / 4, 64)
    int qsh = 0;
    while ((1 << qsh) < C / 4 && qsh < 6) ++qsh;
    return qsh;
}

static inline bool act_known(int act) { return act == NPS_ACT_NONE || act == NPS_ACT_RELU || act == NPS_ACT_LEAKY; }

// the argument checks the entry points share: true, or false with the error set
static bool dims_ok(const char* who, int G, int64_t n, int C) {
    if (!(G >= 1 && G <= NPS_BN_GROUPED_MAX_GROUPS && n >= 1 && C >= 4)) {
        nps::set_error("%s: bad arguments G=%d n=%lld C=%d", who, G, (long long)n, C);
        return false;
    }
    if (C % 4) {
        nps::set_error("%s: C = %d must be a multiple of 4", who, C);
        return false;
    }
    if (n * G >= (1ll << 30) || (n + RPS - 1) / RPS >= 65536 || C > (1 << 20)) {
        nps::set_error("%s: %lld rows x %d channels are more than the kernels index", who, (long long)n * G, C);
        return false;
    }
    return true;
}

}  // namespace bng
}  // namespace nps

using namespace nps::bng;

extern "C" int nopesac_bn_train_grouped_workspace_floats(int G, int64_t n, int C, int64_t* floats) {
    NPS_CHECK_ARG(floats, "bn_train_grouped_workspace_floats: null pointer");
    *floats = 0;
    if (!dims_ok("bn_train_grouped_workspace_floats", G, n, C)) return NPS_E_ARG;
    *floats = NPS_BN_GROUPED_WORKSPACE_FLOATS(G, n, C);
    return 0;
}

extern "C" int nopesac_bn_train_grouped_stats_f32(const float* c, int G, int64_t n, int C, float eps, float momentum, float* mean, float* var,
                                                  float* rstd, float* running_mean, float* running_var, float* ws, int64_t ws_floats,
                                                  void* stream) {
    if (!dims_ok("bn_train_grouped_stats", G, n, C)) return NPS_E_ARG;
    NPS_CHECK_ARG(c && mean && var && rstd && ws, "bn_train_grouped_stats: null pointer");
    NPS_CHECK_ARG(quad_aligned({c, ws}), "bn_train_grouped_stats: c and ws must be 16-byte aligned");
    NPS_CHECK_ARG(n >= 2, "bn_train_grouped_stats: batch statistics need more than one value per channel and group (n = %lld)", (long long)n);
    NPS_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "bn_train_grouped_stats: eps / momentum out of range");
    NPS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn_train_grouped_stats: running_mean and running_var come together");
    NPS_CHECK_ARG(ws_floats >= NPS_BN_GROUPED_WORKSPACE_FLOATS(G, n, C), "bn_train_grouped_stats: workspace too small");
    const int S = (int)((n + RPS - 1) / RPS), qsh = quad_shift(C);
    hipStream_t st = (hipStream_t)stream;
    stats_kernel<<<dim3((C / 4 + (1 << qsh) - 1) >> qsh, S, G), 256, 0, st>>>(c, n, C, qsh, ws);
    finish_kernel<<<(C + 15) / 16, 256, 0, st>>>(ws, S, n, C, G, eps, momentum, mean, var, rstd, running_mean, running_var);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_bn_train_grouped_apply_f32(const float* c, int G, int64_t n, int C, const float* gamma, const float* beta,
                                                  const float* mean, const float* rstd, int act, float* y, void* stream) {
    if (!dims_ok("bn_train_grouped_apply", G, n, C)) return NPS_E_ARG;
    NPS_CHECK_ARG(c && gamma && beta && mean && rstd && y, "bn_train_grouped_apply: null pointer");
    NPS_CHECK_ARG(quad_aligned({c, gamma, beta, mean, rstd, y}), "bn_train_grouped_apply: every pointer must be 16-byte aligned");
    NPS_CHECK_ARG(act_known(act), "bn_train_grouped_apply: bad act %d", act);
    apply_kernel<<<dim3(grid_for(n * (C / 4)), G), 256, 0, (hipStream_t)stream>>>(c, n, C, gamma, beta, mean, rstd, act, y);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_bn_train_grouped_backward_f32(const float* dy, const float* c, int G, int64_t n, int C, const float* gamma,
                                                     const float* beta, const float* mean, const float* rstd, int act, int batch_stats,
                                                     float* dc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream) {
    if (!dims_ok("bn_train_grouped_backward", G, n, C)) return NPS_E_ARG;
    NPS_CHECK_ARG(dy && c && gamma && beta && mean && rstd && dc && dgamma && dbeta && ws, "bn_train_grouped_backward: null pointer");
    NPS_CHECK_ARG(quad_aligned({dy, c, gamma, beta, mean, rstd, dc, dgamma, dbeta, ws}),
                  "bn_train_grouped_backward: every pointer must be 16-byte aligned");
    NPS_CHECK_ARG(act_known(act), "bn_train_grouped_backward: bad act %d", act);
    NPS_CHECK_ARG(ws_floats >= NPS_BN_GROUPED_WORKSPACE_FLOATS(G, n, C), "bn_train_grouped_backward: workspace too small");
    const int S = (int)((n + RPS - 1) / RPS), qsh = quad_shift(C);
    const float inv_n = batch_stats ? 1.f / (float)n : 0.f;
    float* gsum = ws + (long long)G * S * 2 * C;                  // [G][2][C] behind the blocks' partials
    hipStream_t st = (hipStream_t)stream;
    bwd_reduce_kernel<<<dim3((C / 4 + (1 << qsh) - 1) >> qsh, S, G), 256, 0, st>>>(dy, c, n, C, qsh, gamma, beta, mean, rstd, act, ws);
    bwd_sum_kernel<<<(2 * C + 15) / 16, 256, 0, st>>>(ws, S, C, G, gsum, dgamma, dbeta);
    bwd_apply_kernel<<<dim3(grid_for(n * (C / 4)), G), 256, 0, st>>>(dy, c, n, C, gamma, beta, mean, rstd, gsum, act, inv_n, dc);
    NPS_LAUNCH_RET();
}
