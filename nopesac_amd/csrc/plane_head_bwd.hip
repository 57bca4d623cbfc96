// Backward kernels of the plane head's instance heads (training.PlaneInstanceHeadsTrainer; reference planeTR_net/planeTR_head.py:140-192):
// the two f32 products of the folded mask logits
//     M[l,b,q,p] = sum_k F[l,b,q,k] p1[b,p,k] + beta[l,b,q]            (F = E W_pe, beta = E . b_pe; modeling/plane_head.py pe_fold)
// with the 256 -> 2 pixel-centre conv Z[b,c,p] = sum_k Wc[c,k] p1[b,p,k] + bc[c] joined as two more rows per image whose weights are
// shared by the batch, and the sigmoid's derivative.
//   wgrad: dF[l,b,q,k] = sum_p dM[l,b,q,p] p1[b,p,k], dbeta[l,b,q] = sum_p dM[l,b,q,p]; dWc[c,k] = sum_b sum_p dZ[b,c,p] p1[b,p,k], dbc likewise
//   dgrad: dp1[b,p,k]  = sum_{l,q} dM[l,b,q,p] F[l,b,q,k] + sum_c dZ[b,c,p] Wc[c,k]
// Both are per-image GEMMs on v_mfma_f32_32x32x2f32 (exact f32) with a 128 x 256 tile per workgroup: four waves, each 128 x 64 = 4 x 2
// MFMA tiles, operands staged through LDS as As[k][128] / Bs[k][256].  dM is pixel-minor ([L*B][nq][h*w], what the criterion's backward
// returns), p1 pixel-dense NHWC with a channel stride.  Every global load is unconditional from a clamped address and the value is
// selected afterwards; every store lies inside the counted range.  f32 throughout, deterministic: no atomics - the wgrad's pixel
// ranges write partial tiles into the caller's workspace and mask_wgrad_reduce_kernel sums them in split order (the shared rows in
// image order, split order inside an image).  Gated per element against float64 (tests/test_plane_heads_forms_gpu.py).
#include "common.h"

namespace nps {

typedef float mp_f32x4 __attribute__((ext_vector_type(4)));
typedef float mp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int MP_BM = 128, MP_BN = 256;          // workgroup tile: 128 GEMM rows x all 256 channels
constexpr int MP_LDA = MP_BM + 4, MP_LDB = MP_BN + 4;
constexpr int MP_WK = 32;                        // wgrad: pixels per LDS stage
constexpr int MP_DK = 16;                        // dgrad: rows of dM per LDS stage
constexpr int MP_EXTRA = 2;                      // the pixel-centre rows

// row r of image b of the stacked left operand: r < LQ -> dM[(l B + b) nq + q] (l = r / nq, q = r % nq), else the centre row r - LQ
__device__ __forceinline__ const float* mp_row(const float* __restrict__ dM, const float* __restrict__ dZ, int r, int b, int B, int nq, int LQ,
                                               long long HW) {
    const int l = r / nq, q = r - l * nq;
    const float* m = dM + (((long long)l * B + b) * nq + q) * HW;
    const float* z = dZ + ((long long)b * MP_EXTRA + (r - LQ)) * HW;
    return r < LQ ? m : z;
}

// BK k-steps of the 128 x 256 tile: wave `wave` owns columns 64 wave .. 64 wave + 63
template <int BK>
__device__ __forceinline__ void mp_mma(const float* As, const float* Bs, mp_f32x16 (&acc)[4][2], int lane, int wave) {
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
        const int k = kk + (lane >> 5);
        float af[4], bf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = As[k * MP_LDA + i * 32 + (lane & 31)];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = Bs[k * MP_LDB + wave * 64 + j * 32 + (lane & 31)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
}

__device__ __forceinline__ void mp_zero(mp_f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// ---- wgrad: grid (row tiles, B, splits).  Split z covers the pixels [z chunk, min((z + 1) chunk, HW)) (chunk a multiple of MP_WK) and
// writes its whole tile - zeros for an empty range - into wsF[z][b][R][256] and the row sums into wsB[z][b][R].
__global__ __launch_bounds__(256) void mask_wgrad_kernel(const float* __restrict__ dM, const float* __restrict__ dZ, const float* __restrict__ p1,
                                                         float* __restrict__ wsF, float* __restrict__ wsB, int B, int nq, int LQ, int R,
                                                         int HW, long long p1_ps, int chunk) {
    __shared__ __attribute__((aligned(16))) float As[MP_WK * MP_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[MP_WK * MP_LDB];
    const int b = blockIdx.y, z = blockIdx.z;
    const int r0 = blockIdx.x * MP_BM;
    const int p_begin = z * chunk < HW ? z * chunk : HW;
    const int p_end = p_begin + chunk < HW ? p_begin + chunk : HW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // A: thread -> row tid / 2, pixels 16 (tid % 2) .. + 15 of the stage;  B: thread -> channels 4 (tid % 64) .. + 3, pixels tid / 64 + 4 i
    const int arow = tid >> 1, ahalf = tid & 1;
    const bool arow_ok = r0 + arow < R;
    const float* asrc = mp_row(dM, dZ, arow_ok ? r0 + arow : R - 1, b, B, nq, LQ, HW);
    const int c4 = (tid & 63) * 4;
    const float* bsrc = p1 + (long long)b * HW * p1_ps + c4;

    mp_f32x16 acc[4][2];
    mp_zero(acc);
    float ra[16];
    mp_f32x4 rb[8];
    float bsum = 0.f;
    auto load = [&](int kc) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = kc + ahalf * 16 + j;
            const float v = asrc[p < HW ? p : HW - 1];
            ra[j] = (arow_ok && p < p_end) ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int p = kc + (tid >> 6) + 4 * i;
            const mp_f32x4 v = *(const mp_f32x4*)(bsrc + (long long)(p < HW ? p : HW - 1) * p1_ps);
            const mp_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            rb[i] = p < p_end ? v : zero;
        }
    };
    if (p_begin < p_end) load(p_begin);
    for (int kc = p_begin; kc < p_end; kc += MP_WK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            As[(ahalf * 16 + j) * MP_LDA + arow] = ra[j];
            bsum += ra[j];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) *(mp_f32x4*)(Bs + ((tid >> 6) + 4 * i) * MP_LDB + c4) = rb[i];
        __syncthreads();
        if (kc + MP_WK < p_end) load(kc + MP_WK);
        mp_mma<MP_WK>(As, Bs, acc, lane, wave);
    }
    // D[row][col]: lane l, register r -> row 8 (r / 4) + 4 (l / 32) + r % 4, col l % 32
    float* out = wsF + ((long long)z * B + b) * R * MP_BN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wave * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (row < R) out[(long long)row * MP_BN + col] = acc[i][j][r];
            }
        }
    // the row sums: the two pixel halves of a row in order
    __syncthreads();
    As[ahalf * MP_BM + arow] = bsum;
    __syncthreads();
    if (tid < MP_BM && r0 + tid < R) wsB[((long long)z * B + b) * R + r0 + tid] = As[tid] + As[MP_BM + tid];
}

// ---- the fixed-order sums of the partial tiles: one thread per output element
__global__ __launch_bounds__(256) void mask_wgrad_reduce_kernel(const float* __restrict__ wsF, const float* __restrict__ wsB, int B, int nq, int LQ,
                                                                int R, int splits, float* __restrict__ dF, long long dF_ld,
                                                                float* __restrict__ dbeta, long long dbeta_st, float* __restrict__ dWc,
                                                                float* __restrict__ dbc) {
    const long long nF = (long long)B * LQ * MP_BN, nb = (long long)B * LQ;
    const long long nW = R > LQ ? (long long)MP_EXTRA * MP_BN : 0, nc = R > LQ ? MP_EXTRA : 0;
    const long long total = nF + nb + nW + nc;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < nF) {                                   // dF, in output order (l, b, q, k)
            const int k = (int)(i % MP_BN);
            const long long row = i / MP_BN;
            const int q = (int)(row % nq), b = (int)((row / nq) % B), l = (int)(row / ((long long)nq * B));
            float s = 0.f;
            for (int z = 0; z < splits; ++z) s += wsF[(((long long)z * B + b) * R + l * nq + q) * MP_BN + k];
            dF[row * dF_ld + k] = s;
        } else if (i < nF + nb) {                       // dbeta (l, b, q)
            const long long row = i - nF;
            const int q = (int)(row % nq), b = (int)((row / nq) % B), l = (int)(row / ((long long)nq * B));
            float s = 0.f;
            for (int z = 0; z < splits; ++z) s += wsB[((long long)z * B + b) * R + l * nq + q];
            dbeta[row * dbeta_st] = s;
        } else if (i < nF + nb + nW) {                  // the shared centre weights: images in order, splits in order inside an image
            const long long e = i - nF - nb;
            const int k = (int)(e % MP_BN), c = (int)(e / MP_BN);
            float s = 0.f;
            for (int b = 0; b < B; ++b)
                for (int z = 0; z < splits; ++z) s += wsF[(((long long)z * B + b) * R + LQ + c) * MP_BN + k];
            dWc[e] = s;
        } else {
            const int c = (int)(i - nF - nb - nW);
            float s = 0.f;
            for (int b = 0; b < B; ++b)
                for (int z = 0; z < splits; ++z) s += wsB[((long long)z * B + b) * R + LQ + c];
            dbc[c] = s;
        }
    }
}

// ---- dgrad: grid (pixel tiles of 128, B); the K loop runs over the R stacked rows of the image in stages of MP_DK (zeros beyond R)
__global__ __launch_bounds__(256) void mask_dgrad_kernel(const float* __restrict__ dM, const float* __restrict__ dZ, const float* __restrict__ F,
                                                         long long F_ld, const float* __restrict__ Wc, float* __restrict__ dp1, int B, int nq,
                                                         int LQ, int R, int HW, long long dp1_ps) {
    __shared__ __attribute__((aligned(16))) float As[MP_DK * MP_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[MP_DK * MP_LDB];
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * MP_BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // A: thread -> pixel tid % 128, rows tid / 128 + 2 i of the stage;  B: thread -> channels 4 (tid % 64) .. + 3, rows tid / 64 + 4 i
    const int apx = tid & 127;
    const bool apx_ok = p0 + apx < HW;
    const int ap = apx_ok ? p0 + apx : HW - 1;
    const int c4 = (tid & 63) * 4;

    mp_f32x16 acc[4][2];
    mp_zero(acc);
    float ra[8];
    mp_f32x4 rb[4];
    auto load = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = kc + (tid >> 7) + 2 * i;
            const float v = mp_row(dM, dZ, r < R ? r : R - 1, b, B, nq, LQ, HW)[ap];
            ra[i] = (apx_ok && r < R) ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = kc + (tid >> 6) + 4 * i;
            const int rc = r < R ? r : R - 1;
            const int l = rc / nq, q = rc - l * nq;
            const float* f = F + (((long long)l * B + b) * nq + q) * F_ld;
            const float* wc = Wc + (long long)(rc - LQ) * MP_BN;
            const mp_f32x4 v = *(const mp_f32x4*)((rc < LQ ? f : wc) + c4);
            const mp_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            rb[i] = r < R ? v : zero;
        }
    };
    load(0);
    for (int kc = 0; kc < R; kc += MP_DK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[((tid >> 7) + 2 * i) * MP_LDA + apx] = ra[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *(mp_f32x4*)(Bs + ((tid >> 6) + 4 * i) * MP_LDB + c4) = rb[i];
        __syncthreads();
        if (kc + MP_DK < R) load(kc + MP_DK);
        mp_mma<MP_DK>(As, Bs, acc, lane, wave);
    }
    float* out = dp1 + (long long)b * HW * dp1_ps;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wave * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (p < HW) out[(long long)p * dp1_ps + col] = acc[i][j][r];
            }
        }
}

// ---- out = g y (1 - y) for the output y of a sigmoid and its gradient g
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y, long long n,
                                                          float* __restrict__ out) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = y[i];
        out[i] = g[i] * (v * (1.f - v));
    }
}

static int mp_grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

static bool mp_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace nps

#define MP_CHECK_DIMS(name)                                                                                                          \
    NPS_CHECK_ARG(C == 256, name ": C = %d (the kernels are specialised to 256 channels)", C);                                       \
    NPS_CHECK_ARG(nq >= 1 && nq <= 128, name ": nq = %d not in [1, 128]", nq);                                                       \
    NPS_CHECK_ARG(L >= 1 && L <= 3, name ": L = %d not in [1, 3]", L);                                                               \
    NPS_CHECK_ARG(B >= 1 && B < 65536 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 30), name ": bad dims B=%d h=%d w=%d", B, h, w)

static_assert(NPS_MASK_PRODUCT_WS_ROW_FLOATS == nps::MP_BN + 1, "workspace row: 256 partial sums + the row sum");

extern "C" int64_t nopesac_mask_product_wgrad_workspace_floats(int L, int B, int nq, int center_rows, int splits) {
    return L >= 0 && B >= 0 && nq >= 0 && center_rows >= 0 && splits >= 0 ? NPS_MASK_PRODUCT_WGRAD_WORKSPACE_FLOATS(L, B, nq, center_rows, splits) : 0;
}

extern "C" int nopesac_mask_product_wgrad_f32(const float* d_logits, const float* d_center, const float* p1, float* d_fold, int64_t d_fold_ld,
                                              float* d_beta, int64_t d_beta_stride, float* d_wc, float* d_bc, float* ws, int64_t ws_floats,
                                              int L, int B, int nq, int h, int w, int C, int64_t p1_pstride, int64_t p1_bstride, int splits,
                                              void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(d_logits && p1 && d_fold && d_beta && ws, "mask_product_wgrad: null pointer");
    NPS_CHECK_ARG((d_center != nullptr) == (d_wc != nullptr) && (d_center != nullptr) == (d_bc != nullptr),
                  "mask_product_wgrad: d_center, d_wc and d_bc go together");
    MP_CHECK_DIMS("mask_product_wgrad");
    const int HW = h * w, LQ = L * nq, R = LQ + (d_center ? MP_EXTRA : 0);
    NPS_CHECK_ARG(p1_pstride >= C && p1_pstride % 4 == 0 && p1_bstride == (int64_t)HW * p1_pstride && mp_aligned16(p1),
                  "mask_product_wgrad: p1 must be pixel-dense NHWC, channel stride >= 256 and %% 4 == 0, 16-byte aligned");
    NPS_CHECK_ARG(d_fold_ld >= C && d_beta_stride >= 1, "mask_product_wgrad: d_fold_ld %lld / d_beta_stride %lld", (long long)d_fold_ld,
                  (long long)d_beta_stride);
    NPS_CHECK_ARG(splits >= 1 && splits <= 1024, "mask_product_wgrad: splits %d not in [1, 1024]", splits);
    NPS_CHECK_ARG(ws_floats >= nopesac_mask_product_wgrad_workspace_floats(L, B, nq, R - LQ, splits), "mask_product_wgrad: workspace too small");
    int chunk = (HW + splits - 1) / splits;
    chunk = (chunk + MP_WK - 1) / MP_WK * MP_WK;                // split boundaries on LDS-stage boundaries
    float* wsF = ws;
    float* wsB = ws + (long long)splits * B * R * MP_BN;
    hipStream_t st = (hipStream_t)stream;
    mask_wgrad_kernel<<<dim3((R + MP_BM - 1) / MP_BM, B, splits), 256, 0, st>>>(d_logits, d_center ? d_center : d_logits, p1, wsF, wsB, B, nq, LQ, R,
                                                                                  HW, p1_pstride, chunk);
    mask_wgrad_reduce_kernel<<<mp_grid_for((long long)B * LQ * (MP_BN + 1) + MP_EXTRA * (MP_BN + 1)), 256, 0, st>>>(
        wsF, wsB, B, nq, LQ, R, splits, d_fold, d_fold_ld, d_beta, d_beta_stride, d_wc, d_bc);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_mask_product_dgrad_f32(const float* d_logits, const float* d_center, const float* fold, int64_t fold_ld, const float* wc,
                                              float* d_p1, int L, int B, int nq, int h, int w, int C, int64_t dp1_pstride, int64_t dp1_bstride,
                                              void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(d_logits && fold && d_p1, "mask_product_dgrad: null pointer");
    NPS_CHECK_ARG((d_center != nullptr) == (wc != nullptr), "mask_product_dgrad: d_center and wc go together");
    MP_CHECK_DIMS("mask_product_dgrad");
    const int HW = h * w, LQ = L * nq, R = LQ + (d_center ? MP_EXTRA : 0);
    NPS_CHECK_ARG(dp1_pstride >= C && dp1_bstride == (int64_t)HW * dp1_pstride,
                  "mask_product_dgrad: d_p1 must be pixel-dense NHWC with a channel stride >= 256");
    NPS_CHECK_ARG(fold_ld >= C && fold_ld % 4 == 0 && mp_aligned16(fold) && (!wc || mp_aligned16(wc)),
                  "mask_product_dgrad: fold rows (stride %lld) and wc must be 16-byte aligned", (long long)fold_ld);
    mask_dgrad_kernel<<<dim3((HW + MP_BM - 1) / MP_BM, B), 256, 0, (hipStream_t)stream>>>(d_logits, d_center ? d_center : d_logits, fold, fold_ld,
                                                                                         wc ? wc : fold, d_p1, B, nq, LQ, R, HW, dp1_pstride);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_sigmoid_backward_f32(const float* g, const float* y, int64_t n, float* out, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(g && y && out, "sigmoid_backward: null pointer");
    NPS_CHECK_ARG(n > 0, "sigmoid_backward: n = %lld", (long long)n);
    sigmoid_bwd_kernel<<<mp_grid_for(n), 256, 0, (hipStream_t)stream>>>(g, y, n, out);
    NPS_LAUNCH_RET();
}
