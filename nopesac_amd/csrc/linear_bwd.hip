// Backward of a Linear layer y = act(x W^T + b) with every operand read in place (training._LinearInPlace; PlaneEncoderTrainer):
//   dx [M][K] = g' W,   dW [N][K] = g'^T x,   db [N] = column sums of g',
// where g' is the gradient g [M][N] at the layer's output behind two optional gates applied AS THE TILES ARE LOADED: the ReLU of the
// saved output (y > 0) and the counter-based dropout of csrc/dropout.h at the row-major index m * N + n, times 1 / (1 - p).  No launch
// writes a transposed or gated copy of x, g or y.  Exact-f32 MFMA (v_mfma_f32_32x32x2f32), LDS-staged 128 x 128 tiles, f32 throughout.
//   dgrad: rows = M, columns = K, reduction over N.  g' is reduction-minor, so its tile is staged row-major [m][n]; W [N][K] is staged as
//          it lies.
//   wgrad: rows = N, columns = K, reduction over M, both operands M-major (conv_bwd.hip's wgrad_kernel): blockIdx.z = a range of rows of
//          M, each range writes its whole tile (zeros for an empty range) into ws[split][N][K]; the workgroups of the first column tile
//          also sum their g' tiles over the rows into ws[splits N K + split N + n].  linear_bwd_reduce_kernel sums the splits in order.
// Deterministic: no atomics.  Every global load comes from a clamped address with a select behind it; every store is bounds-checked.
#include "common.h"
#include "dropout.h"

namespace nps {

typedef float lb_f32x4 __attribute__((ext_vector_type(4)));
typedef float lb_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LB_BM = NPS_LINEAR_BWD_TILE, LB_BN = NPS_LINEAR_BWD_TILE, LB_BK = NPS_LINEAR_BWD_STAGE;
constexpr int LB_LD = LB_BM + 4;          // row pitch of a reduction-major stage [LB_BK][128]
constexpr int LB_LDA = LB_BK + 4;         // row pitch of dgrad's row-major g' stage [128][LB_BK]
static_assert(LB_BM == 128 && LB_BK == 16, "the thread mappings below are written for 128 x 128 tiles and 16-deep stages");

struct LinGate {
    const float* y;        // the Linear's saved output (ReLU gate), or null
    long long y_stride;
    uint64_t key;          // dropout_key(seed, stream)
    uint32_t threshold;    // floor(p 2^32); 0 = no dropout (the hash is skipped)
    float inv_keep;        // (float)(1 / (1 - p))
};

// g'[m][n .. n + 3] for in-range (m, n) given as clamped coordinates; `live` selects between the loaded value and zero.
__device__ __forceinline__ lb_f32x4 lb_gated(const float* __restrict__ g, long long g_stride, const LinGate& gate, long long m, int n, int N,
                                             bool live) {
    lb_f32x4 v = *(const lb_f32x4*)(g + m * g_stride + n);
    if (gate.y) {
        const lb_f32x4 yv = *(const lb_f32x4*)(gate.y + m * gate.y_stride + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = yv[j] > 0.f ? v[j] : 0.f;
    }
    if (gate.threshold != 0u) {
        const long long idx = m * (long long)N + n;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = dropout_keep_keyed(gate.key, idx + j, gate.threshold) ? v[j] * gate.inv_keep : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = live ? v[j] : 0.f;
    return v;
}

__device__ __forceinline__ void lb_zero(lb_f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// ---- dgrad: dx[m][k] = sum_n g'[m][n] W[n][k].  grid = (K tiles, M tiles).
__global__ __launch_bounds__(256) void linear_dgrad_kernel(const float* __restrict__ g, long long g_stride, LinGate gate,
                                                           const float* __restrict__ w, float* __restrict__ dx, long long dx_stride,
                                                           long long M, int K, int N) {
    __shared__ __attribute__((aligned(16))) float As[LB_BM * LB_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[LB_BK * LB_LD];
    const long long m0 = (long long)blockIdx.y * LB_BM;
    const int k0 = blockIdx.x * LB_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // A stage: 128 rows x 16 reduction columns = 512 float4, two per thread: row tid / 4 + 64 i, reduction column (tid % 4) * 4
    const int an = (tid & 3) * 4;
    // B stage: 16 reduction rows x 128 columns, two per thread: reduction row tid / 32 + 8 i, column (tid % 32) * 4
    const int bc = (tid & 31) * 4;
    const bool bc_ok = k0 + bc < K;
    const int bcc = bc_ok ? k0 + bc : K - 4;

    lb_f32x16 acc[2][2];
    lb_zero(acc);
    lb_f32x4 ra[2], rb[2];
    auto load = [&](int nc) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long m = m0 + (tid >> 2) + 64 * i;
            const int n = nc + an;
            const bool a_ok = m < M && n < N;
            ra[i] = lb_gated(g, g_stride, gate, m < M ? m : M - 1, n < N ? n : N - 4, N, a_ok);
            const int nr = nc + (tid >> 5) + 8 * i;
            const bool b_ok = bc_ok && nr < N;
            const lb_f32x4 wv = *(const lb_f32x4*)(w + (long long)(nr < N ? nr : N - 1) * K + bcc);
#pragma unroll
            for (int j = 0; j < 4; ++j) rb[i][j] = b_ok ? wv[j] : 0.f;
        }
    };
    load(0);
    for (int nc = 0; nc < N; nc += LB_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(lb_f32x4*)(As + ((tid >> 2) + 64 * i) * LB_LDA + an) = ra[i];
            *(lb_f32x4*)(Bs + ((tid >> 5) + 8 * i) * LB_LD + bc) = rb[i];
        }
        __syncthreads();
        if (nc + LB_BK < N) load(nc + LB_BK);
#pragma unroll
        for (int kk = 0; kk < LB_BK; kk += 2) {
            const int k = kk + (lane >> 5);
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[(wm * 64 + i * 32 + (lane & 31)) * LB_LDA + k];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[k * LB_LD + wn * 64 + j * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // D[row][col]: lane l, register r -> row 8 (r / 4) + 4 (l / 32) + r % 4, col l % 32
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + wn * 64 + j * 32 + (lane & 31);
            if (k >= K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (m < M) dx[m * dx_stride + k] = acc[i][j][r];
            }
        }
}

// ---- wgrad (+ the bias partials): ws[z][n][k] = sum over the rows m of range z of g'[m][n] x[m][k].  grid = (K tiles, N tiles, splits);
// do_dw == 0: only the bias partials are wanted (grid.x == 1, x is not read, no tile is written).
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ g, long long g_stride, LinGate gate,
                                                           const float* __restrict__ x, long long x_stride, float* __restrict__ ws,
                                                           float* __restrict__ ws_db, long long M, int K, int N, long long chunk, int do_dw) {
    __shared__ __attribute__((aligned(16))) float As[LB_BK * LB_LD];
    __shared__ __attribute__((aligned(16))) float Bs[LB_BK * LB_LD];
    const int n0 = blockIdx.y * LB_BM, k0 = blockIdx.x * LB_BN;
    const long long p_begin = (long long)blockIdx.z * chunk;
    const long long p_end = p_begin + chunk < M ? p_begin + chunk : M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // global -> LDS mapping: 16 rows of M x 128 columns per operand = 512 float4, two per thread: row tid / 32 + 8 i, column (tid % 32) * 4
    const int c4 = (tid & 31) * 4;
    const bool na_ok = n0 + c4 < N;
    const int na = na_ok ? n0 + c4 : N - 4;
    const bool kb_ok = do_dw && k0 + c4 < K;
    const int kb = k0 + c4 < K ? k0 + c4 : K - 4;
    const bool bias = ws_db != nullptr && blockIdx.x == 0;

    lb_f32x16 acc[2][2];
    lb_zero(acc);
    lb_f32x4 colsum = {0.f, 0.f, 0.f, 0.f};
    lb_f32x4 ra[2], rb[2];
    auto load = [&](long long pc) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long p = pc + (tid >> 5) + 8 * i;
            const bool live = p < p_end;
            const long long pm = live ? p : M - 1;
            ra[i] = lb_gated(g, g_stride, gate, pm, na, N, live && na_ok);
            lb_f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (do_dw) {                                            // (wave-uniform: x may be null otherwise)
                const lb_f32x4 xv = *(const lb_f32x4*)(x + pm * x_stride + kb);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = live && kb_ok ? xv[j] : 0.f;
            }
            rb[i] = b;
        }
    };
    if (p_begin < p_end) load(p_begin);
    for (long long pc = p_begin; pc < p_end; pc += LB_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (tid >> 5) + 8 * i;
            *(lb_f32x4*)(As + r * LB_LD + c4) = ra[i];
            *(lb_f32x4*)(Bs + r * LB_LD + c4) = rb[i];
            colsum += ra[i];
        }
        __syncthreads();
        if (pc + LB_BK < p_end) load(pc + LB_BK);
        if (!do_dw) continue;
#pragma unroll
        for (int kk = 0; kk < LB_BK; kk += 2) {
            const int k = kk + (lane >> 5);
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[k * LB_LD + wm * 64 + i * 32 + (lane & 31)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[k * LB_LD + wn * 64 + j * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    if (do_dw) {
        float* out = ws + (long long)blockIdx.z * N * K;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + wn * 64 + j * 32 + (lane & 31);
                if (k >= K) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                    if (n < N) out[(long long)n * K + k] = acc[i][j][r];
                }
            }
    }
    if (bias) {                                                     // (block-uniform) the eight row groups of a column, summed in order
        __syncthreads();
        *(lb_f32x4*)(As + (tid >> 5) * LB_LD + c4) = colsum;
        __syncthreads();
        if (tid < LB_BM && n0 + tid < N) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) s += As[r * LB_LD + tid];
            ws_db[(long long)blockIdx.z * N + n0 + tid] = s;
        }
    }
}

// ---- the splits summed in order: dw[i] = sum_z ws[z][i] (i < N K, when dw is not null), db[n] = sum_z ws_db[z][n] (when db is not null)
__global__ __launch_bounds__(256) void linear_bwd_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ ws_db,
                                                                float* __restrict__ dw, float* __restrict__ db, long long NK, int N, int splits) {
    const long long n_dw = dw ? NK : 0, total = n_dw + (db ? N : 0);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float s = 0.f;
        if (i < n_dw) {
            for (int z = 0; z < splits; ++z) s += ws[(long long)z * NK + i];
            dw[i] = s;
        } else {
            const long long n = i - n_dw;
            for (int z = 0; z < splits; ++z) s += ws_db[(long long)z * N + n];
            db[n] = s;
        }
    }
}

}  // namespace nps

extern "C" int64_t nopesac_linear_backward_workspace_floats(int N, int K, int splits) {
    return N >= 0 && K >= 0 && splits >= 0 ? NPS_LINEAR_BWD_WORKSPACE_FLOATS(N, K, splits) : 0;
}

extern "C" int nopesac_linear_backward_f32(const float* x, int64_t x_stride, const float* w, const float* g, int64_t g_stride, const float* y,
                                           int64_t y_stride, double p, int64_t seed, int64_t stream_id, float* dx, int64_t dx_stride,
                                           float* dw, float* db, float* ws, int64_t ws_floats, int64_t M, int K, int N, int splits,
                                           void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(p >= 0.0 && p < 1.0, "linear_backward: p = %g is not in [0, 1)", p);
    NPS_CHECK_ARG(g != nullptr && (dx || dw || db), "linear_backward: null gradient, or no output asked for");
    NPS_CHECK_ARG(M > 0 && M < (1ll << 31) && K > 0 && N > 0 && K % 4 == 0 && N % 4 == 0 && K <= (1 << 20) && N <= (1 << 20),
                  "linear_backward: bad dims M=%lld K=%d N=%d (M in 1 .. 2^31 - 1; K, N multiples of 4 up to 2^20)", (long long)M, K, N);
    NPS_CHECK_ARG(g_stride >= N && g_stride % 4 == 0 && (uintptr_t)g % 16 == 0, "linear_backward: g needs a row stride >= N that is a multiple of 4 and 16-byte alignment");
    NPS_CHECK_ARG(!y || (y_stride >= N && y_stride % 4 == 0 && (uintptr_t)y % 16 == 0), "linear_backward: y needs a row stride >= N that is a multiple of 4 and 16-byte alignment");
    NPS_CHECK_ARG(!dx || (w && dx_stride >= K && dx_stride % 4 == 0 && (uintptr_t)w % 16 == 0),
                  "linear_backward: dx needs w (16-byte aligned) and a row stride >= K that is a multiple of 4");
    NPS_CHECK_ARG(!dw || (x && x_stride >= K && x_stride % 4 == 0 && (uintptr_t)x % 16 == 0),
                  "linear_backward: dw needs x with a row stride >= K that is a multiple of 4 and 16-byte alignment");
    NPS_CHECK_ARG(splits >= 1 && splits <= 1024, "linear_backward: splits %d not in [1, 1024]", splits);
    LinGate gate;
    gate.y = y;
    gate.y_stride = y_stride;
    gate.key = dropout_key(seed, stream_id);
    gate.threshold = (uint32_t)(uint64_t)(p * 4294967296.0);
    gate.inv_keep = (float)(1.0 / (1.0 - p));
    hipStream_t st = (hipStream_t)stream;
    const unsigned mt = (unsigned)((M + LB_BM - 1) / LB_BM), kt = (unsigned)((K + LB_BN - 1) / LB_BN), nt = (unsigned)((N + LB_BM - 1) / LB_BM);
    if (dw || db) {
        NPS_CHECK_ARG(ws && ws_floats >= nopesac_linear_backward_workspace_floats(N, K, splits), "linear_backward: workspace too small (%lld floats, %lld needed)",
                      (long long)ws_floats, (long long)nopesac_linear_backward_workspace_floats(N, K, splits));
    }
    if (dx) {
        NPS_CHECK_ARG(mt <= 65535u, "linear_backward: M = %lld needs more than 65535 row tiles", (long long)M);
        linear_dgrad_kernel<<<dim3(kt, mt), 256, 0, st>>>(g, (long long)g_stride, gate, w, dx, (long long)dx_stride, (long long)M, K, N);
    }
    if (dw || db) {
        long long chunk = (M + splits - 1) / splits;
        chunk = (chunk + LB_BK - 1) / LB_BK * LB_BK;               // range boundaries on LDS-stage boundaries
        const long long NK = (long long)N * K;
        float* ws_db = db ? ws + (long long)splits * NK : nullptr;
        linear_wgrad_kernel<<<dim3(dw ? kt : 1u, nt, (unsigned)splits), 256, 0, st>>>(g, (long long)g_stride, gate, x, (long long)x_stride, ws, ws_db,
                                                                                      (long long)M, K, N, chunk, dw ? 1 : 0);
        const long long total = (dw ? NK : 0) + (db ? N : 0);
        const long long blocks = (total + 255) / 256;
        linear_bwd_reduce_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, st>>>(ws, ws_db, dw, db, NK, N, splits);
    }
    NPS_LAUNCH_RET();
}
