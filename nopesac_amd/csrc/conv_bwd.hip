// Backward kernels of the pixel pose net's conv stacks (training.CameraHeadTrainer with conv_stacks=True; reference
// __forward_PixelCameraHead, camera_net/camera_head.py:642-683): conv dgrad / wgrad, inference-mode BatchNorm + (Leaky)ReLU, GroupNorm,
// 2x2 max-pool, nearest 2x upsample-add and the correlation softmax.  f32 throughout, NHWC activations, caller-allocated buffers.
// Deterministic: no atomics; every cross-workgroup sum is written as partials and reduced in a fixed order.
// Gated against float64 torch.autograd (tests/test_conv_backward_gpu.py, tests/test_pose_net_training_gpu.py); the stride-1 dgrad - the
// weight rotation bit for bit, then the f32 conv kernel per element - also by tests/test_conv_f32_forms_gpu.py (tests/conv_f32_forms.py).
#include "common.h"

namespace nps {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- dgrad operand: w [Cout][Cin][KH][KW] (state-dict layout) -> wf [Cin][KH][KW][Cout], taps rotated by 180 degrees, so that the
// input gradient of a stride-1 conv is the forward conv of dY with wf and padding KH - 1 - pad.
__global__ __launch_bounds__(256) void dgrad_weight_kernel(const float* __restrict__ w, float* __restrict__ wf, int Cout, int Cin, int KH,
                                                           int KW) {
    const long long n = (long long)Cout * Cin * KH * KW;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int co = (int)(i % Cout);
        long long r = i / Cout;
        const int kw = (int)(r % KW); r /= KW;
        const int kh = (int)(r % KH);
        const int ci = (int)(r / KH);
        wf[i] = w[(((long long)co * Cin + ci) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)];
    }
}

// ---- dgrad of a strided conv (the pose branches' stride-2 layers, <= 0.03 GFLOP per pair): one thread per input element gathers the
// taps whose output position is integral: (ih + pad - kh) % stride == 0.
__global__ __launch_bounds__(256) void dgrad_gather_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                           int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                                           int OH, int OW, long long dy_cs, long long dx_cs) {
    const long long n = (long long)B * H * W * Cin;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        const long long px = i / Cin;
        const int iw = (int)(px % W), ih = (int)((px / W) % H), b = (int)(px / ((long long)H * W));
        float s = 0.f;
        for (int kh = 0; kh < KH; ++kh) {
            const int th = ih + pad - kh;
            if (th < 0 || th % stride) continue;
            const int oh = th / stride;
            if (oh >= OH) continue;
            for (int kw = 0; kw < KW; ++kw) {
                const int tw = iw + pad - kw;
                if (tw < 0 || tw % stride) continue;
                const int ow = tw / stride;
                if (ow >= OW) continue;
                const float* g = dy + (((long long)b * OH + oh) * OW + ow) * dy_cs;
                const float* wp = w + ((long long)ci * KH + kh) * KW + kw;
                const long long wst = (long long)Cin * KH * KW;
                for (int co = 0; co < Cout; ++co) s += g[co] * wp[co * wst];
            }
        }
        dx[px * dx_cs + ci] = s;
    }
}

// ---- wgrad: dW[co][n] = sum over output pixels p of dY[p][co] * X(p, tap)[ci], n = (kh * KW + kw) * Cin + ci.  GEMM with M = Cout,
// N = KH * KW * Cin, K = B * OH * OW, both operands K-major; 128 x 128 tile per workgroup (2 x 2 waves of 64 x 64 = 2 x 2 tiles of
// v_mfma_f32_32x32x2f32), 16 pixels per LDS stage, blockIdx.z = split of the pixel range.  Each split writes its whole tile (zeros for an
// empty range) into ws[split][Cout][N]; wgrad_reduce_kernel sums the splits in order and writes the state-dict layout.
constexpr int WG_BM = 128, WG_BN = 128, WG_BK = 16, WG_LD = WG_BM + 4;

__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ ws, int B,
                                                    int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW,
                                                    long long x_cs, long long dy_cs, int chunk) {
    __shared__ __attribute__((aligned(16))) float As[WG_BK * WG_LD];
    __shared__ __attribute__((aligned(16))) float Bs[WG_BK * WG_LD];
    const int N = KH * KW * Cin;
    const long long P = (long long)B * OH * OW;
    const int m0 = blockIdx.y * WG_BM, n0 = blockIdx.x * WG_BN;
    const long long p_begin = (long long)blockIdx.z * chunk;
    const long long p_end = p_begin + chunk < P ? p_begin + chunk : P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // global -> LDS mapping: 16 pixels x 128 columns per operand = 512 float4, two per thread: pixel r = tid / 32 + 8 i, column c4
    const int c4 = (tid & 31) * 4;
    // this thread's B column (fixed over the pixels): tap + channel
    const int nb = n0 + c4;
    const bool nb_ok = nb < N;
    const int tap = nb_ok ? nb / Cin : 0, ci = nb_ok ? nb - (nb / Cin) * Cin : 0;
    const int kh = tap / KW, kw = tap - (tap / KW) * KW;
    const bool ma_ok = m0 + c4 < Cout;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x4 ra[2], rb[2];
    auto load = [&](long long kc) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long p = kc + (tid >> 5) + 8 * i;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (p < p_end) {
                if (ma_ok) a = *(const f32x4*)(dy + p * dy_cs + m0 + c4);
                if (nb_ok) {
                    const int ow = (int)(p % OW);
                    const long long t = p / OW;
                    const int oh = (int)(t % OH), bi = (int)(t / OH);
                    const int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
                    if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                        b = *(const f32x4*)(x + (((long long)bi * H + ih) * W + iw) * x_cs + ci);
                }
            }
            ra[i] = a;
            rb[i] = b;
        }
    };
    if (p_begin < p_end) load(p_begin);
    for (long long kc = p_begin; kc < p_end; kc += WG_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (tid >> 5) + 8 * i;
            *(f32x4*)(As + r * WG_LD + c4) = ra[i];
            *(f32x4*)(Bs + r * WG_LD + c4) = rb[i];
        }
        __syncthreads();
        if (kc + WG_BK < p_end) load(kc + WG_BK);
#pragma unroll
        for (int kk = 0; kk < WG_BK; kk += 2) {
            const int k = kk + (lane >> 5);
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[k * WG_LD + wm * 64 + i * 32 + (lane & 31)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[k * WG_LD + wn * 64 + j * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // D[row][col]: lane l, register r -> row 8 (r / 4) + 4 (l / 32) + r % 4, col l % 32
    float* out = ws + (long long)blockIdx.z * Cout * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + (lane & 31);
            if (n >= N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (m < Cout) out[(long long)m * N + n] = acc[i][j][r];
            }
        }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Cout, int Cin, int KH,
                                                           int KW, int splits) {
    const int N = KH * KW * Cin;
    const long long total = (long long)Cout * N;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float s = 0.f;
        for (int z = 0; z < splits; ++z) s += ws[(long long)z * total + i];
        const int co = (int)(i / N), n = (int)(i % N);
        const int tap = n / Cin, ci = n % Cin;
        dw[((long long)co * Cin + ci) * KH * KW + tap] = s;
    }
}

// ---- per-channel partial sums [S][2][C] -> a[C], b[C] (fixed order over S)
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, int S, int C, float* __restrict__ a,
                                                           float* __restrict__ b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * C) return;
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += part[(long long)z * 2 * C + i];
    if (i < C) a[i] = s;
    else b[i - C] = s;
}

__device__ __forceinline__ float bn_scale(const float* gamma, const float* var, float eps, int c) { return gamma[c] / sqrtf(var[c] + eps); }

// ---- inference-mode BatchNorm + activation, forward: y = act(c * s + (beta - mean * s)), s = gamma / sqrt(var + eps)
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ c, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean,
                                                         const float* __restrict__ var, float eps, int act, long long n, int C,
                                                         float* __restrict__ y) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % C);
        const float s = bn_scale(gamma, var, eps, ch);
        y[i] = apply_act(c[i] * s + (beta[ch] - mean[ch] * s), act);
    }
}

// ---- ... backward: dZ = dY * act'(z) (z recomputed from the saved conv output c as in the forward), dC = dZ * s, and per split of
// BN_RPS rows the partials of dgamma = sum dZ (c - mean) / sqrt(var + eps), dbeta = sum dZ.  Block: 64 channels x 4 row lanes.
constexpr int BN_RPS = 256;

__global__ __launch_bounds__(256) void bn_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ c,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ var, float eps, int act,
                                                         int rows, int C, float* __restrict__ dc, float* __restrict__ part) {
    __shared__ float sg[4][64], sb[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int ch = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * BN_RPS, r1 = min(rows, r0 + BN_RPS);
    float ag = 0.f, ab = 0.f;
    if (ch < C) {
        const float rstd = 1.f / sqrtf(var[ch] + eps);
        const float s = bn_scale(gamma, var, eps, ch), mu = mean[ch], sh = beta[ch] - mu * s;
        const float neg = act == NPS_ACT_LEAKY ? 0.01f : 0.f;
        for (int r = r0 + rl; r < r1; r += 4) {
            const long long i = (long long)r * C + ch;
            const float cv = c[i];
            const float z = cv * s + sh;
            const float dz = act == NPS_ACT_NONE ? dy[i] : (z > 0.f ? dy[i] : neg * dy[i]);
            dc[i] = dz * s;
            ag += dz * ((cv - mu) * rstd);
            ab += dz;
        }
    }
    sg[rl][cl] = ag;
    sb[rl][cl] = ab;
    __syncthreads();
    if (rl == 0 && ch < C) {
        float* o = part + (long long)blockIdx.y * 2 * C;
        o[ch] = (sg[0][cl] + sg[1][cl]) + (sg[2][cl] + sg[3][cl]);
        o[C + ch] = (sb[0][cl] + sb[1][cl]) + (sb[2][cl] + sb[3][cl]);
    }
}

// ---- GroupNorm backward: one workgroup per (image, group); statistics recomputed from the saved input x (two passes, fixed order),
// optional ReLU mask from the recomputed output.  dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dz gamma; per-image partials
// of dgamma = sum dz xh, dbeta = sum dz into part[image][2][C].
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void gn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int HW, int C, int groups, float eps, int relu,
                                                     float* __restrict__ dx, float* __restrict__ part) {
    __shared__ float sh[4];
    __shared__ float pc[256][2];
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    const int cpg = C / groups;                                // divides 256 (checked by the entry point)
    const int cl = threadIdx.x % cpg, pl = threadIdx.x / cpg, pstep = 256 / cpg;
    const int ch = g * cpg + cl;
    const long long base = (long long)b * HW * C + ch;
    const float cnt = (float)HW * cpg;
    float s = 0.f;
    for (int p = pl; p < HW; p += pstep) s += x[base + (long long)p * C];
    const float mu = block_sum_256(s, sh) / cnt;
    float v = 0.f;
    for (int p = pl; p < HW; p += pstep) {
        const float d = x[base + (long long)p * C] - mu;
        v += d * d;
    }
    const float rstd = 1.f / sqrtf(block_sum_256(v, sh) / cnt + eps);
    const float ga = gamma[ch], be = beta[ch];
    float s_dz = 0.f, s_dzx = 0.f;
    for (int p = pl; p < HW; p += pstep) {
        const long long i = base + (long long)p * C;
        const float xh = (x[i] - mu) * rstd;
        const float dz = (!relu || xh * ga + be > 0.f) ? dy[i] : 0.f;
        s_dz += dz;
        s_dzx += dz * xh;
    }
    pc[threadIdx.x][0] = s_dzx;
    pc[threadIdx.x][1] = s_dz;
    const float m1 = block_sum_256(s_dz * ga, sh) / cnt;       // mean(dxh)
    const float m2 = block_sum_256(s_dzx * ga, sh) / cnt;      // mean(dxh xh)
    if (threadIdx.x < cpg) {                                   // this channel's sums over the pixel lanes, in lane order
        float a = 0.f, bb = 0.f;
        for (int q = 0; q < pstep; ++q) {
            a += pc[q * cpg + cl][0];
            bb += pc[q * cpg + cl][1];
        }
        float* o = part + (long long)b * 2 * C;
        o[ch] = a;
        o[C + ch] = bb;
    }
    for (int p = pl; p < HW; p += pstep) {
        const long long i = base + (long long)p * C;
        const float xh = (x[i] - mu) * rstd;
        const float dz = (!relu || xh * ga + be > 0.f) ? dy[i] : 0.f;
        dx[i] = rstd * (dz * ga - m1 - xh * m2);
    }
}

// ---- 2x2 / stride-2 max-pool backward: the window's FIRST maximum in row-major order (torch.max_pool2d) gets dY, recomputed from x
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                           int B, int H, int W, int C) {
    const int OH = H / 2, OW = W / 2;
    const long long n = (long long)B * H * W * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long px = i / C;
        const int w = (int)(px % W), h = (int)((px / W) % H), b = (int)(px / ((long long)H * W));
        const int oh = h >> 1, ow = w >> 1;
        float g = 0.f;
        if (oh < OH && ow < OW) {
            const long long top = (((long long)b * H + 2 * oh) * W + 2 * ow) * C + c;
            const float v[4] = {x[top], x[top + C], x[top + (long long)W * C], x[top + (long long)W * C + C]};
            int arg = 0;
            for (int k = 1; k < 4; ++k)
                if (v[k] > v[arg]) arg = k;
            if (arg == (h & 1) * 2 + (w & 1)) g = dy[(((long long)b * OH + oh) * OW + ow) * C + c];
        }
        dx[i] = g;
    }
}

// ---- nearest 2x upsample-add backward, coarse branch: the 2x2 block sum of dY (fixed order)
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dxc, int B, int H, int W, int C) {
    const long long n = (long long)B * H * W * C;
    const long long row = 2ll * W * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long px = i / C;
        const int w = (int)(px % W), h = (int)((px / W) % H), b = (int)(px / ((long long)H * W));
        const long long top = (((long long)b * 2 * H + 2 * h) * 2 * W + 2 * w) * C + c;
        dxc[i] = (dy[top] + dy[top + C]) + (dy[top + row] + dy[top + row + C]);
    }
}

// ---- correlation softmax backward, dS = A (dA - sum_c dA A) over the first C channels of each row (one wave per row); written as
// ds [rows][C] and, per batch entry of P rows, transposed into dst [B][C][P].
__global__ __launch_bounds__(256) void corr_softmax_bwd_kernel(const float* __restrict__ a, const float* __restrict__ da, int rows, int P, int C,
                                                               long long a_ld, long long da_ld, float* __restrict__ ds, float* __restrict__ dst) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* ar = a + (long long)row * a_ld;
    const float* gr = da + (long long)row * da_ld;
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) dot += gr[c] * ar[c];
    dot = wave_sum(dot);
    const int b = row / P, p = row % P;
    for (int c = lane; c < C; c += 64) {
        const float v = ar[c] * (gr[c] - dot);
        ds[(long long)row * C + c] = v;
        dst[((long long)b * C + c) * P + p] = v;
    }
}

// ---- batched 2-D transpose: x [B][rows][cols] -> y [B][cols][rows], 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_batched_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int cols) {
    __shared__ float t[32][33];
    const long long off = (long long)blockIdx.z * rows * cols;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && c0 + tx < cols) t[k][tx] = x[off + (long long)(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < cols && r0 + tx < rows) y[off + (long long)(c0 + k) * rows + r0 + tx] = t[tx][k];
}

static int grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

}  // namespace nps

extern "C" int nopesac_conv2d_dgrad_f32(const float* dy, const float* w, float* dx, float* w_ws, int64_t w_ws_bytes, int B, int H, int W,
                                        int Cin, int Cout, int KH, int KW, int stride, int pad, int64_t dy_cstride, int64_t dx_cstride,
                                        void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(dy && w && dx, "conv2d_dgrad: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv2d_dgrad: bad dims B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
    NPS_CHECK_ARG((KH == 1 || KH == 3) && KW == KH && (stride == 1 || stride == 2) && pad >= 0 && pad < KH,
                  "conv2d_dgrad: k=%dx%d s=%d p=%d (supported: k 1 or 3, stride 1 or 2, pad < k)", KH, KW, stride, pad);
    NPS_CHECK_ARG(dy_cstride >= Cout && dx_cstride >= Cin, "conv2d_dgrad: channel stride smaller than channel count");
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    NPS_CHECK_ARG(OH > 0 && OW > 0, "conv2d_dgrad: empty output");
    hipStream_t st = (hipStream_t)stream;
    if (stride == 2) {
        dgrad_gather_kernel<<<grid_for((long long)B * H * W * Cin), 256, 0, st>>>(dy, w, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW,
                                                                                   dy_cstride, dx_cstride);
        NPS_LAUNCH_RET();
    }
    NPS_CHECK_ARG(OH == H && OW == W, "conv2d_dgrad: stride 1 needs a same-size conv (pad = (k - 1) / 2)");
    NPS_CHECK_ARG(w_ws && w_ws_bytes >= (int64_t)Cin * Cout * KH * KW * 4, "conv2d_dgrad: weight workspace too small");
    dgrad_weight_kernel<<<grid_for((long long)Cin * Cout * KH * KW), 256, 0, st>>>(w, w_ws, Cout, Cin, KH, KW);
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_error("launch failed: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    // the library's f32 implicit-GEMM conv (v_mfma_f32_32x32x2f32): M = B H W input pixels, N = Cin, K = KH KW Cout
    return nopesac_conv2d_nhwc_ex(dy, w_ws, nullptr, nullptr, nullptr, dx, B, H, W, Cout, Cin, KH, KW, 1, KH - 1 - pad, dy_cstride, dx_cstride,
                                  0, 0, NPS_ACT_NONE, NPS_DT_F32, NPS_DT_F32, NPS_CONV_AUTO, stream);
}

extern "C" int64_t nopesac_conv2d_wgrad_workspace_bytes(int Cout, int Cin, int KH, int KW, int splits) {
    return (int64_t)splits * Cout * Cin * KH * KW * (int64_t)sizeof(float);
}

extern "C" int nopesac_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* ws, int64_t ws_bytes, int B, int H, int W, int Cin,
                                        int Cout, int KH, int KW, int stride, int pad, int64_t x_cstride, int64_t dy_cstride, int splits,
                                        void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && dy && dw && ws, "conv2d_wgrad: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0,
                  "conv2d_wgrad: bad dims B=%d H=%d W=%d Cin=%d Cout=%d k=%dx%d s=%d p=%d", B, H, W, Cin, Cout, KH, KW, stride, pad);
    NPS_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && x_cstride >= Cin && dy_cstride >= Cout && x_cstride % 4 == 0 && dy_cstride % 4 == 0 &&
                      (uintptr_t)x % 16 == 0 && (uintptr_t)dy % 16 == 0,
                  "conv2d_wgrad: needs Cin %% 4 == 0, Cout %% 4 == 0 and 16-byte aligned rows");
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    NPS_CHECK_ARG(OH > 0 && OW > 0, "conv2d_wgrad: empty output");
    const long long P = (long long)B * OH * OW;
    NPS_CHECK_ARG(splits >= 1 && splits <= 1024, "conv2d_wgrad: splits %d not in [1, 1024]", splits);
    NPS_CHECK_ARG(ws_bytes >= nopesac_conv2d_wgrad_workspace_bytes(Cout, Cin, KH, KW, splits), "conv2d_wgrad: workspace too small");
    long long chunk = (P + splits - 1) / splits;
    chunk = (chunk + WG_BK - 1) / WG_BK * WG_BK;               // split boundaries on LDS-stage boundaries
    NPS_CHECK_ARG(chunk < (1ll << 30), "conv2d_wgrad: pixel range too large");
    const int N = KH * KW * Cin;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((N + WG_BN - 1) / WG_BN, (Cout + WG_BM - 1) / WG_BM, splits);
    wgrad_kernel<<<grid, 256, 0, st>>>(x, dy, ws, B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, x_cstride, dy_cstride, (int)chunk);
    wgrad_reduce_kernel<<<grid_for((long long)Cout * N), 256, 0, st>>>(ws, dw, Cout, Cin, KH, KW, splits);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_bn_act_forward_f32(const float* c, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                          int act, int64_t rows, int C, float* y, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(c && gamma && beta && mean && var && y, "bn_act_forward: null pointer");
    NPS_CHECK_ARG(rows > 0 && C > 0 && eps > 0.f, "bn_act_forward: bad dims rows=%lld C=%d", (long long)rows, C);
    NPS_CHECK_ARG(act == NPS_ACT_NONE || act == NPS_ACT_RELU || act == NPS_ACT_LEAKY, "bn_act_forward: bad act %d", act);
    bn_act_fwd_kernel<<<grid_for(rows * C), 256, 0, (hipStream_t)stream>>>(c, gamma, beta, mean, var, eps, act, rows * C, C, y);
    NPS_LAUNCH_RET();
}

extern "C" int64_t nopesac_bn_act_backward_workspace_floats(int rows, int C) {
    return (int64_t)((rows + nps::BN_RPS - 1) / nps::BN_RPS) * 2 * C;
}

extern "C" int nopesac_bn_act_backward_f32(const float* dy, const float* c, const float* gamma, const float* beta, const float* mean,
                                           const float* var, float eps, int act, int rows, int C, float* dc, float* dgamma, float* dbeta,
                                           float* ws, int64_t ws_floats, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(dy && c && gamma && beta && mean && var && dc && dgamma && dbeta && ws, "bn_act_backward: null pointer");
    NPS_CHECK_ARG(rows > 0 && C > 0 && eps > 0.f, "bn_act_backward: bad dims rows=%d C=%d", rows, C);
    NPS_CHECK_ARG(act == NPS_ACT_NONE || act == NPS_ACT_RELU || act == NPS_ACT_LEAKY, "bn_act_backward: bad act %d", act);
    const int S = (rows + BN_RPS - 1) / BN_RPS;
    NPS_CHECK_ARG(S < 65536 && ws_floats >= (int64_t)S * 2 * C, "bn_act_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    bn_act_bwd_kernel<<<dim3((C + 63) / 64, S), 256, 0, st>>>(dy, c, gamma, beta, mean, var, eps, act, rows, C, dc, ws);
    sum_partials_kernel<<<(2 * C + 255) / 256, 256, 0, st>>>(ws, S, C, dgamma, dbeta);
    NPS_LAUNCH_RET();
}

extern "C" int64_t nopesac_groupnorm_backward_workspace_floats(int B, int C) { return B > 0 && C > 0 ? (int64_t)B * 2 * C : 0; }

extern "C" int nopesac_groupnorm_backward_f32(const float* x, const float* dy, const float* gamma, const float* beta, int B, int HW, int C,
                                              int groups, float eps, int relu, float* dx, float* dgamma, float* dbeta, float* ws,
                                              int64_t ws_floats, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && dy && gamma && beta && dx && dgamma && dbeta && ws, "groupnorm_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && HW > 0 && C > 0 && groups > 0 && eps > 0.f, "groupnorm_backward: bad dims B=%d HW=%d C=%d groups=%d", B, HW, C, groups);
    NPS_CHECK_ARG(C % groups == 0 && 256 % (C / groups) == 0, "groupnorm_backward: channels per group must divide 256");
    NPS_CHECK_ARG(ws_floats >= nopesac_groupnorm_backward_workspace_floats(B, C), "groupnorm_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    gn_bwd_kernel<<<B * groups, 256, 0, st>>>(x, dy, gamma, beta, HW, C, groups, eps, relu ? 1 : 0, dx, ws);
    sum_partials_kernel<<<(2 * C + 255) / 256, 256, 0, st>>>(ws, B, C, dgamma, dbeta);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_maxpool2x2_backward_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && dy && dx, "maxpool2x2_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && H >= 2 && W >= 2 && C > 0, "maxpool2x2_backward: bad dims B=%d H=%d W=%d C=%d", B, H, W, C);
    maxpool2_bwd_kernel<<<grid_for((long long)B * H * W * C), 256, 0, (hipStream_t)stream>>>(x, dy, dx, B, H, W, C);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_upsample2x_nearest_add_backward_f32(const float* dy, float* dx_coarse, int B, int H, int W, int C, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(dy && dx_coarse, "upsample2x_nearest_add_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "upsample2x_nearest_add_backward: bad dims B=%d H=%d W=%d C=%d", B, H, W, C);
    upsample2_bwd_kernel<<<grid_for((long long)B * H * W * C), 256, 0, (hipStream_t)stream>>>(dy, dx_coarse, B, H, W, C);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_corr_softmax_backward_f32(const float* a, const float* da, int B, int P, int C, int64_t a_ld, int64_t da_ld, float* ds,
                                                 float* ds_t, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(a && da && ds && ds_t, "corr_softmax_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && P > 0 && C > 0 && a_ld >= C && da_ld >= C, "corr_softmax_backward: bad dims B=%d P=%d C=%d", B, P, C);
    const int rows = B * P;
    corr_softmax_bwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(a, da, rows, P, C, a_ld, da_ld, ds, ds_t);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_transpose_batched_f32(const float* x, int B, int rows, int cols, float* y, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && y, "transpose_batched: null pointer");
    NPS_CHECK_ARG(B > 0 && B < 65536 && rows > 0 && cols > 0, "transpose_batched: bad dims B=%d rows=%d cols=%d", B, rows, cols);
    transpose_batched_kernel<<<dim3((cols + 31) / 32, (rows + 31) / 32, B), 256, 0, (hipStream_t)stream>>>(x, y, rows, cols);
    NPS_LAUNCH_RET();
}
