// Backward kernels of the ResNet-50 backbone (training.BackboneTrainer): the input gradient of the stride-2 convs as an implicit GEMM on
// the f32 MFMA, the backward of the stem's 3x3 / stride-2 / pad-1 max-pool, and the gate of FrozenBN + ReLU from the saved
// post-activation output.  f32 throughout, NHWC activations, caller-allocated buffers.  Deterministic: no atomics, every sum runs in
// a fixed order.  Gated against float64 torch.autograd (tests/test_backbone_forms_gpu.py, tests/test_backbone_training_gpu.py).
#include "common.h"

namespace nps {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static int bb_grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

// ---- dgrad operand of the strided conv: w [Cout][Cin][KH][KW] (state-dict layout) -> wp [KH][KW][Cout][Cin]: one tap's [Cout][Cin]
// matrix is a K x N block of the GEMM below, rows contiguous in Cin.
__global__ __launch_bounds__(256) void dgrad_s2_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int KH,
                                                              int KW) {
    const long long n = (long long)Cout * Cin * KH * KW;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        long long r = i / Cin;
        const int co = (int)(r % Cout); r /= Cout;
        const int kw = (int)(r % KW);
        const int kh = (int)(r / KW);
        wp[i] = w[(((long long)co * Cin + ci) * KH + kh) * KW + kw];
    }
}

// ---- dgrad of a stride-2 conv (k 1 or 3, pad (k - 1) / 2), decomposed by the parity of the input pixel so that no multiply meets an
// inserted zero.  Input row ih receives output row oh through tap kh iff ih + pad - kh = 2 oh: a row of parity ph sees the taps
// kh = kh0 + 2 t, kh0 = (ph + pad) & 1 - for k = 3 one tap (kh = 1) on even rows and two (kh = 0, 2) on odd rows, for k = 1 one tap on
// even rows and none on odd rows; columns alike.  Each of the four classes (ph, pw) is a GEMM with M = the class's pixels (b, r, c ->
// ih = 2 r + ph, iw = 2 c + pw), N = Cin, K = taps x Cout (tap-major, then co); a tap whose output row / column does not exist
// (oh >= OH: the last odd row of an even H) contributes zeros.  A class without taps is written as exact zeros by the same epilogue.
// One launch covers the four classes: blockIdx.x runs over the pixel tiles of class 0, then 1, 2, 3 (tile_end = running totals),
// blockIdx.y over the channel tiles.  128 pixels x 128 channels per workgroup (2 x 2 waves of 64 x 64 = 2 x 2 tiles of
// v_mfma_f32_32x32x2f32), 16 K values per LDS stage, the next stage's global loads in flight during the MFMAs.  Every global load is
// unconditional from a clamped address, followed by a select.
constexpr int DS_BM = NPS_DGRAD_S2_PIXELS, DS_BN = NPS_DGRAD_S2_CHANNELS, DS_BK = NPS_DGRAD_S2_STAGE, DS_LD = DS_BM + 4;
static_assert(DS_BM == 128 && DS_BN == 128 && DS_BK == 16, "the thread mappings below are written for 128 x 128 x 16");

struct DgradS2Tiles {
    int tile_end[4];                                           // running total of pixel tiles after class 0 .. 3 (class = 2 ph + pw)
};

__global__ __launch_bounds__(256) void dgrad_s2_kernel(const float* __restrict__ dy, const float* __restrict__ wp, float* __restrict__ dx, int B,
                                                       int H, int W, int Cin, int Cout, int KS, int pad, int OH, int OW, long long dy_cs,
                                                       long long dx_cs, DgradS2Tiles tiles) {
    __shared__ __attribute__((aligned(16))) float As[DS_BK * DS_LD];      // [k][pixel]
    __shared__ __attribute__((aligned(16))) float Bs[DS_BK * DS_LD];      // [k][channel]
    __shared__ long long pix_off[DS_BM];                                  // dX offset of the tile's pixels (-1: past the class)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int cls = 0, tile = blockIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if ((int)blockIdx.x >= tiles.tile_end[c]) {
            cls = c + 1;
            tile = blockIdx.x - tiles.tile_end[c];
        }
    const int ph = cls >> 1, pw = cls & 1;
    const int Hc = (H - ph + 1) >> 1, Wc = (W - pw + 1) >> 1;              // rows / columns of this parity
    const long long Mc = (long long)B * Hc * Wc;                           // > 0: a class without pixels has no tile
    const int kh0 = (ph + pad) & 1, kw0 = (pw + pad) & 1;
    const int nth = (KS - kh0 + 1) >> 1, ntw = (KS - kw0 + 1) >> 1;        // taps of this parity in [0, KS)
    const int Kc = nth * ntw * Cout;
    const long long m0 = (long long)tile * DS_BM;
    const int n0 = blockIdx.y * DS_BN;

    // A (dY) global -> LDS: 128 pixels x 16 k = 512 float4, two per thread: pixel tid / 4 + 64 i, k4 = 4 (tid % 4)
    const int ka = (tid & 3) * 4;
    int a_ih[2], a_iw[2];
    long long a_img[2];
    bool a_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + (tid >> 2) + 64 * i;
        a_ok[i] = m < Mc;
        const long long mc = a_ok[i] ? m : Mc - 1;
        const int c = (int)(mc % Wc);
        const long long t = mc / Wc;
        a_ih[i] = 2 * (int)(t % Hc) + ph;
        a_iw[i] = 2 * c + pw;
        a_img[i] = (t / Hc) * OH;
    }
    // B (weights) global -> LDS: 16 k x 128 channels = 512 float4, two per thread: k = tid / 32 + 8 i, channel 4 (tid % 32)
    const int nb = n0 + (tid & 31) * 4;
    const bool nb_ok = nb < Cin;
    const int nbc = nb_ok ? nb : 0;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x4 ra[2], rb[2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto load = [&](int kc) {
        {
            const int k = kc + ka;
            const bool k_ok = k < Kc;
            const int kk = k_ok ? k : 0;
            const int ti = kk / Cout, co = kk - ti * Cout;
            const int th = ti / ntw, tw = ti - th * ntw;
            const int kh = kh0 + 2 * th, kw = kw0 + 2 * tw;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int oh = (a_ih[i] + pad - kh) >> 1, ow = (a_iw[i] + pad - kw) >> 1;      // >= 0 for every tap of the parity
                const bool ok = k_ok && a_ok[i] && oh < OH && ow < OW;
                const int ohc = oh < OH ? oh : OH - 1, owc = ow < OW ? ow : OW - 1;
                const f32x4 v = *(const f32x4*)(dy + ((a_img[i] + ohc) * OW + owc) * dy_cs + co);
                ra[i] = ok ? v : zero4;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = kc + (tid >> 5) + 8 * i;
            const bool k_ok = k < Kc;
            const int kk = k_ok ? k : 0;
            const int ti = kk / Cout, co = kk - ti * Cout;
            const int th = ti / ntw, tw = ti - th * ntw;
            const int kh = kh0 + 2 * th, kw = kw0 + 2 * tw;
            const f32x4 v = *(const f32x4*)(wp + ((long long)(kh * KS + kw) * Cout + co) * Cin + nbc);
            rb[i] = (k_ok && nb_ok) ? v : zero4;
        }
    };
    if (Kc > 0) load(0);
    for (int kc = 0; kc < Kc; kc += DS_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = (tid >> 2) + 64 * i;
#pragma unroll
            for (int j = 0; j < 4; ++j) As[(ka + j) * DS_LD + m] = ra[i][j];
            *(f32x4*)(Bs + ((tid >> 5) + 8 * i) * DS_LD + (tid & 31) * 4) = rb[i];
        }
        __syncthreads();
        if (kc + DS_BK < Kc) load(kc + DS_BK);
#pragma unroll
        for (int kk = 0; kk < DS_BK; kk += 2) {
            const int k = kk + (lane >> 5);
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[k * DS_LD + wm * 64 + i * 32 + (lane & 31)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[k * DS_LD + wn * 64 + j * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // the tile's pixels in dX
    if (tid < DS_BM) {
        const long long m = m0 + tid;
        long long off = -1;
        if (m < Mc) {
            const int c = (int)(m % Wc);
            const long long t = m / Wc;
            const int r = (int)(t % Hc);
            off = (((t / Hc) * H + 2 * r + ph) * W + 2 * c + pw) * dx_cs;
        }
        pix_off[tid] = off;
    }
    __syncthreads();
    // D[row][col]: lane l, register r -> row 8 (r / 4) + 4 (l / 32) + r % 4, col l % 32
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + (lane & 31);
            if (n >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long off = pix_off[wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)];
                if (off >= 0) dx[off + n] = acc[i][j][r];
            }
        }
}

// ---- 3x3 / stride-2 / pad-1 max-pool backward (the stem's pool), gather form: an input element looks at the up-to-four windows that
// contain it (rows oh with 2 oh - 1 <= h <= 2 oh + 1), recomputes each window's FIRST maximum in row-major order over its in-bounds taps
// (torch.max_pool2d: strict >, a NaN takes over, padding never wins) and adds that window's dY if the first maximum is the element
// itself; the additions run over the windows in row-major order.  The taps are loaded unconditionally from clamped addresses.
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                             int B, int H, int W, int C, int OH, int OW) {
    const long long n = (long long)B * H * W * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long px = i / C;
        const int w = (int)(px % W), h = (int)((px / W) % H);
        const long long b = px / ((long long)H * W);
        const float* xb = x + b * H * W * C + c;
        const int oh_lo = h >> 1, oh_hi = (h + 1) >> 1, ow_lo = w >> 1, ow_hi = (w + 1) >> 1;      // equal for an even coordinate
        float g = 0.f;
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            if (oh >= OH) continue;
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                if (ow >= OW) continue;
                const int hs = 2 * oh - 1, ws = 2 * ow - 1;
                float best = 0.f;
                int arg = -1;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int th = hs + t / 3, tw = ws + t % 3;
                    const bool in = th >= 0 && th < H && tw >= 0 && tw < W;
                    const int thc = th < 0 ? 0 : (th < H ? th : H - 1), twc = tw < 0 ? 0 : (tw < W ? tw : W - 1);
                    const float v = xb[((long long)thc * W + twc) * C];
                    const bool take = in && (arg < 0 || v > best || v != v);
                    best = take ? v : best;
                    arg = take ? t : arg;
                }
                const float d = dy[((b * OH + oh) * OW + ow) * C + c];
                g += arg == (h - hs) * 3 + (w - ws) ? d : 0.f;
            }
        }
        dx[i] = g;
    }
}

// ---- FrozenBN + act backward from the saved POST-activation output y: dz = act == RELU ? (y > 0 ? g : 0) : g, dc = dz * scale[c]
// (-0.0 and +0.0 are both "not > 0"); dz is written when the conv had a residual (whose gradient it is).
__global__ __launch_bounds__(256) void frozen_bn_act_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                                const float* __restrict__ scale, int relu, long long rows, int C,
                                                                long long g_ld, long long y_ld, float* __restrict__ dc,
                                                                float* __restrict__ dz) {
    const long long n = rows * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / C;
        const int c = (int)(i - r * C);
        const float gv = g[r * g_ld + c], yv = y[r * y_ld + c];
        const float z = relu ? (yv > 0.f ? gv : 0.f) : gv;
        dc[i] = z * scale[c];
        if (dz) dz[i] = z;
    }
}

}  // namespace nps

extern "C" int nopesac_conv2d_dgrad_s2_f32(const float* dy, const float* w, float* dx, float* w_ws, int64_t w_ws_bytes, int B, int H, int W,
                                           int Cin, int Cout, int KH, int KW, int pad, int64_t dy_cstride, int64_t dx_cstride, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(dy && w && dx && w_ws, "conv2d_dgrad_s2: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv2d_dgrad_s2: bad dims B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
    NPS_CHECK_ARG((KH == 1 || KH == 3) && KW == KH && pad == (KH - 1) / 2, "conv2d_dgrad_s2: k=%dx%d p=%d (supported: k 1 or 3, pad (k - 1) / 2)",
                  KH, KW, pad);
    NPS_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && dy_cstride >= Cout && dx_cstride >= Cin && dy_cstride % 4 == 0 &&
                      (uintptr_t)dy % 16 == 0 && (uintptr_t)w_ws % 16 == 0,
                  "conv2d_dgrad_s2: needs Cin %% 4 == 0, Cout %% 4 == 0, dy channel stride %% 4 == 0 and 16-byte aligned dy / workspace");
    NPS_CHECK_ARG(w_ws_bytes >= NPS_DGRAD_S2_WORKSPACE_BYTES(Cin, Cout, KH, KW), "conv2d_dgrad_s2: weight workspace too small");
    NPS_CHECK_ARG((long long)KH * KW * Cout < (1ll << 30), "conv2d_dgrad_s2: K too large");
    const int OH = (H + 2 * pad - KH) / 2 + 1, OW = (W + 2 * pad - KW) / 2 + 1;
    DgradS2Tiles tiles;
    long long total = 0;
    for (int cls = 0; cls < 4; ++cls) {
        const int ph = cls >> 1, pw = cls & 1;
        const long long Mc = (long long)B * ((H - ph + 1) / 2) * ((W - pw + 1) / 2);
        total += (Mc + DS_BM - 1) / DS_BM;
        NPS_CHECK_ARG(total < (1ll << 30), "conv2d_dgrad_s2: pixel range too large");
        tiles.tile_end[cls] = (int)total;
    }
    const int ntiles = (Cin + DS_BN - 1) / DS_BN;
    NPS_CHECK_ARG(ntiles < 65536, "conv2d_dgrad_s2: Cin %d too large", Cin);
    hipStream_t st = (hipStream_t)stream;
    dgrad_s2_weight_kernel<<<bb_grid_for((long long)Cin * Cout * KH * KW), 256, 0, st>>>(w, w_ws, Cout, Cin, KH, KW);
    dgrad_s2_kernel<<<dim3((unsigned)total, ntiles), 256, 0, st>>>(dy, w_ws, dx, B, H, W, Cin, Cout, KH, pad, OH, OW, dy_cstride, dx_cstride,
                                                                  tiles);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_maxpool3x3s2_backward_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && dy && dx, "maxpool3x3s2_backward: null pointer");
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "maxpool3x3s2_backward: bad dims B=%d H=%d W=%d C=%d", B, H, W, C);
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    maxpool3s2_bwd_kernel<<<bb_grid_for((long long)B * H * W * C), 256, 0, (hipStream_t)stream>>>(x, dy, dx, B, H, W, C, OH, OW);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_frozen_bn_act_backward_f32(const float* g, const float* y, const float* scale, int act, int64_t rows, int C,
                                                  int64_t g_stride, int64_t y_stride, float* dc, float* dz, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(g && y && scale && dc, "frozen_bn_act_backward: null pointer");
    NPS_CHECK_ARG(rows > 0 && C > 0 && rows < (1ll << 40), "frozen_bn_act_backward: bad dims rows=%lld C=%d", (long long)rows, C);
    NPS_CHECK_ARG(act == NPS_ACT_NONE || act == NPS_ACT_RELU, "frozen_bn_act_backward: act %d (supported: NONE, RELU)", act);
    NPS_CHECK_ARG(g_stride >= C && y_stride >= C, "frozen_bn_act_backward: row stride smaller than C");
    frozen_bn_act_bwd_kernel<<<bb_grid_for(rows * C), 256, 0, (hipStream_t)stream>>>(g, y, scale, act == NPS_ACT_RELU ? 1 : 0, rows, C, g_stride,
                                                                                    y_stride, dc, dz);
    NPS_LAUNCH_RET();
}
