/*
 * nopesac_hip.h — C ABI of libnopesac_hip.so: the MI355X (gfx950) kernels behind NopeSAC's inference
 * hot path.
 *
 * The reference (IceTTTb/NopeSAC) is pure Python on torch/cuDNN and has NO native interface
 * (SURVEY.md fact 1); this ABI is therefore build-defined (SURVEY.md §8b last row).  Each entry point
 * names the reference computation it replaces (path:line under NopeSAC_Net/modeling/).  The host side
 * that binds it is nopesac_amd/_lib.py (ctypes); INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer on the current device (tensor.data_ptr()); the caller owns all
 *    buffers and allocates outputs; nothing is retained after return;
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *    enqueued on it, no call synchronises, so every call is capturable into a hipGraph;
 *  - an entry point declared `nps_status` returns 0 = enqueued, <0 = argument error (NPS_E_*), >0 = hipError_t from the launch, and
 *    leaves the reason in nopesac_last_error(); one declared plain int / int64_t / long long returns a VALUE that its comment names
 *    (the host side raises on a non-zero nps_status by itself and hands values through: nopesac_amd/_lib.py);
 *  - activations are NHWC ("pixels x channels", channels contiguous); conv weights are
 *    [Cout][KH][KW][Cin] (K-contiguous rows); token matrices are [rows][features] row-major;
 *  - dtype codes: 0 = f32, 1 = bf16.  Accumulation is always f32.
 *  - ragged per-pair sizes (n1, n2, m) live in int32 device arrays; padded rows are ignored/zeroed.
 */
#ifndef NOPESAC_HIP_H
#define NOPESAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPS_DT_F32 0
#define NPS_DT_BF16 1
#define NPS_DT_F32_BF16W 2 /* conv in_dt only: x is f32 in memory, w is bf16; x is rounded to bf16 while staged */
#define NPS_DT_FP8 3       /* OCP e4m3fn bytes (gfx950's fp8).  As out_dt: the epilogue result is saturated to +-448 and rounded to
                            * nearest even; only with a channel count / stride that is a multiple of 8 and no residual */

#define NPS_ACT_NONE 0
#define NPS_ACT_RELU 1
#define NPS_ACT_LEAKY 2   /* LeakyReLU(0.01), camera_modules.py:47 */
#define NPS_ACT_SIGMOID 3
#define NPS_ACT_RES_AFTER 0x100 /* OR-able flag: add `residual` AFTER the activation (planeTR_head.py:244-250) */
#define NPS_ACT_BIAS_BATCHED 0x200 /* OR-able flag, batched weights only: `bias` is [B][Cout] (one row per batch entry) */

#define NPS_E_ARG (-1)
#define NPS_E_UNSUPPORTED (-2)
typedef int nps_status; /* 0 = enqueued, < 0 = NPS_E_*, > 0 = hipError_t */

/* library / ABI version (major*10000 + minor*100 + patch; never negative) */
int nopesac_version(void);
/* last error string of this thread's most recent failing call ("" if none) */
const char* nopesac_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer with fused epilogue (MFMA).
 *   y[b,oh,ow,n] = act( (sum_{kh,kw,c} x[b, oh*s-p+kh, ow*s-p+kw, c] * w[n,kh,kw,c]) * scale[n] + bias[n]
 *                       + residual[b,oh,ow,n] )        (or act(...) + residual with NPS_ACT_RES_AFTER)
 * Replaces every torch conv2d/linear(+BN/bias/residual/activation) on the path: d2 ResNet-50
 * (meta_arch/siamese_planeTR.py:456), planeTR_net/planeTR_head.py:126,148-162,209-215,
 * camera_net/camera_modules.py:36-48,271-321, camera_net/camera_head.py:957-962,983-990,
 * transformer linears, matching_net/matching_head.py:101-113.
 *   in_dt/out_dt : NPS_DT_*; weights have dtype in_dt (bf16 for NPS_DT_F32_BF16W).
 *   x_cstride / y_cstride / r_cstride : elements between consecutive pixels (>= channels) so that
 *       inputs/outputs can live inside wider (concatenated) buffers.
 *   w_bstride : elements between per-image weight sets (0 = shared weights).  With w_bstride != 0
 *       the call is a batched GEMM  y[b] = x[b] * w[b]^T  (mask einsum planeTR_head.py:150, attention-
 *       free correlations camera_head.py:1128, descriptor scores matching_head.py:113).
 *   scale/bias : f32[Cout] or NULL; residual: out_dt NHWC or NULL.
 */
nps_status nopesac_conv2d_nhwc(const void* x, const void* w, const float* scale, const float* bias,
                               const void* residual, void* y,
                               int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                               int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int64_t w_bstride,
                               int act, int in_dt, int out_dt, void* stream);

/* Same, with an explicit kernel configuration (chosen per layer shape by the load-time autotuner of
 * nopesac_amd/ops.py; every configuration computes the same result): NPS_CONV_AUTO = built-in heuristic,
 * T128 / T64 = register-staged 128x128 / 64x64 tiles, DMA64 / DMA32 = LDS-DMA kernel with BK = 64 / 32
 * (bf16 with Cin % 64 == 0 only; silently falls back to the heuristic when not applicable). */
#define NPS_CONV_AUTO 0
#define NPS_CONV_T128 1
#define NPS_CONV_T64 2
#define NPS_CONV_DMA64 3
#define NPS_CONV_DMA32 4
nps_status nopesac_conv2d_nhwc_ex(const void* x, const void* w, const float* scale, const float* bias,
                                  const void* residual, void* y,
                                  int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                  int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int64_t w_bstride,
                                  int act, int in_dt, int out_dt, int kernel_cfg, void* stream);

/* bf16 conv with the weights in MFMA FRAGMENT-MAJOR order ([Cout][KH*KW*Cin] re-ordered as in nopesac_bottleneck_tail_bf16):
 * activations go through a 3-deep LDS-DMA ring (variant 3: K-tile 64, 3 workgroups/CU; variant 32: K-tile 32, 4-deep ring, 4 workgroups/CU),
 * every wave streams the weight fragments of its own 32 output channels from L2 (csrc/conv_igemm.hip, conv_igemm_bfrag_kernel).  Same semantics as nopesac_conv2d_nhwc for x / w bf16;
 * needs Cin % 64 == 0, Cout % 128 == 0; act may carry NPS_ACT_RES_AFTER; out_dt may also be NPS_DT_FP8 (no residual). */
nps_status nopesac_conv2d_nhwc_bfrag(const void* x, const void* w_frag, const float* scale, const float* bias, const void* residual,
                                     void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                     int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int act, int out_dt, int variant,
                                     void* stream);

/* bf16 conv on 256 x 256 x 64 workgroup tiles (csrc/conv_p8.hip, conv_igemm_p8_kernel): 8 waves, both operands through LDS-DMA,
 * the two waves of a SIMD alternate LDS-read / MFMA phases, counted vmcnt across barriers.  For the MFMA-bound layers: twice the
 * FLOPs per byte pulled from L2 of the 128 x 128 kernels.  x / w as for nopesac_conv2d_nhwc with in_dt BF16 (w = plain
 * [Cout][KH][KW][Cin] rows, NOT fragment-major); needs Cin % 64 == 0, Cout % 256 == 0, x_cstride % 8 == 0; act may carry
 * NPS_ACT_RES_AFTER; out_dt F32 / BF16 / FP8 (FP8: no residual).  variant: 0 = static wave priority for the lagging half (default),
 * 1 = priority raised around every MFMA cluster, 2 = no priority hints (tuning aid; results are identical).
 * Replaces: the same reference convolutions as nopesac_conv2d_nhwc (detectron2 Conv2d + FrozenBN + ReLU; camera_modules.py conv stacks). */
nps_status nopesac_conv2d_nhwc_p8(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                                  int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                  int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int act, int out_dt, int variant, void* stream);

/* The same kernel with STREAM-K work distribution (conv_igemm_p8_kernel<.., SK>; round 5): the K-tiles of each XCD's run of output tiles
 * are cut evenly over that XCD's persistent workgroups, so a layer of 300 (150) tiles costs 1.17 (0.59) tile times on 256 CUs instead of
 * 2 (1) rounds.  A tile whose K range is shared is completed by whichever contributor arrives LAST on the tile's counter (nobody waits for
 * another workgroup); partial accumulators travel through `workspace` as f32 slabs and are summed in K order - results do not depend on
 * the arrival order, and equal the plain kernel's up to the K-split's summation order.
 * workspace: nopesac_conv2d_p8_sk_workspace_bytes() bytes, 16-byte aligned; its first 16 KB (arrival counters) must be ZERO on entry and
 * are zero again on completion - one workspace serves all launches of ONE stream (the byte count is a value, always positive).
 * variant: as nopesac_conv2d_nhwc_p8 (24 not allowed).
 * Replaces: the same reference convolutions as nopesac_conv2d_nhwc_p8. */
int64_t nopesac_conv2d_p8_sk_workspace_bytes(void);
nps_status nopesac_conv2d_nhwc_p8_sk(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                                     int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                     int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int act, int out_dt, int variant,
                                     void* workspace, int64_t workspace_bytes, void* stream);

/* The 256 x 128-tile sibling for layers with Cout % 128 == 0 that the 256-wide kernel cannot take (csrc/conv_p8n.hip,
 * conv_igemm_p8n_kernel; round 5): the 3x3 128 -> 128 convs of res3 and of the top-down / pose-net stacks.  Same structure (persistent
 * 8-wave workgroups, LDS-DMA operands, counted vmcnt, staggered wave groups), two 8-MFMA phases per K-tile, a three-deep K-tile ring.
 * bf16 in / bf16 out, y = act(conv * scale + bias) with act in {NPS_ACT_NONE, NPS_ACT_RELU, NPS_ACT_LEAKY}, no residual; scale / bias may
 * be NULL; Cin % 64 == 0, x_cstride % 8 == 0, y_cstride % 8 == 0; variant: 0, + 32 = channel-major K order.
 * Replaces: the same reference convolutions as nopesac_conv2d_nhwc (detectron2 BottleneckBlock conv2 + FrozenBN + ReLU, Base.yaml:2-12;
 * camera_modules.py:271-321 pixel-decoder convs). */
nps_status nopesac_conv2d_nhwc_p8n(const void* x, const void* w, const float* scale, const float* bias, void* y, int B, int H, int W,
                                   int Cin, int Cout, int KH, int KW, int stride, int pad, int64_t x_cstride, int64_t y_cstride, int act,
                                   int variant, void* stream);
/* The same kernel with SPLIT-K work units (round 6) for layers with few tiles and a long K loop - the pose net's first conv (3x3, 2048 -> 128
 * at 15 x 20: 75 tiles x 288 K-tiles; reference camera_head.py:97-112 convs_trans / convs_rots are fed by it through the correlation, the
 * layer itself is the pixel decoder's `layer_3` output conv, camera_modules.py:271-321).  A unit = (tile, slice of the 64-channel groups);
 * partial tiles leave as f32 into workspace[splits][M][Cout] (M = B * OH * OW; >= splits * M * Cout * 4 bytes, 16-byte aligned, < 2 GB) and a
 * second launch on the same stream sums the slices in fixed order (deterministic) and applies the epilogue.  variant must carry + 32
 * (channel-major K order); 2 <= splits <= min(Cin / 64, 16).  Everything else as nopesac_conv2d_nhwc_p8n.
 * nopesac_conv2d_p8n_splitk_workspace_bytes: splits * M * Cout * 4, the size the launcher checks (a value; 0 for an argument <= 0). */
int64_t nopesac_conv2d_p8n_splitk_workspace_bytes(int splits, int64_t M, int Cout);
nps_status nopesac_conv2d_nhwc_p8n_splitk(const void* x, const void* w, const float* scale, const float* bias, void* y, int B, int H, int W,
                                          int Cin, int Cout, int KH, int KW, int stride, int pad, int64_t x_cstride, int64_t y_cstride, int act,
                                          int variant, int splits, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- which of the kernels above may run one convolution (csrc/conv_forms.h; host only: no HIP call, needs no GPU) -----------------
 * A kernel configuration of nopesac_amd.ops.conv2d is NPS_CONV_AUTO .. NPS_CONV_DMA32 (nopesac_conv2d_nhwc_ex) or one of: */
#define NPS_CONV_CFG_BFRAG3 7     /* nopesac_conv2d_nhwc_bfrag, variant 3 */
#define NPS_CONV_CFG_BFRAG32 8    /* nopesac_conv2d_nhwc_bfrag, variant 32 */
#define NPS_CONV_CFG_HALO16 9     /* nopesac_conv3x3_halo_bf16, tile 0 */
#define NPS_CONV_CFG_HALO8 10     /* nopesac_conv3x3_halo_bf16, tile 1 */
#define NPS_CONV_CFG_P8 11        /* nopesac_conv2d_nhwc_p8 */
#define NPS_CONV_CFG_P8_SK 12     /* nopesac_conv2d_nhwc_p8_sk */
#define NPS_CONV_CFG_P8N 13       /* nopesac_conv2d_nhwc_p8n, channel-major K order */
#define NPS_CONV_CFG_P8N_TAP 14   /* nopesac_conv2d_nhwc_p8n, tap-major K order */
#define NPS_CONV_CFG_P8N_SPLIT 15 /* nopesac_conv2d_nhwc_p8n_splitk */
/* Returns the bitmask (1 << configuration) of the configurations the autotuner may time for the call, or NPS_E_ARG (stride <= 0);
 * *splits (optional) receives the slice count it hands nopesac_conv2d_nhwc_p8n_splitk.  x_dt / w_dt / out_dt: NPS_DT_* of the buffers
 * in memory; batched: w_bstride != 0; act: the whole act word; aligned: x, w, y, residual, scale and bias are all 16-byte aligned.
 * The call is taken to be well formed (positive dims, a non-empty output, channel strides >= channel counts: the entry points check
 * that).  Bits 0-4 are always set: T128 .. DMA32 fall back to the heuristic where they do not apply.  The entry points above check
 * their arguments with the same predicates and refuse a call outside its bit before any HIP call.  An entry point asks for a little
 * more than its bit says, because the bfrag / halo / p8 bits are part of the autotuner's routing keys and stay as they were tuned:
 * bfrag and halo need their own pointers 16-byte aligned whatever the other buffers are, bfrag with an fp8 output needs no residual
 * and 8-channel-aligned y / scale / bias, p8 needs B * OH * OW < 2^23. */
int nopesac_conv2d_nhwc_forms(int x_dt, int w_dt, int out_dt, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                              int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int batched, int has_residual, int has_scale,
                              int has_bias, int act, int aligned, int* splits);

/* ---- a stack of Linear(+bias)(+activation) layers in ONE launch (csrc/mlp_chain.hip) --------------------------------------------
 * Replaces one nopesac_conv2d_nhwc launch per layer for the row-wise MLP stacks of the heads in bf16 mode (reference:
 * camera_net/camera_head.py:957-990 geo_encoder / geo_proj_s1 / decoder_rot / geo_proj_s2 / decoder_tran / decoder_rot2 /
 * decoder_tran2 / rots / trans; :685-735 rot_emb_proj / trans_emb_proj; :1090-1100 normal_score_proj / param_score_proj).
 * Row r of the chain input = [ xb[r / xb_rows_per][0 .. xb_width) | x[r][0 .. x_width) ] (the broadcast prefix is optional:
 * xb_width = 0).  Layer l: y = act(y_prev . W_l^T + bias_l); f32 accumulation, operands rounded to bf16 (RNE) exactly where the
 * per-layer launches round them.  A layer with `out` != NULL also writes its f32 output rows to out[r * out_ld + n] (n < N); the
 * last layer must.  Weights: bf16, packed for K padded to nopesac_mlp_padded_k(N, K) and N padded to a multiple of 32 (zeros) in
 * MFMA fragment-major order [Np/32][Kp/16][64 lanes][8] (nopesac_amd.ops.mlp_pack); bias: f32[Np] (zero padded) or NULL.
 * Limits: chain input <= NOPESAC_MLP_MAX_IN columns, every N <= NOPESAC_MLP_MAX_WIDTH, <= NOPESAC_MLP_MAX_LAYERS layers.
 * nopesac_mlp_padded_k / nopesac_mlp_packed_elems return values: the padded K and the element count of one layer's packed weights, 0
 * for sizes outside the limits (never negative). */
#define NOPESAC_MLP_MAX_IN 1280
#define NOPESAC_MLP_MAX_WIDTH 1024
#define NOPESAC_MLP_MAX_LAYERS 12
#define NOPESAC_MLP_RESTART 1   /* nopesac_mlp_layer.reserved: this layer reads the chain INPUT again instead of the previous layer's
                                 * output - several stacks over the same rows (e.g. the plane head's embedding / prob / param / center
                                 * MLPs, planeTR_head.py:170-188) run in one launch */
typedef struct nopesac_mlp_layer {
    const void* w;
    const float* bias;
    float* out;
    int64_t out_ld;
    int K, N, act, reserved;
} nopesac_mlp_layer;
typedef struct nopesac_mlp_chain {
    const float* x;
    int64_t x_ld;
    const float* xb;
    int64_t xb_ld;
    int x_width, xb_width, xb_rows_per, rows, n_layers, reserved;
    nopesac_mlp_layer layers[NOPESAC_MLP_MAX_LAYERS];
} nopesac_mlp_chain;
int nopesac_mlp_padded_k(int N, int K);
int64_t nopesac_mlp_packed_elems(int N, int K);
nps_status nopesac_mlp_chain_bf16(const nopesac_mlp_chain* chain, void* stream);

/* fp8 (OCP e4m3fn) conv on the gfx950 K=64 fp8 MFMA (v_mfma_f32_32x32x64_f8f6f4, unit block scales; 2x the bf16 MFMA rate): x is
 * fp8 NHWC, w_frag8 the fp8 [Cout][KH*KW*Cin] matrix in the fp8 fragment-major order
 *   [Cout/32][K/64][2][64][16]:  byte j of piece h of lane l = w[nt*32 + (l & 31)][kf*64 + 32*(l >> 5) + 16*h + j]
 * (ops.mfma_fragment_major_fp8).  Accumulation is f32; `scale` must already contain the de-quantisation factors
 * (bn_scale[n] * w_scale[n] * x_scale) - the kernel is otherwise nopesac_conv2d_nhwc_bfrag (same structure: activations through an
 * LDS-DMA ring - half the bytes per K step -, weights streamed from L2).  out_dt: F32, BF16 or FP8.  residual (if any) has out_dt's
 * type (not allowed with FP8).  Needs Cin % 64 == 0, Cout % 128 == 0, x_cstride % 16 == 0.  variant 3: K-tile 128 (Cin % 128 == 0),
 * variant 32: K-tile 64.  Replaces: the reference has no reduced-precision path; BASELINE config 5 ("fp8 MFMA backbone weights"). */
nps_status nopesac_conv2d_nhwc_fp8(const void* x, const void* w_frag8, const float* scale, const float* bias, const void* residual,
                                   void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                   int64_t x_cstride, int64_t y_cstride, int64_t r_cstride, int act, int out_dt, int variant,
                                   void* stream);

/* bf16 3x3 / stride 1 / pad 1 conv with 64 -> 64 channels + folded BN + activation (conv2 of the res2 bottlenecks): 16x16 pixel
 * tiles computed out of an 18x18 halo kept in LDS (csrc/conv3x3_c64.hip).  x, y bf16 NHWC [B,H,W,64]; w_frag = the
 * [64][3*3*64] weight matrix in MFMA fragment-major order. */
nps_status nopesac_conv3x3_c64_bf16(const void* x, const void* w_frag, const float* scale, const float* bias, void* y, int B, int H, int W,
                                    int act, void* stream);

/* bf16 3x3 / stride 1 / pad 1 conv, Cin % 64 == 0, Cout % 128 == 0, + folded BN + activation, computed from LDS halo tiles
 * (csrc/conv3x3_halo.hip): tile 0 = 16x16 pixels, 1 = 16 rows x 8 columns per workgroup.  x [B,H,W,Cin], y [B,H,W,Cout] bf16
 * (pixel-dense), w_frag = the [Cout][3*3*Cin] weights in MFMA fragment-major order. */
nps_status nopesac_conv3x3_halo_bf16(const void* x, const void* w_frag, const float* scale, const float* bias, void* y, int B, int H, int W,
                                     int Cin, int Cout, int act, int tile, void* stream);

/* Fused bf16 ResNet stem: y = maxpool3x3/s2/p1( relu( bn( conv7x7/s2/p3(x) ) ) ) in one kernel (d2 BasicStem).
 *   x bf16 NHWC [B,H,W,4] (RGB + zero pad channel); w bf16 [64][7][8][4] (kw padded 7 -> 8 with zeros, i.e. 224 per
 *   output channel); scale/bias f32[64] (folded FrozenBN); y bf16 NHWC [B,PH,PW,64]. */
nps_status nopesac_stem_fused_bf16(const void* x, const void* w, const float* scale, const float* bias, void* y,
                                   int B, int H, int W, void* stream);
/* Same, fed directly with the f32 NCHW images [B,3,H,W] of preprocess_image (siamese_planeTR.py:534-542): the normalisation
 * (v - mean[c]) / std[c] and the rounding to bf16 happen while the input patch is staged, bit-identical to
 * nopesac_preprocess_nchw_to_nhwc followed by nopesac_stem_fused_bf16. */
nps_status nopesac_stem_fused_raw_bf16(const float* x_nchw, const float* mean, const float* std, const void* w, const float* scale,
                                       const float* bias, void* y, int B, int H, int W, void* stream);
/* Raw-image stem with the normalisation folded into its operands (round 4): the staged patch holds v - 128, exact in bf16 for the
 * 8-bit pixel values preprocess_image receives, so the input operand carries no rounding error (the normalised image of the entry
 * above is rounded to 8 significant bits).  The caller folds: w_folded[o][kh][kw][c] = bf16(w[o][kh][kw][c] / std[c]),
 * bias_folded[o] = bias[o] + scale[o] * sum_{kh,kw,c} (w / std[c]) * (128 - mean[c]), pad3[c] = mean[c] - 128 (the raw value whose
 * folded contribution is the reference's zero padding of the NORMALISED image; siamese_planeTR.py:534-542 + d2 BasicStem). */
nps_status nopesac_stem_fused_raw_shifted_bf16(const float* x_nchw, const float* pad3, const void* w_folded, const float* scale,
                                               const float* bias_folded, void* y, int B, int H, int W, void* stream);

/* Fused tail of a bf16 ResNet bottleneck (d2 BottleneckBlock.forward: conv3 + shortcut + ReLU) plus, optionally, the NEXT
 * block's 1x1 reduce conv, in one launch (all tensors bf16 NHWC, pixel-dense; FrozenBN as f32 scale/bias):
 *   y = relu(scale3 * (w3 . b) + bias3 + shortcut),  shortcut = residual [B,OH,OW,C4]                      (identity block)
 *                                                    or scale_sc * (wsc . x2[:, ::s, ::s]) + bias_sc        (projection block)
 *   o = relu(scale1 * (w1 . y) + bias1)  if CN > 0   [B,OH,OW,CN]
 * b [B,OH,OW,C], x2 [B,x2_H,x2_W,C2].  Exactly one of residual / x2 is non-NULL.
 * The three weight matrices w3 [C4][C], wsc [C4][C2], w1 [CN][C4] are passed FRAGMENT-MAJOR: a [N][K] matrix is stored as
 * [N/32][K/16][2][32][8], i.e. element (n, k) at ((((n/32)*(K/16) + k/16)*2 + (k%16)/8)*32 + n%32)*8 + k%8 - the order in which
 * the 64 lanes of a wave consume it as MFMA operands, so every weight load is 1 KB contiguous (nopesac_amd.ops.mfma_fragment_major).
 * Supported (C, C4, CN, C2): (64,256,{0,64,128},0), (64,256,{0,64},64), (128,512,{0,128,256},0), (128,512,{0,128},256),
 * (256,1024,{0,256,512},0), (256,1024,{0,256},512);
 * anything else returns an error (the caller then uses
 * nopesac_conv2d_nhwc per layer). */
nps_status nopesac_bottleneck_tail_bf16(const void* b, const void* w3, const float* scale3, const float* bias3, const void* residual,
                                        const void* x2, const void* wsc, const float* scale_sc, const float* bias_sc, int B, int OH, int OW,
                                        int x2_H, int x2_W, int x2_stride, int C, int C4, int C2, void* y, const void* w1,
                                        const float* scale1, const float* bias1, int CN, void* o, void* stream);
/* Same; o_dt = NPS_DT_BF16, or NPS_DT_FP8: o is written as OCP e4m3fn bytes (the next block's 3x3 conv then runs on
 * nopesac_conv2d_nhwc_fp8; scale1 / bias1 must already contain the 1 / x_scale of that conv's input quantisation). */
nps_status nopesac_bottleneck_tail_bf16_ex(const void* b, const void* w3, const float* scale3, const float* bias3, const void* residual,
                                           const void* x2, const void* wsc, const float* scale_sc, const float* bias_sc, int B, int OH, int OW,
                                           int x2_H, int x2_W, int x2_stride, int C, int C4, int C2, void* y, const void* w1,
                                           const float* scale1, const float* bias1, int CN, void* o, int o_dt, void* stream);

/* The kernel forms of the bottleneck tail (csrc/pwchain.hip).  rt4 / rt4_late / rt4_proj / rt8 store whole 128-pixel tiles and rt4h
 * whole 64-pixel tiles: they are eligible only when B*OH*OW is a multiple of that. */
#define NPS_TAIL_PW 0        /* pw_chain_kernel: 64 pixels per workgroup (C = 64) or 32 (C = 128); any M */
#define NPS_TAIL_RT4 1       /* pw_chain_rt4_kernel, identity blocks of res2 / res3, residual prefetch before GEMM 1 (C = 64) */
#define NPS_TAIL_RT4_LATE 2  /* the same kernel with the residual prefetch behind GEMM 1 (for C = 128 both builds are one kernel) */
#define NPS_TAIL_RT4_PROJ 3  /* pw_chain_rt4_kernel with the projection GEMM: res2.0, a same-resolution stride-1 source */
#define NPS_TAIL_RT4H 4      /* pw_chain_rt4h_kernel: res3's edge blocks, 64 pixels per four-wave workgroup */
#define NPS_TAIL_RT8 5       /* pw_chain_rt8_kernel: res3's edge blocks (C = 128) or res4 identity blocks (C = 256, CN = 256) */
#define NPS_TAIL_STREAM 6    /* pw_chain_stream_kernel: res4 identity blocks; any M */
#define NPS_TAIL_WIDE 7      /* pw_chain_wide_kernel: every C = 256 configuration; any M */
#define NPS_TAIL_FORMS 8
/* A/B switch bits of the default selection: the environment variables NOPESAC_TAIL_NO_RT4, _NO_RT8, _RT4_LATE (read once per process by
 * nopesac_bottleneck_tail_bf16_ex), _NO_RT4H, _RT8_WIDE and _NO_STREAM (read at every call). */
#define NPS_TAIL_SW_NO_RT4 1
#define NPS_TAIL_SW_NO_RT8 2
#define NPS_TAIL_SW_RT4_LATE 4
#define NPS_TAIL_SW_NO_RT4H 8
#define NPS_TAIL_SW_RT8_WIDE 16
#define NPS_TAIL_SW_NO_STREAM 32
/* Host only (no GPU, no HIP call): the form nopesac_bottleneck_tail_bf16_ex launches for (C, C4, CN, C2) over M = B*OH*OW pixels under
 * the switch bits, or -1 for an unsupported configuration.  C2 = 0 for an identity block; x2_same_res: x2_H == OH and x2_W == OW.
 * *eligible (optional) receives the bitmask (1 << NPS_TAIL_*) of every form that can run the call, whatever the switches. */
int nopesac_bottleneck_tail_forms(int C, int C4, int CN, int C2, long long M, int x2_stride, int x2_same_res, int switches,
                                  unsigned* eligible);
/* nopesac_bottleneck_tail_bf16_ex on the given form.  A form that is not eligible for the call returns NPS_E_ARG before any HIP call. */
nps_status nopesac_bottleneck_tail_bf16_form(const void* b, const void* w3, const float* scale3, const float* bias3, const void* residual,
                                             const void* x2, const void* wsc, const float* scale_sc, const float* bias_sc, int B, int OH, int OW,
                                             int x2_H, int x2_W, int x2_stride, int C, int C4, int C2, void* y, const void* w1,
                                             const float* scale1, const float* bias1, int CN, void* o, int o_dt, int form, void* stream);

/* (x - mean[c]) / std[c], NCHW f32 -> NHWC (C padded with zeros to Cpad), out_dt f32/bf16.
 * siamese_planeTR.py:85-89,534-542. */
nps_status nopesac_preprocess_nchw_to_nhwc(const float* x, void* y, const float* mean, const float* std,
                                           int B, int C, int H, int W, int Cpad, int out_dt, void* stream);

/* max-pool K x K / stride / pad on NHWC (d2 BasicStem 3/2/1; camera_head.py:81-87 2/2/0). */
nps_status nopesac_maxpool_nhwc(const void* x, void* y, int B, int H, int W, int C, int K, int stride, int pad,
                                int dt, void* stream);

/* y = act(bilinear_x2(x) [align_corners=False]) (+ addend) ; planeTR_head.py:225,246-250. */
nps_status nopesac_upsample2x_bilinear_nhwc(const void* x, const void* addend, void* y, int B, int H, int W, int C,
                                            int act, int dt, void* stream);
/* y = lateral + nearest_x2(x) ; camera_modules.py:346. */
nps_status nopesac_upsample2x_nearest_add_nhwc(const void* x, const void* lateral, void* y, int B, int H, int W,
                                               int C, int dt, void* stream);

/* GroupNorm(G groups, eps) [+ReLU] on NHWC, per image; camera_modules.py:271-303 (d2 get_norm "GN").
 * workspace: nopesac_groupnorm_workspace_floats(B, G) = B * 16 * G * 2 floats of scratch for the split statistics (NULL selects the
 * slower single-kernel path).  The size is a value (0 for an argument <= 0). */
int64_t nopesac_groupnorm_workspace_floats(int B, int G);
nps_status nopesac_groupnorm_nhwc(const void* x, const float* gamma, const float* beta, void* y,
                                  int B, int HW, int C, int G, float eps, int act, int dt, float* workspace, void* stream);

/* y = LayerNorm(x [+ res]) * gamma + beta over the last dim D (<= 1024, multiple of 64);
 * optional second output y2 = y + addend (addend row index = row % addend_rows), used for the
 * "with_pos_embed" sums of transformer/transformer.py:180-199,304-321.  f32 only. */
nps_status nopesac_layernorm(const float* x, const float* res, const float* gamma, const float* beta,
                             float* y, const float* addend, int addend_rows, float* y2,
                             int rows, int D, float eps, void* stream);

/* Same, with optional bf16 copies of both results (y_bf16, y2_bf16) for the GEMMs that consume them; any of the four
 * outputs may be NULL (at least one must not be). */
nps_status nopesac_layernorm_ex(const float* x, const float* res, const float* gamma, const float* beta,
                                float* y, const float* addend, int addend_rows, float* y2, void* y_bf16, void* y2_bf16,
                                int rows, int D, float eps, void* stream);

/* out = a + b (b row index = row % b_rows); f32. */
nps_status nopesac_add_rows(const float* a, const float* b, float* out, int rows, int D, int b_rows, void* stream);

/* rows[b] = [t(3) | q(4) | n1 | n2 | m | t_err | r_err | pair_idx0 + b | nonfinite[0] | 0 | 0] as f32 [B][16]: the per-pair result rows
 * the runner all-gathers (the reference gathers the same numbers as python objects over Gloo, mp3d_evaluation.py:316-319).  t_err, r_err
 * and nonfinite (device int32[1]) may be NULL.  One launch, no host synchronisation. */
nps_status nopesac_metric_rows(const float* trans, const float* rot, const int32_t* n1, const int32_t* n2, const int32_t* m,
                               const float* t_err, const float* r_err, const int32_t* nonfinite, int pair_idx0, float* rows, int B, void* stream);

/* out[r] = [a[r] | b[r]] (f32 rows of Da and Db elements): the 7-vector (t, q) the matcher takes (camera_head.py:455). */
nps_status nopesac_concat_cols(const float* a, int Da, const float* b, int Db, float* out, int rows, void* stream);

/* a and a + b as bf16 (a_bf16, ab_bf16: [rows, D], D % 4 == 0): the operands of the first encoder layer's v and q|k projections
 * (src and src + pos, transformer.py: TransformerEncoderLayer.forward_post) in one pass over the f32 rows. */
nps_status nopesac_add_rows_bf16(const float* a, const float* b, void* a_bf16, void* ab_bf16, int rows, int D, int b_rows, void* stream);

/* row softmax over the last dim (<= 1024); camera_head.py:1131 (after the NHWC re-layout the 300
 * view-2 positions are the channel dim). f32. */
nps_status nopesac_softmax_rows(const float* x, float* y, int rows, int D, void* stream);

/* The same softmax written into rows of out_ld >= D elements (columns D .. out_ld-1 = 0), f32 or bf16 (out_dt = NPS_DT_F32 /
 * NPS_DT_BF16): the affinity volume in the channel-padded layout and the type the branch convs read (camera_head.py:1131-1133). */
nps_status nopesac_softmax_rows_pad(const float* x, void* y, int rows, int D, int out_ld, int out_dt, void* stream);

/* Multi-head softmax attention for short sequences (<= 512 keys), head dim 32.
 *   o[b,i,h,:] = softmax_j( scale * q[b,i,h,:].k[b,j,h,:] ) v[b,j,h,:]
 * q/k/v/o are row-major token matrices with arbitrary row strides (elements); batch b's rows start at
 * b*Lq (resp. b*Lk).  qlen/klen: optional int32[B] of valid rows per batch (NULL = all);
 * rows >= qlen[b] are written as zeros.  nn.MultiheadAttention (transformer/transformer.py:166,242-243)
 * and FullAttention (transformer/gnn.py:19-44). f32. */
nps_status nopesac_attention_small(const float* q, int64_t q_stride, const float* k, int64_t k_stride,
                                   const float* v, int64_t v_stride, float* o, int64_t o_stride,
                                   int B, int Lq, int Lk, int heads, float scale,
                                   const int32_t* qlen, const int32_t* klen, void* stream);

/* Same contract, mixed-precision MFMA kernel: q/k/v are rounded to bf16 while staged, scores / softmax
 * statistics / output accumulate in f32 (used when MODEL.AMD.COMPUTE_DTYPE = bfloat16). Rows 16-byte aligned. */
nps_status nopesac_attention_small_bf16(const float* q, int64_t q_stride, const float* k, int64_t k_stride,
                                        const float* v, int64_t v_stride, float* o, int64_t o_stride,
                                        int B, int Lq, int Lk, int heads, float scale,
                                        const int32_t* qlen, const int32_t* klen, void* stream);

/* Same kernel with q/k/v/o stored as bf16 (strides in elements, rows 16-byte aligned): the producing / consuming GEMMs round
 * to bf16 anyway, so this only halves the traffic. */
nps_status nopesac_attention_small_bf16io(const void* q, int64_t q_stride, const void* k, int64_t k_stride,
                                          const void* v, int64_t v_stride, void* o, int64_t o_stride,
                                          int B, int Lq, int Lk, int heads, float scale,
                                          const int32_t* qlen, const int32_t* klen, void* stream);

/* gather rows of a [B, H*W, C] map into (w,h) order: y[b, w*H + h, :] = x[b, h*W + w, :]
 * (camera_head.py:1120-1124). f32. */
nps_status nopesac_transpose_hw_rows(const float* x, float* y, int B, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Plane post-selection, fused (meta_arch/siamese_planeTR.py:625-803), per image.
 *   cls_logits f32[B,nq,2]; mask_prob f32[B,h,w,nq] = sigmoid(mask logits) at 1/4 resolution;
 *   params f32[B,nq,3]; query_feat f32[B,nq,D].
 * Outputs (caller-allocated, per image b):
 *   n_kept int32[B]; kept_idx int32[B,nq] (ascending query index, -1 padded);
 *   planes f32[B,nq,3]; feats f32[B,nq,D]; scores f32[B,nq]; areas int32[B,nq]; centers f32[B,nq,2];
 *   winner uint8[B,H,W]: low 7 bits = arg-max query id, bit 7 = weighted prob > mask_thr
 *       (plane masks are decoded from it: mask_q = (id==q) & bit7, or id==q in the fallback case);
 *   flags int32[B]: bit0 = zero_flag (no query passed the score test), bit1 = overlap fallback used.
 *   work int32[B, 9*nq+8]: scratch, zeroed by the call.
 */
nps_status nopesac_postselect_planes(const float* cls_logits, const float* mask_prob, const float* params,
                                     const float* query_feat,
                                     int B, int nq, int D, int h, int w, int H, int W,
                                     float score_thr, float mask_thr, float overlap_thr,
                                     int32_t* n_kept, int32_t* kept_idx, float* planes, float* feats, float* scores,
                                     int32_t* areas, float* centers, uint8_t* winner, int32_t* flags, int32_t* work,
                                     void* stream);
/* Same; prob_planar = 1: mask_prob is laid out [B,nq,h,w] (what nopesac_mask_head_bf16 writes with flag bit 1): only the planes
 * of the queries that pass the score test are read. */
nps_status nopesac_postselect_planes_ex(const float* cls_logits, const float* mask_prob, const float* params,
                                        const float* query_feat,
                                        int B, int nq, int D, int h, int w, int H, int W,
                                        float score_thr, float mask_thr, float overlap_thr,
                                        int32_t* n_kept, int32_t* kept_idx, float* planes, float* feats, float* scores,
                                        int32_t* areas, float* centers, uint8_t* winner, int32_t* flags, int32_t* work,
                                        int prob_planar, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Matching head tail: geometric priors + log-space Sinkhorn with dustbin + mutual-NN assignment,
 * one persistent workgroup per pair (matching_net/matching_head.py:75-96,113-128,228-306;
 * camera_net/camera_modules.py:15-34).
 *   desc_dot f32[B,nq,nq] = D1.D2^T / sqrt(256) (from nopesac_conv2d_nhwc batched);
 *   planes1/2 f32[B,nq,3]; cam7 f32[B,7] = (t, q); n1,n2 int32[B].
 *   log_scores f32[B,nq+1,nq+1]: rows/cols [0,n) are planes, index nq is the dustbin, the rest -inf-like
 *       padding (-1e30); assignment f32[B,nq,nq] in {0,1}.
 */
nps_status nopesac_matcher_sinkhorn(const float* desc_dot, const float* planes1, const float* planes2,
                                    const float* cam7, const int32_t* n1, const int32_t* n2,
                                    const float* bin_score, float offset_mult, float normal_mult,
                                    int iters, float match_thr, int B, int nq,
                                    float* log_scores, float* assignment, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Neural one-plane RANSAC, wavefront-level parts (camera_net/camera_head.py:512-569,925-1115).
 *
 * geo_sequence: matched pairs in row-major order of `assignment` -> geo_local f32[B,nq,6],
 *   geo_global f32[B,nq,6] (under init pose), sig f32[B,nq], geo_enc f32[B,nq,8] (the MLP input,
 *   :937-957), m int32[B].  (:1352-1425, :568-569)
 */
nps_status nopesac_geo_sequence(const float* assignment, const float* planes1, const float* planes2,
                                const int32_t* n1, const int32_t* n2, const float* init_trans, const float* init_rot,
                                int B, int nq, int warp_in_ref,
                                float* geo_local, float* geo_global, float* sig, float* geo_enc, int32_t* m,
                                void* stream);

/* hypothesis scoring maps (:990-1006,1018-1035): for pair b, hypothesis h in [0,nq] (0 = initial pose,
 * h>=1 from rot_raw/trans_raw row h-1) and matched pair j in [0,nq):
 *   normal_score[b,h,j] = exp(-|n(R_h p0_j) - n(flip p1_j)|) * mask, param_score[b,h,j] =
 *   exp(-|warp(p0_j; R_h,t_h) - flip p1_j|) * mask, mask = (h<=m)&(j<m).
 * Also writes rots_all f32[B,nq+1,4] (normalised) and trans_all f32[B,nq+1,3], and the diagnostic maps
 * l2_dist / normal_angle / offset_dist f32[B,nq+1,nq] if non-NULL, and the row sums used by
 * 'min-cost' (dn_sum, dl2_sum f32[B,nq+1]). */
nps_status nopesac_ransac_score_maps(const float* geo_local, const float* rot_raw, const float* trans_raw,
                                     const float* init_rot, const float* init_trans, const int32_t* m,
                                     int B, int nq,
                                     float* rots_all, float* trans_all, float* normal_score, float* param_score,
                                     float* l2_dist, float* normal_angle, float* offset_dist,
                                     float* dn_sum, float* dl2_sum, void* stream);

/* masked softmax over the m+1 hypotheses + soft / average aggregation of the 256-d pose features +
 * final pose regression (:1009-1014,1038-1087) and the m==0 / m<=1 special cases (:964-969,1068-1075).
 *   score_feat_{rot,trans} f32[B,nq+1,64] (outputs of the score MLPs), reg_{rot,trans}_{w f32[64], b f32[1]};
 *   init_{rot,trans}_feat f32[B,256]; fused_{rot,trans}_feat f32[B,nq,256] (already ReLU'd);
 *   rots_{w f32[4,256], b f32[4]}, trans_{w f32[3,256], b f32[3]}.
 *   mode: 0 soft, 1 avg-all, 2 min-cost, 3 max-score; + 16 = the TRAINING-side twin (__forward_PlaneCamRefHead,
 *   camera_head.py:737-923): no m == 0 / m <= 1 shortcuts, scores clamped to [0.01, 0.9], masked and renormalised
 *   (:814-818, :852-854), avg_* from the per-plane features only (:858-867), pred_* = the soft pose (:869-875).
 * Outputs: pred_rot f32[B,4], pred_trans f32[B,3], avg_rot f32[B,4], avg_trans f32[B,3],
 *   score_rot/score_trans f32[B,nq+1]. */
nps_status nopesac_ransac_soft_vote(const float* score_feat_rot, const float* score_feat_trans,
                                    const float* reg_rot_w, const float* reg_rot_b,
                                    const float* reg_trans_w, const float* reg_trans_b,
                                    const float* init_rot_feat, const float* init_trans_feat,
                                    const float* fused_rot_feat, const float* fused_trans_feat,
                                    const float* rots_w, const float* rots_b, const float* trans_w, const float* trans_b,
                                    const float* rots_all, const float* trans_all, const float* dn_sum, const float* dl2_sum,
                                    const float* init_rot, const float* init_trans, const int32_t* m,
                                    int B, int nq, int mode,
                                    float* pred_rot, float* pred_trans, float* avg_rot, float* avg_trans,
                                    float* score_rot, float* score_trans, void* stream);

/* The seven refinement losses of the training-side twin (camera_head.py:883-921, CameraPoseLoss camera_modules.py:355-365)
 * from the outputs of nopesac_ransac_score_maps (rots_all, trans_all, l2_dist - the diagnostic map is REQUIRED here) and
 * nopesac_ransac_soft_vote in mode 16 (pred_* = soft pose, avg_*, score_*); gt_pose f32[B,7] = trans | quaternion (normalised
 * inside), m int32[B] (>= 1 each, as in the reference: the parameter loss divides by it).
 * losses f32[7] = { tran_planeAvgReg, rot_planeAvgReg, tran_planeSoftReg, rot_planeSoftReg, rotIdx * 0.01, transIdx * 0.02,
 * paramL2_dist * 0.1 } * weight.  Its vector-Jacobian product is nopesac_refine_losses_backward. */
nps_status nopesac_plane_cam_ref_losses(const float* pred_rot, const float* pred_trans, const float* avg_rot,
                                        const float* avg_trans, const float* rots_all, const float* trans_all,
                                        const float* score_rot, const float* score_trans, const float* l2_dist,
                                        const int32_t* m, const float* gt_pose, int B, int nq, float weight,
                                        float* losses, void* stream);

/* CameraPoseLoss, reduce=True without mask (camera_modules.py:355-365) - also the form of the AIM's reconstruction losses
 * (camera_head.py:700-705, :725-731, with trans_eps = 1e-10 as the reference adds it to the re-embedded translation):
 *   out[0] = mean_b |gt_trans[b] + trans_eps - est_trans[b]|_2 * weight, out[1] = mean_b |n(gt_rot[b]) - n(est_rot[b])|_2 * weight.
 * est_trans f32[B,3], est_rot f32[B,4]; gt_trans / gt_rot are rows of `stride` floats (7 and 7 for a [B,7] pose tensor with
 * gt_rot = gt_pose + 3).  Its vector-Jacobian product (both pose arguments) is nopesac_camera_pose_loss_backward. */
nps_status nopesac_camera_pose_loss(const float* est_trans, const float* est_rot, const float* gt_trans, int gt_trans_stride,
                                    const float* gt_rot, int gt_rot_stride, int B, float trans_eps, float weight, float* out,
                                    void* stream);

/* assignment re-filter under the refined pose (:605-629): keep matches with normal angle < 45 deg and
 * offset distance < 1; `rot` is sign-canonicalised inside (w >= 0). In/out f32[B,nq,nq]. */
nps_status nopesac_refilter_assignment(const float* assignment_in, const float* planes1, const float* planes2,
                                       const int32_t* n1, const int32_t* n2, const float* rot, const float* trans,
                                       int B, int nq, float* assignment_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Launch tape (csrc/tape.hip): the host-side executor of a captured forward.  The reference submits its ~1700 kernels per pair from
 * the Python interpreter (inference_on_dataset, test_NopeSAC.py:157-179: one model(inputs) call per pair); here a static-shape
 * forward is captured once into a hipGraph, `nopesac_tape_create` reads the graph's nodes back (kernel function / grid / block /
 * dynamic LDS / argument block, memset and memcpy parameters) into a flat list in a dependency-respecting order, and
 * `nopesac_tape_replay` issues them as plain launches on `stream` - what the eager path enqueues, without Python (4-5 ms -> ~1 ms
 * per 32-pair forward) and without the whole-graph launch that serialises batches in flight.  `hip_graph` is a hipGraph_t that must
 * outlive the tape (its nodes own the argument blocks).  counts4 (optional) receives {kernels, memsets, memcpys, streams used}.  Unsupported node kinds (host callbacks, child graphs, memory nodes, module launches with packed arguments) -> NPS_E_ARG. */
nps_status nopesac_tape_create(void* hip_graph, void** tape_out, int32_t* counts4);
/* the same with a cap on the number of streams the tape may use (1 = everything on the caller's stream; default 4): parallel branches
 * of the captured graph (the capture's side streams) are issued on the tape's own side streams, joined by events. */
nps_status nopesac_tape_create_ex(void* hip_graph, int max_streams, void** tape_out, int32_t* counts4);
nps_status nopesac_tape_replay(void* tape, void* stream);
/* nopesac_tape_replay with the side chains on the caller's streams: side_streams[k] (hipStream_t) runs chain k + 1, a null / missing
 * entry falls back to the tape's own stream.  Two streams that share a hardware queue execute in submission order, so the placement
 * of the side chains decides how well replays of several tapes overlap (nopesac_amd/streams.py picks streams by queue). */
nps_status nopesac_tape_replay_on(void* tape, void* stream, void* const* side_streams, int n_side);
nps_status nopesac_tape_destroy(void* tape);

/* Diagnostic: `workgroups` x 256 threads fill `lds_bytes` of their LDS with a pattern, spin `spin_cycles`, verify, `rounds` times.
 * *count (uint32, zeroed by the caller) += mismatching dwords; log4 (optional, log_cap x 4 uint32) = {workgroup, dword, expected, found}
 * of the first mismatches.  Run on one stream while other kernels run on others (scripts/lds_victim.py). */
nps_status nopesac_lds_canary(int workgroups, int lds_bytes, int64_t spin_cycles, int rounds, uint32_t* count, uint32_t* log4, int log_cap,
                              void* stream);

/* BENCHMARK-ONLY K control (not part of the reference: it has no such knob - the reference benchmark would need
 * trained weights to keep K planes per view).  Per pair b: the K highest-scoring queries of view 1 (score = logits[b,q,0] -
 * logits[b,q,1], logits f32 [>=B, nq, n_cls]) in ascending query order become rows 0..K-1 of feats[b] (query_feat f32 [>=B,nq,D]);
 * feats[B+b, k] = feats[b, perm[b,k]] + noise[b,k] (perm int64 [B,K], noise f32 [B,K,D]); rows >= K are zeroed; n_kept[0..2B) = K.
 * One launch (the first version was 18 torch launches inside bench.py's timed region). */
nps_status nopesac_force_k_select(const float* logits, int n_cls, const float* query_feat, const int64_t* perm, const float* noise,
                                  int B, int nq, int K, int D, float* feats, int32_t* n_kept, void* stream);

/* small pose utilities on [B,*]: L2-normalise rows of a [rows,D] matrix (F.normalize, eps 1e-12),
 * optionally flip the sign so that component 0 >= 0 (camera_head.py:436-437,695-696). */
nps_status nopesac_normalize_rows(const float* x, float* y, int rows, int D, int canonical_sign, void* stream);

/* Adds the number of non-finite (Inf / NaN) values of x[0..n) to *count (int32 on the device, zeroed by the caller).  The reference
 * traps NaN poses with pdb.set_trace() (camera_net/camera_head.py:185-187, 681-682, 1072-1074); the drop-in counts them on the
 * device and raises FloatingPointError when the results are fetched (MODEL.AMD.CHECK_FINITE). */
nps_status nopesac_count_nonfinite(const float* x, int64_t n, int32_t* count, void* stream);
/* uint8 -> float32, exact (8-bit image planes handed over by the data mapper; the reference mapper converts on the host,
 * data/planercnn_transforms.py:225-227, and sends 4 bytes per sample over PCIe).  x, y 16-byte aligned device pointers. */
nps_status nopesac_u8_to_f32(const uint8_t* x, float* y, int64_t n, void* stream);

/* Engine-clock probe: one wave spins for spin_cycles shader cycles; out2[0] = shader cycles, out2[1] = 100 MHz reference ticks of
 * the same interval (device memory, 2 x uint64).  Shader clock [MHz] = 100 * out2[0] / out2[1].  Meant to be launched on a side
 * stream while a workload runs: it reads the clock the firmware grants under that load. */
nps_status nopesac_clock_probe(uint64_t* out2, int64_t spin_cycles, void* stream);

/* the same for up to NOPESAC_NONFINITE_MAX_TENSORS tensors in ONE launch: x / n are HOST arrays of device pointers / element counts */
#define NOPESAC_NONFINITE_MAX_TENSORS 16
nps_status nopesac_count_nonfinite_batch(const float* const* x, const int64_t* n, int n_tensors, int32_t* count, void* stream);

/* ---- Baseline-JPEG decode (the reference's image reader: detectron2 utils.read_image = PIL / libjpeg-turbo,
 * NopeSAC_Net/data/planercnn_transforms.py:210-227 and :306-314 - the ScanNet colour frames).  Bit-exact with libjpeg-turbo's default
 * decompression (JDCT_ISLOW, fancy upsampling, RGB).  The host (nopesac_amd/jpeg.py) walks the markers, splits the entropy-coded data
 * at the restart markers, removes the byte stuffing and lays out the tables; all arrays below are DEVICE memory:
 *   img32 [n_images][NOPESAC_JPEG_IMG_I32] int32: 0 width, 1 height, 2 components (1 | 3), 3 / 4 luma sampling h / v (1 | 2; chroma is
 *     1x1), 5 / 6 MCUs per row / column, 7 MCUs per restart interval (all of them when the file has none), 8..10 blocks per row of
 *     component c, 11..13 block rows, 14..16 downsampled_width, 17..19 downsampled_height, 20..22 index of the component's DC table
 *     (0 | 1), 23..25 index of its AC table (2 | 3), 26 first block of the image in the batch-wide block list, 27 its block count
 *   img64 [n_images][NOPESAC_JPEG_IMG_I64] int64: 0..2 element offset of component c's coefficients in `coef` ([block rows][blocks per
 *     row][64] int16, ZIGZAG order, DC prediction resolved), 3..5 byte offset of its sample plane in `planes` ([block rows * 8][blocks
 *     per row * 8] uint8), 6 byte offset (a multiple of 16) of the image in `out` ([height][width][3] uint8), 7 offset of the image's first interval in
 *     `words`; img32 28 / 29: first lane / subsequence count for nopesac_jpeg_huffman_parallel (29 = 0: not a parallel image)
 *   tables [n_images][NOPESAC_JPEG_TABLES_BYTES]: Huffman tables DC0, DC1, AC0, AC1 (NOPESAC_JPEG_HUFF_BYTES each: 9-bit look-ahead
 *     uint16[512] = (code length << 8) | symbol, 0 = longer code; maxcode int32[18]; valoffset int32[18]; huffval uint8[256] - jdhuff.c's
 *     derived table), then the components' quantisation tables uint16[64] in NATURAL order
 *   seg32 [n_segments][NOPESAC_JPEG_SEG_I32] int32: image, first MCU, MCU count, 0; seg64 [n_segments][NOPESAC_JPEG_SEG_I64] int64:
 *     offset into `words`, word count.  words: the intervals' bytes without the stuffing as 32-bit words, first bit = most significant,
 *     each interval followed by four zero words.
 * nopesac_jpeg_huffman: one wave per segment, n_words = length of `words`, `coef` zero-filled by the caller.  nopesac_jpeg_idct: n_blocks = sum of img32[.][27].
 * nopesac_jpeg_color: max_pixels = the largest width * height of the batch; bgr != 0 writes B, G, R. */
#define NOPESAC_JPEG_HUFF_BYTES 1536
#define NOPESAC_JPEG_TABLES_BYTES (4 * NOPESAC_JPEG_HUFF_BYTES + 3 * 128)
#define NOPESAC_JPEG_IMG_I32 32
#define NOPESAC_JPEG_IMG_I64 8
#define NOPESAC_JPEG_SEG_I32 4
#define NOPESAC_JPEG_SEG_I64 2
nps_status nopesac_jpeg_huffman(const int32_t* img32, const int64_t* img64, const uint8_t* tables, const int32_t* seg32, const int64_t* seg64,
                                int n_segments, const uint32_t* words, int64_t n_words, int16_t* coef, const int32_t* par_done, void* stream);
/* Files WITHOUT restart markers (one serial chain of codes per image): self-synchronising parallel decode.  The stream of image i is
 * cut into img32[i][29] subsequences of NOPESAC_JPEG_SUB_WORDS words, one lane each (lanes img32[i][28] .. of the batch-wide lane list,
 * every image's share padded to a multiple of 64 lanes; lane_img[lane] = image; img32[i][29] = 0: the image is left to
 * nopesac_jpeg_huffman; img64[i][7] = offset of the image's words).  Lanes decode from guessed states, then re-decode from their
 * predecessor's exit state for NOPESAC_JPEG_SYNC_PASSES passes (csrc/jpeg.hip); an image whose lanes no longer change gets
 * par_done[i] = 1 and its coefficients written (DC prediction resolved by a scan); par_done[i] = 0: call nopesac_jpeg_huffman with
 * the same par_done afterwards - it decodes exactly the images still open.  Work arrays (device, n_lanes entries unless noted):
 * exit_state, entry_used (int64, entry_used initialised to -1), n_blk (int32), first_block (int64), changed (int32
 * [NOPESAC_JPEG_SYNC_PASSES][n_images], zeroed), par_done (int32 [n_images], zeroed). */
/* HOST function (no device work, thread-safe): one pass over the entropy-coded bytes that follow a scan header - stuffed zero bytes
 * removed, the stream cut at RSTn markers when has_restart != 0, every interval written to `words` as 32-bit words whose most
 * significant bit is the first bit of the stream, padded to whole words and followed by four zero words (the layout
 * nopesac_jpeg_huffman / _parallel read).  seg_off / seg_cnt / seg_bytes [max_segs]: word offset, word count and byte length of every
 * interval; *consumed = offset of the marker that ended the scan (or n).  Returns the number of intervals, -1 when `words` (capacity
 * words_cap; n / 4 + 5 * max_segs + 8 always suffices) or max_segs is too small.  (RSTn inside a scan without a restart interval
 * ends the scan like any other marker: has_restart = 0.) */
int64_t nopesac_jpeg_prepare_scan(const uint8_t* data, int64_t n, int has_restart, uint32_t* words, int64_t words_cap, int64_t* seg_off,
                                  int64_t* seg_cnt, int64_t* seg_bytes, int64_t max_segs, int64_t* consumed);
/* HOST functions: the whole host side of a BATCH of JPEG files on the library's own threads (csrc/jpeg_host.hip) - file read, marker walk,
 * supported-subset checks, nopesac_jpeg_prepare_scan, derived Huffman tables and the launch arrays above; replaces the per-file Python of
 * nopesac_amd/jpeg.py (parse_markers / prepare_batch), i.e. the reference's per-image utils.read_image call (planercnn_transforms.py:306-314),
 * which held the interpreter lock next to the thread that launches the model.
 *   scan:  status[n] = 0 or why file i keeps the batch off this path (-1 not a JPEG, -2 unsupported, -3 malformed, -6 unreadable);
 *          totals[8] = words, restart intervals, lanes, 8x8 blocks, largest image (pixels), coef / plane / output elements of the batch;
 *          returns an opaque batch (NULL on bad arguments);
 *   fill:  only if every status is 0: img32 [n][32], img64 [n][8], tables [n][TABLES_BYTES], seg32 [segs][4], seg64 [segs][2], words,
 *          lane_img [lanes] (NULL if none), geometry [n][2] = (height, width); 0, -1 bad arguments, -2 bad Huffman table;
 *   free:  always. */
void* nopesac_jpeg_batch_scan_host(const char* const* paths, int n, int threads, int parallel, int* status, int64_t* totals);
int nopesac_jpeg_batch_fill_host(void* batch, int32_t* img32, int64_t* img64, uint8_t* tables, int32_t* seg32, int64_t* seg64, uint32_t* words,
                                 int32_t* lane_img, int32_t* geometry);
void nopesac_jpeg_batch_free_host(void* batch);
#define NOPESAC_JPEG_SUB_WORDS 64
#define NOPESAC_JPEG_SYNC_PASSES 12
nps_status nopesac_jpeg_huffman_parallel(const int32_t* img32, const int64_t* img64, const uint8_t* tables, int n_images, const int32_t* lane_img,
                                         int64_t n_lanes, const uint32_t* words, int64_t n_words, int64_t* exit_state, int64_t* entry_used,
                                         int32_t* n_blk, int64_t* first_block, int32_t* changed, int32_t* par_done, int16_t* coef, void* stream);
nps_status nopesac_jpeg_idct(const int32_t* img32, const int64_t* img64, const uint8_t* tables, int n_images, int n_blocks, const int16_t* coef,
                             uint8_t* planes, void* stream);
nps_status nopesac_jpeg_color(const int32_t* img32, const int64_t* img64, int n_images, int max_pixels, const uint8_t* planes, uint8_t* out,
                              int bgr, void* stream);

/* Result fetch (replaces the per-tensor `.cpu()` copies of siamese_planeTR.py:384-450 at the drop-in boundary): n_segments byte
 * ranges (HOST arrays of device pointers / sizes / destination offsets, n_segments <= NOPESAC_GATHER_MAX_SEGMENTS) are copied into
 * `dst` by ONE kernel.  dst is device memory or device-mapped pinned host memory (hipHostMalloc / torch pin_memory): the latter is the
 * intended use - the batch's small result tensors reach the host in one launch that a captured graph can hold.  Ranges may be
 * unaligned (16-byte vectors are used when a segment's source and destination addresses allow it).  size_dev: NULL, or a HOST array
 * of device pointers (entries may be NULL) to the number of VALID bytes of a segment when only the device knows it (the run-length
 * strings of a batch: a buffer of fixed capacity, filled to a data-dependent length); min(size[i], *size_dev[i]) bytes are copied. */
#define NOPESAC_GATHER_MAX_SEGMENTS 32
nps_status nopesac_gather_bytes(const void* const* src, const int64_t* size, const int64_t* const* size_dev, const int64_t* dst_off,
                                int n_segments, void* dst, void* stream);

/* One GNN layer of the plane matcher (transformer/gnn.py:73-96) for n_sets plane sets, one workgroup per set, bf16 MFMA
 * operands / f32 residual stream (csrc/gnn_layer.hip).  Feature buffers are f32 [sets][nq][256] (nq <= 64); workgroup b updates
 * set x_off + b attending to set src_off + b (same buffer and offset = 'self' layer) and writes set out_off + b of `out`
 * (out may share a buffer with x / src only for disjoint set ranges).  qlen / klen: int32 valid rows per set, indexed like
 * x / src (NULL = nq).  All six weight matrices are bf16 in MFMA fragment-major order (see nopesac_bottleneck_tail_bf16):
 * wq (pre-multiplied by 1/sqrt(32)), wk, wv, wmerge [256][256]; w0 = mlp.0 [512][512] (input = [x | msg]); w2 = mlp.2 [256][512]. */
nps_status nopesac_gnn_layer_bf16(const float* x, int x_off, const float* src, int src_off, float* out, int out_off, int n_sets, int nq,
                                  const int32_t* qlen, const int32_t* klen, const void* wq, const void* wk, const void* wv,
                                  const void* wmerge, const void* w0, const void* w2, const float* ln1_g, const float* ln1_b,
                                  const float* ln2_g, const float* ln2_b, void* stream);
/* The same launch + a weight prefetch for the NEXT one (one pair per call: one or two workgroups per launch, each layer's 1.28 MB of
 * weights cold in L2): next_weights6 = HOST array of the next launch's six fragment-major weight pointers (wq, wk, wv, wmerge, w0,
 * w2), next_sets = its n_sets; 128 extra workgroups of this launch, dealt over the XCDs like the next launch's workgroups will be,
 * read those weights into the L2s that will need them and exit.  No prefetch workgroups are added when this launch has more than 16
 * layer workgroups.  next_weights6 = NULL: exactly nopesac_gnn_layer_bf16. */
nps_status nopesac_gnn_layer_bf16_pf(const float* x, int x_off, const float* src, int src_off, float* out, int out_off, int n_sets,
                                     int nq, const int32_t* qlen, const int32_t* klen, const void* wq, const void* wk, const void* wv,
                                     const void* wmerge, const void* w0, const void* w2, const float* ln1_g, const float* ln1_b,
                                     const float* ln2_g, const float* ln2_b, const void* const* next_weights6, int next_sets, void* stream);

/* Finest top-down level + mask head of the PlaneTR head in one launch (planeTR_head.py:148-162, 241-252), bf16:
 *   p1 = relu(scale * (w_lateral . c1) + bias) + relu(bilinear_2x(t1));   prob = [sigmoid](mask_w[b] . p1 + mask_b[b])
 * c1 [B,H,W,256], t1 [B,H/2,W/2,256] bf16; w_lateral [256][256] and mask_w [B][NQP][256] (rows >= nq zero) bf16 in MFMA
 * fragment-major order; mask_b f32 [B][NQP]; NQP = 64 for nq <= 64, 128 for nq <= 128; prob f32 [B,H,W,nq] (nq even, <= 128);
 * p1_out optional bf16 [B,H,W,256].
 * H*W must be a multiple of 128.  apply_sigmoid: bit 0 = apply the sigmoid, bit 1 = write prob planar, [B,nq,H,W], bit 2 = tuning
 * aid / test: one pixel per item in the bilinear phase (default: four consecutive pixels share their eight taps; identical results). */
nps_status nopesac_mask_head_bf16(const void* c1, const void* t1, const void* w_lateral, const float* scale, const float* bias,
                                  const void* mask_w, const float* mask_b, float* prob, void* p1_out, int B, int H, int W, int nq,
                                  int apply_sigmoid, void* stream);

/* The two per-image operands of nopesac_mask_head_bf16 from the folded plane embeddings (fold f32 [B * nq][ld]: columns 0..255 mask
 * weights, column 256 mask bias - the pixel-embedding conv folded into the plane-embedding MLP, planeTR_head.py:170-188): mask_w bf16
 * in the kernel's per-image MFMA fragment order for nqp = 64 / 128 planes (planes >= nq zero), mask_b f32 [B][nqp].  One launch. */
nps_status nopesac_mask_operands(const float* fold, int ld, void* mask_w, float* mask_b, int B, int nq, int nqp, void* stream);

/* Tail of one post-norm transformer encoder layer (transformer/transformer.py:183-199) for M tokens of width 256, FFN 1024:
 *   y1 = LN1(src + attn . wo^T + bo);  y2 = LN2(y1 + relu(y1 . w1^T + b1) . w2^T + b2)
 * attn bf16 [M][256] (attention output), src f32 [M][256]; wo [256][256], w1 [1024][256], w2 [256][1024] bf16 in MFMA
 * fragment-major order; outputs (each nullable): y f32, y_bf16, ypos_bf16 = bf16(y2 + pos[token % pos_rows]). */
nps_status nopesac_encoder_tail_bf16(const void* attn, const float* src, const void* wo, const float* bo, const float* ln1_g,
                                     const float* ln1_b, const void* w1, const float* b1, const void* w2, const float* b2,
                                     const float* ln2_g, const float* ln2_b, const float* pos, int pos_rows, float* y, void* y_bf16,
                                     void* ypos_bf16, int M, void* stream);

/* cv2.resize(img, (OW, OH)) with the default INTER_LINEAR on uint8 HWC images (the ScanNet input path,
 * data/planercnn_transforms.py:314): OpenCV's 11-bit fixed-point algorithm (csrc/resize.hip). src [H][W][C], dst [OH][OW][C]. */
nps_status nopesac_resize_bilinear_u8(const uint8_t* src, int H, int W, int C, uint8_t* dst, int OH, int OW, void* stream);
/* The same for n images of one size that lie src_stride bytes apart (the GPU JPEG decoder's output buffer), one launch; chw = 1: dst is
 * [n][C][OH][OW] (the mapper's CHW tensors: the reference's transpose after cv2.resize, planercnn_transforms.py:314-320), else [n][OH][OW][C]. */
nps_status nopesac_resize_bilinear_u8_batch(const uint8_t* src, int n, int64_t src_stride, int H, int W, int C, uint8_t* dst, int OH, int OW, int chw,
                                            void* stream);

/* Training-time image augmentation (csrc/augment.hip): the reference mapper's ColorJitter / RandomGrayscale / GaussianBlur chain
 * (data/planercnn_transforms.py:183-191, data/augmentation.py:22) on n uint8 HWC images of one size, src_stride bytes apart, with
 * Pillow's 8-bit arithmetic per pixel.  One nopesac_aug_row per image: flags (NPS_AUG_JITTER | NPS_AUG_GREY | NPS_AUG_BLUR), the
 * order the four jitter operations run in (a permutation of NPS_AUG_BRIGHTNESS .. NPS_AUG_HUE), their factors indexed by operation,
 * and the blur's sigma.  A row without flags copies its image.  Channels are taken in MEMORY order (channel 0 is Pillow's red). */
#define NPS_AUG_OPS 4
#define NPS_AUG_BRIGHTNESS 0
#define NPS_AUG_CONTRAST 1
#define NPS_AUG_SATURATION 2
#define NPS_AUG_HUE 3
#define NPS_AUG_JITTER 1
#define NPS_AUG_GREY 2
#define NPS_AUG_BLUR 4
#define NPS_AUG_MAX_SIGMA 2 /* the reference draws sigma from [0.1, 2.0]: box radius 0 or 1, six passes reach NPS_AUG_APRON pixels */
#define NPS_AUG_APRON 6
#define NPS_AUG_TILE 32     /* the fused pass works on NPS_AUG_TILE x NPS_AUG_TILE output pixels per workgroup */
#define NPS_AUG_PARTIALS 64 /* luma partial sums per image of the contrast pre-pass */
typedef struct nopesac_aug_row {
    int flags;
    int order[NPS_AUG_OPS];
    float factor[NPS_AUG_OPS];
    float sigma;
} nopesac_aug_row;
/* nopesac_augment_workspace_bytes: bytes[0] = n * NPS_AUG_PARTIALS * 4, the uint32 luma partials of the contrast pre-pass (0 for an
 * argument <= 0; H and W do not enter it).  bytes is a HOST pointer; a status, not a value: null bytes is NPS_E_ARG. */
nps_status nopesac_augment_workspace_bytes(int n, int H, int W, int64_t* bytes);
/* rows_host: the table in HOST memory, checked here before any launch; rows_dev: the same table in device memory, read by the kernels.
 * Outputs (each nullable, at least one): chw_out uint8 [n][3][H][W]; nhwc_out f32 [n][H][W][4] = (v - mean[c]) / std[c] with a zero pad
 * channel (what nopesac_preprocess_nchw_to_nhwc writes from the float image; mean, std: f32[3] on the device).
 * NPS_E_ARG before any launch: C != 3, H * W * 255 >= 2^32, a workspace shorter than nopesac_augment_workspace_bytes states, unknown flags, an
 * order that is no permutation of 0-3, a hue factor outside [-0.5, 0.5], sigma <= 0 or > NPS_AUG_MAX_SIGMA.  Two launches (contrast
 * luma partials in fixed order, then the fused pass); deterministic. */
nps_status nopesac_augment_u8(const uint8_t* src, int n, int64_t src_stride, int H, int W, int C, const nopesac_aug_row* rows_host,
                              const nopesac_aug_row* rows_dev, uint8_t* chw_out, float* nhwc_out, const float* mean, const float* std,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* Ground truth for training (csrc/train_targets.hip; nopesac_amd/targets.py): a dataset's per-view record -> the targets of
 * nopesac_plane_criterion (prepare_targets, siamese_planeTR.py:475-532; get_coordinate_map, :815-839).  Deterministic: integer sums, and
 * tables whose CONTENT does not depend on the order of their atomics.  Argument errors -> NPS_E_ARG before any launch.
 * nopesac_label_ids: labels int32 [B][H][W] (any int32 value) -> per image the distinct values in ascending SIGNED order, the first
 *   dropped when it is 0 (torch.unique, then `if plane_ids[0] == 0`: with a negative label present 0 stays a plane): ids int32
 *   [B][NPS_LABEL_MAX_IDS] (0 from n_all[b] on), n_all[b] = their number, n[b] = min(n_all[b], nmax_limit), bad[b] = 1 when the image holds
 *   more than NPS_LABEL_MAX_IDS distinct values (0 included) - then n_all[b] = n[b] = 0 and the row of ids is 0.  One workgroup per image:
 *   an open-addressed table of NPS_LABEL_TABLE_SLOTS slots in LDS (slot = value mod slots, linear probing), then a rank sort.
 * nopesac_label_targets: labels, ids (row stride NPS_LABEL_MAX_IDS, ascending), n int32 [B] (clamped to [0, nmax]) -> masks uint8
 *   [B][nmax][H][W] = (ids[b][j] == label), rows j >= n[b] zero; plane_centers f32 [B][nmax][2] = (float)(sum x / W / count), (float)(sum y / H
 *   / count) in f64 from exact integer sums (what nopesac_plane_targets computes from the masks, bit for bit), rows j >= n[b] zero;
 *   pixel_centers f32 [B][2][H][W] = the centre of the pixel's plane, 0 where no plane lies.  1 <= nmax <= NPS_PLANE_MAX_TARGETS, H W <= 2^30.
 *   Three launches: integer partial sums per NPS_LABEL_CHUNK pixels into the workspace (nopesac_label_targets_workspace_bytes writes
 *   its size to the HOST pointer `bytes`, 0 for an argument <= 0; a status: null bytes is NPS_E_ARG), the centres, then the mask pass (the label map is read once per pixel, every plane row written from registers,
 *   16 bytes per lane where H W % 16 == 0 and the buffers are 16-byte aligned).
 * nopesac_bits_to_masks: bits int32 [n_rows][ceil(H W / 32)] in the layout of nopesac_rle_runs_to_bits (bit p & 31 of word p >> 5 is pixel
 *   p = x H + y), offsets int64 [B + 1] on the device (view b owns rows offsets[b] .. offsets[b + 1]) -> masks uint8 [B][nmax][H][W]
 *   row-major; a view with more than nmax rows keeps its first nmax, the rows it lacks are zero.
 * nopesac_depth_u16_to_f32: out[i] = (float)src[i] / scale, an IEEE division (the reference's astype(float32) / 1000.), scale > 0.
 * nopesac_coordinate_map: kinv f32 [B][9] row-major (the host inverts K in f64 and rounds once) -> out f32 [B][3][H][W],
 *   out[c] = fma(kinv[3c + 1], y, kinv[3c] * x) + kinv[3c + 2] with x = (float)col / W * 640, y = (float)row / H * 480 in f32. */
#define NPS_LABEL_MAX_IDS 1024
#define NPS_LABEL_TABLE_SLOTS 2048
#define NPS_LABEL_CHUNK 4096
nps_status nopesac_label_ids(const int32_t* labels, int B, int H, int W, int nmax_limit, int32_t* ids, int32_t* n_all, int32_t* n,
                             int32_t* bad, void* stream);
nps_status nopesac_label_targets_workspace_bytes(int B, int nmax, int H, int W, int64_t* bytes);
nps_status nopesac_label_targets(const int32_t* labels, const int32_t* ids, const int32_t* n, int B, int nmax, int H, int W, uint8_t* masks,
                                 float* plane_centers, float* pixel_centers, void* workspace, int64_t workspace_bytes, void* stream);
nps_status nopesac_bits_to_masks(const int32_t* bits, int64_t n_rows, const int64_t* offsets, int B, int nmax, int H, int W, uint8_t* masks,
                                 void* stream);
nps_status nopesac_depth_u16_to_f32(const uint16_t* src, int64_t n, float scale, float* out, void* stream);
nps_status nopesac_coordinate_map(const float* kinv, int B, int H, int W, float* out, void* stream);

/* Pre-norm counterpart for the decoder layers (transformer/transformer.py:293-322, after the cross-attention), same kernel:
 *   s = tgt + attn . wo^T + bo;  u = s + relu(LN3(s) . w1^T + b1) . w2^T + b2;  n = LN_next(u)
 * y = u (f32 residual stream), y_bf16 = bf16(n), ypos_bf16 = bf16(n + pos[row % pos_rows]), yn = n in f32 (each nullable);
 * LN_next = the next layer's norm1, or the decoder's final norm after the last layer. */
nps_status nopesac_decoder_tail_bf16(const void* attn, const float* tgt, const void* wo, const float* bo, const float* ln3_g,
                                     const float* ln3_b, const void* w1, const float* b1, const void* w2, const float* b2,
                                     const float* lnn_g, const float* lnn_b, const float* pos, int pos_rows, float* y, void* y_bf16,
                                     void* ypos_bf16, float* yn, int M, void* stream);

/* General form of the two tails above, followed by the input projections of the NEXT attention - one launch:
 *   pre_norm = 0 (encoder layer, transformer.py:183-199):  n = LN_b(y1 + FFN(y1)), y1 = LN_a(src + out_proj(attn));  y = n
 *   pre_norm = 1 (decoder layer after the cross-attention, :308-322):  u = s + FFN(LN_a(s)), s = src + out_proj(attn); n = LN_b(u); y = u
 *   skip_ffn = 1 (decoder layer after the SELF-attention, :300-306):  s = src + out_proj(attn), n = LN_a(s), y = s (w1 / w2 / ln_b unused)
 *   proj_pos [M][n_pos] = bf16((n + pos) Wpos^T + bpos),  proj [M][n_proj] = bf16(n Wp^T + bp): the next self-attention's q|k and v, or
 *   the cross-attention's q (nn.MultiheadAttention in_proj slices); weights in mfma_fragment_major order (K = 256), widths multiples of 32.
 * Outputs y / y_bf16 / ypos_bf16 / yn as in the two entries above; every output is optional (at least one). */
nps_status nopesac_transformer_tail_bf16(const void* attn, const float* src, const void* wo, const float* bo, const float* lna_g,
                                         const float* lna_b, const void* w1, const float* b1, const void* w2, const float* b2,
                                         const float* lnb_g, const float* lnb_b, const float* pos, int pos_rows, float* y, void* y_bf16,
                                         void* ypos_bf16, float* yn, int pre_norm, int skip_ffn, const void* w_pos, const float* b_pos,
                                         void* proj_pos, int n_pos, const void* w_proj, const float* b_proj, void* proj, int n_proj, int M,
                                         void* stream);
/* The same launch + a weight prefetch for the NEXT one (few workgroups - one pair per call): next_ptrs / next_bytes = HOST arrays of up to
 * 8 device byte ranges (the next tail's wo / w1 / w2 and projection matrices), next_workgroups = the next launch's workgroup count; with
 * at most 64 layer workgroups in THIS launch, 128 extra workgroups read those ranges into the L2s of the XCDs the next launch will
 * run on and exit (csrc/enc_tail.hip, like nopesac_gnn_layer_bf16_pf).  n_next = 0: exactly nopesac_transformer_tail_bf16. */
nps_status nopesac_transformer_tail_bf16_pf(const void* attn, const float* src, const void* wo, const float* bo, const float* lna_g,
                                            const float* lna_b, const void* w1, const float* b1, const void* w2, const float* b2,
                                            const float* lnb_g, const float* lnb_b, const float* pos, int pos_rows, float* y, void* y_bf16,
                                            void* ypos_bf16, float* yn, int pre_norm, int skip_ffn, const void* w_pos, const float* b_pos,
                                            void* proj_pos, int n_pos, const void* w_proj, const float* b_proj, void* proj, int n_proj, int M,
                                            const void* const* next_ptrs, const int64_t* next_bytes, int n_next, int next_workgroups, void* stream);

/* The kernel forms of the transformer tail (csrc/enc_tail.hip).  The 64- / 96- / 128-token kernels compute the post-norm tail only
 * (pre_norm = 0, skip_ffn = 0); the 32-token kernel computes every form with n_pos + n_proj <= 1024. */
#define NPS_ETAIL_32 0       /* enc_tail_kernel: 32 tokens per workgroup, the only form with the weight prefetch of the _pf entry */
#define NPS_ETAIL_64 1       /* enc_tail64_kernel: 64 tokens, bit-identical to the 32-token kernel */
#define NPS_ETAIL_96 2       /* enc_tail128_kernel with 3 row tiles: 96 tokens */
#define NPS_ETAIL_128 3      /* enc_tail128_kernel with 4 row tiles: 128 tokens */
#define NPS_ETAIL_FORMS 4
/* A/B switch bits of the default selection, from the environment at every call: NOPESAC_ENC_TAIL_32 set, NOPESAC_ENC_TAIL_64 set,
 * NOPESAC_ENC_TAIL_ROWS set, and NOPESAC_ENC_TAIL_ROWS = 3 (any other value forces 128 tokens). */
#define NPS_ETAIL_SW_32 1
#define NPS_ETAIL_SW_64 2
#define NPS_ETAIL_SW_ROWS 4
#define NPS_ETAIL_SW_ROWS3 8
/* Host only (no GPU, no HIP call): the form the transformer_tail / encoder_tail / decoder_tail entries launch for M tokens under the switch
 * bits (n_proj_total = n_pos + n_proj of the requested projections).  *eligible (optional) receives the bitmask (1 << NPS_ETAIL_*) of every
 * form that computes the call correctly, whatever the switches; the default is not in it when n_proj_total > 1024 (the call is refused).
 * The result is a form id, NPS_ETAIL_32 .. NPS_ETAIL_128 (never negative). */
int nopesac_transformer_tail_forms(long long M, int pre_norm, int skip_ffn, long long n_proj_total, int switches, unsigned* eligible);
/* nopesac_transformer_tail_bf16_pf on the given form.  A form that is not eligible for the call returns NPS_E_ARG before any HIP call. */
nps_status nopesac_transformer_tail_bf16_form(const void* attn, const float* src, const void* wo, const float* bo, const float* lna_g,
                                              const float* lna_b, const void* w1, const float* b1, const void* w2, const float* b2,
                                              const float* lnb_g, const float* lnb_b, const float* pos, int pos_rows, float* y, void* y_bf16,
                                              void* ypos_bf16, float* yn, int pre_norm, int skip_ffn, const void* w_pos, const float* b_pos,
                                              void* proj_pos, int n_pos, const void* w_proj, const float* b_proj, void* proj, int n_proj, int M,
                                              const void* const* next_ptrs, const int64_t* next_bytes, int n_next, int next_workgroups, int form,
                                              void* stream);

/* ---- COCO RLE of the kept plane masks (replaces pycocotools.mask.encode / toBbox at
 *      meta_arch/siamese_planeTR.py:703-704, 747-748; consumed by evaluation/mp3d_evaluation.py:203-205) ----
 * labels: winner uint8[V,H,W] (+ kept_idx int32[V,nq], n_kept int32[V], flags int32[V] from nopesac_postselect_planes)
 *   -> uint8[V,W,H] COLUMN-major map of kept-plane ordinals (0xFF = none; bit-7 test skipped when flags bit1 = fallback). */
nps_status nopesac_rle_labels(const uint8_t* winner, const int32_t* kept_idx, const int32_t* n_kept, const int32_t* flags,
                              uint8_t* labels, int V, int H, int W, int nq, void* stream);
/* transitions: counts int32[V,nq] = number of 0<->1 flips of plane p's mask along the column-major scan (N = H*W);
 *   if positions != NULL the ascending flip positions of (v,p) are written at positions[offsets[v*nq+p] ...]
 *   (call once with NULLs to size, exclusive-scan the counts, call again). */
nps_status nopesac_rle_transitions(const uint8_t* labels, const int32_t* n_kept, const int64_t* offsets, int32_t* counts,
                                   uint32_t* positions, int V, int N, int nq, void* stream);
/* Dense boolean masks of the kept planes of V views in one launch (`pred_plane_masks`, siamese_planeTR.py:685 / :743): for view v and
 * its p-th kept plane, masks[(offsets[v] + p) * H * W + pixel] = 1 iff the pixel's arg-max query is kept_idx[v][p] and the pixel
 * passed the mask threshold (bit 7 of the winner byte) or the view is a fallback view (flags bit 1).  offsets: device int64 [V],
 * exclusive prefix sums of n_kept.  masks: uint8 [sum(n_kept), H, W]. */
nps_status nopesac_decode_masks(const uint8_t* winner, const int32_t* kept_idx, const int32_t* n_kept, const int32_t* flags,
                                const int64_t* offsets, uint8_t* masks, int V, int H, int W, int nq, void* stream);

/* HOST function (no device work): one mask's flip positions -> COCO compressed "counts" string (not NUL terminated,
 *   returns its length, or NPS_E_ARG with nopesac_last_error set: bad arguments, `cap` too small) and bbox4 = [x, y, w, h] (cocoapi
 *   rleToString / rleToBbox). */
int nopesac_rle_compress_host(const uint32_t* positions, int n_pos, int H, int W, char* out, int cap, double* bbox4);
/* The same on the device for n_masks masks at once (mask i owns positions[offsets[i] .. offsets[i] + counts[i]); all pointers device
 * memory).  Pass 1, out == NULL: lens[i] = length of mask i's string, bbox4[4 i ..] = its [x, y, w, h] box.  Pass 2, out != NULL: the
 * strings are written at out + out_off[i] (the caller's exclusive prefix sums of lens). */
nps_status nopesac_rle_compress_device(const uint32_t* positions, const int64_t* offsets, const int32_t* counts, int n_masks, int H, int W,
                                       int32_t* lens, double* bbox4, char* out, const int64_t* out_off, void* stream);
/* Pass 2 of nopesac_rle_compress_device into a buffer of fixed capacity `cap` bytes, so that the caller needs no host round trip for
 * the total string length: string i is written at out + out_off[i] only when out_off[i] + lens[i] <= cap (lens: pass 1's output).
 * The strings' consumer (siamese_planeTR.py:703-720, instances[k]["segmentation"]) gets the same bytes as from the unbounded form. */
nps_status nopesac_rle_compress_device_capped(const uint32_t* positions, const int64_t* offsets, const int32_t* counts, int n_masks, int H, int W,
                                              const int32_t* lens, char* out, const int64_t* out_off, int64_t cap, void* stream);
/* Batch form of nopesac_rle_compress_host: mask i owns positions[offsets[i] .. +counts[i]); strings are packed back to back into
 * `out` (mask i at out + out_off[i], out_off[n_masks] = total), boxes at bbox4 + 4 i.  Returns the total length, or NPS_E_ARG with
 * nopesac_last_error set. */
long long nopesac_rle_compress_batch_host(const uint32_t* positions, const long long* offsets, const int* counts, int n_masks,
                                          int H, int W, char* out, long long cap, long long* out_off, double* bbox4);

/* ---- plane AP evaluator (evaluation/mp3d_evaluation.py:467-743 `evaluate_for_planes` and the pycocotools.mask.iou it calls) ----
 * Ragged quantities use exclusive-offset arrays, int64 [n + 1], so that one launch serves every view of a batch.  Pixel order is
 * COCO's column-major scan p = x H + y; bit p of a mask is bit (p & 31) of word (p >> 5); a mask has ceil(H W / 32) words and the
 * unused high bits of its last word are zero.  All four are deterministic (integer counts, no atomics); n_masks = 0 / V = 0 is a
 * valid call that enqueues nothing.
 * string_runs: compressed COCO `counts` strings (cocoapi rleFrString), concatenated in `bytes`, string i = bytes[str_off[i] ..
 *   str_off[i + 1]) -> run lengths.  A mask has at most as many runs as bytes: mask i's runs go to runs + str_off[i] (runs: int32
 *   [str_off[n_masks]]) and their count to n_runs[i]. */
nps_status nopesac_rle_string_runs(const uint8_t* bytes, const int64_t* str_off, int n_masks, int32_t* runs, int32_t* n_runs, void* stream);
/* runs_to_bits: mask i owns runs[run_off[i] .. run_off[i] + n_runs[i]) (n_runs[i] <= run_off[i + 1] - run_off[i]); odd-indexed runs
 *   are ones.  bits uint32 [n_masks, ceil(H W / 32)], area int32 [n_masks] (number of ones), bad int32 [n_masks]: 1 when a run is
 *   negative, the running sum passes H W, the runs do not sum to H W, or n_runs[i] does not fit its slice - the mask's words are then
 *   zero and its area 0.  starts: int32 scratch laid out like runs (the first pixel of every run).  H W < 2^31 - 32. */
nps_status nopesac_rle_runs_to_bits(const int32_t* runs, const int64_t* run_off, const int32_t* n_runs, int n_masks, int H, int W,
                                    int32_t* starts, uint32_t* bits, int32_t* area, int32_t* bad, void* stream);
#define NPS_POLY_COORD_MAX 536870912  /* poly_to_bits: |5 x + 0.5| of every coordinate must stay below this (2^29) */
#define NPS_POLY_POINT_FACTOR 16      /* poly_to_bits: a polygon may have at most NPS_POLY_POINT_FACTOR (H W + H + W) + */
#define NPS_POLY_POINT_FLOOR 1048576  /*   NPS_POLY_POINT_FLOOR upsampled boundary points */
/* poly_to_bits: COCO polygon lists -> masks in the layout of runs_to_bits (csrc/plane_eval.hip): cocoapi's rleFrPoly per polygon
 *   (upsampling by 5, truncating casts, crossings at x H + y, y clamped to [0, H]) and rleMerge(intersect = 0) across a mask's
 *   polygons, bit for bit.  xy: double [2 n_points], all polygons concatenated, x first; polygon j owns points poly_off[j] ..
 *   poly_off[j + 1] (int64 [n_polys + 1]); mask i owns polygons mask_off[i] .. mask_off[i + 1] (int64 [n_masks + 1]).
 *   bits uint32 [n_masks, ceil(H W / 32)], area int32 [n_masks], bad int32 [n_masks]: 1 when the mask has no polygon, an offset lies
 *   outside [0, n_polys] / [0, n_points], a polygon has fewer than 3 (or more than 2^30) points, a coordinate is not finite or
 *   reaches NPS_POLY_COORD_MAX after upsampling, or a polygon's upsampled point count sum(max(dx, dy) + 1) exceeds the cap above -
 *   all checked before a point is generated; the mask's words are then zero and its area 0.  toggles: uint32 scratch of the size of
 *   `bits` (the kernel clears it itself and leaves it zero).  One launch for all masks, a workgroup per mask.  Deterministic: integer
 *   results, and its only atomics are XOR / exchange on scratch words, which do not depend on order.  H W < 2^31 - 32; n_masks = 0
 *   enqueues nothing. */
nps_status nopesac_poly_to_bits(const double* xy, const int64_t* poly_off, const int64_t* mask_off, int64_t n_points, int64_t n_polys,
                                int n_masks, int H, int W, uint32_t* toggles, uint32_t* bits, int32_t* area, int32_t* bad, void* stream);
/* mask_iou_bits: for view v, predictions = rows dt_off[v] .. dt_off[v + 1] of dt_bits (areas in dt_area), GT masks = rows gt_off[v] ..
 *   gt_off[v + 1] of gt_bits (gt_area; iscrowd uint8 per GT mask, NULL = none).  inter = popcount(dt & gt), union = area_dt + area_gt -
 *   inter (area_dt for a crowd GT), iou = union > 0 ? (double)inter / (double)union : 0, written at iou_off[v] + i n_gt(v) + j of
 *   `iou` and `inter`.  max_dt / max_gt: upper bounds of a view's counts; they size the grid only (any count is computed). */
nps_status nopesac_mask_iou_bits(const uint32_t* dt_bits, const int32_t* dt_area, const int64_t* dt_off, const uint32_t* gt_bits,
                                 const int32_t* gt_area, const int64_t* gt_off, const uint8_t* iscrowd, const int64_t* iou_off, int V,
                                 int words, int max_dt, int max_gt, double* iou, int32_t* inter, void* stream);
#define NPS_PLANE_AP_COLS 10 /* doubles per prediction row of nopesac_plane_ap_assign */
/* plane_ap_assign: the per-view loop of mp3d_evaluation.py:570-649.  Per view: the IoU block (layout of mask_iou_bits), score f32,
 *   pred_label int32 (already the dataset category id), pred_plane f32 [.,3]; gt_label int32, gt_plane f32 [.,3].  rows: NPS_PLANE_AP_COLS doubles
 *   per prediction, in the predictions' own order: score, label, tp_mask, tp_plane, tp_normal, tp_offset, normal_err_deg,
 *   offset_err, best_iou, gt_id.  Predictions are taken in descending score order (ties: lower index first); gt_id = first maximum
 *   of the IoU row; true positive for a criterion = equal labels, iou > iou_thresh, normal_err < normal_thresh and / or offset_err <
 *   offset_thresh, and gt_id not yet taken for THAT criterion.  Errors (utils/metrics.py:6-24) in float64 from the f32 planes.  A view
 *   without GT: gt_id = -1, best_iou = 0, flags 0, NaN errors.  max_dt <= NPS_PLANE_MAX_QUERIES, max_gt <= 255 (upper bounds of a
 *   view's counts; a view beyond them is left unwritten), else NPS_E_ARG. */
nps_status nopesac_plane_ap_assign(const double* iou, const int64_t* iou_off, const int64_t* dt_off, const int64_t* gt_off, const float* score,
                                   const int32_t* pred_label, const float* pred_plane, const int32_t* gt_label, const float* gt_plane, int V,
                                   int max_dt, int max_gt, double iou_thresh, double normal_thresh, double offset_thresh, double* rows,
                                   void* stream);
#define NPS_RECON_AP_COLS 8 /* doubles per predicted entry of nopesac_recon_ap_assign */
/* recon_ap_assign: the per-pair part of the reference's offline `eval.py --evaluate AP` (evaluate_ap_by_idx :343-619, get_maskiou_merged
 *   :657-779, evaluate_by_idx / inst_bench_image :830-913, get_plane_params_in_global utils/mesh_utils.py:89-105).  Pair i owns views
 *   2 i and 2 i + 1 of dt_off / gt_off / iou_off (int64 [2 P + 1], the layout mask_iou_bits writes), the cameras pred_cam / gt_cam
 *   (7 doubles per pair: position, then quaternion w x y z; it need not be a unit quaternion) and the correspondences
 *   pred_corr[pred_corr_off[i] .. pred_corr_off[i + 1]) / gt_corr likewise: int32 pairs (plane of view 0, plane of view 1), the
 *   predicted ones in row-major order of the assignment matrix.  Both views' planes go to view 1's frame (view 0 through the camera);
 *   entries = view 0's unmatched planes in index order, view 1's, then one per correspondence (prediction: offset mean, score max,
 *   normal = top eigenvector of the two unit normals' outer products; GT: view 0's plane).  Errors [predicted entries, GT entries] in
 *   float64: |offset difference|, acos|normal dot| in degrees, merged mask IoU (single - single: the view's IoU or 0 across views;
 *   merged - single: the IoU in the single's view; merged - merged: the mean of both views).  Criteria all, -offset, -normal, -mask,
 *   -normal-offset: iou >= (.5 .5 .5 0 .5), normal <= (30 30 1000 30 1000), offset <= (1 1000 1 1 1000).  Entries are visited IN ENTRY
 *   ORDER; each claims the first GT entry its criterion flags and is a true positive iff nobody claimed it before.
 *   rows: NPS_RECON_AP_COLS doubles per predicted entry - score, the five flags, the entry's plane in view 0 and in view 1 (-1: none) -
 *   pair i's entries from row dt_off[2 i] - pred_corr_off[i] on; n_rows = dt_off[2 P] - pred_corr_off[P] rows in all.
 *   n_gt_entries int32 [P].  bad int32 [P]: 1 for a pair with a correspondence index out of range, a plane in two correspondences, or
 *   counts beyond the limits / offsets that do not fit n_rows - none of its rows is written and n_gt_entries is 0.
 *   errs (NULL: none): pair i's three matrices [3][predicted entries][GT entries] (offset, normal, IoU) at errs + err_off[i].
 *   max_dt <= NPS_PLANE_MAX_QUERIES, max_gt <= 255 per VIEW, else NPS_E_ARG.  Deterministic, no atomics; P = 0 enqueues nothing. */
nps_status nopesac_recon_ap_assign(const double* iou, const int64_t* iou_off, const int64_t* dt_off, const int64_t* gt_off, const float* score,
                                   const float* pred_plane, const float* gt_plane, const double* pred_cam, const double* gt_cam,
                                   const int32_t* pred_corr, const int64_t* pred_corr_off, const int32_t* gt_corr, const int64_t* gt_corr_off,
                                   int P, int max_dt, int max_gt, int64_t n_rows, double* rows, int32_t* n_gt_entries, int32_t* bad,
                                   double* errs, const int64_t* err_off, void* stream);
#define NPS_MESH_LDS_WORDS 15360 /* recon_mesh_count / _fill: a mask at its stride must fit this many 32-bit LDS words (60 KiB), see below */
/* The two-view reconstruction as textured meshes (csrc/recon_mesh.hip; the reference's vis_NopeSAC.py save_pair_objects on the dense
 * route of utils/vis.py get_single_image_mesh(reduce_size=False)).  Deterministic, no atomics, every output written once; P = 0 / n = 0
 * enqueues nothing.
 * recon_mesh_merge: merge_plane_params_from_local_params for P pairs, float64, a workgroup per pair.  Pair i owns views 2 i and 2 i + 1
 *   of view_off (int64 [2 P + 1], rows of planes f32 [total, 3]), the camera cams + 7 i (position, then quaternion w x y z; it need
 *   not be a unit quaternion) and the correspondences corr[corr_off[i] .. corr_off[i + 1]): int32 pairs (plane of view 0, plane of
 *   view 1).  A pair without correspondences keeps its planes (widened to double).  Otherwise every plane of the pair goes to view 1's
 *   frame (get_plane_params_in_global, offset = max(|.|, 1e-5); view 0 through the camera), a correspondence replaces both its planes by
 *   normalize(n0 + n1) times the mean offset, and every plane comes back through get_plane_params_in_local -> merged double [total, 3].
 *   For n0 . n1 < 0 the merged normal is normalize(n0 - n1), the orientation of view 0's plane (csrc/two_view.h has the rule, shared
 *   with recon_ap_assign).  bad int32 [P]: 1 for a pair with a correspondence index out of range, a plane in two correspondences, more
 *   than max_n planes in a view or offsets outside [0, total] - none of its planes is written.  max_n <= NPS_PLANE_MAX_QUERIES.
 * recon_mesh_count: per instance (bits: the layout of runs_to_bits, uint32 [n, ceil(H W / 32)]) the vertex and face counts of the
 *   mask m[::stride, ::stride]: one vertex per set pixel; per vertex (y, x) a triangle when (y, x + 1) and (y + 1, x + 1) are set and
 *   one when (y + 1, x) and (y + 1, x + 1) are set.  A workgroup per instance holds the strided mask row-major in LDS:
 *   Hs (RW | 1) + 2 (Hs + 1) words with Hs = ceil(H / stride), RW = ceil(ceil(W / stride) / 32) must not exceed NPS_MESH_LDS_WORDS
 *   (480 x 640 at stride 1: 11042), else NPS_E_ARG; so do stride < 1 and H W >= 2^31 - 32.
 * recon_mesh_fill: instance i writes rows vert_off[i] .. vert_off[i + 1] of verts f32 [n_verts, 3] and uvs f32 [n_verts, 2] and rows
 *   face_off[i] .. face_off[i + 1] of faces int32 [n_faces, 3] (int64 [n + 1] exclusive scans of the counts).  Vertices in row-major
 *   order of the strided mask, pixel (x, y) = stride (xs, ys): ray = kinv [x, y, 1], depth = |p| / ((p / |p|) . ray) with p = planes
 *   + 3 i (double, the plane in its view's frame), v = depth ray in plain IEEE arithmetic; then v [1, -1, -1] turned by the quaternion
 *   of cams + 7 view (q v q^-1, divided by |q|^2) plus its position; uv = (x / W, 1 - y / H).  view = inst_view[i] indexes kinv (double
 *   [n_views, 9], row-major K^-1) and cams (double [n_views, 7]; an identity row for the view that is the common frame).  Faces in
 *   vertex order, ids local to the instance from 0: [id(y, x), id(y + 1, x + 1), id(y, x + 1)], then [id(y, x), id(y + 1, x),
 *   id(y + 1, x + 1)].  Float64 arithmetic, f32 stores.  bad int32 [n]: 1 for an instance whose counts differ from its offset ranges,
 *   whose ranges leave [0, n_verts] / [0, n_faces] or whose view is outside [0, n_views) - nothing else of it is written. */
nps_status nopesac_recon_mesh_merge(const float* planes, const int64_t* view_off, const double* cams, const int32_t* corr,
                                    const int64_t* corr_off, int P, int max_n, int64_t total, double* merged, int32_t* bad, void* stream);
nps_status nopesac_recon_mesh_count(const uint32_t* bits, int n, int H, int W, int stride, int32_t* n_vert, int32_t* n_face, void* stream);
nps_status nopesac_recon_mesh_fill(const uint32_t* bits, int n, int H, int W, int stride, const double* planes, const int32_t* inst_view,
                                   int n_views, const double* kinv, const double* cams, const int64_t* vert_off, const int64_t* face_off,
                                   int64_t n_verts, int64_t n_faces, float* verts, float* uvs, int32_t* faces, int32_t* bad, void* stream);


/* Layers 1..5 of both branches of the pixel pose net (camera_net/camera_modules.py `convs_trans` / `convs_rots`: Conv3x3 + BatchNorm +
 * LeakyReLU(0.01), strides 2,1,2,1,2 behind the stride-1 first layer; call site camera_head.py:642-735) in one launch, one workgroup per
 * (image pair, branch), activations resident in LDS.  x_trans / x_rots: the branches' layer-0 outputs [B][15][20][128] bf16;
 * w10 / scale10 / bias10: 10 pointers each, index = branch * 5 + (layer - 1), branch 0 = trans: bf16 weights [128][3*3*128] in
 * nopesac MFMA fragment-major order (K index = (kh*3 + kw)*128 + c), folded-BatchNorm f32 scale / shift [128];
 * y_trans / y_rots: [B][2][3][128] f32 (NHWC: the FC stack's input).  H, W, C must be 15, 20, 128 (the 480 x 640 geometry). */
nps_status nopesac_posenet_branch_tail_bf16(const void* x_trans, const void* x_rots, const void* const* w10, const float* const* scale10,
                                            const float* const* bias10, float* y_trans, float* y_rots, int B, int H, int W, int C, void* stream);

/* ---- backward kernels of the camera head's training-side twin (csrc/refine_bwd.hip) ----------------------------
 * Vector-Jacobian products of nopesac_plane_cam_ref_losses, nopesac_ransac_soft_vote (mode | 16) and nopesac_ransac_score_maps - the
 * forward of the reference's __forward_PlaneCamRefHead (camera_net/camera_head.py:737-923; CameraPoseLoss camera_modules.py:355-365).
 * All f32, [B, ...] layouts exactly as the forward kernels'; no atomics: parameter gradients of the vote kernel are written PER PAIR
 * (pb_* = [B, size of the parameter]) and summed over the pairs by nopesac_col_sum_f32.  The Linear / MLP stacks in between are
 * differentiated with nopesac_conv2d_nhwc (f32): dX = dY W, dW = dY^T X, plus the helpers below (nopesac_amd/training.py).
 *  losses_backward:     g_loss [7] (d total / d each loss of nopesac_plane_cam_ref_losses) -> gradients of the four poses ([B,4] / [B,3],
 *                       with respect to the NORMALISED quaternions the vote kernel returns), of the scores [B,nq+1] (the hypothesis the
 *                       index losses pick is a constant, as in autograd) and of l2_dist [B,nq+1,nq] (its diagonal entries).
 *  vote_backward:       -> gradients of the score features [B,nq+1,64] x 2, the initial pose features [B,256] x 2, the per-plane features
 *                       [B,nq,256] x 2 and, per pair, of rots / trans weights + biases and of the two score regressors.
 *  score_maps_backward: gradients of normal_score / param_score / l2_dist [B,nq+1,nq] -> rot_raw [B,nq,4] (through its normalisation),
 *                       trans_raw [B,nq,3], init_rot [B,4], init_trans [B,3].
 * m int32[B]: the parameter loss and the average pose divide by m, so a pair with m = 0 is 0 / 0 by the reference's own definition.
 * nopesac_plane_cam_ref_losses leaves such a pair out of its sums (it adds nothing; the mean still divides by B - the convention of the
 * embedding loss for a batch that selects nothing) and losses_backward writes exact zeros for it; the vote kernel's average pose of
 * that pair stays 0 / 0 and vote_backward is specified for it only under those zero cotangents (it then writes zeros).  The other pairs
 * of the launch are not affected by it.  score_maps_backward is defined at m = 0: both scores are masked out there, so
 * only g_l2_dist (which is never masked) reaches the gradients, for every hypothesis and every plane of the pair.
 * Every element of every output is written by each call (exact zeros: g_score_* off the picked hypothesis, g_l2_dist off the
 * diagonal [b, 1 + j, j], g_sf_* rows h > m, g_fused_* rows k >= m).  Held per element to float64 VJPs by tests/test_refine_bwd_forms_gpu.py. */
nps_status nopesac_refine_losses_backward(const float* pred_rot, const float* pred_trans, const float* avg_rot, const float* avg_trans,
                                          const float* rots_all, const float* trans_all, const float* score_rot, const float* score_trans,
                                          const int32_t* m, const float* gt_pose, const float* g_loss, int B, int nq, float weight,
                                          float* g_pred_rot, float* g_pred_trans, float* g_avg_rot, float* g_avg_trans, float* g_score_rot,
                                          float* g_score_trans, float* g_l2_dist, void* stream);
nps_status nopesac_refine_vote_backward(const float* sf_rot, const float* sf_trans, const float* reg_rot_w, const float* reg_rot_b,
                                        const float* reg_trans_w, const float* reg_trans_b, const float* init_rot_feat,
                                        const float* init_trans_feat, const float* fused_rot, const float* fused_trans, const float* rots_w,
                                        const float* rots_b, const float* trans_w, const float* trans_b, const int32_t* m, int B, int nq,
                                        const float* g_pred_rot, const float* g_pred_trans, const float* g_avg_rot, const float* g_avg_trans,
                                        const float* g_score_rot, const float* g_score_trans, float* g_sf_rot, float* g_sf_trans,
                                        float* g_init_rot_feat, float* g_init_trans_feat, float* g_fused_rot, float* g_fused_trans,
                                        float* pb_rots_w, float* pb_rots_b, float* pb_trans_w, float* pb_trans_b, float* pb_reg_rot_w,
                                        float* pb_reg_rot_b, float* pb_reg_trans_w, float* pb_reg_trans_b, void* stream);
nps_status nopesac_refine_score_maps_backward(const float* geo_local, const float* rot_raw, const float* trans_raw, const float* init_rot,
                                              const float* init_trans, const int32_t* m, int B, int nq, const float* g_normal_score,
                                              const float* g_param_score, const float* g_l2_dist, float* g_rot_raw, float* g_trans_raw,
                                              float* g_init_rot, float* g_init_trans, void* stream);
/* backward of nopesac_camera_pose_loss (CameraPoseLoss camera_modules.py:355-365 and the AIM's reconstruction losses camera_head.py:700-705,
 * :725-731): g_out [2] -> gradients of BOTH pose arguments ([B,3] / [B,4] dense; the "ground truth" of a reconstruction loss is the pixel
 * pose, an output of trainable layers). */
nps_status nopesac_camera_pose_loss_backward(const float* est_trans, const float* est_rot, const float* gt_trans, int gt_trans_stride,
                                             const float* gt_rot, int gt_rot_stride, int B, float trans_eps, float weight, const float* g_out,
                                             float* g_est_trans, float* g_est_rot, float* g_gt_trans, float* g_gt_rot, void* stream);
/* helpers of the Linear backward and the optimiser (f32): y [cols,rows] = x^T (x rows strided by x_ld); out [cols] = column sums (fixed
 * summation order); out = y > 0 ? g : 0; J^T g of row-wise x / max(|x|, 1e-12) (D <= 4; canonical_sign: the forward also flipped rows with x[0] < 0); torch.optim.AdamW / SGD(momentum) updates of one
 * tensor (train_NopeSAC.py:150-157). */
nps_status nopesac_transpose_f32(const float* x, int rows, int cols, int64_t x_ld, float* y, void* stream);
nps_status nopesac_col_sum_f32(const float* x, int rows, int cols, int64_t x_ld, float* out, void* stream);
nps_status nopesac_relu_backward_f32(const float* g, const float* y, int64_t n, float* out, void* stream);
nps_status nopesac_normalize_rows_backward(const float* x, const float* g, int rows, int D, int canonical_sign, float* out, void* stream);
/* full-model gradient clipping (train_NopeSAC.py:139-148 -> torch.nn.utils.clip_grad_norm_): out[0] += sum x^2 (one launch per tensor on the
 * same accumulator, fixed order); coef[0] = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)); x *= coef[0].
 * sumsq: n <= 16384 is one workgroup and ws may be null; above, slices of chunk = ((n + 255) / 256 + 4095) / 4096 * 4096 elements (at
 * most 256) leave one partial each in ws, summed in slice order by a second launch.  nopesac_sumsq_workspace_floats(n) = that slice
 * count (a value; 0 for n <= 16384); a null or shorter ws is NPS_E_ARG - the algorithm, and so the sum's bits, depend on n alone. */
int64_t nopesac_sumsq_workspace_floats(int64_t n);
nps_status nopesac_sumsq_accumulate_f32(const float* x, int64_t n, float* out, float* ws, int64_t ws_floats, void* stream);
nps_status nopesac_clip_coefficient(const float* sumsq, float max_norm, float* coef, void* stream);
nps_status nopesac_scale_by_f32(float* x, int64_t n, const float* coef, void* stream);
nps_status nopesac_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, void* stream);
nps_status nopesac_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                            int first_step, void* stream);

/* ---- model-wide optimiser step (csrc/optimizer.hip; nopesac_amd/optim.py::ModelOptimizer) ----------------------------------------------
 * One gather launch and one step launch for ANY number of tensors.  State lives in three flat f32 arenas of the caller (arena_floats
 * each): G = the gathered gradients, M1 / M2 = AdamW's moments (SGD: M1 = the momentum buffer, M2 unused and may be null).  Every
 * tensor (SEGMENT) owns the slice [offset, offset + n) of each arena; offset is a multiple of NPS_OPT_ALIGN floats, segments do not
 * overlap, and the padding between them is zero and stays zero (the gather writes zeros there, the step never touches it), so a sum
 * of squares over the whole of G is the gradient norm.  Work is cut into UNITS of NPS_OPT_CHUNK elements, one 256-thread workgroup
 * each (four float4 per thread); a unit never crosses a segment end, and the static map `units` tells workgroup u its (segment, chunk
 * index) in one load - chunk c covers the elements [c NPS_OPT_CHUNK, min(n, (c + 1) NPS_OPT_CHUNK)) of its segment.
 *   segments  device, static: nopesac_opt_segment[n_segments]
 *   sources   device, written per step: nopesac_opt_source[n_segments] = where this step's gradient of the segment lies (contiguous f32,
 *             any 4-byte alignment) and flags: NPS_OPT_PRESENT, NPS_OPT_FIRST (SGD: the segment's first momentum step, buffer = gradient)
 *   units     device, static: nopesac_opt_unit[n_units]
 * nopesac_opt_gather: G[offset + i] = src[i] of every present segment, 0 of every absent one.
 * nopesac_opt_step: per element of every PRESENT segment g = G[i] * coef[0] (coef null: 1), then the update of nopesac_adamw_step /
 * nopesac_sgd_step in the same operation order with the segment's group {lr, weight_decay} - the bits of nopesac_scale_by_f32 followed
 * by the per-tensor entry.  AdamW's bias corrections are 1 - powf(beta, (float)step), formed on the host as nopesac_adamw_step forms
 * them.  Absent segments are skipped whole: parameter and moments untouched.  float4 accesses where the pointer on the caller's side
 * (src / param) is 16-byte aligned, scalar ones otherwise; the arenas must be 16-byte aligned.  A unit whose segment index, chunk or
 * arena range lies outside the tables' own bounds is skipped by the kernel (the tables are the caller's: a wrong one must not fault). */
#define NPS_OPT_CHUNK 4096
#define NPS_OPT_ALIGN 64
#define NPS_OPT_MAX_GROUPS 16
#define NPS_OPT_MAX_SEGMENTS 65536
#define NPS_OPT_PRESENT 1
#define NPS_OPT_FIRST 2
#define NPS_OPT_ADAMW 0
#define NPS_OPT_SGD 1
typedef struct nopesac_opt_segment {
    float* param;
    int64_t offset;
    int64_t n;
    int group, reserved;
} nopesac_opt_segment;
typedef struct nopesac_opt_source {
    const float* src;
    int flags, reserved;
} nopesac_opt_source;
typedef struct nopesac_opt_unit {
    int segment, chunk;
} nopesac_opt_unit;
typedef struct nopesac_opt_group {
    float lr, weight_decay;
} nopesac_opt_group;
typedef struct nopesac_opt_step_args {
    const nopesac_opt_segment* segments;
    const nopesac_opt_source* sources;
    const nopesac_opt_unit* units;
    int64_t n_units;
    int64_t arena_floats;
    float* G;
    float* M1;
    float* M2;
    const float* coef;
    int n_segments, mode, n_groups, step;
    float beta1, beta2, eps, momentum;
    nopesac_opt_group groups[NPS_OPT_MAX_GROUPS];
} nopesac_opt_step_args;
nps_status nopesac_opt_gather(const nopesac_opt_segment* segments, const nopesac_opt_source* sources, const nopesac_opt_unit* units,
                              int n_segments, int64_t n_units, float* G, int64_t arena_floats, void* stream);
nps_status nopesac_opt_step(const nopesac_opt_step_args* a, void* stream);

/* ---- backward of the pixel pose net's conv stacks (csrc/conv_bwd.hip; training.CameraHeadTrainer(conv_stacks=True)) ------------------
 * f32, NHWC activations, f32 accumulation; every buffer (workspaces included) is the caller's - this holds for the whole library: no
 * entry point allocates or frees device memory (no hipMalloc* under csrc/), and every split reduction has a *_workspace_floats / _bytes
 * entry that returns the size its launcher checks; no atomics: cross-workgroup sums are reduced in a fixed order, so two runs give
 * bit-identical results.
 *  conv2d_dgrad:  dY [B,OH,OW,Cout] (channel stride dy_cstride), w [Cout][Cin][KH][KW] (state-dict layout) -> dX [B,H,W,Cin] (channel
 *                 stride dx_cstride).  k 1 or 3, stride 1 or 2, pad < k.  Stride 1 (same-size conv): w is rotated / transposed into w_ws
 *                 ([Cin][KH][KW][Cout], Cin * Cout * KH * KW floats) and dX is the f32 MFMA implicit-GEMM conv of dY with it; stride 2: a
 *                 gather over the taps with an integral output position (w_ws unused, may be null).
 *  conv2d_wgrad:  x [B,H,W,Cin] (channel stride x_cstride >= Cin: the extra channels get no gradient), dY -> dW [Cout][Cin][KH][KW].
 *                 MFMA GEMM (M = Cout, N = KH KW Cin, K = B OH OW pixels) split into `splits` pixel ranges, partial tiles in ws
 *                 (nopesac_conv2d_wgrad_workspace_bytes), then summed in split order.  Needs Cin, Cout and both channel strides % 4 == 0.
 *  bn_act_forward / bn_act_backward: inference-mode BatchNorm (stored mean / var, affine gamma / beta) + act (NONE / RELU / LEAKY) on
 *                 c [rows][C]: y = act(c s + beta - mean s), s = gamma / sqrt(var + eps); backward from the saved c: dc, dgamma, dbeta
 *                 (ws: nopesac_bn_act_backward_workspace_floats).
 *  groupnorm_backward: x (the GroupNorm input) [B][HW][C], dY -> dX, dgamma, dbeta (optional ReLU after the affine; C / groups divides
 *                 256; ws: nopesac_groupnorm_backward_workspace_floats(B, C) = B * 2 * C floats).
 *  maxpool2x2_backward: 2x2 / stride 2 pool of x [B,H,W,C]: dY goes to the window's first maximum in row-major order (torch's choice).
 *  upsample2x_nearest_add_backward: y = lateral + nearest-2x(coarse [B,H,W,C]): dcoarse = 2x2 block sums of dY (dlateral = dY).
 *  corr_softmax_backward: rows of a softmax A over C channels (row stride a_ld; padding beyond C ignored), dA -> dS = A (dA - sum dA A)
 *                 as ds [B*P][C] and transposed per batch entry as ds_t [B][C][P].
 *  transpose_batched: x [B][rows][cols] -> y [B][cols][rows].
 * The three *_workspace_* entries return a size (a value, never negative). */
nps_status nopesac_conv2d_dgrad_f32(const float* dy, const float* w, float* dx, float* w_ws, int64_t w_ws_bytes, int B, int H, int W, int Cin,
                                    int Cout, int KH, int KW, int stride, int pad, int64_t dy_cstride, int64_t dx_cstride, void* stream);
int64_t nopesac_conv2d_wgrad_workspace_bytes(int Cout, int Cin, int KH, int KW, int splits);
nps_status nopesac_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* ws, int64_t ws_bytes, int B, int H, int W, int Cin, int Cout,
                                    int KH, int KW, int stride, int pad, int64_t x_cstride, int64_t dy_cstride, int splits, void* stream);
nps_status nopesac_bn_act_forward_f32(const float* c, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int act,
                                      int64_t rows, int C, float* y, void* stream);
int64_t nopesac_bn_act_backward_workspace_floats(int rows, int C);
nps_status nopesac_bn_act_backward_f32(const float* dy, const float* c, const float* gamma, const float* beta, const float* mean, const float* var,
                                       float eps, int act, int rows, int C, float* dc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats,
                                       void* stream);
int64_t nopesac_groupnorm_backward_workspace_floats(int B, int C);
nps_status nopesac_groupnorm_backward_f32(const float* x, const float* dy, const float* gamma, const float* beta, int B, int HW, int C, int groups,
                                          float eps, int relu, float* dx, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream);
nps_status nopesac_maxpool2x2_backward_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream);
nps_status nopesac_upsample2x_nearest_add_backward_f32(const float* dy, float* dx_coarse, int B, int H, int W, int C, void* stream);
nps_status nopesac_corr_softmax_backward_f32(const float* a, const float* da, int B, int P, int C, int64_t a_ld, int64_t da_ld, float* ds, float* ds_t,
                                             void* stream);
nps_status nopesac_transpose_batched_f32(const float* x, int B, int rows, int cols, float* y, void* stream);

/* ---- backward kernels of the matching head (csrc/matcher_bwd.hip; nopesac_amd/training.py::MatchingHeadTrainer) ------------------------
 * All f32, deterministic (no atomics), argument errors -> NPS_E_ARG + nopesac_last_error.
 * nopesac_attention_small_backward: gradient of nopesac_attention_small (head dim 32, Lq, Lk <= 128) at q / k / v for the output gradient
 *   d_out; every matrix is row-major with its own row stride (elements), so column slices of a [rows, 768] q|k|v buffer are taken as
 *   they are.  The softmax is recomputed.  Rows >= qlen[b] get zero dq; keys >= klen[b] get zero dk / dv and take no part in the softmax.
 *   qlen / klen may be null (every row / key is live) and are clamped to [0, Lq] / [0, Lk].  A set with klen[b] == 0 gets zero dq on every
 *   row, a set with qlen[b] == 0 zero dk / dv on every key.  All Lq (Lk) rows of every set are written, heads * 32 values each: with a
 *   row stride above heads * 32 the rest of a row is left as it was.
 * nopesac_layernorm_backward: y = LayerNorm(x) gamma + beta over D = 256 -> dx [rows, D], dgamma [D], dbeta [D]; ws holds per-block
 *   partials of the two column reductions (nopesac_layernorm_backward_workspace_floats(rows) floats), reduced in a fixed order.
 * nopesac_matcher_sinkhorn_train: the couplings and the iters log-Sinkhorn iterations of nopesac_matcher_sinkhorn without the
 *   assignment; gt_corr uint8 [B, nq+1, nq+1] in the layout of log_scores (dustbin at index nq; entries outside a pair's live rows
 *   (< n1, nq) x columns (< n2, nq) are ignored).  Outputs: log_scores; uv [B, iters, 2, nq+1] = every iteration's potentials (compact
 *   indices, dustbin at n1 / n2) for the backward pass; pair_stats [B, 2] = (sum of -min(score, 0) over the pair's selected entries,
 *   their count); loss [2] = (2 * sum / count over the WHOLE batch - 0 when nothing is selected -, count).  Pairs with n1 == 0 or
 *   n2 == 0 select nothing and get log_scores = -1e30 everywhere.  The dustbin corner (nq, nq) is a live entry: a gt_corr bit there is
 *   counted.  uv is written at the compact indices 0 .. n1 (u) and 0 .. n2 (v) only: entries beyond them, and every entry of a pair with
 *   n1 == 0 or n2 == 0, are left as they were.  iters == 0: log_scores = couplings - norm, uv has no element and may be null.
 * nopesac_matcher_emb_loss: pair_stats and loss as above from log scores that already exist (the output of nopesac_matcher_sinkhorn):
 *   the training forward runs the inference kernel itself, so its scores are the inference head's bit for bit, and the potentials
 *   are produced by nopesac_matcher_sinkhorn_train as a replay when the backward pass starts.
 * nopesac_matcher_sinkhorn_train_backward: gradient of loss[0] (times g_loss[0], a device scalar) through the UNROLLED iterations ->
 *   d_desc_dot [B, nq, nq] (zero outside the live block) and d_bin_pairs [B] (per-pair partials of d bin_score; sum them in order).
 *   Every element of both is written.  They are exactly zero for a pair with n1 == 0 or n2 == 0, for a pair none of whose selected
 *   scores is <= 0, and for every pair when loss[1] (the batch's count) is 0.  iters == 0: d_desc_dot = -2 g_loss / count on the
 *   selected entries with a score <= 0.
 * nopesac_desc_dot_backward: dots = D0 D1^T / 16 per pair (D = 256) -> dD0 = G D1 / 16, dD1 = G^T D0 / 16 over the live block, zero rows
 *   beyond n1 / n2.
 * nopesac_layernorm_backward_workspace_floats returns a size (a value; 0 for rows <= 0, never negative). */
nps_status nopesac_attention_small_backward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v, int64_t v_stride,
                                            const float* d_out, int64_t do_stride, int B, int Lq, int Lk, int heads, float scale,
                                            const int32_t* qlen, const int32_t* klen, float* dq, int64_t dq_stride, float* dk, int64_t dk_stride,
                                            float* dv, int64_t dv_stride, void* stream);
int64_t nopesac_layernorm_backward_workspace_floats(int rows);
nps_status nopesac_layernorm_backward(const float* x, const float* gamma, const float* dy, int rows, int D, float eps, float* dx, float* dgamma,
                                      float* dbeta, float* ws, int64_t ws_floats, void* stream);
nps_status nopesac_matcher_sinkhorn_train(const float* desc_dot, const float* planes1, const float* planes2, const float* cam7, const int32_t* n1,
                                          const int32_t* n2, const float* bin_score, float offset_mult, float normal_mult, int iters,
                                          const uint8_t* gt_corr, int B, int nq, float* log_scores, float* uv, float* pair_stats, float* loss,
                                          void* stream);
nps_status nopesac_matcher_emb_loss(const float* log_scores, const uint8_t* gt_corr, const int32_t* n1, const int32_t* n2, int B, int nq,
                                    float* pair_stats, float* loss, void* stream);
nps_status nopesac_matcher_sinkhorn_train_backward(const float* desc_dot, const float* planes1, const float* planes2, const float* cam7,
                                                   const int32_t* n1, const int32_t* n2, const float* bin_score, float offset_mult,
                                                   float normal_mult, int iters, const uint8_t* gt_corr, const float* uv, const float* loss,
                                                   const float* g_loss, int B, int nq, float* d_desc_dot, float* d_bin_pairs, void* stream);
nps_status nopesac_desc_dot_backward(const float* d_desc_dot, const float* d0, const float* d1, const int32_t* n1, const int32_t* n2, int B, int nq,
                                     int D, float* dd0, float* dd1, void* stream);

/* ---- set criterion of the plane head (csrc/plane_criterion.hip; nopesac_amd/training.py::PlaneCriterion) -------------------------------
 * Reference: modeling/matcher.py (HungarianMatcher), modeling/criterion.py (SetCriterion), siamese_planeTR.py prepare_targets and
 * process_plane_corr_matrix.  All f32, deterministic (no atomics); argument errors -> NPS_E_ARG + nopesac_last_error before any HIP call.
 * An IMAGE is one (supervised decoder layer, batch element): i = layer * B + b with layer 0 = the last decoder layer and layers 1.. the
 * auxiliary ones (aux_outputs[0], ...); targets are read at b = i % B.  One argument block serves the cost, loss and gradient entries:
 *   predictions  pred_logits [L*B, nq, 2], pred_centers [L*B, nq, 2], pred_params [L*B, nq, 3]; pred_mask_logits with element strides
 *                (image, query, y, x) over h x w; pixel_centers (last layer only, optional) with strides (batch, channel, y, x);
 *   targets      masks uint8 [B, nmax, H, W] (H = s h, W = s w, integer s >= 1), n int32 [B] on the device and n_host, the same values
 *                on the host (1 <= n[b] <= min(nq, nmax, 50): checked), tgt_centers [B, nmax, 2], tgt_params [B, nmax, 3],
 *                tgt_pixel_centers [B, 2, H, W], depth [B, H, W], k_inv_dot_xy1 [B, 3, H, W]; every target is of class 0 (num_classes = 2
 *                logits: plane, no object);
 *   matching     cost [L*B, nq, nmax] (0 at j >= n[b]); match_q int32 [L*B, nmax] = query of target j (-1 at j >= n[b]); match_gt int32
 *                [L*B, nq] = target of query q (-1 if unmatched);
 *   losses       losses [6 L + 2] unweighted: per layer (loss_ce, loss_mask, loss_dice, loss_center_ins, loss_param_l1, loss_param_cos),
 *                then loss_center_pixel and loss_q of the last layer; num_masks <= 0 means max(sum n, 1).  Kept for the backward pass:
 *                mask_stats [L*B, nmax, 4] = (focal sum, sum sigmoid * t, sum sigmoid, sum t) of each matched mask at H x W (0 at
 *                j >= n[b]), q_valid uint8 [B, H, W], q_stats [B, 2] = (sum, count) over the valid pixels; every element is written;
 *   gradients    g_losses [6 L + 2] (device) = one upstream scalar per loss; d_logits, d_centers, d_params in the shapes of the inputs,
 *                d_mask_logits and d_pixel_centers with the STRIDES of pred_mask_logits / pixel_centers: the strides need not be dense,
 *                the gaps are neither read nor written.  Unmatched queries get exactly 0 in d_mask_logits, d_centers and d_params; a
 *                centre (or centre-map pixel) at distance exactly 0 from its target gets the subgradient 0; an image without a valid
 *                pixel adds nothing to loss_q or d_params;
 *   ws           nopesac_plane_criterion_workspace_floats(L, B, nq, nmax, h, w) floats, shared by the three entries (the loss entry's
 *                content must survive until its backward entry has run); the count is a value, 0 for a non-positive dimension
 *                (never negative);
 *   groups       G view groups (0 or 1: none; else 2..NPS_PLANE_MAX_GROUPS, dividing B, or NPS_E_ARG): group g is the batch elements
 *                [g B/G, (g+1) B/G) of every layer's block, as forward_single sees one view at a time.  The loss and gradient entries
 *                then take num_masks, the matched count, the class weight sum and the batch divisor of loss_center_pixel / loss_q per
 *                group: losses and g_losses are [G][6 L + 2], num_masks_groups (HOST, G floats; null: num_masks for every group) the
 *                per-group overrides.  Group g's losses and every gradient element of its images have the bits of an ungrouped call
 *                on those images alone.  The cost and assignment entries are per image and ignore it. */
#define NPS_PLANE_MAX_QUERIES 128
#define NPS_PLANE_MAX_TARGETS 50
#define NPS_PLANE_MAX_LAYERS 8
#define NPS_PLANE_MAX_GROUPS 8
typedef struct nopesac_plane_criterion {
    const float* pred_logits;
    const float* pred_mask_logits;
    const float* pred_centers;
    const float* pred_params;
    const float* pixel_centers;
    int64_t ml_stride_i, ml_stride_q, ml_stride_y, ml_stride_x;
    int64_t pc_stride_b, pc_stride_c, pc_stride_y, pc_stride_x;
    const uint8_t* masks;
    const int32_t* n;
    const int32_t* n_host;
    const float* tgt_centers;
    const float* tgt_params;
    const float* tgt_pixel_centers;
    const float* depth;
    const float* k_inv_dot_xy1;
    int L, B, nq, nmax, h, w, H, W, num_classes, groups;
    float cost_class, cost_mask, cost_dice, cost_center, cost_param, cost_offset, cost_angle;
    float eos_coef, num_masks, reserved_f;
    float* cost;
    int32_t* match_q;
    int32_t* match_gt;
    float* losses;
    float* mask_stats;
    uint8_t* q_valid;
    float* q_stats;
    const float* g_losses;
    float* d_logits;
    float* d_mask_logits;
    float* d_centers;
    float* d_params;
    float* d_pixel_centers;
    float* ws;
    int64_t ws_floats;
    const float* num_masks_groups;
} nopesac_plane_criterion;
int64_t nopesac_plane_criterion_workspace_floats(int L, int B, int nq, int nmax, int h, int w);
/* plane_centers [B, nmax, 2] = centroid of (x / W, y / H) over each mask (0 at j >= n[b]), computed in f64 from the exact integer sums
 * as sum / W / count (two rounded divisions) and then rounded to f32; pixel_centers [B, 2, H, W] = the f32 sum over planes j < n[b], in plane order, of centre * mask (prepare_targets,
 * siamese_planeTR.py:498-504).  An empty mask gives a NaN centre (the reference's 0 / 0); it covers no pixel, so the centre map stays finite. */
nps_status nopesac_plane_targets(const uint8_t* masks, const int32_t* n_host, const int32_t* n, int B, int nmax, int H, int W, float* plane_centers,
                                 float* pixel_centers, void* stream);
/* the matcher's seven-term cost matrix (class probability, focal and dice against the NEAREST-downsampled masks, centre L2, parameter L1,
 * normal angle in degrees, offset) -> a->cost */
nps_status nopesac_plane_match_costs(const nopesac_plane_criterion* a, void* stream);
/* rectangular linear sum assignment per image on the device (n[b] <= nq <= 128): shortest augmenting paths, one wave per image, duals in
 * f64 (integer-valued costs up to 2^20 + small are matched exactly); ties go to an unmatched query first, then to the lowest index.  Only
 * cost[i][q][j < n[b]] is read.  A query whose costs are all +inf is avoided.  A target whose costs are all +inf or NaN cannot be placed:
 * the image keeps the matches of the targets before it, every later target gets match_q = -1 (match_gt accordingly), and the call
 * returns; other images of the launch are not affected.  The loss entries need every target j < n[b] matched. */
nps_status nopesac_plane_assign(const float* cost, const int32_t* n_host, const int32_t* n, int L, int B, int nq, int nmax, int32_t* match_q,
                                int32_t* match_gt, void* stream);
nps_status nopesac_plane_losses(const nopesac_plane_criterion* a, void* stream);
nps_status nopesac_plane_losses_backward(const nopesac_plane_criterion* a, void* stream);
/* gt correspondences of the PREDICTED planes (process_plane_corr_matrix, siamese_planeTR.py:566-623): gt_corrs int32 [B, K, 2] = (gt plane of
 * view 1, of view 2), rows padded with -1; pairs with an index >= 50 are dropped; match1 / match2 int32 [B, nmax] = the last layer's match_q
 * of the two views -> out uint8 [B, nq+1, nq+1] with the dustbin row and column, the form nopesac_matcher_sinkhorn_train takes */
nps_status nopesac_plane_corr_matrix(const int32_t* gt_corrs, int K, const int32_t* match1, const int32_t* match2, int B, int nq, int nmax,
                                     uint8_t* out, void* stream);

/* ---- where the plane head's outputs meet the two-view heads in training (csrc/two_view_train.hip; siamese_planeTR.py:237-299) ------------
 * refine_score_maps_backward_geo: the cotangent of nopesac_ransac_score_maps that nopesac_refine_score_maps_backward leaves out - the
 *   gradients of normal_score / param_score / l2_dist [B,nq+1,nq] -> g_geo_local f32 [B,nq,6] (first plane, second plane).  One thread
 *   per (pair, matched plane) walks the nq + 1 hypotheses in order: the transpose of the other kernel's walk, the same masks and guards
 *   (dn > 0, dl2 > 0, |w_r| >= 1e-12) and the same quaternion normalisation.  Rows j >= m are exact zeros (geo_sequence pads them with zero
 *   planes, whose distances have no gradient).
 * geo_sequence_backward: backward of nopesac_geo_sequence with respect to the planes (init_trans / init_rot are detached in the reference,
 *   camera_head.py:353-368; sig is piecewise constant): g_geo_local [B,nq,6] and g_geo_enc [B,nq,8] at the sequence positions ->
 *   g_planes1 / g_planes2 f32 [B,nq,3].  One workgroup per pair recomputes the row-major positions as the forward does, the cut at nq
 *   pairs included; a plane that occurs in several pairs (a row or a column of the assignment with several ones) receives their sum in
 *   sequence order; unmatched planes and planes at or beyond n1 / n2 get exact zeros.
 * match_compact: x f32 [N,nq,256], params f32 [N,nq,3], match_q int32 [N,nmax], n int32 [N] -> the n[i] queries match_q[i, 0..n[i]-1] of image
 *   i at rows 0 .. n[i]-1 of x_c / params_c in ASCENDING query index (the reference's sorted indices[bi][0], matching_head.py:51-69), zero
 *   rows behind; order int32 [N,nq] = the query at row r or -1, rank int32 [N,nq] = the row of query q or -1.  An image whose input breaks
 *   the contract (an index outside [0,nq), a query named twice, n[i] outside [0, min(nq,nmax)]) is treated as n[i] = 0 and bad[i] = 1
 *   (int32 [N], else 0); nothing is read or written out of bounds.  1 <= nmax <= NPS_PLANE_MAX_QUERIES.
 * match_compact_backward: g_x_c [N,nq,256], rank -> g_x [N,nq,256], the scatter back: an exact copy, zero rows for unmatched queries
 *   (params_c carries no gradient: the matcher detaches its geometry, matching_head.py:98-99).
 * corr_compact: gt_corr uint8 [B,nq+1,nq+1] (nopesac_plane_corr_matrix) gathered through both views' order with the dustbin index nq
 *   mapped to itself: out[r,c] = gt_corr[order1[r], order2[c]] for r < n1 (or r = nq) and c < n2 (or c = nq), 0 elsewhere.
 * All f32 / integer, nq <= NPS_PLANE_MAX_QUERIES, no float atomics, two runs give the same bits; every element of every output is written.
 * Held to float64 VJPs per element and to a numpy restatement by tests/test_two_view_forms_gpu.py. */
nps_status nopesac_refine_score_maps_backward_geo(const float* geo_local, const float* rot_raw, const float* trans_raw, const float* init_rot,
                                                  const float* init_trans, const int32_t* m, int B, int nq, const float* g_normal_score,
                                                  const float* g_param_score, const float* g_l2_dist, float* g_geo_local, void* stream);
nps_status nopesac_geo_sequence_backward(const float* assignment, const float* planes1, const float* planes2, const int32_t* n1,
                                         const int32_t* n2, const float* init_trans, const float* init_rot, int B, int nq, int warp_in_ref,
                                         const float* g_geo_local, const float* g_geo_enc, float* g_planes1, float* g_planes2, void* stream);
nps_status nopesac_match_compact(const float* x, const float* params, const int32_t* match_q, const int32_t* n, int N, int nq, int nmax,
                                 float* x_c, float* params_c, int32_t* order, int32_t* rank, int32_t* bad, void* stream);
nps_status nopesac_match_compact_backward(const float* g_x_c, const int32_t* rank, int N, int nq, float* g_x, void* stream);
nps_status nopesac_corr_compact(const uint8_t* gt_corr, const int32_t* order1, const int32_t* order2, const int32_t* n1, const int32_t* n2,
                                int B, int nq, uint8_t* out, void* stream);

/* ---- backward of the plane head's instance heads (csrc/plane_head_bwd.hip; nopesac_amd/training.py::PlaneInstanceHeadsTrainer) ----------
 * The folded mask logits M[l,b,q,p] = sum_k F[l,b,q,k] p1[b,p,k] + beta[l,b,q] of L <= 3 supervised decoder layers (F = E W_pe,
 * beta = E . b_pe: the pixel-embedding map is never materialised) and, joined as two more rows per image whose weights the batch
 * shares, the 256 -> 2 pixel-centre conv Z[b,c,p] = sum_k wc[c,k] p1[b,p,k] + bc[c].  All f32, exact-f32 MFMA, deterministic (no
 * atomics); C must be 256, nq in [1, 128], L in [1, 3]; argument errors -> NPS_E_ARG before any launch.
 *  d_logits  dM [L*B][nq][h*w], pixel-minor and dense (what nopesac_plane_losses_backward writes for a contiguous [L*B,nq,h,w] input);
 *  d_center  dZ [B][2][h*w], the gradient at the centre map IN FRONT of its sigmoid (nopesac_sigmoid_backward_f32), or null: no centre rows
 *            (then d_wc / d_bc / wc are null too);
 *  p1 / d_p1 [B][h*w][256] NHWC, pixel-dense: batch stride = h*w * pixel stride, pixel stride >= 256 (a channel slice of a wider buffer);
 *            p1 16-byte aligned with a pixel stride % 4 == 0;
 *  fold      F rows [L*B*nq][256] with row stride fold_ld (% 4 == 0, 16-byte aligned), row order (l, b, q); wc [2][256] dense.
 * mask_product_wgrad: d_fold[(l,b,q)][k] = sum_p dM p1 (row stride d_fold_ld), d_beta[(l,b,q)] = sum_p dM (element stride d_beta_stride),
 *            d_wc[c][k] = sum_b sum_p dZ p1, d_bc[c] = sum_b sum_p dZ.  Per image a GEMM (M = L nq + 2, N = 256, K = h w) split into
 *            `splits` pixel ranges (1..1024; ranges beyond the map are empty) whose partial tiles go to ws - at least
 *            NPS_MASK_PRODUCT_WGRAD_WORKSPACE_FLOATS(L, B, nq, center_rows = 0 or 2, splits) floats: per range, image and row 256
 *            partial sums and the row's own sum - and are summed in split order, the shared rows over the images in order.
 * mask_product_dgrad: d_p1[b][p][k] = sum_{l,q} dM F + sum_c dZ wc, written once (M = h w, N = 256, K = L nq + 2 per image).
 * sigmoid_backward: out = g y (1 - y) for the output y of a sigmoid, n elements.
 * nopesac_mask_product_wgrad_workspace_floats: the macro's value for callers that cannot read it (0 for an argument < 0). */
#define NPS_MASK_PRODUCT_WS_ROW_FLOATS 257
#define NPS_MASK_PRODUCT_WGRAD_WORKSPACE_FLOATS(L, B, nq, center_rows, splits) ((int64_t)(splits) * (B) * ((int64_t)(L) * (nq) + (center_rows)) * NPS_MASK_PRODUCT_WS_ROW_FLOATS)
int64_t nopesac_mask_product_wgrad_workspace_floats(int L, int B, int nq, int center_rows, int splits);
nps_status nopesac_mask_product_wgrad_f32(const float* d_logits, const float* d_center, const float* p1, float* d_fold, int64_t d_fold_ld,
                                          float* d_beta, int64_t d_beta_stride, float* d_wc, float* d_bc, float* ws, int64_t ws_floats, int L,
                                          int B, int nq, int h, int w, int C, int64_t p1_pstride, int64_t p1_bstride, int splits, void* stream);
nps_status nopesac_mask_product_dgrad_f32(const float* d_logits, const float* d_center, const float* fold, int64_t fold_ld, const float* wc,
                                          float* d_p1, int L, int B, int nq, int h, int w, int C, int64_t dp1_pstride, int64_t dp1_bstride,
                                          void* stream);
nps_status nopesac_sigmoid_backward_f32(const float* g, const float* y, int64_t n, float* out, void* stream);

/* ---- training kernels of the plane head's transformer decoder (csrc/decoder_train.hip; nopesac_amd/training.py::PlaneDecoderTrainer) ----
 * Dropout is counter based (csrc/dropout.h, docs/kernels.md): element `index` of the dropout site `stream` under `seed` is KEPT when the
 * high 32 bits of mix64(index + mix64(stream + mix64(seed))) are >= floor(p 2^32); nothing is stored, every kernel recomputes the
 * decision.  index = the row-major index in the LOGICAL tensor ([B, heads, Lq, Lk] for attention probabilities, [rows, D] for a matrix):
 * it does not depend on tiles, strides or the launch.  p in [0, 1), else NPS_E_ARG; p == 0 keeps everything and skips the hash.
 * Kept values are multiplied by (float)(1 / (1 - p)).  All f32, deterministic (no atomics).
 * nopesac_dropout_keep_mask: out[i] = 1 if element i (0 <= i < n) is kept, else 0.
 * nopesac_dropout_f32: y[i] = keep(i) ? x[i] / (1 - p) : 0, plus residual[i] when residual is not null; n = rows * D elements, dense.
 *   Without a residual it is its own backward (x = the gradient at y).
 * nopesac_attention_train_forward: nopesac_attention_small's contract (head dim 32, row strides, optional qlen / klen clamped to
 *   [0, Lq] / [0, Lk], rows >= qlen[b] and sets with klen[b] == 0 written as zeros) for ANY Lq, Lk >= 1, tiled over the keys
 *   (NPS_ATT_TRAIN_TK per tile through LDS, NPS_ATT_TRAIN_TQ query rows per workgroup) with an online softmax, and dropout on the
 *   probabilities: O = (keep o softmax(S)) V / (1 - p).
 * nopesac_attention_train_backward: its gradient at q / k / v for d_out, with the contract of nopesac_attention_small_backward (zero dq on
 *   rows >= qlen[b], zero dk / dv on keys >= klen[b], every row written, heads * 32 values each).  Nothing of a forward launch is read:
 *   a statistics kernel recomputes row max, 1 / row sum and D_i = sum_j P_ij dP_ij into ws (at least
 *   NPS_ATT_TRAIN_BACKWARD_WORKSPACE_FLOATS(B, heads, Lq) floats), a dq kernel (one workgroup per query
 *   tile) and a dk / dv kernel (one per key tile) recompute P from them; the mask is regenerated from the counter.
 * nopesac_attention_train_backward_workspace_floats: the macro's value for callers that cannot read it (0 for an argument < 0). */
#define NPS_ATT_TRAIN_TQ 64
#define NPS_ATT_TRAIN_TK 64
#define NPS_ATT_TRAIN_WS_ROW_FLOATS 3
#define NPS_ATT_TRAIN_BACKWARD_WORKSPACE_FLOATS(B, heads, Lq) ((int64_t)(B) * (heads) * (Lq) * NPS_ATT_TRAIN_WS_ROW_FLOATS)
int64_t nopesac_attention_train_backward_workspace_floats(int B, int heads, int Lq);
nps_status nopesac_dropout_keep_mask(uint8_t* out, int64_t n, double p, int64_t seed, int64_t stream_id, void* stream);
nps_status nopesac_dropout_f32(const float* x, const float* residual, float* y, int64_t n, double p, int64_t seed, int64_t stream_id,
                               void* stream);
nps_status nopesac_attention_train_forward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v, int64_t v_stride,
                                           float* o, int64_t o_stride, int B, int Lq, int Lk, int heads, float scale, const int32_t* qlen,
                                           const int32_t* klen, double p, int64_t seed, int64_t stream_id, void* stream);
nps_status nopesac_attention_train_backward(const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v, int64_t v_stride,
                                            const float* d_out, int64_t do_stride, int B, int Lq, int Lk, int heads, float scale,
                                            const int32_t* qlen, const int32_t* klen, double p, int64_t seed, int64_t stream_id, float* dq,
                                            int64_t dq_stride, float* dk, int64_t dk_stride, float* dv, int64_t dv_stride, float* ws,
                                            int64_t ws_floats, void* stream);

/* ---- training kernels of the plane head's top-down pyramid (csrc/pyramid_train.hip; training.PlanePyramidTrainer) ----------------------
 * Training-mode BatchNorm (BATCH statistics, running-statistics update, backward) and the adjoint of the bilinear 2x upsampling.  f32,
 * NHWC, deterministic (no atomics: per-block partials of NPS_BN_TRAIN_RPS rows in ws, finished in a fixed order).
 * The three bn_train entry points take their input v in one of two forms: up = 0: v = src, [n = B H W][C] with channel stride
 * src_cstride >= C (a matrix [rows][C] is B = rows, H = W = 1); up = 1: v = the bilinear 2x upsampling (align_corners = False, the
 * values of nopesac_upsample2x_bilinear_nhwc bit for bit) of src [B][H][W][C], n = B 2H 2W rows, evaluated on the fly, never written.
 * y, dy, addend and the plain form's dsrc are dense [n][C].  A thread works on four channels: C and src_cstride are multiples of 4 and
 * every pointer is 16-byte aligned (else NPS_E_ARG; upsample2x_bilinear_backward too).  ws: at least NPS_BN_TRAIN_WORKSPACE_FLOATS(n, C) floats.
 *  bn_train_stats:    mean, biased variance and rstd = 1 / sqrt(var + eps) per channel over the n values (per-block mean and centred
 *                     sum of squares, merged by Chan's formula: never E[x^2] - E[x]^2).  running_mean / running_var (both or neither)
 *                     are updated in place on the device: r <- (1 - momentum) r + momentum stat, the variance unbiased (n / (n - 1)).
 *                     n < 2: NPS_E_ARG.
 *  bn_train_apply:    y = act(gamma (v - mean) rstd + beta) (+ addend, AFTER the activation); act NPS_ACT_NONE or NPS_ACT_RELU.
 *  bn_train_backward: dy, the same input, gamma, beta, mean, rstd -> dgamma = sum dz xhat, dbeta = sum dz (dz = dy where z > 0 under
 *                     RELU) and dsrc: up = 0: dv = gamma rstd (dz - dbeta / n - xhat dgamma / n), [n][C]; up = 1: the gradient at src,
 *                     up2^T(dv) [B][H][W][C] dense, dv evaluated inside the gather and never written.  batch_stats = 0: mean and rstd
 *                     are stored statistics, constants of the backward: dv = gamma rstd dz (dgamma, dbeta as above).
 *  upsample2x_bilinear_backward: du [B][2H][2W][C] -> dx [B][H][W][C] = up2^T(du), a gather over the at most 4 x 4 outputs an input
 *                     feeds (per axis 0.25, 0.75, 0.75, 0.25; the clamped border taps folded back in).
 * nopesac_bn_train_workspace_floats: the macro's value for callers that cannot read it (0 for an argument < 0). */
#define NPS_BN_TRAIN_RPS 256
#define NPS_BN_TRAIN_WORKSPACE_FLOATS(n, C) ((((int64_t)(n) + NPS_BN_TRAIN_RPS - 1) / NPS_BN_TRAIN_RPS) * 2 * (C))
int64_t nopesac_bn_train_workspace_floats(int64_t n, int C);
nps_status nopesac_bn_train_stats_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, float eps, float momentum,
                                      float* mean, float* var, float* rstd, float* running_mean, float* running_var, float* ws,
                                      int64_t ws_floats, void* stream);
nps_status nopesac_bn_train_apply_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, const float* gamma,
                                      const float* beta, const float* mean, const float* rstd, int act, const float* addend, float* y,
                                      void* stream);
nps_status nopesac_bn_train_backward_f32(const float* dy, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride,
                                         const float* gamma, const float* beta, const float* mean, const float* rstd, int act, int batch_stats,
                                         float* dsrc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream);
nps_status nopesac_upsample2x_bilinear_backward_f32(const float* du, float* dx, int B, int H, int W, int C, void* stream);
/* The same three launchers on VIEW GROUPS: `groups` = G (0 or 1: none, the entries above bit for bit; else 2..NPS_BN_TRAIN_MAX_GROUPS,
 * dividing B, or NPS_E_ARG) cuts the B images (the rows of the matrix form) into G groups of B / G consecutive ones - the two views of a
 * 2B-image batch, view 1 first - each with its own batch statistics, as G module calls on the groups would have them (reference top_down
 * under forward_single per view, siamese_planeTR.py:228-235).  One launch per stage whatever G is; a group's rows are cut into blocks of
 * NPS_BN_TRAIN_RPS from the group's first row and its partials are finished on their own, so every per-group result has the bits of
 * an ungrouped call on that group's sub-tensor.  Both input forms, the addend included; the upsampling and its adjoint never cross an
 * image, so they never cross a group.
 *  stats:    mean, var, rstd are [G][C]; running_mean / running_var [C] take the groups' statistics one after the other (in a
 *            register, stored once), the variance unbiased with the group's n: what G module calls in a row leave.
 *  apply:    y = act(gamma (v - mean_g) rstd_g + beta) (+ addend), g = the row's group.
 *  backward: per group S2_g = sum dz xhat and S1_g = sum dz over its rows -> group_sums [G][2][C] (S2_g, then S1_g; needed for G > 1,
 *            16-byte aligned; not written for G <= 1), dsrc of its rows from them with n = the group's rows; dgamma = sum_g S2_g and
 *            dbeta = sum_g S1_g, added in group order.  No atomics.
 * ws: at least NPS_BN_TRAIN_GROUPS_WORKSPACE_FLOATS(G, n, C) floats, n = all rows of v (= NPS_BN_TRAIN_WORKSPACE_FLOATS(n, C) at G = 1);
 * nopesac_bn_train_groups_workspace_floats writes the macro's value into *floats (a status entry: NPS_E_ARG and 0 for groups outside
 * 0..NPS_BN_TRAIN_MAX_GROUPS, n <= 0, C <= 0 or n not a multiple of G). */
#define NPS_BN_TRAIN_MAX_GROUPS 8
#define NPS_BN_TRAIN_GROUPS_WORKSPACE_FLOATS(G, n, C) ((int64_t)(G) * (((int64_t)(n) / (G) + NPS_BN_TRAIN_RPS - 1) / NPS_BN_TRAIN_RPS) * 2 * (C))
nps_status nopesac_bn_train_groups_workspace_floats(int groups, int64_t n, int C, int64_t* floats);
nps_status nopesac_bn_train_groups_stats_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups, float eps,
                                             float momentum, float* mean, float* var, float* rstd, float* running_mean, float* running_var,
                                             float* ws, int64_t ws_floats, void* stream);
nps_status nopesac_bn_train_groups_apply_f32(const float* src, int up, int B, int H, int W, int C, int64_t src_cstride, int groups,
                                             const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                                             const float* addend, float* y, void* stream);
nps_status nopesac_bn_train_groups_backward_f32(const float* dy, const float* src, int up, int B, int H, int W, int C, int64_t src_cstride,
                                                int groups, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                                int act, int batch_stats, float* dsrc, float* dgamma, float* dbeta, float* group_sums,
                                                float* ws, int64_t ws_floats, void* stream);

/* ---- training-mode BatchNorm of the camera head's conv stacks on GROUPED batch statistics (csrc/camera_bn_train.hip;
 * training.CameraHeadTrainer(batch_stats=True); reference Conv2d + nn.BatchNorm2d(eps 0.001, momentum 0.01) + LeakyReLU, camera_modules.py:36-48) --
 * c [G n][C] f32, dense; group g is the rows [g n, (g + 1) n): every group has its own statistics (the siamese tower runs once per view,
 * camera_head.py:646-647: G = 2 over the 2B-image batch, view 1 first; G = 1 elsewhere).  One call covers all groups.  Deterministic (no
 * atomics: per-block partials of NPS_BN_GROUPED_RPS rows of a group in ws, finished in NPS_BN_GROUPED_SEGMENTS runs in a fixed order); with
 * G > 1 every per-group result has the bits of a G = 1 call on that group's rows.  A thread works on four channels: C % 4 == 0 and every
 * pointer 16-byte aligned, 1 <= G <= NPS_BN_GROUPED_MAX_GROUPS (else NPS_E_ARG, before any launch).  mean, var, rstd: [G][C].
 * ws: at least NPS_BN_GROUPED_WORKSPACE_FLOATS(G, n, C) floats (both launchers).
 *  bn_train_grouped_stats:    per group and channel mean, biased variance, rstd = 1 / sqrt(var + eps) (per-block mean and centred sum of
 *                             squares merged by Chan's formula: never E[x^2] - E[x]^2).  running_mean / running_var [C] (both or neither)
 *                             are updated in place in the same launch, r <- (1 - momentum) r + momentum stat_g for g = 0, 1, .. in that
 *                             order, the variance unbiased (n / (n - 1)): what G module calls in a row leave.  n < 2: NPS_E_ARG.
 *  bn_train_grouped_apply:    y = act(gamma (c - mean_g) rstd_g + beta); act NPS_ACT_NONE, NPS_ACT_RELU or NPS_ACT_LEAKY (slope 0.01).
 *  bn_train_grouped_backward: dz = dy act'(z), z recomputed with apply's own expression (the side of the kink is the forward's, bit for
 *                             bit); per group S1_g = sum dz, S2_g = sum dz xhat; dc = gamma rstd_g (dz - S1_g / n - xhat S2_g / n);
 *                             dbeta = sum_g S1_g, dgamma = sum_g S2_g, added in group order.  batch_stats = 0: mean and rstd are
 *                             constants of the backward, dc = gamma rstd_g dz (dgamma, dbeta as above).
 *  bn_train_grouped_workspace_floats: the macro's value into *floats for callers that cannot read it (a status entry: NPS_E_ARG and 0 for
 *                             arguments the launchers refuse). */
#define NPS_BN_GROUPED_RPS 256
#define NPS_BN_GROUPED_SEGMENTS 16
#define NPS_BN_GROUPED_MAX_GROUPS 64
#define NPS_BN_GROUPED_WORKSPACE_FLOATS(G, n, C) ((int64_t)(G) * ((((int64_t)(n) + NPS_BN_GROUPED_RPS - 1) / NPS_BN_GROUPED_RPS) + 1) * 2 * (C))
nps_status nopesac_bn_train_grouped_workspace_floats(int G, int64_t n, int C, int64_t* floats);
nps_status nopesac_bn_train_grouped_stats_f32(const float* c, int G, int64_t n, int C, float eps, float momentum, float* mean, float* var,
                                              float* rstd, float* running_mean, float* running_var, float* ws, int64_t ws_floats,
                                              void* stream);
nps_status nopesac_bn_train_grouped_apply_f32(const float* c, int G, int64_t n, int C, const float* gamma, const float* beta,
                                              const float* mean, const float* rstd, int act, float* y, void* stream);
nps_status nopesac_bn_train_grouped_backward_f32(const float* dy, const float* c, int G, int64_t n, int C, const float* gamma,
                                                 const float* beta, const float* mean, const float* rstd, int act, int batch_stats,
                                                 float* dc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream);

/* ---- backward of a Linear with its operands read in place (csrc/linear_bwd.hip; training._LinearInPlace, PlaneEncoderTrainer) ---------
 * For y = act(x W^T + b) with x [M][K] (row stride x_stride), W [N][K] dense, and g [M][N] (row stride g_stride) the gradient at the
 * layer's output:  dx [M][K] (row stride dx_stride) = g' W,  dw [N][K] dense = g'^T x,  db [N] = column sums of g'.  g' is g behind two
 * optional gates, applied as the tiles are loaded (no launch writes a gated or transposed copy of x, g or y):
 *   y != null:  g'[m][n] = y[m][n] > 0 ? g[m][n] : 0        (the ReLU of the saved output, row stride y_stride);
 *   p > 0:      g'[m][n] = keep(m N + n) ? g'[m][n] / (1 - p) : 0, keep = csrc/dropout.h's decision under (seed, stream_id) at the
 *               row-major index in [M][N] - a dropout that sits directly behind the Linear (behind its ReLU, if both).
 * Each of dx, dw, db may be null (not computed); w is needed for dx, x for dw.  Exact-f32 MFMA on 128 x 128 tiles
 * (NPS_LINEAR_BWD_TILE); dw and db are split over `splits` (1 .. 1024) ranges of rows of M, rounded up to NPS_LINEAR_BWD_STAGE rows (a
 * range past M contributes zeros), written as partials into ws and summed in a fixed order: no atomics, the same inputs give the same
 * bits.  ws: at least NPS_LINEAR_BWD_WORKSPACE_FLOATS(N, K, splits) floats when dw or db is asked for (else it may be null).
 * NPS_E_ARG: K, N or a stride not a multiple of 4, a stride narrower than its row, a pointer not 16-byte aligned, M outside
 * 1 .. 2^31 - 1 (dx: at most 65535 row tiles), p outside [0, 1), a short workspace.
 * nopesac_linear_backward_workspace_floats: the macro's value for callers that cannot read it (0 for an argument < 0). */
#define NPS_LINEAR_BWD_TILE 128
#define NPS_LINEAR_BWD_STAGE 16
#define NPS_LINEAR_BWD_WORKSPACE_FLOATS(N, K, splits) ((int64_t)(splits) * ((int64_t)(N) * (K) + (N)))
int64_t nopesac_linear_backward_workspace_floats(int N, int K, int splits);
nps_status nopesac_linear_backward_f32(const float* x, int64_t x_stride, const float* w, const float* g, int64_t g_stride, const float* y,
                                       int64_t y_stride, double p, int64_t seed, int64_t stream_id, float* dx, int64_t dx_stride, float* dw,
                                       float* db, float* ws, int64_t ws_floats, int64_t M, int K, int N, int splits, void* stream);

/* ---- backward of the ResNet-50 backbone (csrc/backbone_bwd.hip; nopesac_amd/training.py::BackboneTrainer) --------------------------------
 * f32, NHWC, deterministic (no atomics), caller-owned buffers, argument errors -> NPS_E_ARG + nopesac_last_error.
 * nopesac_conv2d_dgrad_s2_f32: input gradient of a stride-2 conv with k 1 or 3 and pad (k - 1) / 2, any H, W >= 1:
 *   dY [B,OH,OW,Cout] (channel stride dy_cstride), w [Cout][Cin][KH][KW] (state-dict layout) -> dX [B,H,W,Cin] (channel stride dx_cstride).
 *   Implicit GEMM on the exact-f32 MFMA, decomposed by the parity of the input pixel: each of the four classes (row parity, column
 *   parity) is a GEMM with M = the class's pixels, N = Cin, K = its taps x Cout (k = 3: 1 / 2 / 2 / 4 taps; k = 1: one tap for
 *   even / even, and the other three classes are written as exact zeros), so the multiply count is the forward's.  w is repacked into
 *   w_ws as [KH][KW][Cout][Cin] (NPS_DGRAD_S2_WORKSPACE_BYTES: the weights' own size).  A workgroup computes NPS_DGRAD_S2_PIXELS pixels of one class x
 *   NPS_DGRAD_S2_CHANNELS input channels, NPS_DGRAD_S2_STAGE values of K per LDS stage.  Every element of dX is written once; with a channel
 *   stride above Cin the rest of a pixel is left as it was.  NPS_E_ARG: Cin, Cout or dy_cstride not a multiple of 4, dy or w_ws not
 *   16-byte aligned, a stride narrower than its channels, a short workspace.
 * nopesac_maxpool3x3s2_backward_f32: 3x3 / stride 2 / pad 1 max-pool of x [B,H,W,C], dY [B,OH,OW,C], OH = (H - 1) / 2 + 1 -> dX: every
 *   input element sums, in row-major window order, the dY of those of its up-to-four windows whose first maximum in row-major order
 *   over the in-bounds taps (torch.max_pool2d: strict >, padding never wins) is the element itself.
 * nopesac_frozen_bn_act_backward_f32: backward of y = act(c scale + shift [+ residual]) from the saved post-activation y, for g [rows][C]
 *   (row stride g_stride) and y (row stride y_stride): dz = act == RELU ? (y > 0 ? g : 0) : g (both zeros are "not > 0"),
 *   dc [rows][C] dense = dz * scale[c]; dz [rows][C] dense is written when the pointer is not null (the residual's gradient).  act: NONE
 *   or RELU.  No affine gradients: a FrozenBN has none. */
#define NPS_DGRAD_S2_PIXELS 128
#define NPS_DGRAD_S2_CHANNELS 128
#define NPS_DGRAD_S2_STAGE 16
#define NPS_DGRAD_S2_WORKSPACE_BYTES(Cin, Cout, KH, KW) ((int64_t)(Cin) * (Cout) * (KH) * (KW) * 4)
nps_status nopesac_conv2d_dgrad_s2_f32(const float* dy, const float* w, float* dx, float* w_ws, int64_t w_ws_bytes, int B, int H, int W, int Cin,
                                       int Cout, int KH, int KW, int pad, int64_t dy_cstride, int64_t dx_cstride, void* stream);
nps_status nopesac_maxpool3x3s2_backward_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream);
nps_status nopesac_frozen_bn_act_backward_f32(const float* g, const float* y, const float* scale, int act, int64_t rows, int C, int64_t g_stride,
                                              int64_t y_stride, float* dc, float* dz, void* stream);

/* ---- host-side PNG decode for the data mapper (csrc/png_host.hip; no kernel) ---------------------------------------------------------
 * The mp3d split stores 480 x 640 PNG frames (reference: data/planercnn_transforms.py:210-227 -> detectron2 utils.read_image -> PIL).
 * PIL decodes PNGs with the interpreter lock held; these entry points are called through ctypes with the lock released, so the reader
 * threads scale with the host's cores.  nopesac_png_info_host: 0 + geometry (*supported = 1 if the decoder below takes the file), negative
 * if the bytes are not a PNG.  nopesac_png_decode_host: the file's samples as interleaved RGB (bgr = 0) / BGR (bgr = 1) in out
 * [H * W * 3], converted like PIL's convert("RGB") (grey replicated, palette looked up, alpha dropped); 0, or -1 not a PNG, -2
 * unsupported (16-bit / sub-byte / interlaced: the caller falls back to PIL), -3 truncated / corrupt (CRC, inflate, filter type), -4 out
 * too small.  (zlib is optional: only the NOPESAC_PNG_ZLIB_INFLATE=1 A/B path uses it; the default inflate is csrc/inflate_host.h.) */
int nopesac_png_info_host(const unsigned char* data, int64_t n, int* height, int* width, int* channels, int* supported);
int nopesac_png_decode_host(const unsigned char* data, int64_t n, unsigned char* out, int64_t out_bytes, int bgr);
/* A batch of PNG FILES on `threads` threads of the call itself (replaces the per-image Python of the reference mapper,
 * planercnn_transforms.py:210-227, whose open / read / array / transpose steps hold the interpreter lock): file paths[i] -> out + i *
 * image_stride, H x W x 3 interleaved or (flags bit 1) 3 x H x W channel-major - the mapper's CHW layout - in RGB or (flags bit 0) BGR
 * order.  status[i] = 0, a code of nopesac_png_decode_host, -5 geometry is not H x W, -6 unreadable file.  Returns the number of files
 * with a non-zero status (the caller hands those to PIL), negative on bad arguments. */
int nopesac_png_decode_files_host(const char* const* paths, int n, unsigned char* out, int64_t image_stride, int H, int W, int flags,
                                  int threads, int* status);
/* The decoder's own inflate (csrc/inflate_host.h: a whole RFC 1950 / 1951 stream in memory -> a buffer of known size; replaces zlib's
 * streaming inflate, the floor of the PNG path) on its own, for tests: bytes written, or -1 on any malformed stream / overflow. */
int64_t nopesac_inflate_zlib_host(const unsigned char* in, int64_t n, unsigned char* out, int64_t out_cap);

#ifdef __cplusplus
}
#endif
#endif /* NOPESAC_HIP_H */
