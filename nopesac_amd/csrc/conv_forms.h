// Which kernel configurations of the conv family (NPS_CONV_CFG_* of include/nopesac_hip.h) may run a call: every limit of the bfrag,
// halo, p8 and p8n kernels is stated here once.  nopesac_conv2d_nhwc_forms (conv_igemm.hip) turns the predicates into the bitmask the
// autotuner reads; the entry points call the same predicates as their argument check.  Host only.  Not a public header.
#pragma once
#include <initializer_list>

#include "common.h"

namespace nps {

constexpr int P8_SK_MAX_TILES = 4096;      // arrival counters at the head of the stream-K workspace (conv_p8.hip)

// The facts that decide eligibility.  `aligned`: every buffer of the call (x, w, y, residual, scale, bias) is 16-byte aligned.
// `entry`: the call comes from an entry point, which adds the two conditions the tuner's flags never carried (marked below).  The
// bfrag / halo / p8 flags are part of every routing key (profiles/routing_*.json), so the mask keeps them as they were tuned.
struct ConvCall {
    int x_dt, w_dt, out_dt;                // NPS_DT_*
    int B, H, W, Cin, Cout, KH, KW, stride, pad;
    long long x_cs, y_cs, r_cs;
    bool batched, has_residual, has_scale, has_bias;
    int act;                               // the whole act word (NPS_ACT_RES_AFTER / NPS_ACT_BIAS_BATCHED included)
    bool aligned, entry;

    // floor division: the flags of a call with an empty output (OH <= 0) are pinned too (tests/test_conv_routing_cpu.py)
    static long long fdiv(long long a, long long b) { return a / b - ((a % b != 0 && ((a < 0) != (b < 0))) ? 1 : 0); }
    long long OH() const { return fdiv(H + 2ll * pad - KH, stride) + 1; }
    long long OW() const { return fdiv(W + 2ll * pad - KW, stride) + 1; }
    long long M() const { return B * OH() * OW(); }
    long long K() const { return (long long)KH * KW * Cin; }
    long long tiles(int bm, int bn) const { return -fdiv(-M(), bm) * (Cout / bn); }
};

static inline bool conv_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if ((uintptr_t)q % 16 != 0) return false;
    return true;
}

// Every predicate returns nullptr (the call may run) or the reason it may not.
#define NPS_CHECK_CONV(name, expr)                  \
    do {                                            \
        const char* why__ = (expr);                 \
        NPS_CHECK_ARG(!why__, name ": %s", why__);  \
    } while (0)

// ---- can the kernel run it

// a well-formed convolution: what every entry point asks before its kernel's own limits
static inline const char* conv_call_refusal(const ConvCall& c) {
    if (!(c.B > 0 && c.H > 0 && c.W > 0 && c.Cin > 0 && c.Cout > 0 && c.KH > 0 && c.KW > 0 && c.stride > 0 && c.pad >= 0)) return "bad dims";
    if (c.OH() <= 0 || c.OW() <= 0) return "empty output";
    if (c.out_dt != NPS_DT_F32 && c.out_dt != NPS_DT_BF16 && c.out_dt != NPS_DT_FP8) return "bad out_dt";
    if (c.x_cs < c.Cin || c.y_cs < c.Cout || (c.has_residual && c.r_cs < c.Cout)) return "channel stride smaller than channel count";
    if ((c.act & 0xff) > NPS_ACT_SIGMOID) return "bad act";
    return nullptr;
}

// the operands all four kernels share: 16-byte channel runs of 64-channel K-tiles, 32-bit offsets into x
static inline const char* conv_dma_refusal(const ConvCall& c, int cout_tile) {
    const int eb = c.x_dt == NPS_DT_FP8 ? 1 : 2;
    if ((c.x_dt != NPS_DT_BF16 && c.x_dt != NPS_DT_FP8) || c.w_dt != c.x_dt || c.batched) return "needs bf16 (or fp8) x and w, shared weights";
    if (c.Cin % 64 != 0 || c.Cout % cout_tile != 0) return cout_tile == 256 ? "needs Cin % 64 == 0 and Cout % 256 == 0" : "needs Cin % 64 == 0 and Cout % 128 == 0";
    if (c.KH * c.KW > 32) return "more than 32 taps";
    if (c.x_cs % (16 / eb) != 0) return "x_cstride must be a multiple of 16 bytes";
    if (((long long)c.B * c.H * c.W + (long long)c.pad * c.W + c.pad) * c.x_cs * eb >= (1ll << 31)) return "input larger than 2 GB";
    return nullptr;
}

// the 24-bit index math of the p8 / p8n kernels
static inline const char* conv_idx24_refusal(const ConvCall& c) {
    if ((long long)c.B * c.H * c.W >= (1 << 23) || c.x_cs >= (1 << 24) || c.K() >= (1 << 24)) return "pixel count / strides beyond the 24-bit index math of this kernel";
    if (c.Cout * c.K() * 2 >= (1ll << 31)) return "weights larger than 2 GB";
    return nullptr;
}

// conv_igemm_bfrag_kernel (configurations 7 / 8; nopesac_conv2d_nhwc_fp8 with fp8 operands)
static inline const char* conv_bfrag_refusal(const ConvCall& c) {
    if (const char* why = conv_dma_refusal(c, 128)) return why;
    if (c.act & ~(0xff | NPS_ACT_RES_AFTER)) return "unsupported act flags";
    // entry point only: the tuner offers bfrag for such a call, the launch is refused and the tuner drops the candidate
    if (c.entry && c.out_dt == NPS_DT_FP8 && (c.has_residual || c.y_cs % 8 != 0 || !c.aligned)) return "fp8 output needs no residual and 8-channel-aligned y / scale / bias";
    return nullptr;
}

// conv3x3_halo_kernel (9 / 10): bfrag's operands, one fixed geometry and epilogue
static inline const char* conv_halo_refusal(const ConvCall& c) {
    if (const char* why = conv_bfrag_refusal(c)) return why;
    if (c.x_dt != NPS_DT_BF16 || c.out_dt != NPS_DT_BF16) return "bf16 only";
    if (c.KH != 3 || c.KW != 3 || c.stride != 1 || c.pad != 1) return "3x3 / stride 1 / pad 1 only";
    if (c.x_cs != c.Cin || c.y_cs != c.Cout) return "dense channels only";
    if (c.has_residual || !c.has_scale || !c.has_bias || (c.act & ~0xff)) return "y = act(conv * scale + bias) only: scale and bias, no residual";
    return nullptr;
}

// conv_igemm_p8_kernel (11)
static inline const char* conv_p8_refusal(const ConvCall& c) {
    if (const char* why = conv_dma_refusal(c, 256)) return why;
    if (c.x_dt != NPS_DT_BF16) return "bf16 only";
    if (const char* why = conv_idx24_refusal(c)) return why;
    if (c.act & ~(0xff | NPS_ACT_RES_AFTER)) return "unsupported act flags";
    if (c.out_dt != NPS_DT_F32 && c.out_dt != NPS_DT_BF16 && c.out_dt != NPS_DT_FP8) return "bad out_dt";
    const int al = c.out_dt == NPS_DT_F32 ? 4 : 8;
    if (c.has_residual && c.out_dt == NPS_DT_FP8) return "residual with fp8 output";
    if (!c.aligned || c.y_cs % al != 0 || (c.has_residual && c.r_cs % al != 0)) return "every buffer must be 16-byte aligned with 16-byte-aligned y / residual strides";
    if (c.entry && c.M() >= (1 << 23)) return "output pixel count beyond the 24-bit index math of this kernel";       // entry point only
    return nullptr;
}

// conv_igemm_p8_kernel<.., SK> (12)
static inline const char* conv_p8_sk_refusal(const ConvCall& c) {
    if (const char* why = conv_p8_refusal(c)) return why;
    if (c.tiles(256, 256) > P8_SK_MAX_TILES) return "more tiles than the stream-K workspace has arrival counters (use the plain kernel: nothing to balance)";
    return nullptr;
}

// conv_igemm_p8n_kernel (13 / 14).  (M + 256) * y_cs * 2 < 2 GB with y_cs >= Cout >= 128 keeps M inside the 24-bit index math
static inline const char* conv_p8n_refusal(const ConvCall& c) {
    if (const char* why = conv_dma_refusal(c, 128)) return why;
    if (c.x_dt != NPS_DT_BF16 || c.out_dt != NPS_DT_BF16 || c.has_residual) return "bf16 in / bf16 out, no residual";
    if (const char* why = conv_idx24_refusal(c)) return why;
    if (c.act != NPS_ACT_NONE && c.act != NPS_ACT_RELU && c.act != NPS_ACT_LEAKY) return "act must be none / ReLU / LeakyReLU (no residual forms)";
    if (!c.aligned || c.y_cs % 8 != 0) return "every buffer must be 16-byte aligned with y_cstride % 8 == 0";
    if ((c.M() + 256) * c.y_cs * 2 >= (1ll << 31)) return "output larger than 2 GB";
    return nullptr;
}

// conv_igemm_p8n_kernel<.., SPLIT> (15) with `splits` K slices per tile
static inline const char* conv_p8n_split_refusal(const ConvCall& c, int splits) {
    if (const char* why = conv_p8n_refusal(c)) return why;
    if (splits < 2 || splits > c.Cin / 64 || splits > 16) return "2 <= splits <= min(Cin / 64, 16)";
    if (splits * c.M() * c.Cout * 4 >= (1ll << 31)) return "split-K workspace larger than 2 GB";
    return nullptr;
}

// ---- does the tuner offer it (policy: a kernel that can run the call is still not timed where it cannot win)

// stream-K only where whole rounds leave CUs idle: a few tiles per CU and a K loop long enough to cut
static inline bool conv_p8_sk_offered(const ConvCall& c) { return c.tiles(256, 256) <= 1024 && c.K() >= 512; }

// tap-major K order: a 1x1 conv has one tap, both orders are the same launch
static inline bool conv_p8n_tap_offered(const ConvCall& c) { return c.KH * c.KW > 1; }

// split-K: fewer tiles than half the CUs and a K loop of >= 64 K-tiles; slices = CUs / tiles, at most 8 and one per 64-channel group
static inline int conv_p8n_split_slices(const ConvCall& c) {
    const long long tiles = c.Cout % 128 == 0 ? c.tiles(256, 128) : 0;
    if (tiles == 0) return 0;
    long long s = ConvCall::fdiv(256, tiles);
    if (s > c.Cin / 64) s = c.Cin / 64;
    return (int)(s > 8 ? 8 : s);
}
static inline bool conv_p8n_split_offered(const ConvCall& c, int splits) { return c.K() >= 4096 && splits >= 2; }

}  // namespace nps
