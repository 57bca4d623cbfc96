// Model-wide optimiser step (include/nopesac_hip.h "model-wide optimiser step"; nopesac_amd/optim.py): one gather launch and one step
// launch over ANY number of tensors.  The per-tensor kernels of refine_bwd.hip (scale_by_kernel, adamw_step_kernel, sgd_step_kernel) are
// the yardstick: the update below performs their operations in their order on every element, so its results are theirs bit for bit
// (the library is compiled with -ffp-contract=off: no multiply-add is fused here or there).
//
// A workgroup is one UNIT: up to NPS_OPT_CHUNK = 4096 consecutive elements of ONE segment, four float4 per thread.  units[blockIdx.x]
// says which, in one load; everything a workgroup reads from the tables is uniform across it.  The arenas' side of every access is
// 16-byte aligned by construction (offsets are multiples of 64 floats, chunks of 4096); the caller's side (gradient source, parameter)
// decides between the float4 path and the scalar path, per workgroup.  Loads inside the unrolled batches are unconditional from a
// clamped index, the bound only gates the store (README "A guarded load serialises").
#include <math.h>

#include "common.h"

namespace nps {

constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC = NPS_OPT_CHUNK / 4 / OPT_THREADS;        // float4 per thread and unit (4)
constexpr int OPT_SCALAR = NPS_OPT_CHUNK / OPT_THREADS;         // scalar path: elements per thread and unit (16), in batches of 4
static_assert(OPT_VEC * 4 * OPT_THREADS == NPS_OPT_CHUNK && OPT_SCALAR % 4 == 0, "a unit is four float4 per thread");
static_assert(NPS_OPT_CHUNK % NPS_OPT_ALIGN == 0 && NPS_OPT_ALIGN % 4 == 0, "chunks and segments start on float4 boundaries of the arenas");

struct OptUnit {
    const nopesac_opt_segment* seg;
    long long base;      // first element of the unit inside its segment
    int cnt;             // live elements of the unit, 1..NPS_OPT_CHUNK
    int segment;
};

// The unit of this workgroup, or cnt = 0 when the tables do not agree with their own bounds (never the case for tables built by
// optim.unit_map; a workgroup must not fault on a wrong one).
__device__ __forceinline__ OptUnit opt_unit(const nopesac_opt_segment* segments, const nopesac_opt_unit* units, int n_segments, long long arena_floats) {
    OptUnit u;
    const nopesac_opt_unit w = units[blockIdx.x];
    u.segment = w.segment;
    u.cnt = 0;
    u.base = 0;
    u.seg = segments;
    if (w.segment < 0 || w.segment >= n_segments || w.chunk < 0) return u;
    u.seg = segments + w.segment;
    const long long n = u.seg->n, off = u.seg->offset;
    u.base = (long long)w.chunk * NPS_OPT_CHUNK;
    if (n <= 0 || off < 0 || (off % NPS_OPT_ALIGN) != 0 || off > arena_floats - n || u.base >= n) return u;
    const long long left = n - u.base;
    u.cnt = left < NPS_OPT_CHUNK ? (int)left : NPS_OPT_CHUNK;
    return u;
}

__device__ __forceinline__ bool opt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// G[offset + i] = src[i] (present) or 0 (absent).  The float4 stores run to the end of the last, partly live vector: the lanes past
// cnt hold zeros and fall into the segment's own zero padding (n is padded to a multiple of 64 floats).
__global__ __launch_bounds__(OPT_THREADS) void opt_gather_kernel(const nopesac_opt_segment* __restrict__ segments, const nopesac_opt_source* __restrict__ sources,
                                                                 const nopesac_opt_unit* __restrict__ units, int n_segments, float* __restrict__ G,
                                                                 long long arena_floats) {
    const OptUnit u = opt_unit(segments, units, n_segments, arena_floats);
    if (u.cnt == 0) return;
    const nopesac_opt_source so = sources[u.segment];
    const int tid = threadIdx.x, cnt = u.cnt;
    float* __restrict__ g = G + u.seg->offset + u.base;
    const int nvec = (cnt + 3) >> 2, nfull = cnt >> 2;
    if (!(so.flags & NPS_OPT_PRESENT) || so.src == nullptr) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < OPT_VEC; ++j) {
            const int v = j * OPT_THREADS + tid;
            if (v < nvec) reinterpret_cast<float4*>(g)[v] = z;
        }
        return;
    }
    const float* __restrict__ s = so.src + u.base;
    if (opt_aligned16(s)) {
        if (nfull > 0) {
            float4 x[OPT_VEC];
#pragma unroll
            for (int j = 0; j < OPT_VEC; ++j) {
                const int v = j * OPT_THREADS + tid;
                x[j] = reinterpret_cast<const float4*>(s)[v < nfull ? v : nfull - 1];
            }
#pragma unroll
            for (int j = 0; j < OPT_VEC; ++j) {
                const int v = j * OPT_THREADS + tid;
                if (v < nfull) reinterpret_cast<float4*>(g)[v] = x[j];
            }
        }
        if (nvec > nfull && tid < 4) {                           // scalar tail: the 1..3 elements behind the last whole vector
            const int e = nfull * 4 + tid;
            const float x = s[e < cnt ? e : cnt - 1];
            g[e] = e < cnt ? x : 0.f;
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < OPT_SCALAR; b += 4) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = (b + k) * OPT_THREADS + tid;
            x[k] = s[e < cnt ? e : cnt - 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = (b + k) * OPT_THREADS + tid;
            if (e < nvec * 4) g[e] = e < cnt ? x[k] : 0.f;
        }
    }
}

struct OptHyper {
    float lr, wd, beta1, beta2, eps, momentum, bc1, bc2;
    int first;
};
constexpr int OPT_K_ADAMW = 0, OPT_K_SGD_MOMENTUM = 1, OPT_K_SGD_PLAIN = 2;      // the builds of the step kernel: which moments it streams

// One element: scale_by_kernel's multiply, then adamw_step_kernel / sgd_step_kernel, operation for operation.
template <int KIND>
__device__ __forceinline__ void opt_update(float& p, float gi, float& m1, float& m2, const OptHyper& h, float coef) {
    gi = gi * coef;
    if constexpr (KIND == OPT_K_ADAMW) {
        float w = p;
        w *= 1.f - h.lr * h.wd;
        const float a = h.beta1 * m1 + (1.f - h.beta1) * gi;
        const float v = h.beta2 * m2 + (1.f - h.beta2) * gi * gi;
        m1 = a; m2 = v;
        const float denom = sqrtf(v) / sqrtf(h.bc2) + h.eps;
        p = w - (h.lr / h.bc1) * a / denom;
    } else {
        gi = gi + h.wd * p;
        if constexpr (KIND == OPT_K_SGD_MOMENTUM) {
            const float bu = h.first ? gi : h.momentum * m1 + gi;
            m1 = bu;
            gi = bu;
        }
        p -= h.lr * gi;
    }
}

struct OptStepParams {          // the kernel's by-value argument block (bias corrections already formed)
    const nopesac_opt_segment* segments;
    const nopesac_opt_source* sources;
    const nopesac_opt_unit* units;
    long long arena_floats;
    const float* G;
    float* M1;
    float* M2;
    const float* coef;
    int n_segments, reserved;
    float beta1, beta2, eps, momentum, bc1, bc2;
    nopesac_opt_group groups[NPS_OPT_MAX_GROUPS];
};

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void opt_step_kernel(const OptStepParams a) {
    const OptUnit u = opt_unit(a.segments, a.units, a.n_segments, a.arena_floats);
    if (u.cnt == 0) return;
    const int flags = a.sources[u.segment].flags;
    if (!(flags & NPS_OPT_PRESENT)) return;
    OptHyper h;
    h.lr = h.wd = 0.f;
    const int grp = u.seg->group;
#pragma unroll
    for (int k = 0; k < NPS_OPT_MAX_GROUPS; ++k)                 // constant indices: the by-value table stays in the argument segment
        if (k == grp) { h.lr = a.groups[k].lr; h.wd = a.groups[k].weight_decay; }
    h.beta1 = a.beta1; h.beta2 = a.beta2; h.eps = a.eps; h.momentum = a.momentum; h.bc1 = a.bc1; h.bc2 = a.bc2;
    h.first = (flags & NPS_OPT_FIRST) != 0;
    constexpr bool moments2 = KIND == OPT_K_ADAMW, moments1 = KIND != OPT_K_SGD_PLAIN;
    const float coef = a.coef ? a.coef[0] : 1.f;
    const int tid = threadIdx.x, cnt = u.cnt;
    const long long at = u.seg->offset + u.base;
    float* __restrict__ p = u.seg->param + u.base;
    const float* __restrict__ g = a.G + at;
    float* __restrict__ m1 = a.M1 + at;
    float* __restrict__ m2 = moments2 ? a.M2 + at : a.M1 + at;   // (SGD never reads or writes it)
    const int nfull = opt_aligned16(p) ? cnt >> 2 : 0;           // whole vectors on the float4 path; the scalar path takes everything
    if (nfull > 0) {
        float4 pv[OPT_VEC], gv[OPT_VEC], av[OPT_VEC], bv[OPT_VEC];
#pragma unroll
        for (int j = 0; j < OPT_VEC; ++j) {
            const int v = j * OPT_THREADS + tid, vc = v < nfull ? v : nfull - 1;
            pv[j] = reinterpret_cast<const float4*>(p)[vc];
            gv[j] = reinterpret_cast<const float4*>(g)[vc];
            av[j] = bv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (moments1) av[j] = reinterpret_cast<const float4*>(m1)[vc];
            if constexpr (moments2) bv[j] = reinterpret_cast<const float4*>(m2)[vc];
        }
#pragma unroll
        for (int j = 0; j < OPT_VEC; ++j) {
            const int v = j * OPT_THREADS + tid;
            opt_update<KIND>(pv[j].x, gv[j].x, av[j].x, bv[j].x, h, coef);
            opt_update<KIND>(pv[j].y, gv[j].y, av[j].y, bv[j].y, h, coef);
            opt_update<KIND>(pv[j].z, gv[j].z, av[j].z, bv[j].z, h, coef);
            opt_update<KIND>(pv[j].w, gv[j].w, av[j].w, bv[j].w, h, coef);
            if (v < nfull) {
                reinterpret_cast<float4*>(p)[v] = pv[j];
                if constexpr (moments1) reinterpret_cast<float4*>(m1)[v] = av[j];
                if constexpr (moments2) reinterpret_cast<float4*>(m2)[v] = bv[j];
            }
        }
    }
    const int done = nfull * 4;                                  // scalar tail (float4 path: 0..3 elements) or the whole unit (scalar path)
    if (done == cnt) return;
    const int rest = cnt - done;
#pragma unroll
    for (int b = 0; b < OPT_SCALAR; b += 4) {
        if (b * OPT_THREADS >= rest) break;
        float ps[4], gs[4], as[4], bs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = (b + k) * OPT_THREADS + tid, e = done + (r < rest ? r : rest - 1);
            ps[k] = p[e];
            gs[k] = g[e];
            as[k] = bs[k] = 0.f;
            if constexpr (moments1) as[k] = m1[e];
            if constexpr (moments2) bs[k] = m2[e];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = (b + k) * OPT_THREADS + tid, e = done + r;
            opt_update<KIND>(ps[k], gs[k], as[k], bs[k], h, coef);
            if (r < rest) {
                p[e] = ps[k];
                if constexpr (moments1) m1[e] = as[k];
                if constexpr (moments2) m2[e] = bs[k];
            }
        }
    }
}

}  // namespace nps

using namespace nps;

static inline bool opt_finite(float v) { return isfinite(v); }

#define OPT_CHECK_TABLES(name, segments, sources, units, n_segments, n_units, arena_floats)                                                    \
    NPS_CHECK_ARG((segments) && (sources) && (units), name ": null table");                                                                  \
    NPS_CHECK_ARG((n_segments) >= 1 && (n_segments) <= NPS_OPT_MAX_SEGMENTS, name ": n_segments=%d outside 1..%d", (int)(n_segments),        \
                  NPS_OPT_MAX_SEGMENTS);                                                                                                     \
    NPS_CHECK_ARG((n_units) >= (n_segments) && (n_units) <= 0x7fffffffLL, name ": n_units=%lld (at least one per segment, at most 2^31 - 1)", \
                  (long long)(n_units));                                                                                                     \
    NPS_CHECK_ARG((arena_floats) >= (int64_t)NPS_OPT_ALIGN * (n_segments) && (arena_floats) % NPS_OPT_ALIGN == 0 &&                          \
                      (n_units) <= (arena_floats) / NPS_OPT_ALIGN,                                                                           \
                  name ": arena_floats=%lld (a multiple of %d holding every segment and unit)", (long long)(arena_floats), NPS_OPT_ALIGN)

extern "C" int nopesac_opt_gather(const nopesac_opt_segment* segments, const nopesac_opt_source* sources, const nopesac_opt_unit* units, int n_segments,
                                  int64_t n_units, float* G, int64_t arena_floats, void* stream) {
    OPT_CHECK_TABLES("opt_gather", segments, sources, units, n_segments, n_units, arena_floats);
    NPS_CHECK_ARG(G && ((uintptr_t)G & 15) == 0, "opt_gather: G null or not 16-byte aligned");
    hipLaunchKernelGGL(opt_gather_kernel, dim3((unsigned)n_units), dim3(OPT_THREADS), 0, (hipStream_t)stream, segments, sources, units, n_segments, G,
                       (long long)arena_floats);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_opt_step(const nopesac_opt_step_args* a, void* stream) {
    NPS_CHECK_ARG(a != nullptr, "opt_step: null argument block");
    OPT_CHECK_TABLES("opt_step", a->segments, a->sources, a->units, a->n_segments, a->n_units, a->arena_floats);
    NPS_CHECK_ARG(a->mode == NPS_OPT_ADAMW || a->mode == NPS_OPT_SGD, "opt_step: mode=%d (NPS_OPT_ADAMW or NPS_OPT_SGD)", a->mode);
    const bool sgd = a->mode == NPS_OPT_SGD;
    NPS_CHECK_ARG(a->G && ((uintptr_t)a->G & 15) == 0, "opt_step: G null or not 16-byte aligned");
    NPS_CHECK_ARG((sgd && a->momentum == 0.f) || (a->M1 && ((uintptr_t)a->M1 & 15) == 0), "opt_step: M1 null or not 16-byte aligned");
    NPS_CHECK_ARG(sgd || (a->M2 && ((uintptr_t)a->M2 & 15) == 0), "opt_step: M2 null or not 16-byte aligned");
    NPS_CHECK_ARG(a->n_groups >= 1 && a->n_groups <= NPS_OPT_MAX_GROUPS, "opt_step: n_groups=%d outside 1..%d", a->n_groups, NPS_OPT_MAX_GROUPS);
    for (int k = 0; k < a->n_groups; ++k)
        NPS_CHECK_ARG(opt_finite(a->groups[k].lr) && opt_finite(a->groups[k].weight_decay), "opt_step: group %d: lr / weight_decay not finite", k);
    NPS_CHECK_ARG(a->step >= 1, "opt_step: step=%d (counts from 1)", a->step);
    if (sgd) {
        NPS_CHECK_ARG(opt_finite(a->momentum) && a->momentum >= 0.f, "opt_step: momentum=%g", (double)a->momentum);
    } else {
        NPS_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f, "opt_step: betas (%g, %g) outside [0, 1)", (double)a->beta1,
                      (double)a->beta2);
        NPS_CHECK_ARG(opt_finite(a->eps) && a->eps >= 0.f, "opt_step: eps=%g", (double)a->eps);
    }
    OptStepParams k;
    k.segments = a->segments; k.sources = a->sources; k.units = a->units; k.arena_floats = a->arena_floats;
    k.G = a->G; k.M1 = a->M1; k.M2 = a->M2; k.coef = a->coef;
    k.n_segments = a->n_segments; k.reserved = 0;
    k.beta1 = a->beta1; k.beta2 = a->beta2; k.eps = a->eps; k.momentum = a->momentum;
    k.bc1 = 1.f - powf(a->beta1, (float)a->step); k.bc2 = 1.f - powf(a->beta2, (float)a->step);     // as nopesac_adamw_step forms them
    for (int g = 0; g < NPS_OPT_MAX_GROUPS; ++g) k.groups[g] = g < a->n_groups ? a->groups[g] : nopesac_opt_group{0.f, 0.f};
    const dim3 grid((unsigned)a->n_units), block(OPT_THREADS);
    if (!sgd) hipLaunchKernelGGL(opt_step_kernel<OPT_K_ADAMW>, grid, block, 0, (hipStream_t)stream, k);
    else if (a->momentum != 0.f) hipLaunchKernelGGL(opt_step_kernel<OPT_K_SGD_MOMENTUM>, grid, block, 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(opt_step_kernel<OPT_K_SGD_PLAIN>, grid, block, 0, (hipStream_t)stream, k);
    NPS_LAUNCH_RET();
}
