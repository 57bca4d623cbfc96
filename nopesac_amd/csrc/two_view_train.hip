// Where the plane head's outputs meet the two-view heads in training (reference: siamese_planeTR.py:237-299, the joint stage with
// MASK_ON / EMBEDDING_ON / CAMERA_ON): the gradients of the camera head's refinement losses with respect to the PLANES of both views,
// and the matched queries of every image moved to a prefix on the device.
//   (1) refine_score_maps_bwd_geo_kernel : the cotangent of ransac_score_maps_kernel (ransac.hip) that refine_score_maps_bwd_kernel
//       (refine_bwd.hip) leaves out - geo_local.  That kernel owns one hypothesis and walks the planes; this one owns one matched plane
//       and walks the nq + 1 hypotheses in order (the transpose of that walk), so every output element has one owner and one order.
//   (2) geo_sequence_bwd_kernel : backward of geo_sequence_kernel with respect to planes1 / planes2 (the pose is detached in the reference,
//       camera_head.py:353-368; sig is piecewise constant).  The sequence positions are recomputed as the forward computes them.
//   (3) match_compact / its backward / corr_compact : the reference's masked subsets of queries (matching_head.py:51-69) as a prefix in
//       ascending query index, the scatter back, and gt_corr gathered through both views' order.
// Everything is f32 (or integer) and deterministic: no float atomics, every sum runs in a fixed order.  Held per element to float64
// vector-Jacobian products and to a numpy restatement by tests/test_two_view_forms_gpu.py.
#include "common.h"

namespace nps {

constexpr int TT_MAXQ = NPS_PLANE_MAX_QUERIES;

// warp_plane (common.h) differentiated with respect to the PLANE p: out = c u, u = R flip(p), c = ((u + t) . u) / (|u| + 1e-5)^2.
// gp += flip(R^T gu) with gu as warp_plane_bwd (refine_bwd.hip) forms it; a zero plane gets nothing (out = 0 whatever R, t).
__device__ __forceinline__ void warp_plane_bwd_plane(const float p[3], const float R[9], const float t[3], const float g[3], float gp[3]) {
    const float f[3] = {p[0], -p[1], -p[2]};
    float u[3], e[3];
    for (int i = 0; i < 3; ++i) {
        u[i] = R[3 * i] * f[0] + R[3 * i + 1] * f[1] + R[3 * i + 2] * f[2];
        e[i] = u[i] + t[i];
    }
    const float nu = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (nu == 0.f) return;
    const float nb = nu + 1e-5f;
    const float dot = e[0] * u[0] + e[1] * u[1] + e[2] * u[2];
    const float c = dot / (nb * nb);
    const float gu_dot = g[0] * u[0] + g[1] * u[1] + g[2] * u[2];
    float gu[3];
    for (int i = 0; i < 3; ++i) {
        const float dc = (2.f * u[i] + t[i]) / (nb * nb) - 2.f * dot * u[i] / (nb * nb * nb * nu);
        gu[i] = c * g[i] + gu_dot * dc;
    }
    gp[0] += R[0] * gu[0] + R[3] * gu[1] + R[6] * gu[2];
    gp[1] -= R[1] * gu[0] + R[4] * gu[1] + R[7] * gu[2];
    gp[2] -= R[2] * gu[0] + R[5] * gu[1] + R[8] * gu[2];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) grid (ceil(nq / 64), B), 64 threads: thread = matched plane j of pair b.  The hypotheses' rotation matrices and translations are
// staged in LDS once per workgroup, with the quaternion normalisation of the forward.
__global__ __launch_bounds__(64) void refine_score_maps_bwd_geo_kernel(
    const float* __restrict__ geo_local, const float* __restrict__ rot_raw, const float* __restrict__ trans_raw,
    const float* __restrict__ init_rot, const float* __restrict__ init_trans, const int* __restrict__ mp, int nq,
    const float* __restrict__ g_normal_score, const float* __restrict__ g_param_score, const float* __restrict__ g_l2_dist,
    float* __restrict__ g_geo_local) {
    const int b = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * 64 + tid;
    const int NH = nq + 1;
    __shared__ float sR[(TT_MAXQ + 1) * 9], sT[(TT_MAXQ + 1) * 3];
    const int m = min(max(mp[b], 0), nq);
    for (int h = tid; h < NH; h += 64) {
        float q[4], t[3];
        if (h == 0) {
            for (int d = 0; d < 4; ++d) q[d] = init_rot[4 * b + d];
            for (int d = 0; d < 3; ++d) t[d] = init_trans[3 * b + d];
        } else {
            const float* rr = rot_raw + ((long long)b * nq + h - 1) * 4;
            const float nn = fmaxf(sqrtf(rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3]), 1e-12f);
            for (int d = 0; d < 4; ++d) q[d] = rr[d] / nn;
            for (int d = 0; d < 3; ++d) t[d] = trans_raw[((long long)b * nq + h - 1) * 3 + d];
        }
        quat_to_rot(q, sR + 9 * h);
        for (int d = 0; d < 3; ++d) sT[3 * h + d] = t[d];
    }
    __syncthreads();
    if (j >= nq) return;
    float* out = g_geo_local + ((long long)b * nq + j) * 6;
    float g0[3] = {0.f, 0.f, 0.f}, g1[3] = {0.f, 0.f, 0.f};      // gradients of the first plane and of the FLIPPED second plane
    if (j < m) {
        const float* gl = geo_local + ((long long)b * nq + j) * 6;
        const float p0[3] = {gl[0], gl[1], gl[2]};
        const float p1[3] = {gl[3], -gl[4], -gl[5]};
        const float z[3] = {0.f, 0.f, 0.f};
        float n1v[3];
        normalize3(p1, n1v);
        const float np1 = norm3(p1);
        for (int h = 0; h < NH; ++h) {
            const long long o = ((long long)b * NH + h) * nq + j;
            const float mask = h <= m ? 1.f : 0.f;
            const float g_ns = g_normal_score[o] * mask, g_ps = g_param_score[o] * mask, g_l2 = g_l2_dist[o];
            if (g_ns == 0.f && g_ps == 0.f && g_l2 == 0.f) continue;
            const float* R = sR + 9 * h;
            const float* t = sT + 3 * h;
            float w_r[3], w_rt[3], n0[3];
            warp_plane(p0, R, z, w_r);
            warp_plane(p0, R, t, w_rt);
            normalize3(w_r, n0);
            if (g_ns != 0.f) {
                const float d0 = n0[0] - n1v[0], d1 = n0[1] - n1v[1], d2 = n0[2] - n1v[2];
                const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
                const float nw = norm3(w_r);
                if (dn > 0.f) {
                    const float gdn = -expf(-dn) * g_ns;
                    const float gn0[3] = {gdn * d0 / dn, gdn * d1 / dn, gdn * d2 / dn};
                    if (nw >= 1e-12f) {
                        const float dt = gn0[0] * n0[0] + gn0[1] * n0[1] + gn0[2] * n0[2];
                        const float gw[3] = {(gn0[0] - dt * n0[0]) / nw, (gn0[1] - dt * n0[1]) / nw, (gn0[2] - dt * n0[2]) / nw};
                        warp_plane_bwd_plane(p0, R, z, gw, g0);
                    }
                    // the second plane's side: n1v = normalize3(p1), d (n0 - n1v) / d n1v = -1
                    if (np1 >= 1e-12f) {
                        const float dt = gn0[0] * n1v[0] + gn0[1] * n1v[1] + gn0[2] * n1v[2];
                        for (int d = 0; d < 3; ++d) g1[d] -= (gn0[d] - dt * n1v[d]) / np1;
                    } else {
                        for (int d = 0; d < 3; ++d) g1[d] -= gn0[d] / 1e-12f;
                    }
                }
            }
            {
                const float e0 = w_rt[0] - p1[0], e1 = w_rt[1] - p1[1], e2 = w_rt[2] - p1[2];
                const float dl2 = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
                if (dl2 > 0.f) {
                    const float gd = -expf(-dl2) * g_ps + g_l2;
                    const float gw[3] = {gd * e0 / dl2, gd * e1 / dl2, gd * e2 / dl2};
                    warp_plane_bwd_plane(p0, R, t, gw, g0);
                    for (int d = 0; d < 3; ++d) g1[d] -= gw[d];
                }
            }
        }
    }
    out[0] = g0[0]; out[1] = g0[1]; out[2] = g0[2];
    out[3] = g1[0]; out[4] = -g1[1]; out[5] = -g1[2];
}

// J^T g of (s / (|s| + 1e-10) * sg, |s| * sg) at s: g4 = the gradient of those four values
__device__ __forceinline__ void enc_half_bwd(const float s[3], const float g4[4], float sg, float gs[3]) {
    const float o = norm3(s), den = o + 1e-10f;
    const float dot = g4[0] * s[0] + g4[1] * s[1] + g4[2] * s[2];
    const float go = sg * (g4[3] - dot / (den * den));           // through |s|: the fourth value and the three denominators
    for (int d = 0; d < 3; ++d) gs[d] = sg * g4[d] / den + (o > 0.f ? go * s[d] / o : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) one workgroup of 128 threads per pair.  Thread i owns row i of the assignment and with it plane i of view 1: it walks its matches in
// column order, which is sequence order, and sums in registers.  The view-2 side of every sequence position is left in LDS with its column;
// thread j then owns plane j of view 2 and sums the positions that name it in sequence order.
__global__ __launch_bounds__(128) void geo_sequence_bwd_kernel(
    const float* __restrict__ A, const float* __restrict__ planes1, const float* __restrict__ planes2, const int* __restrict__ n1p,
    const int* __restrict__ n2p, const float* __restrict__ init_trans, const float* __restrict__ init_rot, int nq, int warp_in_ref,
    const float* __restrict__ g_geo_local, const float* __restrict__ g_geo_enc, float* __restrict__ g_planes1, float* __restrict__ g_planes2) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ int cnt[129], col[TT_MAXQ];
    __shared__ float gp2[TT_MAXQ * 3];
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    const float* Ab = A + (long long)b * nq * nq;
    int c = 0;
    if (i < n1)
        for (int j = 0; j < n2; ++j) c += Ab[i * nq + j] != 0.f;
    cnt[i] = c;
    __syncthreads();
    if (i == 0) {   // exclusive prefix over <=128 rows, as geo_sequence_kernel
        int run = 0;
        for (int r = 0; r < 128; ++r) { const int t = cnt[r]; cnt[r] = run; run += t; }
        cnt[128] = run;
    }
    __syncthreads();
    const int m = min(cnt[128], nq);                             // the cut at nq pairs
    float Rm[9], q[4] = {init_rot[4 * b], init_rot[4 * b + 1], init_rot[4 * b + 2], init_rot[4 * b + 3]};
    const float t[3] = {init_trans[3 * b], init_trans[3 * b + 1], init_trans[3 * b + 2]}, z[3] = {0.f, 0.f, 0.f};
    quat_to_rot(q, Rm);
    float g1[3] = {0.f, 0.f, 0.f};
    if (i < n1) {
        int k = cnt[i];
        float p1[3];
        for (int d = 0; d < 3; ++d) p1[d] = planes1[((long long)b * nq + i) * 3 + d];
        float w1[3], wa[3];
        warp_plane(p1, Rm, t, w1);
        warp_plane(p1, Rm, z, wa);
        const float sg = (warp_in_ref && w1[0] * wa[0] < 0.f) ? -1.f : 1.f;
        for (int j = 0; j < n2 && k < nq; ++j) {
            if (Ab[i * nq + j] == 0.f) continue;
            const long long o = (long long)b * nq + k;
            float p2[3], ge[8], gs0[3], gs1[3];
            for (int d = 0; d < 3; ++d) p2[d] = planes2[((long long)b * nq + j) * 3 + d];
            for (int d = 0; d < 8; ++d) ge[d] = g_geo_enc[o * 8 + d];
            for (int d = 0; d < 3; ++d) g1[d] += g_geo_local[o * 6 + d];
            float g2[3] = {g_geo_local[o * 6 + 3], g_geo_local[o * 6 + 4], g_geo_local[o * 6 + 5]};
            if (warp_in_ref) {
                const float f2[3] = {p2[0], -p2[1], -p2[2]};
                enc_half_bwd(w1, ge, sg, gs0);
                enc_half_bwd(f2, ge + 4, 1.f, gs1);
                warp_plane_bwd_plane(p1, Rm, t, gs0, g1);
                g2[0] += gs1[0]; g2[1] -= gs1[1]; g2[2] -= gs1[2];
            } else {
                enc_half_bwd(p1, ge, 1.f, gs0);
                enc_half_bwd(p2, ge + 4, 1.f, gs1);
                for (int d = 0; d < 3; ++d) { g1[d] += gs0[d]; g2[d] += gs1[d]; }
            }
            col[k] = j;
            for (int d = 0; d < 3; ++d) gp2[3 * k + d] = g2[d];
            ++k;
        }
    }
    __syncthreads();
    if (i < nq) {
        for (int d = 0; d < 3; ++d) g_planes1[((long long)b * nq + i) * 3 + d] = g1[d];
        float a[3] = {0.f, 0.f, 0.f};
        if (i < n2)
            for (int k = 0; k < m; ++k)
                if (col[k] == i) { a[0] += gp2[3 * k]; a[1] += gp2[3 * k + 1]; a[2] += gp2[3 * k + 2]; }
        for (int d = 0; d < 3; ++d) g_planes2[((long long)b * nq + i) * 3 + d] = a[d];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) one workgroup of 256 threads per image.  cnt[q] counts how often query q is named among the first n[i] entries of match_q (integer
// LDS atomics: the result does not depend on their order); an image that breaks the contract is treated as n = 0 and flagged.
__global__ __launch_bounds__(256) void match_compact_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                            const int* __restrict__ match_q, const int* __restrict__ np, int nq, int nmax,
                                                            float* __restrict__ x_c, float* __restrict__ params_c, int* __restrict__ order,
                                                            int* __restrict__ rank, int* __restrict__ bad) {
    const int i = blockIdx.x, tid = threadIdx.x;
    __shared__ int cnt[TT_MAXQ], ord[TT_MAXQ], rk[TT_MAXQ], flag;
    if (tid < TT_MAXQ) { cnt[tid] = 0; ord[tid] = -1; }
    if (tid == 0) flag = 0;
    __syncthreads();
    int n = np[i];
    const bool n_ok = n >= 0 && n <= min(nq, nmax);
    if (!n_ok) n = 0;
    if (tid < n) {
        const int q = match_q[(long long)i * nmax + tid];
        if (q < 0 || q >= nq) atomicOr(&flag, 1);
        else if (atomicAdd(&cnt[q], 1) != 0) atomicOr(&flag, 1);
    }
    __syncthreads();
    const bool ok = n_ok && flag == 0;
    if (tid < nq) {                                              // the rank of query tid: the named queries below it (<= 127 terms)
        int below = 0;
        for (int q = 0; q < tid; ++q) below += cnt[q] != 0 ? 1 : 0;
        const bool here = ok && cnt[tid] != 0;
        rk[tid] = here ? below : -1;
        if (here) ord[below] = tid;
    }
    if (tid == 0) bad[i] = ok ? 0 : 1;
    __syncthreads();
    const int nl = ok ? n : 0;                                   // (ok: n distinct queries, all in range)
    if (tid < nq) {
        order[(long long)i * nq + tid] = ord[tid];
        rank[(long long)i * nq + tid] = rk[tid];
    }
    for (int r = 0; r < nq; ++r) {
        const long long dst = (long long)i * nq + r;
        const long long src = (long long)i * nq + (r < nl ? ord[r] : 0);
        x_c[dst * 256 + tid] = r < nl ? x[src * 256 + tid] : 0.f;
        if (tid < 3) params_c[dst * 3 + tid] = r < nl ? params[src * 3 + tid] : 0.f;
    }
}

// grid (nq, N), 256 threads: row q of image i takes row rank[i, q] of the compacted gradient, or zeros
__global__ __launch_bounds__(256) void match_compact_bwd_kernel(const float* __restrict__ g_x_c, const int* __restrict__ rank, int nq,
                                                                float* __restrict__ g_x) {
    const int q = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const int r = rank[(long long)i * nq + q];
    const bool ok = r >= 0 && r < nq;
    g_x[((long long)i * nq + q) * 256 + tid] = ok ? g_x_c[((long long)i * nq + r) * 256 + tid] : 0.f;
}

// one workgroup of 256 threads per pair: out[r, c] = gt_corr[order1[r], order2[c]] on the live block, the dustbin index maps to itself
__global__ __launch_bounds__(256) void corr_compact_kernel(const uint8_t* __restrict__ gt_corr, const int* __restrict__ order1,
                                                           const int* __restrict__ order2, const int* __restrict__ n1p,
                                                           const int* __restrict__ n2p, int nq, uint8_t* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x, S = nq + 1;
    __shared__ int o1[TT_MAXQ + 1], o2[TT_MAXQ + 1];
    const int n1 = min(max(n1p[b], 0), nq), n2 = min(max(n2p[b], 0), nq);
    if (tid <= nq) {
        int a = -1, c = -1;
        if (tid == nq) a = c = nq;
        else {
            if (tid < n1) a = order1[(long long)b * nq + tid];
            if (tid < n2) c = order2[(long long)b * nq + tid];
            if (a < 0 || a >= nq) a = -1;
            if (c < 0 || c >= nq) c = -1;
        }
        o1[tid] = a; o2[tid] = c;
    }
    __syncthreads();
    const uint8_t* src = gt_corr + (long long)b * S * S;
    uint8_t* dst = out + (long long)b * S * S;
    for (int e = tid; e < S * S; e += 256) {
        const int a = o1[e / S], c = o2[e % S];
        dst[e] = (a >= 0 && c >= 0) ? src[a * S + c] : (uint8_t)0;
    }
}

}  // namespace nps

extern "C" int nopesac_refine_score_maps_backward_geo(const float* geo_local, const float* rot_raw, const float* trans_raw, const float* init_rot,
                                                      const float* init_trans, const int32_t* m, int B, int nq, const float* g_normal_score,
                                                      const float* g_param_score, const float* g_l2_dist, float* g_geo_local, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(geo_local && rot_raw && trans_raw && init_rot && init_trans && m && g_normal_score && g_param_score && g_l2_dist,
                  "refine_score_maps_backward_geo: null input");
    NPS_CHECK_ARG(g_geo_local, "refine_score_maps_backward_geo: null output");
    NPS_CHECK_ARG(B > 0 && B <= 65535 && nq > 0 && nq <= TT_MAXQ, "refine_score_maps_backward_geo: bad dims (B=%d, nq=%d; nq<=128)", B, nq);
    hipLaunchKernelGGL(refine_score_maps_bwd_geo_kernel, dim3((nq + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, geo_local, rot_raw, trans_raw,
                       init_rot, init_trans, m, nq, g_normal_score, g_param_score, g_l2_dist, g_geo_local);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_geo_sequence_backward(const float* assignment, const float* planes1, const float* planes2, const int32_t* n1,
                                             const int32_t* n2, const float* init_trans, const float* init_rot, int B, int nq, int warp_in_ref,
                                             const float* g_geo_local, const float* g_geo_enc, float* g_planes1, float* g_planes2, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(assignment && planes1 && planes2 && n1 && n2 && init_trans && init_rot && g_geo_local && g_geo_enc,
                  "geo_sequence_backward: null input");
    NPS_CHECK_ARG(g_planes1 && g_planes2, "geo_sequence_backward: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= TT_MAXQ, "geo_sequence_backward: bad dims (B=%d, nq=%d; nq<=128)", B, nq);
    hipLaunchKernelGGL(geo_sequence_bwd_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, assignment, planes1, planes2, n1, n2, init_trans,
                       init_rot, nq, warp_in_ref, g_geo_local, g_geo_enc, g_planes1, g_planes2);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_match_compact(const float* x, const float* params, const int32_t* match_q, const int32_t* n, int N, int nq, int nmax,
                                     float* x_c, float* params_c, int32_t* order, int32_t* rank, int32_t* bad, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(x && params && match_q && n, "match_compact: null input");
    NPS_CHECK_ARG(x_c && params_c && order && rank && bad, "match_compact: null output");
    NPS_CHECK_ARG(N > 0 && nq > 0 && nq <= TT_MAXQ, "match_compact: bad dims (N=%d, nq=%d; nq<=128)", N, nq);
    NPS_CHECK_ARG(nmax >= 1 && nmax <= TT_MAXQ, "match_compact: nmax=%d outside 1..%d", nmax, TT_MAXQ);
    hipLaunchKernelGGL(match_compact_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, x, params, match_q, n, nq, nmax, x_c, params_c, order,
                       rank, bad);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_match_compact_backward(const float* g_x_c, const int32_t* rank, int N, int nq, float* g_x, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(g_x_c && rank, "match_compact_backward: null input");
    NPS_CHECK_ARG(g_x, "match_compact_backward: null output");
    NPS_CHECK_ARG(N > 0 && N <= 65535 && nq > 0 && nq <= TT_MAXQ, "match_compact_backward: bad dims (N=%d, nq=%d; nq<=128)", N, nq);
    hipLaunchKernelGGL(match_compact_bwd_kernel, dim3(nq, N), dim3(256), 0, (hipStream_t)stream, g_x_c, rank, nq, g_x);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_corr_compact(const uint8_t* gt_corr, const int32_t* order1, const int32_t* order2, const int32_t* n1, const int32_t* n2,
                                    int B, int nq, uint8_t* out, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(gt_corr && order1 && order2 && n1 && n2, "corr_compact: null input");
    NPS_CHECK_ARG(out, "corr_compact: null output");
    NPS_CHECK_ARG(B > 0 && nq > 0 && nq <= TT_MAXQ, "corr_compact: bad dims (B=%d, nq=%d; nq<=128)", B, nq);
    hipLaunchKernelGGL(corr_compact_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, gt_corr, order1, order2, n1, n2, nq, out);
    NPS_LAUNCH_RET();
}
