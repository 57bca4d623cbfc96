// Two-view reconstruction AP on the device (the reference's offline eval.py --evaluate AP: evaluate_ap_by_idx :343-619,
// get_maskiou_merged / get_single2merge :657-779, evaluate_by_idx / inst_bench_image :830-913, and get_plane_params_in_global,
// utils/mesh_utils.py:89-105).  Per pair of views: both views' planes in one frame through the camera, the planes a correspondence
// pairs merged into one entry, the three error matrices [predicted entries, GT entries], the five overlap criteria and the walk that
// turns them into true positives.  What is left for the host is the AP over all pairs (evaluation.recon_table).  The global plane,
// the merged normal and the match tables are two_view.h's, shared with recon_mesh.hip.
//
// Ragged quantities use exclusive-offset arrays (int64 [n + 1]) as in plane_eval.hip; pair i owns views 2 i and 2 i + 1 of the view
// arrays.  Everything is float64 (the reference is float64 numpy), deterministic, without atomics, each output written once.
#include "two_view.h"

namespace nps {

constexpr int RE_MAXG = 255;                       // GT planes of one view
constexpr int RE_MAXPE = 2 * TV_MAXN;              // predicted entries of a pair (no correspondence at all)
constexpr int RE_MAXGE = 2 * RE_MAXG;              // GT entries of a pair
constexpr int RE_CRIT = 5;                         // all, -offset, -normal, -mask, -normal-offset
constexpr int RE_T = 64 * RE_CRIT;                 // one wave per criterion in the walk

// Entry tables of one side (predictions or GT) by one wave: the planes of view 0 no correspondence names, in index order, then those
// of view 1, then one entry per correspondence in the order given.  match[v][k] >= 0: plane k of view v is in a correspondence.
// ent[v][e]: entry e's plane in view v, or -1.
template <int MAXV>
__device__ __forceinline__ void re_entries(int lane, int n0, int n1, int nc, const int* __restrict__ corr, const int (*match)[MAXV],
                                           short (*ent)[2 * MAXV]) {
    int base = 0;
    for (int e0 = 0; e0 < n0 + n1; e0 += 64) {
        const int e = e0 + lane, v = e >= n0 ? 1 : 0, k = e - (v ? n0 : 0);
        const bool single = e < n0 + n1 && match[v][k < MAXV ? k : 0] < 0;
        const unsigned long long m = __ballot(single);
        if (single) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            ent[v][pos] = (short)k;
            ent[1 - v][pos] = (short)-1;
        }
        base += __popcll(m);
    }
    for (int c = lane; c < nc; c += 64) {
        ent[0][base + c] = (short)corr[2 * c];
        ent[1][base + c] = (short)corr[2 * c + 1];
    }
}

// One workgroup per pair, five waves.
//  1. the correspondence lists become per-plane match tables in LDS (tv_match_mark / _verify); a `bad` pair writes nothing but the flag.
//  2. wave 0 lays out the predicted entries, wave 1 the GT entries (ballot prefix count over the unmatched planes).
//  3. every thread takes entries: global planes through the camera, the merged plane of a correspondence (offset mean, score max,
//     tv_merged_normal, whose sign |dot| ignores).
//  4. a wave takes a predicted entry, its lanes the GT entries, 64 at a time: the three errors once, the five overlap flags, and
//     per criterion a ballot whose lowest set bit is the first flagged GT entry of this chunk.
//  5. the walk (inst_bench_image with a 0 / 1 overlap) visits the entries in entry order; each claims the FIRST flagged GT entry
//     and is a true positive iff that entry is still free - it never moves on to a later flagged one.  Only entries whose first
//     flagged GT entry is g ever claim g, and the first of them finds it free, so: true positive iff no earlier entry has the
//     same first flagged GT entry.  That needs no carried taken-mask; wave k settles criterion k, a lane per entry.
__global__ __launch_bounds__(RE_T) void recon_ap_assign_kernel(const double* __restrict__ iou, const long long* __restrict__ iou_off,
                                                               const long long* __restrict__ dt_off, const long long* __restrict__ gt_off,
                                                               const float* __restrict__ score, const float* __restrict__ pred_plane,
                                                               const float* __restrict__ gt_plane, const double* __restrict__ pred_cam,
                                                               const double* __restrict__ gt_cam, const int* __restrict__ pred_corr,
                                                               const long long* __restrict__ pred_corr_off, const int* __restrict__ gt_corr,
                                                               const long long* __restrict__ gt_corr_off, long long n_rows,
                                                               double* __restrict__ rows, int* __restrict__ n_gt_entries, int* __restrict__ bad,
                                                               double* __restrict__ errs, const long long* __restrict__ err_off) {
    __shared__ int s_pm[2][TV_MAXN], s_gm[2][RE_MAXG];
    __shared__ short s_pe[2][RE_MAXPE], s_ge[2][RE_MAXGE];
    __shared__ double s_po[RE_MAXPE], s_pn[RE_MAXPE][3], s_go[RE_MAXGE], s_gn[RE_MAXGE][3];
    __shared__ int s_first[RE_CRIT][RE_MAXPE];
    __shared__ int s_bad;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long d0 = dt_off[2 * i], d1 = dt_off[2 * i + 1], g0 = gt_off[2 * i], g1 = gt_off[2 * i + 1];
    const long long n0l = d1 - d0, n1l = dt_off[2 * i + 2] - d1, m0l = g1 - g0, m1l = gt_off[2 * i + 2] - g1;
    const long long pc0 = pred_corr_off[i], npcl = pred_corr_off[i + 1] - pc0, gc0 = gt_corr_off[i], ngcl = gt_corr_off[i + 1] - gc0;
    const long long row0 = d0 - pc0;                                            // entries before this pair = planes - correspondences
    const bool fits = n0l >= 0 && n0l <= TV_MAXN && n1l >= 0 && n1l <= TV_MAXN && m0l >= 0 && m0l <= RE_MAXG && m1l >= 0 && m1l <= RE_MAXG &&
                      npcl >= 0 && npcl <= (n0l < n1l ? n0l : n1l) && ngcl >= 0 && ngcl <= (m0l < m1l ? m0l : m1l) && row0 >= 0 &&
                      row0 + n0l + n1l - npcl <= n_rows;
    if (!fits) {                                                                // (uniform: before any barrier)
        if (tid == 0) { bad[i] = 1; n_gt_entries[i] = 0; }
        return;
    }
    const int n0 = (int)n0l, n1 = (int)n1l, m0 = (int)m0l, m1 = (int)m1l, npc = (int)npcl, ngc = (int)ngcl;
    const int npe = n0 + n1 - npc, nge = m0 + m1 - ngc;
    const int* pc = pred_corr + 2 * pc0;
    const int* gc = gt_corr + 2 * gc0;
    // ---- 1. match tables
    for (int k = tid; k < 2 * TV_MAXN; k += RE_T) (&s_pm[0][0])[k] = -1;
    for (int k = tid; k < 2 * RE_MAXG; k += RE_T) (&s_gm[0][0])[k] = -1;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    tv_match_mark<TV_MAXN>(tid, RE_T, pc, npc, n0, n1, s_pm, s_bad);
    tv_match_mark<RE_MAXG>(tid, RE_T, gc, ngc, m0, m1, s_gm, s_bad);
    __syncthreads();
    tv_match_verify<TV_MAXN>(tid, RE_T, pc, npc, n0, n1, s_pm, s_bad);
    tv_match_verify<RE_MAXG>(tid, RE_T, gc, ngc, m0, m1, s_gm, s_bad);
    __syncthreads();
    if (s_bad) {                                                                // (uniform)
        if (tid == 0) { bad[i] = 1; n_gt_entries[i] = 0; }
        return;
    }
    // ---- 2. entry tables
    if (wave == 0) re_entries<TV_MAXN>(lane, n0, n1, npc, pc, s_pm, s_pe);
    if (wave == 1) re_entries<RE_MAXG>(lane, m0, m1, ngc, gc, s_gm, s_ge);
    __syncthreads();
    // ---- 3. the entries' planes
    const double* pcam = pred_cam + 7 * (long long)i;
    const double* gcam = gt_cam + 7 * (long long)i;
    for (int e = tid; e < npe + nge; e += RE_T) {
        const bool is_gt = e >= npe;
        const int r = is_gt ? e - npe : e;
        const int k0 = is_gt ? s_ge[0][r] : s_pe[0][r], k1 = is_gt ? s_ge[1][r] : s_pe[1][r];
        const float* planes = is_gt ? gt_plane : pred_plane;
        const long long b0 = is_gt ? g0 : d0, b1 = is_gt ? g1 : d1;
        const double* cam = is_gt ? gcam : pcam;
        double g[3], off = 0.0, n[3] = {0.0, 0.0, 0.0};
        if (k0 >= 0) tv_global_plane(planes + 3 * (b0 + k0), cam, false, g, off, n);
        if (k1 >= 0 && (k0 < 0 || !is_gt)) {                                     // a merged GT entry keeps view 0's plane
            double o1, n1v[3];
            tv_global_plane(planes + 3 * (b1 + k1), cam, true, g, o1, n1v);
            if (k0 < 0) {
                off = o1; n[0] = n1v[0]; n[1] = n1v[1]; n[2] = n1v[2];
            } else {
                tv_merged_normal(n, n1v, n);
                off = (off + o1) / 2.0;
            }
        }
        if (is_gt) {
            s_go[r] = off; s_gn[r][0] = n[0]; s_gn[r][1] = n[1]; s_gn[r][2] = n[2];
        } else {
            s_po[r] = off; s_pn[r][0] = n[0]; s_pn[r][1] = n[1]; s_pn[r][2] = n[2];
            float sc = k0 >= 0 ? score[d0 + k0] : score[d1 + k1];
            if (k0 >= 0 && k1 >= 0) { const float s1 = score[d1 + k1]; sc = s1 > sc ? s1 : sc; }
            double* row = rows + (row0 + r) * (long long)NPS_RECON_AP_COLS;
            row[0] = (double)sc; row[1 + RE_CRIT] = (double)k0; row[2 + RE_CRIT] = (double)k1;
        }
    }
    __syncthreads();
    // ---- 4. first flagged GT entry per (criterion, predicted entry)
    const double thr_iou[RE_CRIT] = {0.5, 0.5, 0.5, 0.0, 0.5};
    const double thr_nrm[RE_CRIT] = {30.0, 30.0, 1000.0, 30.0, 1000.0};
    const double thr_off[RE_CRIT] = {1.0, 1000.0, 1.0, 1.0, 1000.0};
    const bool blk0 = n0 > 0 && m0 > 0, blk1 = n1 > 0 && m1 > 0;               // an empty IoU block has no address of its own:
    const double* iou0 = blk0 ? iou + iou_off[2 * i] : pcam;                      // read the camera instead and drop the value
    const double* iou1 = blk1 ? iou + iou_off[2 * i + 1] : pcam;
    double* err = errs ? errs + err_off[i] : nullptr;
    for (int r = wave; r < npe; r += RE_CRIT) {
        const int p0 = s_pe[0][r], p1 = s_pe[1][r];
        const double po = s_po[r], px = s_pn[r][0], py = s_pn[r][1], pz = s_pn[r][2];
        int first[RE_CRIT];
#pragma unroll
        for (int k = 0; k < RE_CRIT; ++k) first[k] = -1;
        for (int c0 = 0; c0 < nge; c0 += 64) {
            const bool in = c0 + lane < nge;
            const int c = in ? c0 + lane : 0;
            const int q0 = s_ge[0][c], q1 = s_ge[1][c];
            const bool has0 = blk0 && p0 >= 0 && q0 >= 0, has1 = blk1 && p1 >= 0 && q1 >= 0;
            const double x0 = iou0[has0 ? (long long)p0 * m0 + q0 : 0], x1 = iou1[has1 ? (long long)p1 * m1 + q1 : 0];   // always-valid address,
            const double a0 = has0 ? x0 : 0.0, a1 = has1 ? x1 : 0.0;                                                       // select afterwards
            const double miou = (p0 >= 0 && p1 >= 0 && q0 >= 0 && q1 >= 0) ? (a0 + a1) / 2.0 : a0 + a1;
            const double oerr = fabs(po - s_go[c]);
            double d = fabs(px * s_gn[c][0] + py * s_gn[c][1] + pz * s_gn[c][2]);
            d = d > 1.0 ? 1.0 : d;
            const double nerr = acos(d) / 3.14159265358979323846 * 180.0;
            if (err && in) {
                const long long o = (long long)r * nge + c, plane = (long long)npe * nge;
                err[o] = oerr; err[plane + o] = nerr; err[2 * plane + o] = miou;
            }
#pragma unroll
            for (int k = 0; k < RE_CRIT; ++k) {
                const unsigned long long m = __ballot(in && miou >= thr_iou[k] && nerr <= thr_nrm[k] && oerr <= thr_off[k]);
                if (first[k] < 0 && m) first[k] = c0 + __ffsll((long long)m) - 1;
            }
        }
        if (lane < RE_CRIT) {
            int f = -1;
#pragma unroll
            for (int k = 0; k < RE_CRIT; ++k) f = lane == k ? first[k] : f;
            s_first[lane][r] = f;
        }
    }
    __syncthreads();
    // ---- 5. the walk, criterion `wave`
    for (int r = lane; r < npe; r += 64) {
        const int g = s_first[wave][r];
        int tp = g >= 0 ? 1 : 0;
        for (int q = 0; q < r; ++q) tp = s_first[wave][q] == g ? 0 : tp;
        rows[(row0 + r) * (long long)NPS_RECON_AP_COLS + 1 + wave] = (double)tp;
    }
    if (tid == 0) { bad[i] = 0; n_gt_entries[i] = nge; }
}

}  // namespace nps

extern "C" nps_status nopesac_recon_ap_assign(const double* iou, const int64_t* iou_off, const int64_t* dt_off, const int64_t* gt_off,
                                              const float* score, const float* pred_plane, const float* gt_plane, const double* pred_cam,
                                              const double* gt_cam, const int32_t* pred_corr, const int64_t* pred_corr_off,
                                              const int32_t* gt_corr, const int64_t* gt_corr_off, int P, int max_dt, int max_gt, int64_t n_rows,
                                              double* rows, int32_t* n_gt_entries, int32_t* bad, double* errs, const int64_t* err_off,
                                              void* stream) {
    using namespace nps;
    static_assert(NPS_RECON_AP_COLS == 3 + RE_CRIT, "score, one flag per criterion, the entry's two plane indices");
    NPS_CHECK_ARG(P >= 0 && n_rows >= 0, "recon_ap_assign: P < 0 or n_rows < 0");
    NPS_CHECK_ARG(max_dt >= 0 && max_dt <= TV_MAXN && max_gt >= 0 && max_gt <= RE_MAXG,
                  "recon_ap_assign: at most %d predictions and %d GT planes per view (got %d, %d)", TV_MAXN, RE_MAXG, max_dt, max_gt);
    if (P == 0) return 0;
    NPS_CHECK_ARG(iou_off && dt_off && gt_off && pred_cam && gt_cam && pred_corr_off && gt_corr_off && n_gt_entries && bad,
                  "recon_ap_assign: null pointer");
    NPS_CHECK_ARG(max_dt == 0 || (score && pred_plane && rows), "recon_ap_assign: null pointer (predictions)");
    NPS_CHECK_ARG(max_gt == 0 || gt_plane, "recon_ap_assign: null pointer (GT)");
    NPS_CHECK_ARG(max_dt == 0 || max_gt == 0 || iou, "recon_ap_assign: null pointer (iou)");
    NPS_CHECK_ARG(!errs || err_off, "recon_ap_assign: errs without err_off");
    hipLaunchKernelGGL(recon_ap_assign_kernel, dim3(P), dim3(RE_T), 0, (hipStream_t)stream, iou, (const long long*)iou_off,
                       (const long long*)dt_off, (const long long*)gt_off, score, pred_plane, gt_plane, pred_cam, gt_cam, pred_corr,
                       (const long long*)pred_corr_off, gt_corr, (const long long*)gt_corr_off, (long long)n_rows, rows, n_gt_entries, bad,
                       errs, (const long long*)err_off);
    NPS_LAUNCH_RET();
}
