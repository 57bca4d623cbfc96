// Set criterion of the plane head (reference: modeling/matcher.py HungarianMatcher, modeling/criterion.py SetCriterion, as
// siamese_planeTR.py forward_single calls them; prepare_targets :498-504; process_plane_corr_matrix :566-623) for
// nopesac_amd/training.py::PlaneCriterion.  An "image" is one (supervised decoder layer, batch element): i = layer * B + b, layer 0 = the
// last decoder layer, layers 1.. = the auxiliary ones; targets are read at b = i % B, so all layers share every launch.
//   (1) targets: per-plane centroids of (x / W, y / H) and the per-pixel centre map;
//   (2) matching costs: one sigmoid / softplus per (query, low-resolution pixel) kept in LDS for 64 pixels at a time and accumulated against
//       the target masks (nearest-downsampled, one 64-bit word of plane bits per pixel) - the [nq, hw] focal tensor never exists in HBM;
//   (3) assignment: shortest augmenting paths over the transposed problem (rows = targets, columns = queries on the lanes of one wave),
//       duals in f64, no host round trip;
//   (4) losses: class NLL, bilinear-upsampled focal + dice per matched mask (a band of low-resolution rows staged in LDS, per-(mask, band)
//       partials, a finishing pass), instance / pixel centres, parameter L1 / cosine, the Q loss;
//   (5) their gradients; the low-resolution mask / centre-map gradient is a gather over each pixel's high-resolution dependants with the
//       transposed bilinear weights (clamped border taps fold onto the border pixel).
// Everything is f32 and deterministic: no atomics, every reduction runs in a fixed order (wave shuffles, LDS partials by index, workspace
// partials summed by index).  Border taps load from a clamped address and select.  Gated against the float64 restatement
// tests/plane_criterion_ref.py (tests/test_plane_criterion_gpu.py).
#include "common.h"

namespace nps {

constexpr int PC_MAXQ = NPS_PLANE_MAX_QUERIES;
constexpr int PC_MAXT = NPS_PLANE_MAX_TARGETS;
constexpr int PC_MAXL = NPS_PLANE_MAX_LAYERS;
constexpr int PC_MAXG = NPS_PLANE_MAX_GROUPS;
constexpr int PC_COST_BLOCKS = 16;     // workgroups per image of the cost partials (each walks 64-pixel chunks blk, blk + 16, ...)
constexpr int PC_CHUNK = 64;           // low-resolution pixels per chunk: one per lane
constexpr int PC_LS = PC_CHUNK + 1;    // LDS row stride of the chunk tiles
constexpr int PC_BAND = 8;             // low-resolution rows per workgroup of the mask / centre-map kernels
constexpr int PC_QCHUNKS = 16;         // workgroups per image of the Q loss
constexpr int PC_PAIRS = (PC_MAXQ + 1) * PC_MAXT / 256 + 1;   // (query | count row, target) pairs per thread of the cost kernel
constexpr float PC_ALPHA = 0.25f;

static inline int pc_bands(int h) { return (h + PC_BAND - 1) / PC_BAND; }
static inline int pc_cost_blocks(int h, int w) { const int c = (h * w + PC_CHUNK - 1) / PC_CHUNK; return c < PC_COST_BLOCKS ? c : PC_COST_BLOCKS; }
// workspace layout (floats): every kernel takes the offsets from these
static inline int64_t pc_ws_cost(int L, int B, int nq, int nmax) { return (int64_t)L * B * PC_COST_BLOCKS * ((int64_t)(nq + 1) * nmax * 2 + 2 * (nq + 1)); }
static inline int64_t pc_ws_mask(int L, int B, int nmax, int h) { return (int64_t)L * B * nmax * pc_bands(h) * 4; }
static inline int64_t pc_ws_loss(int L, int B, int nmax, int h) {
    return pc_ws_mask(L, B, nmax, h) + (int64_t)B * pc_bands(h) + (int64_t)B * PC_QCHUNKS * 2 + (int64_t)L * B * 8 + (int64_t)B * nmax * PC_QCHUNKS * 3;
}

template <typename T> __device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over a workgroup of NW waves, the same value in every thread; `red` holds NW floats
template <int NW> __device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) t += red[k];
    __syncthreads();
    return t;
}
__device__ __forceinline__ int pc_n(const int* n, int b, int nmax) { return min(max(n[b], 0), nmax); }
// View groups: group g is the images [g Bg, (g + 1) Bg) of every layer's block, Bg = B / G.  Every batch-wide reduction of the loss and
// gradient kernels runs over one group, in the order a call on those images alone would take, so a group keeps that call's bits.
struct PcGroups { int G; float nm[PC_MAXG]; };   // nm[g]: the group's num_masks override (<= 0: max(sum of its n, 1))
__device__ __forceinline__ float pc_num_masks(const int* n, int b0, int Bg, int nmax, float override_) {
    if (override_ > 0.f) return override_;
    int t = 0;
    for (int b = b0; b < b0 + Bg; ++b) t += pc_n(n, b, nmax);
    return (float)max(t, 1);
}
// sigmoid and the two softplus values of one logit: sp0 = BCE against 0, sp1 = BCE against 1
__device__ __forceinline__ void pc_sig(float v, float& p, float& sp0, float& sp1) {
    const float e = expf(-fabsf(v)), l = log1pf(e);
    p = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    sp0 = fmaxf(v, 0.f) + l;
    sp1 = fmaxf(-v, 0.f) + l;
}
// source coordinate of F.interpolate(mode="bilinear", align_corners=False): taps i0, i1 (clamped) and the weight of i1
__device__ __forceinline__ void pc_taps(int dst, float inv_s, int size, int& i0, int& i1, float& l1) {
    const float src = fmaxf(((float)dst + 0.5f) * inv_s - 0.5f, 0.f);
    i0 = min((int)src, size - 1);
    i1 = min(i0 + 1, size - 1);
    l1 = src - (float)i0;
}
// weight with which low-resolution index `lo` enters high-resolution index `dst` (both taps may fall on `lo` at the border)
__device__ __forceinline__ float pc_tap_weight(int dst, int lo, float inv_s, int size) {
    int i0, i1;
    float l1;
    pc_taps(dst, inv_s, size, i0, i1, l1);
    return (i0 == lo ? 1.f - l1 : 0.f) + (i1 == lo ? l1 : 0.f);
}
// high-resolution indices that can depend on low-resolution index lo: [first, last]
__device__ __forceinline__ void pc_dependants(int lo, int s, int size_hi, int& first, int& last) {
    const int a = 2 * s * lo - s - 1;                       // 2 * (s (lo - 1/2) - 1/2)
    first = max((a >= 0 ? a / 2 : -((-a + 1) / 2)) + 1, 0);
    last = min((2 * s * lo + 3 * s - 1 + 1) / 2 - 1, size_hi - 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) targets
__global__ __launch_bounds__(256) void pc_plane_centers_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ n, int nmax, int H, int W,
                                                               float* __restrict__ centers) {
    __shared__ double red[3][4];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* out = centers + ((long long)b * nmax + j) * 2;
    if (j >= pc_n(n, b, nmax)) {
        if (tid < 2) out[tid] = 0.f;
        return;
    }
    const uint8_t* m = masks + ((long long)b * nmax + j) * H * W;
    double sx = 0, sy = 0, c = 0;                                   // sums of integers: exact
    for (int e = tid; e < H * W; e += 256) {
        const bool on = m[e] != 0;
        sx += on ? (double)(e % W) : 0.0;
        sy += on ? (double)(e / W) : 0.0;
        c += on ? 1.0 : 0.0;
    }
    sx = wave_sum_t(sx); sy = wave_sum_t(sy); c = wave_sum_t(c);
    if ((tid & 63) == 0) { red[0][tid >> 6] = sx; red[1][tid >> 6] = sy; red[2][tid >> 6] = c; }
    __syncthreads();
    if (tid == 0) {
        const double tx = red[0][0] + red[0][1] + red[0][2] + red[0][3], ty = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double tc = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        out[0] = (float)(tx / (double)W / tc);                      // an empty mask gives NaN, as the reference's 0 / 0 does
        out[1] = (float)(ty / (double)H / tc);
    }
}

__global__ __launch_bounds__(256) void pc_pixel_centers_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ n, int nmax, int HW,
                                                               const float* __restrict__ centers, float* __restrict__ pixel_centers) {
    __shared__ float cs[PC_MAXT * 2];
    const int b = blockIdx.y, nb = pc_n(n, b, nmax);
    if (threadIdx.x < nb * 2) cs[threadIdx.x] = centers[(long long)b * nmax * 2 + threadIdx.x];
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    float ax = 0.f, ay = 0.f;
    for (int j = 0; j < nb; ++j) {
        const bool on = masks[((long long)b * nmax + j) * HW + e] != 0;
        ax += on ? cs[2 * j] : 0.f;
        ay += on ? cs[2 * j + 1] : 0.f;
    }
    pixel_centers[((long long)b * 2) * HW + e] = ax;
    pixel_centers[((long long)b * 2 + 1) * HW + e] = ay;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) matching costs.  Partials: workgroup (blk, i) walks the 64-pixel chunks blk, blk + nblk, ... of image i.  Per chunk, wave v computes
// sigmoid / softplus of the queries v, v + 4, ... (lane = pixel) into two LDS tiles D = focal_pos - focal_neg and S = sigmoid, plus one row of
// ones (S row nq) that counts target pixels; the per-query sums of focal_neg and sigmoid go through a wave reduction.  Then thread t owns
// the (row, target) pairs t, t + 256, ... and adds the tile entries whose pixel carries the target's bit.
__global__ __launch_bounds__(256) void pc_cost_partial_kernel(const float* __restrict__ mlog, long long s_i, long long s_q, long long s_y,
                                                              long long s_x, const uint8_t* __restrict__ masks, const int* __restrict__ n, int B,
                                                              int nq, int nmax, int h, int w, int H, int W, int s, int nblk,
                                                              float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int i = blockIdx.y, b = i % B, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nb = pc_n(n, b, nmax), rows = nq + 1, hw = h * w, nchunks = (hw + PC_CHUNK - 1) / PC_CHUNK, total = rows * nmax;
    float* D = smem;                                  // [rows][65]
    float* S = D + rows * PC_LS;                      // [rows][65]
    float* Fn = S + rows * PC_LS;                     // [rows] sum of focal_neg
    float* Sg = Fn + rows;                            // [rows] sum of sigmoid
    unsigned long long* tb = (unsigned long long*)(Sg + rows);      // [64] target bits of the chunk's pixels (132 rows floats: 8-byte aligned)
    float accA[PC_PAIRS], accB[PC_PAIRS];
#pragma unroll
    for (int k = 0; k < PC_PAIRS; ++k) accA[k] = accB[k] = 0.f;
    for (int q = tid; q < rows; q += 256) Fn[q] = Sg[q] = 0.f;
    __syncthreads();
    for (int c = blk; c < nchunks; c += nblk) {
        const int pix = c * PC_CHUNK + lane;
        const bool ok = pix < hw;
        const int pc = ok ? pix : 0, y = pc / w, x = pc % w;
        if (wv == 3) {                                                              // nearest: sample (s y, s x)
            unsigned long long bits = 0ull;
            const uint8_t* m = masks + (long long)b * nmax * H * W + (long long)(s * y) * W + s * x;
            for (int j = 0; j < nb; ++j) bits |= (m[(long long)j * H * W] != 0 ? 1ull : 0ull) << j;
            tb[lane] = ok ? bits : 0ull;
            D[nq * PC_LS + lane] = 0.f;
            S[nq * PC_LS + lane] = ok ? 1.f : 0.f;
        }
        const float* src = mlog + (long long)i * s_i + y * s_y + x * s_x;
        for (int q = wv; q < nq; q += 4) {
            float p, sp0, sp1;
            pc_sig(src[q * s_q], p, sp0, sp1);
            const float fp = PC_ALPHA * ((1.f - p) * (1.f - p)) * sp1, fn = (1.f - PC_ALPHA) * (p * p) * sp0;
            D[q * PC_LS + lane] = ok ? fp - fn : 0.f;
            S[q * PC_LS + lane] = ok ? p : 0.f;
            const float sfn = wave_sum(ok ? fn : 0.f), ssg = wave_sum(ok ? p : 0.f);
            if (lane == 0) { Fn[q] += sfn; Sg[q] += ssg; }                           // query q always belongs to this wave
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PC_PAIRS; ++k) {
            const int pr = tid + 256 * k;
            if (pr < total) {
                const int q = pr / nmax, j = pr % nmax;
                if (j < nb) {
                    float a = 0.f, bq = 0.f;
                    for (int px = 0; px < PC_CHUNK; ++px) {
                        const bool on = (tb[px] >> j) & 1ull;
                        a += on ? D[q * PC_LS + px] : 0.f;
                        bq += on ? S[q * PC_LS + px] : 0.f;
                    }
                    accA[k] += a;
                    accB[k] += bq;
                }
            }
        }
        __syncthreads();
    }
    float* out = ws + ((long long)i * PC_COST_BLOCKS + blk) * ((long long)total * 2 + 2 * rows);
#pragma unroll
    for (int k = 0; k < PC_PAIRS; ++k) {
        const int pr = tid + 256 * k;
        if (pr < total) { out[pr] = accA[k]; out[total + pr] = accB[k]; }
    }
    for (int q = tid; q < rows; q += 256) { out[2 * total + q] = Fn[q]; out[2 * total + rows + q] = Sg[q]; }
}

struct PcCostW { float cls, mask, dice, center, param, offset, angle; };

__global__ __launch_bounds__(256) void pc_cost_finish_kernel(const float* __restrict__ ws, int nblk, const float* __restrict__ logits,
                                                             const float* __restrict__ centers, const float* __restrict__ params,
                                                             const float* __restrict__ tcenters, const float* __restrict__ tparams,
                                                             const int* __restrict__ n, int B, int nq, int nmax, int hw, PcCostW cw,
                                                             float* __restrict__ C) {
    const int i = blockIdx.y, b = i % B, nb = pc_n(n, b, nmax), rows = nq + 1, total = rows * nmax;
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= nq * nmax) return;
    const int q = pr / nmax, j = pr % nmax;
    float* out = C + ((long long)i * nq + q) * nmax + j;
    if (j >= nb) { *out = 0.f; return; }
    const long long per = (long long)total * 2 + 2 * rows;
    const float* base = ws + (long long)i * PC_COST_BLOCKS * per;
    float A = 0.f, Bq = 0.f, fn = 0.f, sg = 0.f, tj = 0.f;
    for (int k = 0; k < nblk; ++k) {
        const float* p = base + k * per;
        A += p[pr]; Bq += p[total + pr]; fn += p[2 * total + q]; sg += p[2 * total + rows + q]; tj += p[total + nq * nmax + j];
    }
    const float focal = (fn + A) / (float)hw;
    const float dice = 1.f - (2.f * Bq + 1.f) / (sg + tj + 1.f);
    const float* z = logits + ((long long)i * nq + q) * 2;
    const float zm = fmaxf(z[0], z[1]), e0 = expf(z[0] - zm), e1 = expf(z[1] - zm);
    const float cls = -(e0 / (e0 + e1));
    const float* c = centers + ((long long)i * nq + q) * 2;
    const float* tc = tcenters + ((long long)b * nmax + j) * 2;
    const float dx = c[0] - tc[0], dy = c[1] - tc[1], cen = sqrtf(dx * dx + dy * dy);
    const float* p = params + ((long long)i * nq + q) * 3;
    const float* t = tparams + ((long long)b * nmax + j) * 3;
    const float l1 = fabsf(p[0] - t[0]) + fabsf(p[1] - t[1]) + fabsf(p[2] - t[2]);
    const float np_ = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    const float dp = fmaxf(np_, 1e-12f), dt = fmaxf(nt, 1e-12f);
    float cosv = (p[0] / dp) * (t[0] / dt) + (p[1] / dp) * (t[1] / dt) + (p[2] / dp) * (t[2] / dt);
    cosv = fminf(fmaxf(cosv, -0.999999f), 0.999999f);
    const float angle = acosf(cosv) * (float)(180.0 / 3.14159265358979323846);
    const float off = fabsf(np_ - nt);
    *out = cw.mask * focal + cw.cls * cls + cw.dice * dice + cw.center * cen + cw.param * l1 + cw.offset * off + cw.angle * angle;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) assignment: one wave per image.  Rows = targets, columns = queries (lane, lane + 64).  The shortest augmenting path method with dual
// variables (Crouse 2016, the method scipy.optimize.linear_sum_assignment implements): per row, grow the alternating tree from the row by the
// column of least reduced path cost until a free column is reached, update the duals, flip the path.  Duals and path costs are f64.
__global__ __launch_bounds__(64) void pc_assign_kernel(const float* __restrict__ C, const int* __restrict__ n, int B, int nq, int nmax,
                                                       int* __restrict__ match_q, int* __restrict__ match_gt) {
    __shared__ float cs[PC_MAXT * PC_MAXQ];
    __shared__ double u[PC_MAXT];
    __shared__ int col4row[PC_MAXT];
    const int i = blockIdx.x, b = i % B, lane = threadIdx.x, nr = min(pc_n(n, b, nmax), nq);
    const double INF = 1e300;
    for (int e = lane; e < nr * nq; e += 64) {
        const int j = e / nq, q = e % nq;
        cs[e] = C[((long long)i * nq + q) * nmax + j];
    }
    for (int j = lane; j < PC_MAXT; j += 64) { u[j] = 0.0; col4row[j] = -1; }
    double v[2] = {0.0, 0.0};
    int r4c[2] = {-1, -1};
    __syncthreads();
    bool failed = false;
    for (int cur = 0; cur < nr && !failed; ++cur) {
        double spc[2] = {INF, INF};
        int path[2] = {-1, -1};
        bool sc[2] = {false, false};
        double minVal = 0.0;
        int ii = cur, sink = -1;
        for (int step = 0; step <= nq && sink < 0; ++step) {
            const double ui = u[ii];
            double best = INF;
            int bidx = -1, bun = 0;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = lane + 64 * c;
                if (col < nq && !sc[c]) {
                    const double r = minVal + (double)cs[ii * nq + col] - ui - v[c];
                    if (r < spc[c]) { spc[c] = r; path[c] = ii; }
                    const int un = r4c[c] < 0 ? 1 : 0;
                    if (bidx < 0 || spc[c] < best || (spc[c] == best && un > bun)) { best = spc[c]; bidx = col; bun = un; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bidx, o, 64), ou = __shfl_xor(bun, o, 64);
                const bool take = oi >= 0 && (bidx < 0 || ob < best || (ob == best && (ou > bun || (ou == bun && oi < bidx))));
                if (take) { best = ob; bidx = oi; bun = ou; }
            }
            if (bidx < 0 || !(best < INF)) { failed = true; break; }                   // non-finite costs: leave the rest unmatched
            minVal = best;
            const int owner = bidx & 63, oc = bidx >> 6;
            const int rj = __shfl(oc ? r4c[1] : r4c[0], owner, 64);
            if (lane == owner) { if (oc) sc[1] = true; else sc[0] = true; }
            if (rj < 0) sink = bidx; else ii = rj;
        }
        if (sink < 0) { failed = true; break; }
        // duals: every scanned column but the sink is matched to a scanned row
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (sc[c]) {
                const double d = minVal - spc[c];
                if (r4c[c] >= 0) u[r4c[c]] += d;
                v[c] -= d;
            }
        }
        if (lane == 0) u[cur] += minVal;
        __syncthreads();
        // augment along the path back to `cur`
        int j = sink;
        for (int step = 0; step <= nr; ++step) {
            const int owner = j & 63, oc = j >> 6;
            const int pi = __shfl(oc ? path[1] : path[0], owner, 64);
            if (lane == owner) { if (oc) r4c[1] = pi; else r4c[0] = pi; }
            const int prev = col4row[pi];
            __syncthreads();
            if (lane == 0) col4row[pi] = j;
            __syncthreads();
            j = prev;
            if (pi == cur) break;
        }
    }
    for (int j = lane; j < nmax; j += 64) match_q[(long long)i * nmax + j] = j < nr ? col4row[j] : -1;
#pragma unroll
    for (int c = 0; c < 2; ++c)
        if (lane + 64 * c < nq) match_gt[(long long)i * nq + lane + 64 * c] = r4c[c];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (4) losses, forward.
// focal + dice sums of one matched mask over one band of PC_BAND low-resolution rows: the band's rows and one row either side (clamped)
// are staged in LDS, every high-resolution pixel of the band is interpolated from them.  partial = (focal sum, sum sigmoid * t, sum sigmoid, sum t)
__global__ __launch_bounds__(256) void pc_mask_fwd_kernel(const float* __restrict__ mlog, long long s_i, long long s_q, long long s_y, long long s_x,
                                                          const uint8_t* __restrict__ masks, const int* __restrict__ n,
                                                          const int* __restrict__ match_q, int B, int nq, int nmax, int h, int w, int H, int W,
                                                          int s, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    const int band = blockIdx.x, j = blockIdx.y, i = blockIdx.z, b = i % B, tid = threadIdx.x;
    if (j >= pc_n(n, b, nmax)) return;
    const int q = match_q[(long long)i * nmax + j];
    if (q < 0 || q >= nq) return;
    const int y0 = band * PC_BAND;
    const float* src = mlog + (long long)i * s_i + (long long)q * s_q;
    for (int e = tid; e < (PC_BAND + 2) * w; e += 256) {
        const int r = e / w, x = e % w, y = min(max(y0 - 1 + r, 0), h - 1);
        smem[e] = src[y * s_y + x * s_x];
    }
    __syncthreads();
    const int Y0 = s * y0, Y1 = min(s * (y0 + PC_BAND), H);
    const float inv_s = (float)h / (float)H;
    const uint8_t* m = masks + ((long long)b * nmax + j) * H * W;
    float sf = 0.f, sa = 0.f, sg = 0.f, st = 0.f;
    for (int e = tid; e < (Y1 - Y0) * W; e += 256) {
        const int Y = Y0 + e / W, X = e % W;
        int iy0, iy1, ix0, ix1;
        float ly, lx;
        pc_taps(Y, inv_s, h, iy0, iy1, ly);
        pc_taps(X, inv_s, w, ix0, ix1, lx);
        const float* r0 = smem + (iy0 - (y0 - 1)) * w;
        const float* r1 = smem + (iy1 - (y0 - 1)) * w;
        const float v = (1.f - ly) * ((1.f - lx) * r0[ix0] + lx * r0[ix1]) + ly * ((1.f - lx) * r1[ix0] + lx * r1[ix1]);
        const bool t = m[(long long)Y * W + X] != 0;
        float p, sp0, sp1;
        pc_sig(v, p, sp0, sp1);
        sf += t ? PC_ALPHA * ((1.f - p) * (1.f - p)) * sp1 : (1.f - PC_ALPHA) * (p * p) * sp0;
        sa += t ? p : 0.f;
        sg += p;
        st += t ? 1.f : 0.f;
    }
    sf = block_sum<4>(sf, red); sa = block_sum<4>(sa, red); sg = block_sum<4>(sg, red); st = block_sum<4>(st, red);
    if (tid == 0) {
        float* o = part + (((long long)i * nmax + j) * gridDim.x + band) * 4;
        o[0] = sf; o[1] = sa; o[2] = sg; o[3] = st;
    }
}

// |gt - upsampled prediction| of the two-channel centre map over one band of one batch element
__global__ __launch_bounds__(256) void pc_cpix_fwd_kernel(const float* __restrict__ pixc, long long s_b, long long s_c, long long s_y, long long s_x,
                                                          const float* __restrict__ gt, int h, int w, int H, int W, int s,
                                                          float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    const int band = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, y0 = band * PC_BAND, plane = (PC_BAND + 2) * w;
    for (int e = tid; e < 2 * plane; e += 256) {
        const int c = e / plane, r = (e % plane) / w, x = e % w, y = min(max(y0 - 1 + r, 0), h - 1);
        smem[e] = pixc[(long long)b * s_b + c * s_c + y * s_y + x * s_x];
    }
    __syncthreads();
    const int Y0 = s * y0, Y1 = min(s * (y0 + PC_BAND), H);
    const float inv_s = (float)h / (float)H;
    float acc = 0.f;
    for (int e = tid; e < (Y1 - Y0) * W; e += 256) {
        const int Y = Y0 + e / W, X = e % W;
        int iy0, iy1, ix0, ix1;
        float ly, lx, d2 = 0.f;
        pc_taps(Y, inv_s, h, iy0, iy1, ly);
        pc_taps(X, inv_s, w, ix0, ix1, lx);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* r0 = smem + c * plane + (iy0 - (y0 - 1)) * w;
            const float* r1 = smem + c * plane + (iy1 - (y0 - 1)) * w;
            const float v = (1.f - ly) * ((1.f - lx) * r0[ix0] + lx * r0[ix1]) + ly * ((1.f - lx) * r1[ix0] + lx * r1[ix1]);
            const float d = gt[(((long long)b * 2 + c) * H + Y) * W + X] - v;
            d2 += d * d;
        }
        acc += sqrtf(d2);
    }
    acc = block_sum<4>(acc, red);
    if (tid == 0) part[(long long)b * gridDim.x + band] = acc;
}

// p -> p / |p|^2 (normal / offset)
__device__ __forceinline__ void pc_inv_param(const float* p, float* o) {
    const float r2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    o[0] = p[0] / r2; o[1] = p[1] / r2; o[2] = p[2] / r2;
}

// Q loss of the last layer: per pixel X = k_inv_dot_xy1 * depth, the gt planes' |g . X - 1| over their masks decides the valid region, the
// matched predictions' |p . X - 1| is summed over it.  partial = (sum, count); `valid` keeps the region for the backward pass.
__global__ __launch_bounds__(256) void pc_q_fwd_kernel(const float* __restrict__ params, const float* __restrict__ tparams,
                                                       const uint8_t* __restrict__ masks, const int* __restrict__ n, const int* __restrict__ match_q,
                                                       const float* __restrict__ depth, const float* __restrict__ kinv, int nq, int nmax, int HW,
                                                       uint8_t* __restrict__ valid, float* __restrict__ part) {
    __shared__ float gp[PC_MAXT * 3], pp[PC_MAXT * 3];
    __shared__ float red[4];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nb = pc_n(n, b, nmax);
    if (tid < nb) {
        pc_inv_param(tparams + ((long long)b * nmax + tid) * 3, gp + 3 * tid);
        const int q = min(max(match_q[(long long)b * nmax + tid], 0), nq - 1);
        pc_inv_param(params + ((long long)b * nq + q) * 3, pp + 3 * tid);
    }
    __syncthreads();
    float sum = 0.f, cnt = 0.f;
    for (int e = chunk * 256 + tid; e < HW; e += 256 * PC_QCHUNKS) {
        const float d = depth[(long long)b * HW + e];
        const float* k = kinv + (long long)b * 3 * HW + e;
        const float X0 = k[0] * d, X1 = k[HW] * d, X2 = k[2 * (long long)HW] * d;
        float ge = 0.f, pe = 0.f;
        int cover = 0;
        for (int j = 0; j < nb; ++j) {
            const bool on = masks[((long long)b * nmax + j) * HW + e] != 0;
            const float g = fabsf(gp[3 * j] * X0 + gp[3 * j + 1] * X1 + gp[3 * j + 2] * X2 - 1.f);
            const float p = fabsf(pp[3 * j] * X0 + pp[3 * j + 1] * X1 + pp[3 * j + 2] * X2 - 1.f);
            ge += on ? g : 0.f;
            pe += on ? p : 0.f;
            cover += on ? 1 : 0;
        }
        const bool ok = ge < 0.2f && cover > 0;
        valid[(long long)b * HW + e] = ok ? 1 : 0;
        sum += ok ? pe : 0.f;
        cnt += ok ? 1.f : 0.f;
    }
    sum = block_sum<4>(sum, red); cnt = block_sum<4>(cnt, red);
    if (tid == 0) { part[((long long)b * PC_QCHUNKS + chunk) * 2] = sum; part[((long long)b * PC_QCHUNKS + chunk) * 2 + 1] = cnt; }
}

// per image: the band partials of every matched mask summed in band order -> mask_stats [i, j, 4] (kept for the backward pass) and the
// image's sums (0 class NLL numerator, 1 class weight sum, 2 centre distance, 3 param L1, 4 1 - cos, 5 focal mean, 6 dice)
__global__ __launch_bounds__(128) void pc_image_kernel(const float* __restrict__ logits, const float* __restrict__ centers,
                                                       const float* __restrict__ params, const float* __restrict__ tcenters,
                                                       const float* __restrict__ tparams, const int* __restrict__ n,
                                                       const int* __restrict__ match_q, const int* __restrict__ match_gt, int B, int nq, int nmax,
                                                       int nbands, int HW, float eos, const float* __restrict__ mask_part,
                                                       float* __restrict__ mask_stats, float* __restrict__ img) {
    __shared__ float red[2];
    __shared__ float fo[PC_MAXT], di[PC_MAXT];
    const int i = blockIdx.x, b = i % B, q = threadIdx.x, nb = pc_n(n, b, nmax);
    float num = 0.f, den = 0.f, cd = 0.f, l1 = 0.f, cs = 0.f;
    if (q < nq) {
        const int j = match_gt[(long long)i * nq + q];
        const float* z = logits + ((long long)i * nq + q) * 2;
        const float zm = fmaxf(z[0], z[1]), lse = zm + logf(expf(z[0] - zm) + expf(z[1] - zm));
        const float wt = j >= 0 ? 1.f : eos;
        num = wt * (lse - (j >= 0 ? z[0] : z[1]));
        den = wt;
        if (j >= 0 && j < nb) {
            const float* c = centers + ((long long)i * nq + q) * 2;
            const float* tc = tcenters + ((long long)b * nmax + j) * 2;
            const float dx = tc[0] - c[0], dy = tc[1] - c[1];
            cd = sqrtf(dx * dx + dy * dy);
            const float* p = params + ((long long)i * nq + q) * 3;
            const float* t = tparams + ((long long)b * nmax + j) * 3;
            l1 = fabsf(t[0] - p[0]) + fabsf(t[1] - p[1]) + fabsf(t[2] - p[2]);
            const float np_ = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            cs = 1.f - (p[0] * t[0] + p[1] * t[1] + p[2] * t[2]) / (fmaxf(np_, 1e-8f) * fmaxf(nt, 1e-8f));
        }
    }
    num = block_sum<2>(num, red); den = block_sum<2>(den, red); cd = block_sum<2>(cd, red); l1 = block_sum<2>(l1, red); cs = block_sum<2>(cs, red);
    if (q < nmax) {
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
        if (q < nb)
            for (int k = 0; k < nbands; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) s4[c] += mask_part[(((long long)i * nmax + q) * nbands + k) * 4 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) mask_stats[((long long)i * nmax + q) * 4 + c] = s4[c];
        if (q < PC_MAXT) {
            fo[q] = q < nb ? s4[0] / (float)HW : 0.f;
            di[q] = q < nb ? 1.f - (2.f * s4[1] + 1.f) / (s4[2] + s4[3] + 1.f) : 0.f;
        }
    }
    __syncthreads();
    if (q == 0) {
        float f = 0.f, d = 0.f;
        for (int j = 0; j < nb; ++j) { f += fo[j]; d += di[j]; }
        float* o = img + (long long)i * 8;
        o[0] = num; o[1] = den; o[2] = cd; o[3] = l1; o[4] = cs; o[5] = f; o[6] = d; o[7] = 0.f;
    }
}

// losses [G][6 L + 2], one workgroup per view group: per layer (ce, mask, dice, center_ins, param_l1, param_cos), then center_pixel and q of
// the last layer, each over the group's Bg images in their order.  q_stats [B, 2]
__global__ __launch_bounds__(64) void pc_final_kernel(const float* __restrict__ img, const float* __restrict__ cpix_part,
                                                      const float* __restrict__ q_part, const int* __restrict__ n, int L, int B, int Bg, int nmax,
                                                      int nbands, int HW, PcGroups pg, int with_pixel, float* __restrict__ losses,
                                                      float* __restrict__ q_stats) {
    const int t = threadIdx.x, grp = blockIdx.x, b0 = grp * Bg;
    const float nm = pc_num_masks(n, b0, Bg, nmax, pg.nm[grp]);
    losses += (long long)grp * (6 * L + 2);
    int matched = 0;
    for (int b = b0; b < b0 + Bg; ++b) matched += pc_n(n, b, nmax);
    if (t < L) {
        float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = b0; b < b0 + Bg; ++b)
#pragma unroll
            for (int c = 0; c < 7; ++c) s[c] += img[((long long)t * B + b) * 8 + c];
        float* o = losses + t * 6;
        o[0] = s[0] / s[1];
        o[1] = s[5] / nm;
        o[2] = s[6] / nm;
        o[3] = s[2] / (float)matched;
        o[4] = s[3] / (float)matched;
        o[5] = s[4] / (float)matched;
    }
    if (t == 62) {
        float a = 0.f;
        if (with_pixel)
            for (int k = 0; k < Bg * nbands; ++k) a += cpix_part[(long long)b0 * nbands + k];
        losses[6 * L] = a / ((float)Bg * (float)HW);
    }
    if (t == 63) {
        float a = 0.f;
        for (int b = b0; b < b0 + Bg; ++b) {
            float s = 0.f, c = 0.f;
            for (int k = 0; k < PC_QCHUNKS; ++k) { s += q_part[((long long)b * PC_QCHUNKS + k) * 2]; c += q_part[((long long)b * PC_QCHUNKS + k) * 2 + 1]; }
            q_stats[2 * b] = s; q_stats[2 * b + 1] = c;
            a += c > 0.f ? s / c : 0.f;
        }
        losses[6 * L + 1] = a / (float)Bg;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (5) losses, backward.
// d pred_mask_logits of one (image, query, band of low-resolution rows): zero for an unmatched query; otherwise every low-resolution pixel
// sums, over its high-resolution dependants in row-major order, weight_y * weight_x * d(loss) / d(upsampled logit).
__global__ __launch_bounds__(256) void pc_mask_bwd_kernel(const float* __restrict__ mlog, long long s_i, long long s_q, long long s_y, long long s_x,
                                                          const uint8_t* __restrict__ masks, const int* __restrict__ n,
                                                          const int* __restrict__ match_gt, const float* __restrict__ mask_stats,
                                                          const float* __restrict__ g, int B, int Bg, int gstride, int nq, int nmax, int h,
                                                          int w, int H, int W, int s, PcGroups pg, float* __restrict__ dml) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int band = blockIdx.x, q = blockIdx.y, i = blockIdx.z, b = i % B, layer = i / B, tid = threadIdx.x, y0 = band * PC_BAND;
    const int rows = min(PC_BAND, h - y0);
    float* dst = dml + (long long)i * s_i + (long long)q * s_q;
    const int j = match_gt[(long long)i * nq + q];
    if (j < 0 || j >= pc_n(n, b, nmax)) {
        for (int e = tid; e < rows * w; e += 256) dst[(y0 + e / w) * s_y + (e % w) * s_x] = 0.f;
        return;
    }
    const float* src = mlog + (long long)i * s_i + (long long)q * s_q;
    for (int e = tid; e < (PC_BAND + 2) * w; e += 256) {
        const int r = e / w, x = e % w, y = min(max(y0 - 1 + r, 0), h - 1);
        smem[e] = src[y * s_y + x * s_x];
    }
    __syncthreads();
    const int grp = b / Bg;
    const float nm = pc_num_masks(n, grp * Bg, Bg, nmax, pg.nm[grp]);
    g += (long long)grp * gstride;
    const float gm = g[layer * 6 + 1] / (nm * (float)H * (float)W), gd = g[layer * 6 + 2] / nm;
    const float* st = mask_stats + ((long long)i * nmax + j) * 4;
    const float D1 = st[2] + st[3] + 1.f, N1 = 2.f * st[1] + 1.f;
    const float inv_s = (float)h / (float)H;
    const uint8_t* m = masks + ((long long)b * nmax + j) * H * W;
    for (int e = tid; e < rows * w; e += 256) {
        const int y = y0 + e / w, x = e % w;
        int Ya, Yb, Xa, Xb;
        pc_dependants(y, s, H, Ya, Yb);
        pc_dependants(x, s, W, Xa, Xb);
        float acc = 0.f;
        for (int Y = Ya; Y <= Yb; ++Y) {
            const float wy = pc_tap_weight(Y, y, inv_s, h);
            int iy0, iy1;
            float ly;
            pc_taps(Y, inv_s, h, iy0, iy1, ly);
            const float* r0 = smem + (iy0 - (y0 - 1)) * w;
            const float* r1 = smem + (iy1 - (y0 - 1)) * w;
            for (int X = Xa; X <= Xb; ++X) {
                const float wx = pc_tap_weight(X, x, inv_s, w);
                int ix0, ix1;
                float lx;
                pc_taps(X, inv_s, w, ix0, ix1, lx);
                const float v = (1.f - ly) * ((1.f - lx) * r0[ix0] + lx * r0[ix1]) + ly * ((1.f - lx) * r1[ix0] + lx * r1[ix1]);
                const bool t = m[(long long)Y * W + X] != 0;
                float p, sp0, sp1;
                pc_sig(v, p, sp0, sp1);
                const float dfo = t ? -PC_ALPHA * ((1.f - p) * (1.f - p)) * (2.f * p * sp1 + (1.f - p))
                                    : (1.f - PC_ALPHA) * (p * p) * (2.f * (1.f - p) * sp0 + p);
                const float ddi = -((t ? 2.f * D1 : 0.f) - N1) / (D1 * D1) * (p * (1.f - p));
                acc += (wy * wx) * (gm * dfo + gd * ddi);
            }
        }
        dst[y * s_y + x * s_x] = acc;
    }
}

__global__ __launch_bounds__(256) void pc_cpix_bwd_kernel(const float* __restrict__ pixc, long long s_b, long long s_c, long long s_y, long long s_x,
                                                          const float* __restrict__ gt, const float* __restrict__ g, int L, int Bg, int h, int w,
                                                          int H, int W, int s, float* __restrict__ dpix) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int band = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, y0 = band * PC_BAND, plane = (PC_BAND + 2) * w;
    const int rows = min(PC_BAND, h - y0);
    for (int e = tid; e < 2 * plane; e += 256) {
        const int c = e / plane, r = (e % plane) / w, x = e % w, y = min(max(y0 - 1 + r, 0), h - 1);
        smem[e] = pixc[(long long)b * s_b + c * s_c + y * s_y + x * s_x];
    }
    __syncthreads();
    const float scale = g[(long long)(b / Bg) * (6 * L + 2) + 6 * L] / ((float)Bg * (float)H * (float)W), inv_s = (float)h / (float)H;
    for (int e = tid; e < rows * w; e += 256) {
        const int y = y0 + e / w, x = e % w;
        int Ya, Yb, Xa, Xb;
        pc_dependants(y, s, H, Ya, Yb);
        pc_dependants(x, s, W, Xa, Xb);
        float acc0 = 0.f, acc1 = 0.f;
        for (int Y = Ya; Y <= Yb; ++Y) {
            const float wy = pc_tap_weight(Y, y, inv_s, h);
            int iy0, iy1;
            float ly;
            pc_taps(Y, inv_s, h, iy0, iy1, ly);
            for (int X = Xa; X <= Xb; ++X) {
                const float wx = pc_tap_weight(X, x, inv_s, w);
                int ix0, ix1;
                float lx, d[2];
                pc_taps(X, inv_s, w, ix0, ix1, lx);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float* r0 = smem + c * plane + (iy0 - (y0 - 1)) * w;
                    const float* r1 = smem + c * plane + (iy1 - (y0 - 1)) * w;
                    const float v = (1.f - ly) * ((1.f - lx) * r0[ix0] + lx * r0[ix1]) + ly * ((1.f - lx) * r1[ix0] + lx * r1[ix1]);
                    d[c] = v - gt[(((long long)b * 2 + c) * H + Y) * W + X];
                }
                const float dist = sqrtf(d[0] * d[0] + d[1] * d[1]);
                const float k = dist > 0.f ? (wy * wx) / dist : 0.f;
                acc0 += k * d[0];
                acc1 += k * d[1];
            }
        }
        float* o = dpix + (long long)b * s_b + y * s_y + x * s_x;
        o[0] = scale * acc0;
        o[s_c] = scale * acc1;
    }
}

// sum over the valid pixels of target j's mask of sign(p' . X - 1) X, per chunk
__global__ __launch_bounds__(256) void pc_q_bwd_kernel(const float* __restrict__ params, const uint8_t* __restrict__ masks, const int* __restrict__ n,
                                                       const int* __restrict__ match_q, const float* __restrict__ depth,
                                                       const float* __restrict__ kinv, const uint8_t* __restrict__ valid, int nq, int nmax, int HW,
                                                       float* __restrict__ part) {
    __shared__ float red[4];
    const int chunk = blockIdx.x, j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if (j >= pc_n(n, b, nmax)) return;
    const int q = min(max(match_q[(long long)b * nmax + j], 0), nq - 1);
    float pp[3];
    pc_inv_param(params + ((long long)b * nq + q) * 3, pp);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int e = chunk * 256 + tid; e < HW; e += 256 * PC_QCHUNKS) {
        const bool on = valid[(long long)b * HW + e] != 0 && masks[((long long)b * nmax + j) * HW + e] != 0;
        const float d = depth[(long long)b * HW + e];
        const float* k = kinv + (long long)b * 3 * HW + e;
        const float X0 = k[0] * d, X1 = k[HW] * d, X2 = k[2 * (long long)HW] * d;
        const float r = pp[0] * X0 + pp[1] * X1 + pp[2] * X2 - 1.f;
        const float sg = on ? (r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f)) : 0.f;
        a0 += sg * X0; a1 += sg * X1; a2 += sg * X2;
    }
    a0 = block_sum<4>(a0, red); a1 = block_sum<4>(a1, red); a2 = block_sum<4>(a2, red);
    if (tid == 0) {
        float* o = part + (((long long)b * nmax + j) * PC_QCHUNKS + chunk) * 3;
        o[0] = a0; o[1] = a1; o[2] = a2;
    }
}

// d pred_logits, d pred_centers, d pred_params of one image (thread = query)
__global__ __launch_bounds__(128) void pc_small_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ centers,
                                                           const float* __restrict__ params, const float* __restrict__ tcenters,
                                                           const float* __restrict__ tparams, const int* __restrict__ n,
                                                           const int* __restrict__ match_gt, const float* __restrict__ g,
                                                           const float* __restrict__ q_part, const float* __restrict__ q_stats, int L, int B,
                                                           int Bg, int nq, int nmax, float eos, float* __restrict__ dlog, float* __restrict__ dcen,
                                                           float* __restrict__ dpar) {
    const int i = blockIdx.x, b = i % B, layer = i / B, q = threadIdx.x;
    if (q >= nq) return;
    const int grp = b / Bg;
    g += (long long)grp * (6 * L + 2);
    int matched = 0;
    float wsum = 0.f;
    for (int k = grp * Bg; k < (grp + 1) * Bg; ++k) { const int nk = pc_n(n, k, nmax); matched += nk; wsum += (float)nk + eos * (float)(nq - nk); }
    const int j = match_gt[(long long)i * nq + q];
    const bool on = j >= 0 && j < pc_n(n, b, nmax);
    const float* z = logits + ((long long)i * nq + q) * 2;
    const float zm = fmaxf(z[0], z[1]), e0 = expf(z[0] - zm), e1 = expf(z[1] - zm), p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    const float k = g[layer * 6] * (on ? 1.f : eos) / wsum;
    dlog[((long long)i * nq + q) * 2] = k * (p0 - (on ? 1.f : 0.f));
    dlog[((long long)i * nq + q) * 2 + 1] = k * (p1 - (on ? 0.f : 1.f));
    float dc[2] = {0.f, 0.f}, dp[3] = {0.f, 0.f, 0.f};
    if (on) {
        const float inv = 1.f / (float)matched;
        const float* c = centers + ((long long)i * nq + q) * 2;
        const float* tc = tcenters + ((long long)b * nmax + j) * 2;
        const float dx = c[0] - tc[0], dy = c[1] - tc[1], dist = sqrtf(dx * dx + dy * dy);
        if (dist > 0.f) { dc[0] = g[layer * 6 + 3] * inv * dx / dist; dc[1] = g[layer * 6 + 3] * inv * dy / dist; }
        const float* p = params + ((long long)i * nq + q) * 3;
        const float* t = tparams + ((long long)b * nmax + j) * 3;
        const float np_ = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        const float a = fmaxf(np_, 1e-8f), c2 = fmaxf(nt, 1e-8f), dot = p[0] * t[0] + p[1] * t[1] + p[2] * t[2], cosv = dot / (a * c2);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float d = p[e] - t[e];
            dp[e] = g[layer * 6 + 4] * inv * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
            // d (1 - cos) / d p = -(t / (|p| |t|) - cos p / |p|^2)   (|p| above the 1e-8 clamp)
            dp[e] += g[layer * 6 + 5] * inv * -(t[e] / (a * c2) - (np_ > 1e-8f ? cosv * p[e] / (np_ * np_) : 0.f));
        }
        if (layer == 0) {
            const float cnt = q_stats[2 * b + 1];
            if (cnt > 0.f) {
                float G[3] = {0.f, 0.f, 0.f};
                for (int c = 0; c < PC_QCHUNKS; ++c)
#pragma unroll
                    for (int e = 0; e < 3; ++e) G[e] += q_part[(((long long)b * nmax + j) * PC_QCHUNKS + c) * 3 + e];
                const float r2 = np_ * np_, gp = (G[0] * p[0] + G[1] * p[1] + G[2] * p[2]);
                const float kq = g[6 * L + 1] / ((float)Bg * cnt);
#pragma unroll
                for (int e = 0; e < 3; ++e) dp[e] += kq * (G[e] / r2 - 2.f * p[e] * gp / (r2 * r2));      // p' = p / |p|^2
            }
        }
    }
    dcen[((long long)i * nq + q) * 2] = dc[0];
    dcen[((long long)i * nq + q) * 2 + 1] = dc[1];
#pragma unroll
    for (int e = 0; e < 3; ++e) dpar[((long long)i * nq + q) * 3 + e] = dp[e];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gt correspondence matrix of the predicted planes (process_plane_corr_matrix): one workgroup per pair
__global__ __launch_bounds__(256) void pc_corr_matrix_kernel(const int* __restrict__ gt_corrs, int K, const int* __restrict__ match1,
                                                             const int* __restrict__ match2, int nq, int nmax, uint8_t* __restrict__ out) {
    __shared__ uint8_t M[(PC_MAXQ + 1) * (PC_MAXQ + 1)];
    const int b = blockIdx.x, tid = threadIdx.x, S = nq + 1;
    for (int e = tid; e < S * S; e += 256) M[e] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        const int a = gt_corrs[((long long)b * K + k) * 2], c = gt_corrs[((long long)b * K + k) * 2 + 1];
        if (a < 0 || c < 0 || a >= 50 || c >= 50) continue;                     // padding rows; the reference's `< 50` filter
        const int ac = min(a, nmax - 1), cc = min(c, nmax - 1);
        const int m1 = match1[(long long)b * nmax + ac], m2 = match2[(long long)b * nmax + cc];
        const int pa = (a < nmax && a < nq && m1 >= 0) ? m1 : nq, pc = (c < nmax && c < nq && m2 >= 0) ? m2 : nq;
        M[pa * S + pc] = 1;                                                      // equal values: the order of the writes does not matter
    }
    __syncthreads();
    uint8_t* o = out + (long long)b * S * S;
    for (int e = tid; e < nq * nq; e += 256) o[(e / nq) * S + e % nq] = M[(e / nq) * S + e % nq];
    for (int c = tid; c < nq; c += 256) {
        int any_r = 0, any_c = 0;
        for (int r = 0; r < nq; ++r) { any_r |= M[r * S + c]; any_c |= M[c * S + r]; }
        o[nq * S + c] = any_r ? 0 : 1;                                           // dustbin row: no plane of view 1 claims column c
        o[c * S + nq] = any_c ? 0 : 1;                                           // dustbin column
    }
    if (tid == 0) o[nq * S + nq] = 0;
}

// ---- argument checks shared by the struct entry points (before any HIP call)
static int pc_scale(int h, int w, int H, int W) {
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || H % h != 0 || W % w != 0 || H / h != W / w) return 0;
    return H / h;
}
// the groups of an argument block: G = 1 for groups 0 or 1; false if G does not divide B or exceeds PC_MAXG
static bool pc_groups(const nopesac_plane_criterion* a, PcGroups& pg) {
    const int G = a->groups <= 1 ? 1 : a->groups;
    if (a->groups < 0 || G > PC_MAXG || a->B % G != 0) return false;
    pg.G = G;
    for (int g = 0; g < PC_MAXG; ++g) pg.nm[g] = g < G ? (a->num_masks_groups ? a->num_masks_groups[g] : a->num_masks) : 0.f;
    return true;
}
static const char* pc_check_n(const int32_t* n_host, int B, int nq) {
    for (int b = 0; b < B; ++b)
        if (n_host[b] < 1 || n_host[b] > (nq < PC_MAXT ? nq : PC_MAXT)) return "n";
    return nullptr;
}

}  // namespace nps

using namespace nps;

#define PC_CHECK_COMMON(name, a)                                                                                                               \
    NPS_CHECK_ARG((a) != nullptr, name ": null argument block");                                                                               \
    NPS_CHECK_ARG((a)->L >= 1 && (a)->L <= PC_MAXL && (a)->B >= 1, name ": bad dims (L=%d in 1..%d, B=%d)", (a)->L, PC_MAXL, (a)->B);          \
    NPS_CHECK_ARG((a)->nq >= 1 && (a)->nq <= PC_MAXQ, name ": nq=%d outside 1..%d", (a)->nq, PC_MAXQ);                                         \
    NPS_CHECK_ARG((a)->nmax >= 1 && (a)->nmax <= PC_MAXT, name ": nmax=%d outside 1..%d", (a)->nmax, PC_MAXT);                                 \
    NPS_CHECK_ARG((a)->num_classes == 2, name ": classes=%d (the plane head has 2: plane, no object)", (a)->num_classes);                      \
    NPS_CHECK_ARG(pc_scale((a)->h, (a)->w, (a)->H, (a)->W) >= 1, name ": scale: (H, W) = (%d, %d) is no integer multiple s >= 1 of (h, w) = (%d, %d)", \
                  (a)->H, (a)->W, (a)->h, (a)->w);                                                                                             \
    NPS_CHECK_ARG((a)->n_host && (a)->n, name ": null n");                                                                                     \
    NPS_CHECK_ARG(pc_check_n((a)->n_host, (a)->B, (a)->nq < (a)->nmax ? (a)->nq : (a)->nmax) == nullptr, name ": n[b] outside 1..min(nq, nmax, %d)", PC_MAXT); \
    NPS_CHECK_ARG((a)->ws && (a)->ws_floats >= nopesac_plane_criterion_workspace_floats((a)->L, (a)->B, (a)->nq, (a)->nmax, (a)->h, (a)->w),    \
                  name ": workspace too small (%lld floats)", (long long)(a)->ws_floats)

extern "C" int64_t nopesac_plane_criterion_workspace_floats(int L, int B, int nq, int nmax, int h, int w) {
    if (L < 1 || B < 1 || nq < 1 || nmax < 1 || h < 1 || w < 1) return 0;
    const int64_t a = pc_ws_cost(L, B, nq, nmax), b = pc_ws_loss(L, B, nmax, h);
    return a > b ? a : b;
}

extern "C" int nopesac_plane_targets(const uint8_t* masks, const int32_t* n_host, const int32_t* n, int B, int nmax, int H, int W,
                                     float* plane_centers, float* pixel_centers, void* stream) {
    NPS_CHECK_ARG(masks && n_host && n, "plane_targets: null input");
    NPS_CHECK_ARG(plane_centers && pixel_centers, "plane_targets: null output");
    NPS_CHECK_ARG(B >= 1 && nmax >= 1 && nmax <= PC_MAXT && H >= 1 && W >= 1, "plane_targets: bad dims (B=%d, nmax=%d in 1..%d, H=%d, W=%d)", B, nmax,
                  PC_MAXT, H, W);
    for (int b = 0; b < B; ++b) NPS_CHECK_ARG(n_host[b] >= 1 && n_host[b] <= nmax, "plane_targets: n[%d]=%d outside 1..nmax", b, n_host[b]);
    hipStream_t st = (hipStream_t)stream;
    pc_plane_centers_kernel<<<dim3(nmax, B), 256, 0, st>>>(masks, n, nmax, H, W, plane_centers);
    pc_pixel_centers_kernel<<<dim3((H * W + 255) / 256, B), 256, 0, st>>>(masks, n, nmax, H * W, plane_centers, pixel_centers);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_plane_match_costs(const nopesac_plane_criterion* a, void* stream) {
    PC_CHECK_COMMON("plane_match_costs", a);
    NPS_CHECK_ARG(a->pred_logits && a->pred_mask_logits && a->pred_centers && a->pred_params && a->masks && a->tgt_centers && a->tgt_params,
                  "plane_match_costs: null input");
    NPS_CHECK_ARG(a->cost, "plane_match_costs: null output");
    hipStream_t st = (hipStream_t)stream;
    const int LB = a->L * a->B, s = pc_scale(a->h, a->w, a->H, a->W), nblk = pc_cost_blocks(a->h, a->w), rows = a->nq + 1;
    const size_t lds = ((size_t)2 * rows * PC_LS + 2 * rows) * sizeof(float) + PC_CHUNK * sizeof(unsigned long long);
    NPS_ENSURE_LDS(lds, pc_cost_partial_kernel);
    pc_cost_partial_kernel<<<dim3(nblk, LB), 256, lds, st>>>(a->pred_mask_logits, a->ml_stride_i, a->ml_stride_q, a->ml_stride_y, a->ml_stride_x,
                                                             a->masks, a->n, a->B, a->nq, a->nmax, a->h, a->w, a->H, a->W, s, nblk, a->ws);
    const PcCostW cw = {a->cost_class, a->cost_mask, a->cost_dice, a->cost_center, a->cost_param, a->cost_offset, a->cost_angle};
    pc_cost_finish_kernel<<<dim3((a->nq * a->nmax + 255) / 256, LB), 256, 0, st>>>(a->ws, nblk, a->pred_logits, a->pred_centers, a->pred_params,
                                                                                   a->tgt_centers, a->tgt_params, a->n, a->B, a->nq, a->nmax,
                                                                                   a->h * a->w, cw, a->cost);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_plane_assign(const float* cost, const int32_t* n_host, const int32_t* n, int L, int B, int nq, int nmax, int32_t* match_q,
                                    int32_t* match_gt, void* stream) {
    NPS_CHECK_ARG(cost && n_host && n, "plane_assign: null input");
    NPS_CHECK_ARG(match_q && match_gt, "plane_assign: null output");
    NPS_CHECK_ARG(L >= 1 && L <= PC_MAXL && B >= 1, "plane_assign: bad dims (L=%d, B=%d)", L, B);
    NPS_CHECK_ARG(nq >= 1 && nq <= PC_MAXQ, "plane_assign: nq=%d outside 1..%d", nq, PC_MAXQ);
    NPS_CHECK_ARG(nmax >= 1 && nmax <= PC_MAXT, "plane_assign: nmax=%d outside 1..%d", nmax, PC_MAXT);
    NPS_CHECK_ARG(pc_check_n(n_host, B, nq) == nullptr, "plane_assign: n[b] outside 1..min(nq, %d)", PC_MAXT);
    for (int b = 0; b < B; ++b) NPS_CHECK_ARG(n_host[b] <= nmax, "plane_assign: n[%d]=%d above nmax", b, n_host[b]);
    pc_assign_kernel<<<L * B, 64, 0, (hipStream_t)stream>>>(cost, n, B, nq, nmax, match_q, match_gt);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_plane_losses(const nopesac_plane_criterion* a, void* stream) {
    PC_CHECK_COMMON("plane_losses", a);
    NPS_CHECK_ARG(a->pred_logits && a->pred_mask_logits && a->pred_centers && a->pred_params && a->masks && a->tgt_centers && a->tgt_params &&
                      a->depth && a->k_inv_dot_xy1 && a->match_q && a->match_gt && (!a->pixel_centers || a->tgt_pixel_centers),
                  "plane_losses: null input");
    NPS_CHECK_ARG(a->losses && a->mask_stats && a->q_valid && a->q_stats, "plane_losses: null output");
    PcGroups pg;
    NPS_CHECK_ARG(pc_groups(a, pg), "plane_losses: groups=%d must be 0..%d and divide B=%d", a->groups, PC_MAXG, a->B);
    hipStream_t st = (hipStream_t)stream;
    const int LB = a->L * a->B, s = pc_scale(a->h, a->w, a->H, a->W), nb = pc_bands(a->h), HW = a->H * a->W;
    float* mask_part = a->ws;
    float* cpix_part = mask_part + pc_ws_mask(a->L, a->B, a->nmax, a->h);
    float* q_part = cpix_part + (int64_t)a->B * nb;
    float* img = q_part + (int64_t)a->B * PC_QCHUNKS * 2;
    const size_t lds = (size_t)(PC_BAND + 2) * a->w * sizeof(float);
    NPS_CHECK_ARG(2 * lds <= 60 * 1024, "plane_losses: w=%d too wide for the row band in LDS", a->w);
    pc_mask_fwd_kernel<<<dim3(nb, a->nmax, LB), 256, lds, st>>>(a->pred_mask_logits, a->ml_stride_i, a->ml_stride_q, a->ml_stride_y, a->ml_stride_x,
                                                                a->masks, a->n, a->match_q, a->B, a->nq, a->nmax, a->h, a->w, a->H, a->W, s, mask_part);
    if (a->pixel_centers)
        pc_cpix_fwd_kernel<<<dim3(nb, a->B), 256, 2 * lds, st>>>(a->pixel_centers, a->pc_stride_b, a->pc_stride_c, a->pc_stride_y, a->pc_stride_x,
                                                                 a->tgt_pixel_centers, a->h, a->w, a->H, a->W, s, cpix_part);
    pc_q_fwd_kernel<<<dim3(PC_QCHUNKS, a->B), 256, 0, st>>>(a->pred_params, a->tgt_params, a->masks, a->n, a->match_q, a->depth, a->k_inv_dot_xy1,
                                                            a->nq, a->nmax, HW, a->q_valid, q_part);
    pc_image_kernel<<<LB, 128, 0, st>>>(a->pred_logits, a->pred_centers, a->pred_params, a->tgt_centers, a->tgt_params, a->n, a->match_q,
                                        a->match_gt, a->B, a->nq, a->nmax, nb, HW, a->eos_coef, mask_part, a->mask_stats, img);
    pc_final_kernel<<<pg.G, 64, 0, st>>>(img, cpix_part, q_part, a->n, a->L, a->B, a->B / pg.G, a->nmax, nb, HW, pg, a->pixel_centers ? 1 : 0,
                                         a->losses, a->q_stats);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_plane_losses_backward(const nopesac_plane_criterion* a, void* stream) {
    PC_CHECK_COMMON("plane_losses_backward", a);
    NPS_CHECK_ARG(a->pred_logits && a->pred_mask_logits && a->pred_centers && a->pred_params && a->masks && a->tgt_centers && a->tgt_params &&
                      a->depth && a->k_inv_dot_xy1 && a->match_q && a->match_gt && a->mask_stats && a->q_valid && a->q_stats && a->g_losses &&
                      (!a->pixel_centers || a->tgt_pixel_centers),
                  "plane_losses_backward: null input");
    NPS_CHECK_ARG(a->d_logits && a->d_mask_logits && a->d_centers && a->d_params && (!a->pixel_centers || a->d_pixel_centers),
                  "plane_losses_backward: null output");
    PcGroups pg;
    NPS_CHECK_ARG(pc_groups(a, pg), "plane_losses_backward: groups=%d must be 0..%d and divide B=%d", a->groups, PC_MAXG, a->B);
    const int Bg = a->B / pg.G;
    hipStream_t st = (hipStream_t)stream;
    const int LB = a->L * a->B, s = pc_scale(a->h, a->w, a->H, a->W), nb = pc_bands(a->h), HW = a->H * a->W;
    float* q_part = a->ws + pc_ws_loss(a->L, a->B, a->nmax, a->h) - (int64_t)a->B * a->nmax * PC_QCHUNKS * 3;
    const size_t lds = (size_t)(PC_BAND + 2) * a->w * sizeof(float);
    NPS_CHECK_ARG(2 * lds <= 60 * 1024, "plane_losses_backward: w=%d too wide for the row band in LDS", a->w);
    pc_mask_bwd_kernel<<<dim3(nb, a->nq, LB), 256, lds, st>>>(a->pred_mask_logits, a->ml_stride_i, a->ml_stride_q, a->ml_stride_y, a->ml_stride_x,
                                                              a->masks, a->n, a->match_gt, a->mask_stats, a->g_losses, a->B, Bg, 6 * a->L + 2, a->nq,
                                                              a->nmax, a->h, a->w, a->H, a->W, s, pg, a->d_mask_logits);
    if (a->pixel_centers)
        pc_cpix_bwd_kernel<<<dim3(nb, a->B), 256, 2 * lds, st>>>(a->pixel_centers, a->pc_stride_b, a->pc_stride_c, a->pc_stride_y, a->pc_stride_x,
                                                                 a->tgt_pixel_centers, a->g_losses, a->L, Bg, a->h, a->w, a->H, a->W, s,
                                                                 a->d_pixel_centers);
    pc_q_bwd_kernel<<<dim3(PC_QCHUNKS, a->nmax, a->B), 256, 0, st>>>(a->pred_params, a->masks, a->n, a->match_q, a->depth, a->k_inv_dot_xy1,
                                                                     a->q_valid, a->nq, a->nmax, HW, q_part);
    pc_small_bwd_kernel<<<LB, 128, 0, st>>>(a->pred_logits, a->pred_centers, a->pred_params, a->tgt_centers, a->tgt_params, a->n, a->match_gt,
                                            a->g_losses, q_part, a->q_stats, a->L, a->B, Bg, a->nq, a->nmax, a->eos_coef, a->d_logits, a->d_centers,
                                            a->d_params);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_plane_corr_matrix(const int32_t* gt_corrs, int K, const int32_t* match1, const int32_t* match2, int B, int nq, int nmax,
                                         uint8_t* out, void* stream) {
    NPS_CHECK_ARG(gt_corrs && match1 && match2, "plane_corr_matrix: null input");
    NPS_CHECK_ARG(out, "plane_corr_matrix: null output");
    NPS_CHECK_ARG(B >= 1 && K >= 1, "plane_corr_matrix: bad dims (B=%d, K=%d)", B, K);
    NPS_CHECK_ARG(nq >= 1 && nq <= PC_MAXQ, "plane_corr_matrix: nq=%d outside 1..%d", nq, PC_MAXQ);
    NPS_CHECK_ARG(nmax >= 1 && nmax <= PC_MAXT, "plane_corr_matrix: nmax=%d outside 1..%d", nmax, PC_MAXT);
    pc_corr_matrix_kernel<<<B, 256, 0, (hipStream_t)stream>>>(gt_corrs, K, match1, match2, nq, nmax, out);
    NPS_LAUNCH_RET();
}
