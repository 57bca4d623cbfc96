// Ground truth for training: a dataset's per-view record -> the targets the plane criterion reads (prepare_targets,
// siamese_planeTR.py:475-532; get_coordinate_map, :815-839).
//     ids            = torch.unique(semantic_map), the first dropped when it is 0, at most 50 kept
//     masks[j]       = ids[j] == semantic_map
//     plane_centers  = centroid of (x / W, y / H) over each mask: exact integer sums, then (float)(sum / W / count) in f64 - the quotient
//                      pc_plane_centers_kernel (plane_criterion.hip) takes, so both routes give the same bits
//     pixel_centers  = sum_j centre_j * mask_j: label masks are disjoint, so the sum is the centre of the pixel's own plane
//     depth          = uint16 millimetres.astype(float32) / 1000.
//     k_inv_dot_xy1  = K^-1 . (x, y, 1), x = arange(w) / w * 640, y = arange(h) / h * 480 in f32
// The mask pass is the bandwidth pass (nmax bytes written per pixel, 4 read): a thread keeps the plane indices of 16 consecutive
// pixels in four packed words and writes every plane row from them, 16 bytes per lane, 1 KB contiguous per wave and row.  Loads
// come from addresses clamped into the image, stores are predicated: no guarded load anywhere.
#include "common.h"

namespace nps {

constexpr int TT_IDS = NPS_LABEL_MAX_IDS, TT_SLOTS = NPS_LABEL_TABLE_SLOTS, TT_CHUNK = NPS_LABEL_CHUNK, TT_MAXT = NPS_PLANE_MAX_TARGETS;
constexpr int TT_PX = 16;                               // pixels per thread: TT_CHUNK = 256 threads x TT_PX
constexpr uint32_t TT_NONE = 0xffu;                     // plane index of a pixel that lies on no plane (TT_MAXT < 255)
static_assert(TT_CHUNK == 256 * TT_PX && (TT_SLOTS & (TT_SLOTS - 1)) == 0 && TT_SLOTS >= 2 * TT_IDS && TT_MAXT <= 64, "train_targets constants");

__device__ __forceinline__ int tt_n(const int* n, int b, int nmax) { return min(max(n[b], 0), nmax); }

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) distinct labels of an image.  One workgroup per image.  A slot holds 2^32 | value (0 = empty: every int32 is a legal label);
// which slot a value lands in depends on the order of the compare-and-swaps, the SET of values in the table does not, and the rank
// sort below reads nothing but the set.
__global__ __launch_bounds__(1024) void tt_label_ids_kernel(const int* __restrict__ labels, int HW, int vec4, int nmax_limit, int* __restrict__ ids,
                                                            int* __restrict__ n_all, int* __restrict__ n, int* __restrict__ bad) {
    __shared__ unsigned long long table[TT_SLOTS];
    __shared__ int list[TT_IDS], sorted[TT_IDS];
    __shared__ int count, overflow;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int s = tid; s < TT_SLOTS; s += 1024) table[s] = 0ull;
    if (tid == 0) count = overflow = 0;
    __syncthreads();
    const int* m = labels + (long long)b * HW;
    bool have = false;
    int last = 0;
    auto insert = [&](int key) {
        if (have && key == last) return;                            // neighbouring pixels mostly share a label
        have = true; last = key;
        if (*(volatile int*)&count > TT_IDS) return;                // already too many: the image is refused, stop filling the table
        const unsigned long long want = (1ull << 32) | (unsigned long long)(uint32_t)key;
        uint32_t s = (uint32_t)key & (TT_SLOTS - 1);
        for (int probe = 0; probe < TT_SLOTS; ++probe, s = (s + 1) & (TT_SLOTS - 1)) {
            unsigned long long cur = table[s];                      // a stale read is safe: a slot changes once, from 0
            if (cur == 0ull) cur = atomicCAS(&table[s], 0ull, want);
            if (cur == 0ull) {                                      // this thread placed the value: it is new
                const int pos = atomicAdd(&count, 1);
                if (pos < TT_IDS) list[pos] = key;
                return;
            }
            if (cur == want) return;
        }
        overflow = 1;                                               // the table is full of other values
    };
    if (vec4) {
        const int4* m4 = reinterpret_cast<const int4*>(m);
        for (int q = tid; q < HW / 4; q += 1024) {
            const int4 v = m4[q];
            insert(v.x); insert(v.y); insert(v.z); insert(v.w);
        }
    } else {
        for (int e = tid; e < HW; e += 1024) insert(m[e]);
    }
    __syncthreads();
    const int c = count;
    const bool refused = c > TT_IDS || overflow != 0;
    if (!refused)
        for (int i = tid; i < c; i += 1024) {                       // all values differ: the ranks are a permutation
            const int key = list[i];
            int rank = 0;
            for (int j = 0; j < c; ++j) rank += list[j] < key ? 1 : 0;
            sorted[rank] = key;
        }
    __syncthreads();
    const int drop = (!refused && c > 0 && sorted[0] == 0) ? 1 : 0;
    const int total = refused ? 0 : c - drop;
    for (int k = tid; k < TT_IDS; k += 1024) ids[(long long)b * TT_IDS + k] = k < total ? sorted[k + drop] : 0;
    if (tid == 0) {
        n_all[b] = total;
        n[b] = min(total, nmax_limit);
        bad[b] = refused ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) labels -> plane indices.  The labels of TT_PX consecutive pixels from e0 on, read from addresses clamped into the image (what lies
// past the image repeats the last pixels and is never stored).
__device__ __forceinline__ void tt_load16(const int* __restrict__ m, long long e0, int HW, int vec4, int (&v)[TT_PX]) {
    if (vec4) {
#pragma unroll
        for (int k = 0; k < TT_PX / 4; ++k) {
            const long long e = min(e0 + 4 * k, (long long)HW - 4);
            const int4 q = *reinterpret_cast<const int4*>(m + e);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < TT_PX; ++k) v[k] = m[min(e0 + k, (long long)HW - 1)];
    }
}

// index of `key` in the ascending sid[0 .. nb), TT_NONE if it is not there; sid holds 64 readable entries, nb <= 50
__device__ __forceinline__ uint32_t tt_find(const int* sid, int nb, int key) {
    int pos = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int probe = sid[min(pos + step - 1, 63)];
        pos += (pos + step <= nb && probe < key) ? step : 0;
    }
    return (pos < nb && sid[min(pos, 63)] == key) ? (uint32_t)pos : TT_NONE;
}

// integer partial sums (x, y, count) per plane over one chunk of TT_CHUNK pixels: grid (chunks, B) -> ws uint32 [B][chunks][nmax][3]
__global__ __launch_bounds__(256) void tt_label_sums_kernel(const int* __restrict__ labels, const int* __restrict__ ids, const int* __restrict__ n,
                                                            int nmax, int W, int HW, int vec4, uint32_t* __restrict__ ws) {
    __shared__ int sid[64];
    __shared__ uint32_t acc[TT_MAXT * 3];
    const int b = blockIdx.y, tid = threadIdx.x, nb = tt_n(n, b, nmax);
    if (tid < 64) sid[tid] = tid < nb ? ids[(long long)b * TT_IDS + tid] : 0;
    if (tid < TT_MAXT * 3) acc[tid] = 0u;
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * TT_CHUNK + (long long)tid * TT_PX;
    int v[TT_PX];
    tt_load16(labels + (long long)b * HW, e0, HW, vec4, v);
    int x = (int)(e0 % W), y = (int)(e0 / W);
    uint32_t cur = TT_NONE, sx = 0, sy = 0, cnt = 0;                // a run of one plane inside the thread's pixels is added once
#pragma unroll
    for (int k = 0; k < TT_PX; ++k) {
        const uint32_t j = (e0 + k < HW) ? tt_find(sid, nb, v[k]) : TT_NONE;
        if (j != cur) {
            if (cur != TT_NONE) { atomicAdd(&acc[cur * 3], sx); atomicAdd(&acc[cur * 3 + 1], sy); atomicAdd(&acc[cur * 3 + 2], cnt); }
            cur = j; sx = sy = cnt = 0;
        }
        sx += (uint32_t)x; sy += (uint32_t)y; cnt += 1;
        if (++x == W) { x = 0; ++y; }
    }
    if (cur != TT_NONE) { atomicAdd(&acc[cur * 3], sx); atomicAdd(&acc[cur * 3 + 1], sy); atomicAdd(&acc[cur * 3 + 2], cnt); }
    __syncthreads();
    if (tid < nmax * 3) ws[((long long)b * gridDim.x + blockIdx.x) * nmax * 3 + tid] = acc[tid];
}

// the chunks' partials (integers: any order gives the same sums) -> centres; grid (nmax, B), one wave per plane
__global__ __launch_bounds__(64) void tt_label_centers_kernel(const uint32_t* __restrict__ ws, const int* __restrict__ n, int nmax, int chunks, int H,
                                                              int W, float* __restrict__ centers) {
    const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    float* out = centers + ((long long)b * nmax + j) * 2;
    if (j >= tt_n(n, b, nmax)) {
        if (lane < 2) out[lane] = 0.f;
        return;
    }
    unsigned long long sx = 0, sy = 0, c = 0;
    for (int k = lane; k < chunks; k += 64) {
        const uint32_t* p = ws + (((long long)b * chunks + k) * nmax + j) * 3;
        sx += p[0]; sy += p[1]; c += p[2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sx += (unsigned long long)__shfl_xor((long long)sx, o, 64);
        sy += (unsigned long long)__shfl_xor((long long)sy, o, 64);
        c += (unsigned long long)__shfl_xor((long long)c, o, 64);
    }
    if (lane == 0) {
        out[0] = (float)((double)sx / (double)W / (double)c);         // a label that owns no pixel gives NaN, as the reference's 0 / 0 does
        out[1] = (float)((double)sy / (double)H / (double)c);
    }
}

// 0x01 in every byte of `packed` that equals the byte j, 0x00 elsewhere (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t tt_bytes_equal(uint32_t packed, uint32_t j4) {
    const uint32_t x = packed ^ j4;
    return (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu)) >> 7;
}

// the mask pass: grid (chunks, B)
__global__ __launch_bounds__(256) void tt_label_masks_kernel(const int* __restrict__ labels, const int* __restrict__ ids, const int* __restrict__ n,
                                                             int nmax, int HW, int vec4, int wide, const float* __restrict__ centers,
                                                             uint8_t* __restrict__ masks, float* __restrict__ pixel) {
    __shared__ int sid[64];
    __shared__ float cs[TT_MAXT * 2 + 2];
    const int b = blockIdx.y, tid = threadIdx.x, nb = tt_n(n, b, nmax);
    if (tid < 64) sid[tid] = tid < nb ? ids[(long long)b * TT_IDS + tid] : 0;
    if (tid < nmax * 2) cs[tid] = centers[(long long)b * nmax * 2 + tid];
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * TT_CHUNK + (long long)tid * TT_PX;
    int v[TT_PX];
    tt_load16(labels + (long long)b * HW, e0, HW, vec4, v);
    uint32_t pk[TT_PX / 4];
    float cx[TT_PX], cy[TT_PX];
#pragma unroll
    for (int k = 0; k < TT_PX; ++k) {
        const uint32_t j = tt_find(sid, nb, v[k]);
        const uint32_t jc = min(j, (uint32_t)(TT_MAXT - 1));         // a clamped LDS address and a select
        const float x = cs[2 * jc], y = cs[2 * jc + 1];
        cx[k] = j == TT_NONE ? 0.f : x;
        cy[k] = j == TT_NONE ? 0.f : y;
        pk[k >> 2] = (k & 3) == 0 ? j : (pk[k >> 2] | (j << (8 * (k & 3))));
    }
    uint8_t* mrow = masks + (long long)b * nmax * HW + e0;
    float* px = pixel + (long long)b * 2 * HW + e0;
    if (wide) {                                                     // H W % 16 == 0: a thread's 16 pixels are inside the image or all outside
        if (e0 >= HW) return;
        for (int j = 0; j < nmax; ++j) {
            const uint32_t j4 = (uint32_t)j * 0x01010101u;
            *reinterpret_cast<uint4*>(mrow + (long long)j * HW) =
                make_uint4(tt_bytes_equal(pk[0], j4), tt_bytes_equal(pk[1], j4), tt_bytes_equal(pk[2], j4), tt_bytes_equal(pk[3], j4));
        }
#pragma unroll
        for (int k = 0; k < TT_PX; k += 4) {
            *reinterpret_cast<float4*>(px + k) = make_float4(cx[k], cx[k + 1], cx[k + 2], cx[k + 3]);
            *reinterpret_cast<float4*>(px + HW + k) = make_float4(cy[k], cy[k + 1], cy[k + 2], cy[k + 3]);
        }
        return;
    }
    for (int j = 0; j < nmax; ++j) {
        const uint32_t j4 = (uint32_t)j * 0x01010101u;
#pragma unroll
        for (int k = 0; k < TT_PX; ++k)
            if (e0 + k < HW) mrow[(long long)j * HW + k] = (uint8_t)((tt_bytes_equal(pk[k >> 2], j4) >> (8 * (k & 3))) & 1u);
    }
#pragma unroll
    for (int k = 0; k < TT_PX; ++k)
        if (e0 + k < HW) { px[k] = cx[k]; px[HW + k] = cy[k]; }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) bit-packed column-major masks -> byte masks, row-major: grid (chunks, nmax, B).  Whether the row exists is uniform per workgroup.
__global__ __launch_bounds__(256) void tt_bits_to_masks_kernel(const uint32_t* __restrict__ bits, long long n_rows, const long long* __restrict__ offsets,
                                                               int nmax, int H, int W, int HW, int words, int wide, uint8_t* __restrict__ masks) {
    const int b = blockIdx.z, j = blockIdx.y;
    const long long first = offsets[b], have = min(max(offsets[b + 1] - first, 0ll), (long long)nmax);
    const long long e0 = (long long)blockIdx.x * TT_CHUNK + (long long)threadIdx.x * TT_PX;
    uint32_t pk[TT_PX / 4] = {0u, 0u, 0u, 0u};
    if (j < have && n_rows > 0) {
        const uint32_t* row = bits + min(max(first + j, 0ll), n_rows - 1) * words;
        const long long ec = min(e0, (long long)HW - 1);
        int x = (int)(ec % W), y = (int)(ec / W);
#pragma unroll
        for (int k = 0; k < TT_PX; ++k) {
            const long long p = (long long)x * H + y;               // (x, y) stays inside the image: the walk stops at the last pixel
            pk[k >> 2] |= ((row[p >> 5] >> (p & 31)) & 1u) << (8 * (k & 3));
            if (x + 1 < W) ++x;
            else if (y + 1 < H) { x = 0; ++y; }
        }
    }
    uint8_t* o = masks + ((long long)b * nmax + j) * HW + e0;
    if (wide) {
        if (e0 < HW) *reinterpret_cast<uint4*>(o) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < TT_PX; ++k)
        if (e0 + k < HW) o[k] = (uint8_t)((pk[k >> 2] >> (8 * (k & 3))) & 1u);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (4) depth: threads [0, groups) take 8 values each with 16-byte accesses, the threads behind them one value each (the tail, or
// everything when a buffer is not aligned)
__global__ __launch_bounds__(256) void tt_depth_kernel(const uint16_t* __restrict__ src, long long n, long long groups, float scale,
                                                       float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < groups) {
        const uint4 q = reinterpret_cast<const uint4*>(src)[t];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[2 * k] = __fdiv_rn((float)(w[k] & 0xffffu), scale);
            f[2 * k + 1] = __fdiv_rn((float)(w[k] >> 16), scale);
        }
        float4* o = reinterpret_cast<float4*>(out) + 2 * t;
        o[0] = make_float4(f[0], f[1], f[2], f[3]);
        o[1] = make_float4(f[4], f[5], f[6], f[7]);
        return;
    }
    const long long e = groups * 8 + (t - groups);
    const float val = __fdiv_rn((float)src[min(e, n - 1)], scale);
    if (e < n) out[e] = val;
}

// (5) coordinate map: grid (ceil(H W / (256 V)), B), V pixels per thread
template <int V>
__global__ __launch_bounds__(256) void tt_coordinate_map_kernel(const float* __restrict__ kinv, int H, int W, int HW, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e0 >= HW) return;                                           // (nothing is loaded per pixel; V divides H W)
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = kinv[b * 9 + i];
    float r[3][V];
    int x = (int)(e0 % W), y = (int)(e0 / W);
#pragma unroll
    for (int p = 0; p < V; ++p) {
        const float fx = __fmul_rn(__fdiv_rn((float)x, (float)W), 640.f), fy = __fmul_rn(__fdiv_rn((float)y, (float)H), 480.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c][p] = __fadd_rn(__fmaf_rn(k[3 * c + 1], fy, __fmul_rn(k[3 * c], fx)), k[3 * c + 2]);
        if (++x == W) { x = 0; ++y; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + ((long long)b * 3 + c) * HW + e0;
        if (V == 4) *reinterpret_cast<float4*>(o) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
        else o[0] = r[c][0];
    }
}

static inline bool tt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int tt_chunks(int H, int W) { return (int)(((long long)H * W + TT_CHUNK - 1) / TT_CHUNK); }

}  // namespace nps

static int64_t tt_workspace_bytes(int B, int nmax, int H, int W) {
    return (B > 0 && nmax > 0 && H > 0 && W > 0) ? (int64_t)B * nps::tt_chunks(H, W) * nmax * 3 * 4 : 0;
}

#define TT_CHECK_IMAGE(name, B, H, W)                                                                                                      \
    NPS_CHECK_ARG((B) >= 1 && (B) <= 65535 && (H) >= 1 && (W) >= 1 && (H) <= (1 << 19) && (W) <= (1 << 19) && (long long)(H) * (W) <= (1ll << 30), \
                  name ": bad dims (B=%d in 1..65535, H=%d, W=%d in 1..2^19, H W <= 2^30)", B, H, W)

extern "C" int nopesac_label_ids(const int32_t* labels, int B, int H, int W, int nmax_limit, int32_t* ids, int32_t* n_all, int32_t* n, int32_t* bad,
                                 void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(labels, "label_ids: null input");
    NPS_CHECK_ARG(ids && n_all && n && bad, "label_ids: null output");
    TT_CHECK_IMAGE("label_ids", B, H, W);
    NPS_CHECK_ARG(nmax_limit >= 1 && nmax_limit <= TT_IDS, "label_ids: nmax_limit=%d outside 1..%d", nmax_limit, TT_IDS);
    NPS_CHECK_ARG(((uintptr_t)labels & 3) == 0, "label_ids: labels not 4-byte aligned");
    const int HW = H * W, vec4 = (HW % 4 == 0 && tt_aligned16(labels)) ? 1 : 0;
    hipLaunchKernelGGL(tt_label_ids_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, labels, HW, vec4, nmax_limit, ids, n_all, n, bad);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_label_targets_workspace_bytes(int B, int nmax, int H, int W, int64_t* bytes) {
    NPS_CHECK_ARG(bytes, "label_targets_workspace_bytes: null result pointer");
    *bytes = tt_workspace_bytes(B, nmax, H, W);
    return 0;
}

extern "C" int nopesac_label_targets(const int32_t* labels, const int32_t* ids, const int32_t* n, int B, int nmax, int H, int W, uint8_t* masks,
                                     float* plane_centers, float* pixel_centers, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(labels && ids && n, "label_targets: null input");
    NPS_CHECK_ARG(masks && plane_centers && pixel_centers, "label_targets: null output");
    TT_CHECK_IMAGE("label_targets", B, H, W);
    NPS_CHECK_ARG(nmax >= 1 && nmax <= TT_MAXT, "label_targets: nmax=%d outside 1..%d", nmax, TT_MAXT);
    NPS_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= tt_workspace_bytes(B, nmax, H, W),
                  "label_targets: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)tt_workspace_bytes(B, nmax, H, W));
    NPS_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)pixel_centers & 3) == 0, "label_targets: a 4-byte buffer is not 4-byte aligned");
    const int HW = H * W, chunks = tt_chunks(H, W);
    const int vec4 = (HW % 4 == 0 && tt_aligned16(labels)) ? 1 : 0;
    const int wide = (HW % 16 == 0 && tt_aligned16(masks) && tt_aligned16(pixel_centers)) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tt_label_sums_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, st, labels, ids, n, nmax, W, HW, vec4, (uint32_t*)workspace);
    hipLaunchKernelGGL(tt_label_centers_kernel, dim3((unsigned)nmax, (unsigned)B), dim3(64), 0, st, (const uint32_t*)workspace, n, nmax, chunks, H, W, plane_centers);
    hipLaunchKernelGGL(tt_label_masks_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, st, labels, ids, n, nmax, HW, vec4, wide,
                       (const float*)plane_centers, masks, pixel_centers);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_bits_to_masks(const int32_t* bits, int64_t n_rows, const int64_t* offsets, int B, int nmax, int H, int W, uint8_t* masks,
                                     void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(offsets && (bits || n_rows == 0) && n_rows >= 0, "bits_to_masks: null input");
    NPS_CHECK_ARG(masks, "bits_to_masks: null output");
    TT_CHECK_IMAGE("bits_to_masks", B, H, W);
    NPS_CHECK_ARG(nmax >= 1 && nmax <= TT_MAXT, "bits_to_masks: nmax=%d outside 1..%d", nmax, TT_MAXT);
    const int HW = H * W, wide = (HW % 16 == 0 && tt_aligned16(masks)) ? 1 : 0;
    hipLaunchKernelGGL(tt_bits_to_masks_kernel, dim3((unsigned)tt_chunks(H, W), (unsigned)nmax, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)bits, (long long)n_rows, (const long long*)offsets, nmax, H, W, HW, (HW + 31) / 32, wide, masks);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_depth_u16_to_f32(const uint16_t* src, int64_t n, float scale, float* out, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(src, "depth_u16_to_f32: null input");
    NPS_CHECK_ARG(out, "depth_u16_to_f32: null output");
    NPS_CHECK_ARG(n >= 1 && n <= (1ll << 31), "depth_u16_to_f32: n=%lld outside 1..2^31", (long long)n);
    NPS_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "depth_u16_to_f32: scale %g is not a positive finite number", (double)scale);
    NPS_CHECK_ARG(((uintptr_t)src & 1) == 0 && ((uintptr_t)out & 3) == 0, "depth_u16_to_f32: a buffer is not aligned to its element");
    const long long groups = (tt_aligned16(src) && tt_aligned16(out)) ? n / 8 : 0, threads = groups + (n - 8 * groups);
    hipLaunchKernelGGL(tt_depth_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (long long)n, groups, scale, out);
    NPS_LAUNCH_RET();
}

extern "C" int nopesac_coordinate_map(const float* kinv, int B, int H, int W, float* out, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(kinv, "coordinate_map: null input");
    NPS_CHECK_ARG(out, "coordinate_map: null output");
    TT_CHECK_IMAGE("coordinate_map", B, H, W);
    NPS_CHECK_ARG(((uintptr_t)out & 3) == 0, "coordinate_map: out not 4-byte aligned");
    const int HW = H * W;
    if (HW % 4 == 0 && tt_aligned16(out))
        hipLaunchKernelGGL(tt_coordinate_map_kernel<4>, dim3((unsigned)((HW / 4 + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, kinv, H, W, HW, out);
    else
        hipLaunchKernelGGL(tt_coordinate_map_kernel<1>, dim3((unsigned)((HW + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, kinv, H, W, HW, out);
    NPS_LAUNCH_RET();
}
