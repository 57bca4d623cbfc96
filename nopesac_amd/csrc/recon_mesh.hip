// The two-view reconstruction as textured meshes (the reference's vis_NopeSAC.py save_pair_objects: merge_plane_params_from_local_params,
// the dense route of utils/vis.py get_single_image_mesh(reduce_size=False) + get_pcd, utils/mesh_utils.py transform_meshes).  Three
// kernels: the merged plane parameters of a pair (float64, a workgroup per pair, on the rules of two_view.h, shared with
// recon_eval.hip), the vertex / face counts of every instance, and the fill that writes vertices, texture coordinates and triangles
// at offsets the host scanned from the counts.
//
// Ragged quantities use exclusive-offset arrays (int64 [n + 1]) as in plane_eval.hip; pair i owns views 2 i and 2 i + 1 of the view
// arrays.  Masks come bit-packed in the layout of nopesac_rle_runs_to_bits (column-major: bit p & 31 of word p >> 5, p = x H + y).
// Deterministic, without atomics, each output written once.
#include "two_view.h"

namespace nps {

constexpr int RM_T = 256;                          // threads of the count and fill workgroups
constexpr int RM_WAVES = RM_T / 64;

// get_plane_params_in_local: the point a + b - (a . b / |b|^2) b of the plane b seen from the camera at a, turned back by q^-1 and
// flipped.
__device__ __forceinline__ void rm_local(const double b[3], const double cam[7], double* __restrict__ out) {
    const double ax = cam[0], ay = cam[1], az = cam[2];
    const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double s = (ax * b[0] + ay * b[1] + az * b[2]) / (nb * nb);
    const double wx = ax + b[0] - s * b[0], wy = ay + b[1] - s * b[1], wz = az + b[2] - s * b[2];
    const double qi[4] = {cam[3], -cam[4], -cam[5], -cam[6]};                  // the inverse turns the other way; |q|^2 drops out
    double r[3];
    tv_rotate(qi, wx - ax, wy - ay, wz - az, r);
    out[0] = r[0]; out[1] = -r[1]; out[2] = -r[2];
}

// One workgroup (a wave) per pair.  The correspondence list becomes per-plane match tables in LDS (tv_match_mark / _verify); a `bad`
// pair writes nothing but the flag.  A pair without correspondences keeps its planes as they are (the reference merges only when the
// list is not empty).  Otherwise every plane goes to the common frame (tv_global_plane: view 0 through the camera, view 1 through the
// identity), a correspondence (a, b) replaces both planes by tv_merged_normal times the mean offset, and every plane, matched or not,
// comes back through get_plane_params_in_local.
__global__ __launch_bounds__(64) void recon_mesh_merge_kernel(const float* __restrict__ planes, const long long* __restrict__ view_off,
                                                              const double* __restrict__ cams, const int* __restrict__ corr,
                                                              const long long* __restrict__ corr_off, long long total,
                                                              double* __restrict__ out, int* __restrict__ bad) {
    __shared__ int s_m[2][TV_MAXN];
    __shared__ int s_bad;
    const int i = blockIdx.x, tid = threadIdx.x;
    const long long v0 = view_off[2 * i], v1 = view_off[2 * i + 1], n0l = v1 - v0, n1l = view_off[2 * i + 2] - v1;
    const long long c0 = corr_off[i], ncl = corr_off[i + 1] - c0;
    const bool fits = v0 >= 0 && n0l >= 0 && n0l <= TV_MAXN && n1l >= 0 && n1l <= TV_MAXN && v1 + n1l <= total && c0 >= 0 && ncl >= 0 &&
                      ncl <= (n0l < n1l ? n0l : n1l);
    if (!fits) {                                                                // (uniform: before any barrier)
        if (tid == 0) bad[i] = 1;
        return;
    }
    const int n0 = (int)n0l, n1 = (int)n1l, nc = (int)ncl;
    const int* pc = corr + 2 * c0;
    for (int k = tid; k < 2 * TV_MAXN; k += 64) (&s_m[0][0])[k] = -1;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    tv_match_mark<TV_MAXN>(tid, 64, pc, nc, n0, n1, s_m, s_bad);
    __syncthreads();
    tv_match_verify<TV_MAXN>(tid, 64, pc, nc, n0, n1, s_m, s_bad);
    __syncthreads();
    if (s_bad) {                                                                // (uniform)
        if (tid == 0) bad[i] = 1;
        return;
    }
    double cam0[7];
    const double ident[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 7; ++k) cam0[k] = cams[7 * (long long)i + k];
    for (int e = tid; e < n0 + n1; e += 64) {
        const int v = e >= n0 ? 1 : 0, k = v ? e - n0 : e;
        const float* p = planes + 3 * ((v ? v1 : v0) + k);
        double* o = out + 3 * ((v ? v1 : v0) + k);
        if (nc == 0) {
            o[0] = (double)p[0]; o[1] = (double)p[1]; o[2] = (double)p[2];
            continue;
        }
        double g[3], off, n[3];
        tv_global_plane(p, cam0, v == 1, g, off, n);
        const int c = s_m[v][k];
        if (c >= 0) {                                                           // both sides compute the same merged plane
            const int other = v ? pc[2 * c] : pc[2 * c + 1];
            double g2[3], off2, n2[3], m[3];
            tv_global_plane(planes + 3 * ((v ? v0 : v1) + other), cam0, v == 0, g2, off2, n2);
            tv_merged_normal(v ? n2 : n, v ? n : n2, m);                        // view 0's normal, view 1's
            const double mean = ((v ? off2 : off) + (v ? off : off2)) / 2.0;
            g[0] = m[0] * mean; g[1] = m[1] * mean; g[2] = m[2] * mean;
        }
        rm_local(g, v ? ident : cam0, o);
    }
    if (tid == 0) bad[i] = 0;
}

// ---- the strided mask of one instance, row-major in LDS --------------------------------------------------------------------------
// ms[ys][xs] = m[ys s][xs s], Hs = ceil(H / s) rows of RW = ceil(Ws / 32) words (bit xs & 31 of word xs >> 5; the bits past Ws are
// zero), row stride RS = RW | 1 words (odd: threads that walk down a column of words hit different banks).  Behind the rows two
// exclusive row prefixes of Hs + 1 ints each: vertices (set pixels) and faces.
struct RmShape {
    int H, W, s, Hs, Ws, RW, RS;
};

__host__ __device__ inline RmShape rm_shape(int H, int W, int s) {
    RmShape q;
    q.H = H; q.W = W; q.s = s;
    q.Hs = (H + s - 1) / s; q.Ws = (W + s - 1) / s;
    q.RW = (q.Ws + 31) / 32; q.RS = q.RW | 1;
    return q;
}

__host__ __device__ inline long long rm_lds_words(const RmShape& q) { return (long long)q.Hs * q.RS + 2LL * (q.Hs + 1); }

__device__ __forceinline__ unsigned rm_word(const unsigned* __restrict__ m, const RmShape& q, int ys, int w) {
    return (ys < q.Hs && w < q.RW) ? m[ys * q.RS + w] : 0u;
}

// The 64 pixels of row ys from word w on, as a 64-bit mask, and the same row one pixel to the right.
__device__ __forceinline__ void rm_chunk(const unsigned* __restrict__ m, const RmShape& q, int ys, int w, unsigned long long& cur,
                                         unsigned long long& right) {
    cur = (unsigned long long)rm_word(m, q, ys, w) | ((unsigned long long)rm_word(m, q, ys, w + 1) << 32);
    right = (cur >> 1) | ((unsigned long long)(rm_word(m, q, ys, w + 2) & 1u) << 63);
}

// Stage and transpose: a thread per LDS word gathers its 32 pixels from the column-major bits (threads that follow each other take
// rows that follow each other, so a wave reads a few neighbouring words per step).  Then a thread per row counts the row's vertices
// and faces - upper triangle of (y, x): (y, x), (y, x + 1), (y + 1, x + 1) set; lower: (y, x), (y + 1, x), (y + 1, x + 1) set - and
// wave 0 scans the rows, 64 at a time.
__device__ __forceinline__ void rm_stage(const unsigned* __restrict__ bits, const RmShape& q, unsigned* __restrict__ m, int* __restrict__ vrow,
                                         int* __restrict__ frow) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < q.Hs * q.RW; idx += RM_T) {
        const int ys = idx % q.Hs, w = idx / q.Hs;
        unsigned word = 0u;
        for (int j = 0; j < 32; ++j) {
            const int xs = 32 * w + j;
            if (xs < q.Ws) {
                const long long p = (long long)xs * q.s * q.H + (long long)ys * q.s;      // < H W
                word |= ((bits[p >> 5] >> (p & 31)) & 1u) << j;
            }
        }
        m[ys * q.RS + w] = word;
    }
    __syncthreads();
    for (int ys = tid; ys < q.Hs; ys += RM_T) {
        int nv = 0, nf = 0;
        for (int w = 0; w < q.RW; ++w) {
            const unsigned cur = m[ys * q.RS + w], bel = rm_word(m, q, ys + 1, w);
            const unsigned curR = (cur >> 1) | (rm_word(m, q, ys, w + 1) << 31), belR = (bel >> 1) | (rm_word(m, q, ys + 1, w + 1) << 31);
            nv += __popc(cur);
            nf += __popc(cur & curR & belR) + __popc(cur & bel & belR);
        }
        vrow[ys + 1] = nv; frow[ys + 1] = nf;
    }
    __syncthreads();
    if (tid < 64) {
        int cv = 0, cf = 0;
        for (int r0 = 0; r0 < q.Hs; r0 += 64) {
            const int r = r0 + tid;
            int a = r < q.Hs ? vrow[r + 1] : 0, b = r < q.Hs ? frow[r + 1] : 0;
            for (int d = 1; d < 64; d <<= 1) {
                const int ua = __shfl_up(a, d, 64), ub = __shfl_up(b, d, 64);
                if (tid >= d) { a += ua; b += ub; }
            }
            if (r < q.Hs) { vrow[r + 1] = cv + a; frow[r + 1] = cf + b; }
            cv += __shfl(a, 63, 64); cf += __shfl(b, 63, 64);
        }
        if (tid == 0) { vrow[0] = 0; frow[0] = 0; }
    }
    __syncthreads();
}

// A workgroup per instance: its vertex and face count.
__global__ __launch_bounds__(RM_T) void recon_mesh_count_kernel(const unsigned* __restrict__ bits, long long words, int H, int W, int s,
                                                                int* __restrict__ n_vert, int* __restrict__ n_face) {
    extern __shared__ unsigned rm_lds[];
    const RmShape q = rm_shape(H, W, s);
    unsigned* m = rm_lds;
    int* vrow = (int*)(rm_lds + q.Hs * q.RS);
    int* frow = vrow + q.Hs + 1;
    const int i = blockIdx.x;
    rm_stage(bits + (long long)i * words, q, m, vrow, frow);
    if (threadIdx.x == 0) { n_vert[i] = vrow[q.Hs]; n_face[i] = frow[q.Hs]; }
}

// A workgroup per instance.  The mask is staged and scanned as in the count; an instance whose totals differ from the range the
// offsets give it (or whose view index is out of range) sets bad[i] and writes nothing else.  Then every wave walks a contiguous
// block of rows, 64 pixels at a time, with three running ranks - vertices of this row, vertices of the next row, faces - so that a
// lane's rank is the running value plus a popcount of the lower lanes: set pixels that follow each other write addresses that follow
// each other, and every rank is below the counted total.
//   vertex (get_pcd):  ray = K^-1 [x, y, 1], depth = |p| / ((p / |p|) . ray), v = depth ray - plain IEEE, a grazing or back-facing
//   plane gives what the formula gives; then (transform_meshes) v * [1, -1, -1] turned by the view's camera quaternion, plus its
//   position.  uv = (x / W, 1 - y / H).  x = xs s, y = ys s.  Float64 arithmetic, f32 stores.
//   faces of vertex (y, x), local ids:  [id(y, x), id(y + 1, x + 1), id(y, x + 1)], then [id(y, x), id(y + 1, x), id(y + 1, x + 1)].
__global__ __launch_bounds__(RM_T) void recon_mesh_fill_kernel(const unsigned* __restrict__ bits, long long words, int H, int W, int s,
                                                               const double* __restrict__ planes, const int* __restrict__ inst_view,
                                                               int n_views, const double* __restrict__ kinv, const double* __restrict__ cams,
                                                               const long long* __restrict__ vert_off, const long long* __restrict__ face_off,
                                                               long long n_verts, long long n_faces, float* __restrict__ verts,
                                                               float* __restrict__ uvs, int* __restrict__ faces, int* __restrict__ bad) {
    extern __shared__ unsigned rm_lds[];
    const RmShape q = rm_shape(H, W, s);
    unsigned* m = rm_lds;
    int* vrow = (int*)(rm_lds + q.Hs * q.RS);
    int* frow = vrow + q.Hs + 1;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    rm_stage(bits + (long long)i * words, q, m, vrow, frow);
    const long long vo = vert_off[i], fo = face_off[i];
    const int view = inst_view[i];
    const bool ok = vo >= 0 && fo >= 0 && vert_off[i + 1] - vo == vrow[q.Hs] && face_off[i + 1] - fo == frow[q.Hs] &&
                    vert_off[i + 1] <= n_verts && face_off[i + 1] <= n_faces && view >= 0 && view < n_views;
    if (!ok) {                                                                  // (uniform)
        if (tid == 0) bad[i] = 1;
        return;
    }
    if (tid == 0) bad[i] = 0;
    const double px = planes[3 * (long long)i], py = planes[3 * (long long)i + 1], pz = planes[3 * (long long)i + 2];
    const double off = sqrt(px * px + py * py + pz * pz);
    const double nx = px / off, ny = py / off, nz = pz / off;
    double ki[9], cam[7];
    for (int k = 0; k < 9; ++k) ki[k] = kinv[9 * (long long)view + k];
    for (int k = 0; k < 7; ++k) cam[k] = cams[7 * (long long)view + k];
    float* vout = verts + 3 * vo;
    float* tout = uvs + 2 * vo;
    int* fout = faces + 3 * fo;
    const unsigned long long lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);
    const int per = (q.Hs + RM_WAVES - 1) / RM_WAVES;
    const int r1 = min(q.Hs, (wave + 1) * per);
    for (int ys = wave * per; ys < r1; ++ys) {
        int vrun = vrow[ys], nrun = vrow[ys + 1], frun = frow[ys];              // (nrun: the first id of row ys + 1)
        for (int w = 0; w < q.RW; w += 2) {
            unsigned long long cur, curR, bel, belR;
            rm_chunk(m, q, ys, w, cur, curR);
            rm_chunk(m, q, ys + 1, w, bel, belR);
            const unsigned long long up = cur & curR & belR, lo = cur & bel & belR;
            if ((cur >> lane) & 1ull) {
                const int id = vrun + __popcll(cur & lt);
                const double x = (double)((32 * w + lane) * s), y = (double)(ys * s);
                const double rx = ki[0] * x + ki[1] * y + ki[2], ry = ki[3] * x + ki[4] * y + ki[5], rz = ki[6] * x + ki[7] * y + ki[8];
                const double depth = off / (nx * rx + ny * ry + nz * rz);
                double r[3];
                tv_rotate(cam + 3, depth * rx, -(depth * ry), -(depth * rz), r);
                vout[3 * (long long)id] = (float)(r[0] + cam[0]);
                vout[3 * (long long)id + 1] = (float)(r[1] + cam[1]);
                vout[3 * (long long)id + 2] = (float)(r[2] + cam[2]);
                tout[2 * (long long)id] = (float)(x / (double)W);
                tout[2 * (long long)id + 1] = (float)(1.0 - y / (double)H);
                const int below = nrun + __popcll(bel & lt), diag = nrun + __popcll(bel & le);      // id(y + 1, x), id(y + 1, x + 1)
                int f = frun + __popcll(up & lt) + __popcll(lo & lt);
                if ((up >> lane) & 1ull) {
                    fout[3 * (long long)f] = id; fout[3 * (long long)f + 1] = diag; fout[3 * (long long)f + 2] = id + 1;
                    ++f;
                }
                if ((lo >> lane) & 1ull) {
                    fout[3 * (long long)f] = id; fout[3 * (long long)f + 1] = below; fout[3 * (long long)f + 2] = diag;
                }
            }
            vrun += __popcll(cur); nrun += __popcll(bel); frun += __popcll(up) + __popcll(lo);
        }
    }
}

static bool rm_mask_fits(int H, int W, int stride) {
    return rm_lds_words(rm_shape(H, W, stride)) <= (long long)NPS_MESH_LDS_WORDS;
}

}  // namespace nps

#define RM_CHECK_MASK(name)                                                                                                          \
    NPS_CHECK_ARG(n >= 0, name ": n < 0");                                                                                            \
    NPS_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffdfLL, name ": H, W > 0 and H W < 2^31 - 32");                         \
    NPS_CHECK_ARG(stride >= 1, name ": stride >= 1 (got %d)", stride);                                                                \
    NPS_CHECK_ARG(rm_mask_fits(H, W, stride),                                                                                         \
                  name ": a %d x %d mask at stride %d needs %lld LDS words, NPS_MESH_LDS_WORDS is %d", H, W, stride,                  \
                  rm_lds_words(rm_shape(H, W, stride)), (int)NPS_MESH_LDS_WORDS)

extern "C" nps_status nopesac_recon_mesh_merge(const float* planes, const int64_t* view_off, const double* cams, const int32_t* corr,
                                               const int64_t* corr_off, int P, int max_n, int64_t total, double* merged, int32_t* bad,
                                               void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(P >= 0 && total >= 0, "recon_mesh_merge: P < 0 or total < 0");
    NPS_CHECK_ARG(max_n >= 0 && max_n <= TV_MAXN, "recon_mesh_merge: at most %d planes per view (got %d)", TV_MAXN, max_n);
    if (P == 0) return 0;
    NPS_CHECK_ARG(view_off && cams && corr_off && bad, "recon_mesh_merge: null pointer");
    NPS_CHECK_ARG(total == 0 || (planes && merged), "recon_mesh_merge: null pointer (planes)");
    hipLaunchKernelGGL(recon_mesh_merge_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, planes, (const long long*)view_off, cams, corr,
                       (const long long*)corr_off, (long long)total, merged, bad);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_recon_mesh_count(const uint32_t* bits, int n, int H, int W, int stride, int32_t* n_vert, int32_t* n_face,
                                               void* stream) {
    using namespace nps;
    RM_CHECK_MASK("recon_mesh_count");
    if (n == 0) return 0;
    NPS_CHECK_ARG(bits && n_vert && n_face, "recon_mesh_count: null pointer");
    const RmShape q = rm_shape(H, W, stride);
    hipLaunchKernelGGL(recon_mesh_count_kernel, dim3(n), dim3(RM_T), (size_t)rm_lds_words(q) * 4, (hipStream_t)stream, bits,
                       ((long long)H * W + 31) / 32, H, W, stride, n_vert, n_face);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_recon_mesh_fill(const uint32_t* bits, int n, int H, int W, int stride, const double* planes,
                                              const int32_t* inst_view, int n_views, const double* kinv, const double* cams,
                                              const int64_t* vert_off, const int64_t* face_off, int64_t n_verts, int64_t n_faces, float* verts,
                                              float* uvs, int32_t* faces, int32_t* bad, void* stream) {
    using namespace nps;
    RM_CHECK_MASK("recon_mesh_fill");
    NPS_CHECK_ARG(n_views >= 0 && n_verts >= 0 && n_faces >= 0, "recon_mesh_fill: n_views, n_verts or n_faces < 0");
    if (n == 0) return 0;
    NPS_CHECK_ARG(bits && planes && inst_view && kinv && cams && vert_off && face_off && bad, "recon_mesh_fill: null pointer");
    NPS_CHECK_ARG(n_verts == 0 || (verts && uvs), "recon_mesh_fill: null pointer (vertices)");
    NPS_CHECK_ARG(n_faces == 0 || faces, "recon_mesh_fill: null pointer (faces)");
    const RmShape q = rm_shape(H, W, stride);
    hipLaunchKernelGGL(recon_mesh_fill_kernel, dim3(n), dim3(RM_T), (size_t)rm_lds_words(q) * 4, (hipStream_t)stream, bits,
                       ((long long)H * W + 31) / 32, H, W, stride, planes, inst_view, n_views, kinv, cams, (const long long*)vert_off,
                       (const long long*)face_off, (long long)n_verts, (long long)n_faces, verts, uvs, faces, bad);
    NPS_LAUNCH_RET();
}
