// Plane AP evaluator on the device (the reference's evaluate_for_planes, evaluation/mp3d_evaluation.py:467-743, and the
// pycocotools.mask.iou it calls): compressed COCO RLE strings -> run lengths -> bit-packed masks -> pairwise IoU by popcount ->
// score-ordered true-positive assignment for the four AP criteria with the plane-parameter errors (utils/metrics.py:6-24).
//
// Ragged quantities use exclusive-offset arrays (int64 [n + 1]), so one launch serves every view of a batch.  Pixel order is COCO's
// column-major scan p = x H + y; bit p of a mask is bit (p & 31) of word (p >> 5); a mask has ceil(H W / 32) words and the unused
// high bits of its last word are zero.  Every kernel is deterministic: integer counts, no atomics, each output written once.
// Polygon annotations reach the same bit-packed form through poly_to_bits_kernel (below; deterministic too, its atomics are XOR on words).
#include "common.h"

namespace nps {

constexpr int PE_T = 256;                      // threads of the per-mask workgroups (4 waves)

// Exclusive scan of one value per thread over a 256-thread workgroup; `total` = the workgroup's sum.  Two barriers.
template <typename T>
__device__ __forceinline__ T pe_block_excl(T v, T* wave_tot, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __syncthreads();                           // the previous use of wave_tot has been read
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T wbase = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PE_T / 64; ++w) {
        const T t = wave_tot[w];
        if (w < wave) wbase += t;
        total += t;
    }
    return wbase + incl - v;
}

// ---- cocoapi rleFrString: one workgroup per mask ---------------------------------------------------------------------------------
// A character carries 5 data bits and a continuation bit (after subtracting 48); a number ends at a character without the
// continuation bit and is sign-extended from bit 4 of that character; from the fourth number on the value is a difference to the
// number two places before.  Pass 1 scans the end marks, which gives every number its index, and leaves the position of number j's
// last character in runs[j] (a mask has at most as many numbers as bytes, so its slice of `runs` holds them).  Pass 2 takes 256
// numbers at a time: assembles the raw values, then undoes the delta coding with two interleaved prefix sums (even and odd
// indices) that carry their running totals from chunk to chunk.  Characters behind the last end mark (a cut string) are ignored.
__global__ __launch_bounds__(PE_T) void rle_string_runs_kernel(const uint8_t* __restrict__ bytes, const long long* __restrict__ str_off,
                                                               int* __restrict__ runs, int* __restrict__ n_runs) {
    __shared__ int wave_tot[PE_T / 64];
    __shared__ int par_tot[PE_T / 64][2];
    __shared__ int carry_end;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b0 = str_off[i], L64 = str_off[i + 1] - b0;
    const int L = L64 < 0 ? 0 : (L64 > 0x7fffffffLL ? 0x7fffffff : (int)L64);
    const uint8_t* s = bytes + b0;
    int* out = runs + b0;
    int n = 0;
    for (int k0 = 0; k0 < L; k0 += PE_T) {
        const int k = k0 + tid;
        const int end = (k < L && !((s[k] - 48) & 0x20)) ? 1 : 0;
        int total;
        const int idx = n + pe_block_excl(end, wave_tot, total);
        if (end) out[idx] = k;
        n += total;
    }
    if (tid == 0) n_runs[i] = n;
    __syncthreads();                           // the end positions are in memory for the whole workgroup
    int base_par[2] = {0, 0};                  // running sums of the even / odd chain (out[2] and out[1] seed them)
    for (int j0 = 0; j0 < n; j0 += PE_T) {     // PE_T is even: a thread's parity is the number's parity
        const int j = j0 + tid;
        long long x = 0;
        int e = -1;
        if (j < n) {
            e = out[j];
            const int st = j == 0 ? 0 : (tid == 0 ? carry_end : out[j - 1]) + 1;
            int k = 0;
            for (int c = st; c <= e; ++c, ++k) {
                const long long ch = (long long)s[c] - 48;
                if (k < 12) x |= (ch & 0x1f) << (5 * k);
                if (c == e && (ch & 0x10) && k < 12) x |= (long long)(~0ULL << (5 * (k + 1)));
            }
        }
        __syncthreads();                       // every end position of this chunk has been read: the slots may take the values
        if (tid == PE_T - 1) carry_end = e;
        // chains: out[j] = sum of the raw values of j's parity from index 1 (odd) or 2 (even) up to j; out[0] stands alone
        int v = (j < n && j > 0) ? (int)x : 0, incl = v;
#pragma unroll
        for (int d = 2; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane >= 62) par_tot[wave][lane & 1] = incl;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PE_T / 64; ++w) {
            const int t = par_tot[w][tid & 1];
            if (w < wave) wbase += t;
            total += t;
        }
        if (j < n) out[j] = j == 0 ? (int)x : base_par[tid & 1] + wbase + incl;
        base_par[tid & 1] += total;
        __syncthreads();                       // par_tot and carry_end are free for the next chunk
    }
}

// ---- run lengths -> bit-packed mask: one workgroup per mask ---------------------------------------------------------------------
// Pass 1: prefix sums of the runs (64-bit, 8 runs per thread and step) give every run its first pixel (`starts`, scratch laid out
// like `runs`), the area (odd runs are ones) and the verdict: a negative run, a running sum beyond N or a total other than N make
// the mask bad.  Pass 2: a thread owns whole words; it finds the run that holds the word's first pixel by binary search (the last
// run that starts at or before it: zero-length runs share a start) and walks runs until the word is full.  A bad mask gets zero words.
constexpr int PE_RPT = 8;
__global__ __launch_bounds__(PE_T) void rle_runs_to_bits_kernel(const int* __restrict__ runs, const long long* __restrict__ run_off,
                                                                const int* __restrict__ n_runs, int N, int words, int* __restrict__ starts,
                                                                uint32_t* __restrict__ bits, int* __restrict__ area, int* __restrict__ bad) {
    __shared__ long long wave_tot[PE_T / 64];
    __shared__ int any_bad[PE_T / 64];
    __shared__ long long area_w[PE_T / 64];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = run_off[i], room = run_off[i + 1] - r0;
    const int n = n_runs[i];
    const int* rn = runs + r0;
    int* st = starts + r0;
    uint32_t* bw = bits + (long long)i * words;
    int is_bad = (n < 0 || (long long)n > room) ? 1 : 0;          // a count that does not fit its slice: nothing of it is read
    const int nn = is_bad ? 0 : n;
    long long base = 0, ones = 0;
    for (int j0 = 0; j0 < nn; j0 += PE_T * PE_RPT) {
        const int j = j0 + tid * PE_RPT;
        int r[PE_RPT];
        long long mine = 0;
#pragma unroll
        for (int e = 0; e < PE_RPT; ++e) {
            r[e] = j + e < nn ? rn[j + e] : 0;
            if (r[e] < 0) is_bad = 1;
            mine += r[e];
        }
        long long total;
        long long pos = base + pe_block_excl(mine, wave_tot, total);
#pragma unroll
        for (int e = 0; e < PE_RPT; ++e) {
            if (j + e < nn) {
                st[j + e] = (int)(pos < 0 ? 0 : (pos > N ? N : pos));
                pos += r[e];
                if (pos > N) is_bad = 1;                                   // the running sum passes N
                if ((j + e) & 1) ones += r[e];
            }
        }
        base += total;
    }
    if (base != N) is_bad = 1;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        is_bad |= __shfl_xor(is_bad, d, 64);
        ones += __shfl_xor(ones, d, 64);
    }
    if (lane == 0) { any_bad[wave] = is_bad; area_w[wave] = ones; }
    __syncthreads();                           // also: `starts` is in memory for the whole workgroup
    is_bad = 0; ones = 0;
#pragma unroll
    for (int w = 0; w < PE_T / 64; ++w) { is_bad |= any_bad[w]; ones += area_w[w]; }
    if (tid == 0) { bad[i] = is_bad; area[i] = is_bad ? 0 : (int)ones; }
    for (int w = tid; w < words; w += PE_T) {
        uint32_t m = 0;
        if (!is_bad) {
            const int p0 = w * 32, pe = min(p0 + 32, N);
            int lo = 0, hi = nn;                                           // last run with st[run] <= p0 (st[0] = 0 <= p0)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (st[mid] <= p0) lo = mid; else hi = mid;
            }
            int run = lo, pos = p0;
            while (pos < pe && run < nn) {
                const int run_end = st[run] + rn[run], e = min(run_end, pe);
                if ((run & 1) && e > pos) {
                    const int len = e - pos;
                    m |= (len >= 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << (pos - p0);
                }
                pos = max(pos, e);
                if (run_end <= pe) ++run;
            }
        }
        bw[w] = m;
    }
}

// ---- pairwise IoU by popcount ---------------------------------------------------------------------------------------------------------
// A workgroup takes one view, a block of 16 predictions and a block of 8 GT masks (and strides over further blocks when the grid is
// smaller than the view).  The GT words travel through LDS 512 words per mask at a time, so a GT word leaves memory once per 16
// predictions; a wave owns 4 predictions, a lane the words lane, lane + 64, ... of the staged piece, and keeps 4 x 8 integer counts,
// which are added up across the wave at the end.  inter is exact, so iou = inter / union is the float64 quotient of two integers.
constexpr int IOU_PB = 16, IOU_GB = 8, IOU_CH = 512;
__global__ __launch_bounds__(256) void mask_iou_bits_kernel(const uint32_t* __restrict__ dt_bits, const int* __restrict__ dt_area,
                                                            const long long* __restrict__ dt_off, const uint32_t* __restrict__ gt_bits,
                                                            const int* __restrict__ gt_area, const long long* __restrict__ gt_off,
                                                            const uint8_t* __restrict__ iscrowd, const long long* __restrict__ iou_off,
                                                            int words, double* __restrict__ iou, int* __restrict__ inter) {
    __shared__ uint32_t g_lds[IOU_GB][IOU_CH];
    const int v = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long d0 = dt_off[v], g0 = gt_off[v];
    const int n_dt = (int)(dt_off[v + 1] - d0), n_gt = (int)(gt_off[v + 1] - g0);
    if (n_dt <= 0 || n_gt <= 0) return;
    const long long o0 = iou_off[v];
    for (int db = blockIdx.x * IOU_PB; db < n_dt; db += gridDim.x * IOU_PB) {
        for (int gb = blockIdx.y * IOU_GB; gb < n_gt; gb += gridDim.y * IOU_GB) {
            int acc[4][IOU_GB];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int g = 0; g < IOU_GB; ++g) acc[a][g] = 0;
            const uint32_t* drow[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int di = db + wave * 4 + a;
                drow[a] = di < n_dt ? dt_bits + (d0 + di) * (long long)words : nullptr;
            }
            for (int c0 = 0; c0 < words; c0 += IOU_CH) {
                __syncthreads();               // the previous piece has been consumed
                for (int t = tid; t < IOU_GB * IOU_CH; t += 256) {
                    const int g = t / IOU_CH, c = t % IOU_CH;
                    g_lds[g][c] = (gb + g < n_gt && c0 + c < words) ? gt_bits[(g0 + gb + g) * (long long)words + c0 + c] : 0u;
                }
                __syncthreads();
#pragma unroll 2
                for (int c = lane; c < IOU_CH; c += 64) {
                    if (c0 + c >= words) break;
                    uint32_t dw[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) dw[a] = drow[a] ? drow[a][c0 + c] : 0u;
#pragma unroll
                    for (int g = 0; g < IOU_GB; ++g) {
                        const uint32_t gw = g_lds[g][c];
#pragma unroll
                        for (int a = 0; a < 4; ++a) acc[a][g] += __popc(dw[a] & gw);
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int g = 0; g < IOU_GB; ++g) {
                    int s = acc[a][g];
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
                    acc[a][g] = s;
                }
            if (lane < 4 * IOU_GB) {           // lane = a * 8 + g writes pair (a, g)
                const int a = lane / IOU_GB, g = lane % IOU_GB;
                int s = 0;
#pragma unroll
                for (int aa = 0; aa < 4; ++aa)
#pragma unroll
                    for (int gg = 0; gg < IOU_GB; ++gg) s = (aa == a && gg == g) ? acc[aa][gg] : s;
                const int di = db + wave * 4 + a, gj = gb + g;
                if (di < n_dt && gj < n_gt) {
                    const long long ad = dt_area[d0 + di], ag = gt_area[g0 + gj];
                    const long long uni = (iscrowd && iscrowd[g0 + gj]) ? ad : ad + ag - s;
                    const long long o = o0 + (long long)di * n_gt + gj;
                    iou[o] = uni > 0 ? (double)s / (double)uni : 0.0;
                    inter[o] = s;
                }
            }
        }
    }
}

// ---- true-positive assignment: one wave per view --------------------------------------------------------------------------------------
// The reference walks a view's predictions in descending score order and keeps four lists of GT ids already taken, one per
// criterion (mp3d_evaluation.py:570-649).  A GT id enters a criterion's list exactly when a prediction is a true positive for it, so
// a prediction is a true positive for criterion c iff its own conditions for c hold and no prediction BEFORE it in that order has
// the same GT id and conditions for c that hold too: the first such prediction takes the GT, all later ones find it taken.  That form
// has no carried state: every lane settles its two predictions (lane, lane + 64) against the table of all predictions in LDS.
// "Before" = higher score, or equal score and lower index (a stable descending order).
__global__ __launch_bounds__(64) void plane_ap_assign_kernel(const double* __restrict__ iou, const long long* __restrict__ iou_off,
                                                             const long long* __restrict__ dt_off, const long long* __restrict__ gt_off,
                                                             const float* __restrict__ score, const int* __restrict__ pred_label,
                                                             const float* __restrict__ pred_plane, const int* __restrict__ gt_label,
                                                             const float* __restrict__ gt_plane, double iou_thresh, double normal_thresh,
                                                             double offset_thresh, double* __restrict__ rows) {
    __shared__ float s_score[NPS_PLANE_MAX_QUERIES];
    __shared__ int s_gt[NPS_PLANE_MAX_QUERIES];
    __shared__ int s_cond[NPS_PLANE_MAX_QUERIES];
    const int v = blockIdx.x, lane = threadIdx.x;
    const long long d0 = dt_off[v], g0 = gt_off[v], o0 = iou_off[v];
    const long long nd64 = dt_off[v + 1] - d0, ng64 = gt_off[v + 1] - g0;
    if (nd64 <= 0 || nd64 > NPS_PLANE_MAX_QUERIES || ng64 < 0 || ng64 > 255) return;      // (the entry point refuses such a batch)
    const int n_dt = (int)nd64, n_gt = (int)ng64;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double best[2], nerr[2], oerr[2];
    int gid[2], cond[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        best[h] = 0.0; nerr[h] = nan; oerr[h] = nan; gid[h] = -1; cond[h] = 0;
        if (i < n_dt && n_gt > 0) {
            const double* row = iou + o0 + (long long)i * n_gt;
            double b = row[0];
            int g = 0;
            for (int j = 1; j < n_gt; ++j) {                               // first maximum
                const double x = row[j];
                if (x > b) { b = x; g = j; }
            }
            const float* pp = pred_plane + 3 * (d0 + i);
            const float* gp = gt_plane + 3 * (g0 + g);
            const double px = pp[0], py = pp[1], pz = pp[2], gx = gp[0], gy = gp[1], gz = gp[2];
            const double po = sqrt(px * px + py * py + pz * pz) + 1e-5, go = sqrt(gx * gx + gy * gy + gz * gz) + 1e-5;
            const double dx = px / po - gx / go, dy = py / po - gy / go, dz = pz / po - gz / go;
            double d = sqrt(dx * dx + dy * dy + dz * dz);
            d = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
            nerr[h] = 2.0 * asin(d / 2.0) / 3.14159265358979323846 * 180.0;
            oerr[h] = fabs(po - go);
            best[h] = b; gid[h] = g;
            if (pred_label[d0 + i] == gt_label[g0 + g] && b > iou_thresh) {
                const bool n_ok = nerr[h] < normal_thresh, o_ok = oerr[h] < offset_thresh;
                cond[h] = 1 | (n_ok && o_ok ? 2 : 0) | (n_ok ? 4 : 0) | (o_ok ? 8 : 0);      // mask, plane, normal, offset
            }
        }
        if (i < n_dt) { s_score[i] = score[d0 + i]; s_gt[i] = gid[h]; s_cond[i] = cond[h]; }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i >= n_dt) continue;
        const float sc = s_score[i];
        int taken = 0;
        for (int j = 0; j < n_dt; ++j) {
            const float sj = s_score[j];
            if ((sj > sc || (sj == sc && j < i)) && s_gt[j] == gid[h]) taken |= s_cond[j];
        }
        const int tp = cond[h] & ~taken;
        double* r = rows + (d0 + i) * (long long)NPS_PLANE_AP_COLS;
        r[0] = (double)sc; r[1] = (double)pred_label[d0 + i];
        r[2] = (double)(tp & 1); r[3] = (double)((tp >> 1) & 1); r[4] = (double)((tp >> 2) & 1); r[5] = (double)((tp >> 3) & 1);
        r[6] = nerr[h]; r[7] = oerr[h]; r[8] = best[h]; r[9] = (double)gid[h];
    }
}

// ---- COCO polygon lists -> bit-packed masks: one workgroup per mask ---------------------------------------------------------------
// cocoapi's rleFrPoly (maskApi.c) followed by rleMerge(intersect = 0), written in the layout of rle_runs_to_bits_kernel, so that GT
// masks annotated as polygons feed mask_iou_bits_kernel directly (the reference: mask_util.frPyObjects + merge, mp3d_evaluation.py:544-554).
// cocoapi upsamples a polygon by 5, walks every edge one upsampled unit at a time, turns every change of the upsampled x between
// two consecutive boundary points into a "crossing" at a flat position p = x H + y, SORTS the positions and differences them into
// runs.  The runs say: pixel q is set iff an odd number of crossings lie at or before q.  This kernel never sorts: it XORs every
// crossing into a toggle bitmap and takes the prefix parity of that bitmap along the flat bit order (shift-XOR inside a word, a
// scan of the words' popcount parities across words), then ORs the polygon into the mask.  Every per-point operation (the
// truncating casts, the separate multiply and add, the division by 5.0) is cocoapi's, one IEEE double operation at a time
// (-ffp-contract=off).  Integer results only; the atomics are XOR on words, which does not depend on order: two runs give the same bytes.
//
// One workgroup per mask.  Pass 0 checks the mask (offsets, vertex counts, finite and bounded coordinates, the point cap) before
// any point is generated.  Then per polygon: 256 edges at a time, the per-edge point counts are scanned so that threads take POINTS
// (not edges: a contour has hundreds of 6-point edges, a box four edges of thousands), each point forms the pair with its
// predecessor - across an edge junction the previous edge's last point, computed from the same formula, which is not always the
// vertex - and toggles its crossing; after a barrier one pass reads and clears the toggles, 256 words per step, and writes the words.
constexpr int PM_MAX_VERTS = 1 << 30;          // vertices of one polygon (the chunk loop counts in int)

// X = (int)(5 x + 0.5), cocoapi's upsampling (the cast truncates toward zero).  false: not finite, or beyond NPS_POLY_COORD_MAX.
__device__ __forceinline__ bool pm_upsample(double c, int& C) {
    const double r = 5.0 * c + 0.5;
    const bool ok = fabs(r) < (double)NPS_POLY_COORD_MAX;      // (false for NaN)
    C = (int)(ok ? r : 0.0);
    return ok;
}

__device__ __forceinline__ int pm_edge_len(int xs, int ys, int xe, int ye) { return max(abs(xe - xs), abs(ye - ys)); }

// The edge's slope along its longer axis, after cocoapi's flip; 0 for an edge of length 0 (cocoapi's 0 / 0 is never used).
__device__ __forceinline__ double pm_slope(int xs, int ys, int xe, int ye) {
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    const bool wide = dx >= dy;
    const bool flip = wide ? xs > xe : ys > ye;
    const int num = wide ? (flip ? ys - ye : ye - ys) : (flip ? xs - xe : xe - xs), den = wide ? dx : dy;
    return den ? (double)num / (double)den : 0.0;
}

// Point d (0 .. length) of the edge (xs, ys) -> (xe, ye), counted in the edge's own direction.
__device__ __forceinline__ void pm_point(int xs, int ys, int xe, int ye, double s, int d, int& u, int& v) {
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    const bool wide = dx >= dy;
    const bool flip = wide ? xs > xe : ys > ye;
    const int x0 = flip ? xe : xs, y0 = flip ? ye : ys, n = wide ? dx : dy;
    const int t = flip ? n - d : d;
    const double st = s * (double)t;
    const int c = (int)((double)(wide ? y0 : x0) + st + 0.5);
    u = n == 0 ? xs : (wide ? x0 + t : c);
    v = n == 0 ? ys : (wide ? c : y0 + t);
}

// Flat position of the crossing between a boundary point and its predecessor, or -1 when there is none.
__device__ __forceinline__ long long pm_crossing(int u, int v, int pu, int pv, int H, int W) {
    if (u == pu) return -1;
    double xd = (double)(u < pu ? u : u - 1);
    xd = (xd + 0.5) / 5.0 - 0.5;
    if (floor(xd) != xd || xd < 0.0 || xd > (double)(W - 1)) return -1;
    double yd = (double)(v < pv ? v : pv);
    yd = (yd + 0.5) / 5.0 - 0.5;
    yd = yd < 0.0 ? 0.0 : (yd > (double)H ? (double)H : yd);
    yd = ceil(yd);
    return (long long)(int)xd * H + (int)yd;
}

__global__ __launch_bounds__(PE_T) void poly_to_bits_kernel(const double* __restrict__ xy, const long long* __restrict__ poly_off,
                                                            const long long* __restrict__ mask_off, long long n_points, long long n_polys,
                                                            int H, int W, int N, int words, long long cap, uint32_t* __restrict__ toggles,
                                                            uint32_t* __restrict__ bits, int* __restrict__ area, int* __restrict__ bad) {
    // a chunk's vertices: slot s holds vertex j0 - 1 + s of the polygon; edge slot e joins vertex slots e and e + 1 (edge j0 - 1 + e)
    __shared__ int sX[PE_T + 2], sY[PE_T + 2];
    __shared__ double sS[PE_T + 1];
    __shared__ long long sStart[PE_T];
    __shared__ long long wave_ll[PE_T / 64];
    __shared__ int wave_i[2][PE_T / 64];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* tg = toggles + (long long)i * words;
    uint32_t* bw = bits + (long long)i * words;
    const long long m0 = mask_off[i], m1 = mask_off[i + 1];
    int is_bad = (m0 < 0 || m1 > n_polys || m1 <= m0) ? 1 : 0;            // (a mask without polygons is bad)
    const long long n_mine = is_bad ? 0 : m1 - m0;

    // ---- pass 0: nothing is generated for a mask that fails any check
    for (long long q = 0; q < n_mine; ++q) {
        const long long a = poly_off[m0 + q], b = poly_off[m0 + q + 1];
        if (a < 0 || b > n_points || b - a < 3 || b - a > PM_MAX_VERTS) {   // (the same for every thread)
            is_bad = 1;
            continue;
        }
        const int k = (int)(b - a);
        const double* p = xy + 2 * a;
        long long mine = 0;
        for (int j0 = 0; j0 < k; j0 += PE_T) {
            const int j = min(j0 + tid, k - 1), jn = j + 1 == k ? 0 : j + 1;
            const double x0 = p[2 * j], y0 = p[2 * j + 1], x1 = p[2 * jn], y1 = p[2 * jn + 1];
            int X0, Y0, X1, Y1;
            const bool ok0 = pm_upsample(x0, X0), ok1 = pm_upsample(y0, Y0), ok2 = pm_upsample(x1, X1), ok3 = pm_upsample(y1, Y1);
            if (!(ok0 && ok1 && ok2 && ok3)) is_bad = 1;
            mine += j0 + tid < k ? (long long)pm_edge_len(X0, Y0, X1, Y1) + 1 : 0;
        }
        long long total;
        pe_block_excl(mine, wave_ll, total);
        if (total > cap) is_bad = 1;
    }
    {
        const int any = __ballot(is_bad) != 0ull ? 1 : 0;
        __syncthreads();                       // wave_i is free
        if (lane == 0) wave_i[0][wave] = any;
        __syncthreads();
        is_bad = wave_i[0][0] | wave_i[0][1] | wave_i[0][2] | wave_i[0][3];
    }
    if (is_bad) {
        for (int w = tid; w < words; w += PE_T) bw[w] = 0u;
        if (tid == 0) { bad[i] = 1; area[i] = 0; }
        return;
    }
    for (int w = tid; w < words; w += PE_T) tg[w] = 0u;
    __threadfence();                           // the zeros have reached memory before another wave's XOR on the same word can

    int ones = 0;
    for (long long q = 0; q < n_mine; ++q) {
        const long long a = poly_off[m0 + q];
        const int k = (int)(poly_off[m0 + q + 1] - a);
        const double* p = xy + 2 * a;
        // ---- crossings of polygon q -> toggles
        for (int j0 = 0; j0 < k; j0 += PE_T) {
            __syncthreads();                   // the previous chunk's slots have been read; the toggle words are zero for everybody
            for (int s = tid; s < PE_T + 2; s += PE_T) {
                const int j = j0 - 1 + s, jj = (j < 0 || j >= k) ? 0 : j;      // vertex k is vertex 0; slots beyond it are not used
                pm_upsample(p[2 * jj], sX[s]);
                pm_upsample(p[2 * jj + 1], sY[s]);
            }
            __syncthreads();
            const int n_edges = min(PE_T, k - j0);
            for (int e = tid; e < PE_T + 1; e += PE_T) sS[e] = pm_slope(sX[e], sY[e], sX[e + 1], sY[e + 1]);
            const long long cnt = tid < n_edges ? (long long)pm_edge_len(sX[tid + 1], sY[tid + 1], sX[tid + 2], sY[tid + 2]) + 1 : 0;
            long long total;
            sStart[tid] = pe_block_excl(cnt, wave_ll, total);
            __syncthreads();
            for (long long f = tid; f < total; f += PE_T) {
                int lo = 0, hi = n_edges;                                  // the last edge that starts at or before point f
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (sStart[mid] <= f) lo = mid; else hi = mid;
                }
                const int d = (int)(f - sStart[lo]), e = lo + 1;
                if (d == 0 && lo == 0 && j0 == 0) continue;                // the polygon's first point has no predecessor
                int u, v, pu, pv;
                pm_point(sX[e], sY[e], sX[e + 1], sY[e + 1], sS[e], d, u, v);
                const int pe = d == 0 ? e - 1 : e;                         // across a junction: the previous edge's last point
                const int pxs = sX[pe], pys = sY[pe], pxe = sX[pe + 1], pye = sY[pe + 1];
                pm_point(pxs, pys, pxe, pye, sS[pe], d == 0 ? pm_edge_len(pxs, pys, pxe, pye) : d - 1, pu, pv);
                const long long pos = pm_crossing(u, v, pu, pv, H, W);
                if (pos >= 0 && pos < N) atomicXor(&tg[pos >> 5], 1u << (int)(pos & 31));
            }
        }
        __threadfence();
        __syncthreads();                       // every toggle of the polygon has been made, and has reached memory
        // ---- prefix parity of the toggles (read and cleared), OR into the mask
        int carry = 0;
        for (int w0 = 0; w0 < words; w0 += PE_T) {
            const int w = w0 + tid, buf = (w0 / PE_T) & 1;
            const bool in = w < words;
            const uint32_t t = in ? atomicExch(&tg[w], 0u) : 0u;
            uint32_t x = t;                    // bit b of x = parity of bits 0 .. b of t
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
            const unsigned long long odd = __ballot(__popc(t) & 1);
            if (lane == 0) wave_i[buf][wave] = __popcll(odd) & 1;
            __syncthreads();                   // (two buffers: the step after the next one writes this one again, a barrier later)
            int cin = carry ^ (__popcll(odd & ((1ull << lane) - 1ull)) & 1);
#pragma unroll
            for (int ww = 0; ww < PE_T / 64; ++ww) {
                const int tp = wave_i[buf][ww];
                if (ww < wave) cin ^= tp;
                carry ^= tp;
            }
            if (cin) x = ~x;
            if (in) {
                if (w == words - 1 && (N & 31)) x &= (1u << (N & 31)) - 1u;
                const uint32_t o = q == 0 ? x : (bw[w] | x);
                bw[w] = o;
                if (q == n_mine - 1) ones += __popc(o);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ones += __shfl_xor(ones, d, 64);
    __syncthreads();                           // wave_i is free
    if (lane == 0) wave_i[0][wave] = ones;
    __syncthreads();
    if (tid == 0) { bad[i] = 0; area[i] = wave_i[0][0] + wave_i[0][1] + wave_i[0][2] + wave_i[0][3]; }
}

}  // namespace nps

extern "C" nps_status nopesac_rle_string_runs(const uint8_t* bytes, const int64_t* str_off, int n_masks, int32_t* runs, int32_t* n_runs,
                                              void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(n_masks >= 0, "rle_string_runs: n_masks < 0");
    if (n_masks == 0) return 0;
    NPS_CHECK_ARG(bytes && str_off && runs && n_runs, "rle_string_runs: null pointer");
    hipLaunchKernelGGL(rle_string_runs_kernel, dim3(n_masks), dim3(PE_T), 0, (hipStream_t)stream, bytes, (const long long*)str_off, runs, n_runs);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_rle_runs_to_bits(const int32_t* runs, const int64_t* run_off, const int32_t* n_runs, int n_masks, int H, int W,
                                               int32_t* starts, uint32_t* bits, int32_t* area, int32_t* bad, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(n_masks >= 0, "rle_runs_to_bits: n_masks < 0");
    NPS_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffdfLL, "rle_runs_to_bits: H, W > 0 and H W < 2^31 - 32");
    if (n_masks == 0) return 0;
    NPS_CHECK_ARG(runs && run_off && n_runs && starts && bits && area && bad, "rle_runs_to_bits: null pointer");
    const int N = H * W;
    hipLaunchKernelGGL(rle_runs_to_bits_kernel, dim3(n_masks), dim3(PE_T), 0, (hipStream_t)stream, runs, (const long long*)run_off, n_runs, N,
                       (N + 31) / 32, starts, bits, area, bad);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_mask_iou_bits(const uint32_t* dt_bits, const int32_t* dt_area, const int64_t* dt_off, const uint32_t* gt_bits,
                                            const int32_t* gt_area, const int64_t* gt_off, const uint8_t* iscrowd, const int64_t* iou_off,
                                            int V, int words, int max_dt, int max_gt, double* iou, int32_t* inter, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(V >= 0 && V <= 65535, "mask_iou_bits: 0 <= V <= 65535");
    NPS_CHECK_ARG(words > 0 && max_dt >= 0 && max_gt >= 0, "mask_iou_bits: words > 0, max_dt >= 0, max_gt >= 0");
    if (V == 0 || max_dt == 0 || max_gt == 0) return 0;
    NPS_CHECK_ARG(dt_bits && dt_area && dt_off && gt_bits && gt_area && gt_off && iou_off && iou && inter, "mask_iou_bits: null pointer");
    const int gx = min((max_dt + IOU_PB - 1) / IOU_PB, 1024), gy = min((max_gt + IOU_GB - 1) / IOU_GB, 1024);
    hipLaunchKernelGGL(mask_iou_bits_kernel, dim3(gx, gy, V), dim3(256), 0, (hipStream_t)stream, dt_bits, dt_area, (const long long*)dt_off,
                       gt_bits, gt_area, (const long long*)gt_off, iscrowd, (const long long*)iou_off, words, iou, inter);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_plane_ap_assign(const double* iou, const int64_t* iou_off, const int64_t* dt_off, const int64_t* gt_off,
                                              const float* score, const int32_t* pred_label, const float* pred_plane, const int32_t* gt_label,
                                              const float* gt_plane, int V, int max_dt, int max_gt, double iou_thresh, double normal_thresh,
                                              double offset_thresh, double* rows, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(V >= 0, "plane_ap_assign: V < 0");
    NPS_CHECK_ARG(max_dt >= 0 && max_dt <= NPS_PLANE_MAX_QUERIES && max_gt >= 0 && max_gt <= 255,
                  "plane_ap_assign: at most %d predictions and 255 GT planes per view (got %d, %d)", NPS_PLANE_MAX_QUERIES, max_dt, max_gt);
    if (V == 0 || max_dt == 0) return 0;
    NPS_CHECK_ARG(iou_off && dt_off && gt_off && score && pred_label && pred_plane && rows, "plane_ap_assign: null pointer");
    NPS_CHECK_ARG(max_gt == 0 || (iou && gt_label && gt_plane), "plane_ap_assign: null pointer (GT)");
    hipLaunchKernelGGL(plane_ap_assign_kernel, dim3(V), dim3(64), 0, (hipStream_t)stream, iou, (const long long*)iou_off, (const long long*)dt_off,
                       (const long long*)gt_off, score, pred_label, pred_plane, gt_label, gt_plane, iou_thresh, normal_thresh, offset_thresh, rows);
    NPS_LAUNCH_RET();
}

extern "C" nps_status nopesac_poly_to_bits(const double* xy, const int64_t* poly_off, const int64_t* mask_off, int64_t n_points,
                                           int64_t n_polys, int n_masks, int H, int W, uint32_t* toggles, uint32_t* bits, int32_t* area,
                                           int32_t* bad, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(n_masks >= 0 && n_points >= 0 && n_polys >= 0, "poly_to_bits: n_masks, n_points or n_polys < 0");
    NPS_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffdfLL, "poly_to_bits: H, W > 0 and H W < 2^31 - 32");
    if (n_masks == 0) return 0;
    NPS_CHECK_ARG(xy && poly_off && mask_off && toggles && bits && area && bad, "poly_to_bits: null pointer");
    const int N = H * W;
    const long long cap = (long long)NPS_POLY_POINT_FACTOR * ((long long)N + H + W) + NPS_POLY_POINT_FLOOR;
    hipLaunchKernelGGL(poly_to_bits_kernel, dim3(n_masks), dim3(PE_T), 0, (hipStream_t)stream, xy, (const long long*)poly_off,
                       (const long long*)mask_off, (long long)n_points, (long long)n_polys, H, W, N, (N + 31) / 32, cap, toggles, bits, area, bad);
    NPS_LAUNCH_RET();
}
