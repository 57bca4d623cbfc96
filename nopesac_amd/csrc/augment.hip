// Training-time image augmentation: with cfg.DATALOADER.AUGMENTATION the reference mapper draws, per view,
//     RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.2), RandomGrayscale(p=0.2), RandomApply([GaussianBlur(sigma)], p=0.5), ToTensor()*255
// (data/planercnn_transforms.py:183-191, data/augmentation.py:22) and runs it on PIL images on the host.  torchvision and Pillow are
// third-party dependencies that are not in the reference tree; these kernels restate their published 8-bit arithmetic - the order of
// operations from torchvision's transforms.ColorJitter / RandomApply / RandomGrayscale and functional_pil, every pixel operation from
// Pillow (ImageEnhance -> Image.blend, convert "L" / "HSV" / "RGB", ImageFilter.GaussianBlur -> BoxBlur.c) - uint8 in, uint8 out,
// quantised after every operation:
//     L          = (19595 c0 + 38470 c1 + 7471 c2 + 0x8000) >> 16
//     blend      = clip(deg + f * (v - deg)) truncated, f32 with a separate multiply and add (a fused multiply-add moves single pixels);
//                  deg = 0 (brightness), int(mean(L) + 0.5) of the image as it stands (contrast), L of the pixel (saturation)
//     hue        = RGB -> HSV (colorsys.py in f32 / f64 as Convert.c mixes them), H += uint8(f * 255) mod 256, HSV -> RGB
//     grey       = L in all three channels
//     blur       = three extended box blurs per axis, rows first: s2 = sigma^2 / 3, L = sqrt(12 s2 + 1), l = floor((L - 1) / 2),
//                  a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), r = l + a;  ww = uint32(2^24 / (2r + 1)) (an f32 division),
//                  fw = (2^24 - (2l + 1) ww) / 2;  out = (ww * sum_{|d| <= l} v[x + d] + fw * (v[x - l - 1] + v[x + l + 1]) + 2^23) >> 24,
//                  indices clamped to the image in every pass
// Quirk kept from the reference: the mapper reads the image in cfg.INPUT.FORMAT (BGR) and hands that array to Image.fromarray
// (planercnn_transforms.py:219-221, :316-318), so Pillow takes memory channel 0 for red.  The luma weights and the direction of the hue
// rotation therefore apply to the channels in MEMORY order whatever the format says, and so they do here.
#include "common.h"

namespace nps {

constexpr int AUG_T = NPS_AUG_TILE, AUG_A = NPS_AUG_APRON, AUG_R = AUG_T + 2 * AUG_A;      // tile, apron, tile with apron (44)

struct AugBox { int radius; uint32_t ww, fw; };

// BoxBlur.c _gaussian_blur_radius + ImagingHorizontalBoxBlur's weights, in its types (float where it says float, double where a double
// literal widens the expression).  Host (the launcher's check) and device.
__host__ __device__ inline AugBox aug_box(float radius) {
    const int passes = 3;
    float sigma2, L, l, a;
    sigma2 = radius * radius / passes;
    L = sqrt(12.0 * sigma2 + 1.0);
    l = floor((L - 1.0) / 2.0);
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float fr = l + a;
    AugBox b;
    b.radius = (int)fr;
    b.ww = (uint32_t)((uint32_t)(1 << 24) / (fr * 2 + 1));
    b.fw = ((1 << 24) - (b.radius * 2 + 1) * b.ww) / 2;
    return b;
}

__device__ __forceinline__ int aug_luma(int c0, int c1, int c2) { return (19595 * c0 + 38470 * c1 + 7471 * c2 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f).  Blend.c clips only for f outside [0, 1]; inside, the value lies between its two operands, so one form serves.
__device__ __forceinline__ int aug_blend(int deg, int v, float f) {
    const float t = __fadd_rn((float)deg, __fmul_rn(f, (float)(v - deg)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// functional_pil.adjust_hue: convert("HSV"), H += shift (uint8 wrap-around), convert("RGB") - Convert.c rgb2hsv_row / hsv2rgb.
__device__ __forceinline__ void aug_hue(int& c0, int& c1, int& c2, int shift) {
    const int maxc = max(c0, max(c1, c2)), minc = min(c0, min(c1, c2));
    if (minc == maxc) return;                                     // S = 0: HSV -> RGB writes V three times
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - c0) / cr, gc = (float)(maxc - c1) / cr, bc = (float)(maxc - c2) / cr;
    float h;
    if (c0 == maxc) h = bc - gc;
    else if (c1 == maxc) h = (float)(2.0 + rc - bc);
    else h = (float)(4.0 + gc - rc);
    const double hq = h / 6.0 + 1.0;
    h = (float)(hq - floor(hq));                                  // fmod(., 1.0) of a value in [0.5, 2)
    const int uh = (min(max((int)(h * 255.0), 0), 255) + shift) & 255;
    const int us = min(max((int)(s * 255.0), 0), 255);
    if (us == 0) { c0 = c1 = c2 = maxc; return; }
    const int i = (int)floor((float)uh * 6.0 / 255.0);
    const float f = (float)((float)uh * 6.0 / 255.0 - (float)i);
    const float fs = (float)(((float)us) / 255.0);
    const int p = min(max((int)round((float)maxc * (1.0 - fs)), 0), 255);
    const int q = min(max((int)round((float)maxc * (1.0 - fs * f)), 0), 255);
    const int t = min(max((int)round((float)maxc * (1.0 - fs * (1.0 - f))), 0), 255);
    const int v = maxc;
    switch (i % 6) {
        case 0: c0 = v; c1 = t; c2 = p; break;
        case 1: c0 = q; c1 = v; c2 = p; break;
        case 2: c0 = p; c1 = v; c2 = t; break;
        case 3: c0 = p; c1 = q; c2 = v; break;
        case 4: c0 = t; c1 = p; c2 = v; break;
        default: c0 = v; c1 = p; c2 = q; break;
    }
}

// a[k] by selects: a runtime index into a by-value row would put the row into scratch memory
template <typename T>
__device__ __forceinline__ T aug_sel(const T (&a)[NPS_AUG_OPS], int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : (k == 2 ? a[2] : a[3])); }

// The jitter operations order[first .. last) of a row on one pixel (the row is workgroup-uniform: every branch here is scalar).
__device__ __forceinline__ void aug_jitter(const nopesac_aug_row& row, int first, int last, int mean, int& c0, int& c1, int& c2) {
    for (int k = first; k < last; ++k) {
        const int op = aug_sel(row.order, k);
        const float f = aug_sel(row.factor, op);
        if (op == NPS_AUG_BRIGHTNESS) {
            c0 = aug_blend(0, c0, f); c1 = aug_blend(0, c1, f); c2 = aug_blend(0, c2, f);
        } else if (op == NPS_AUG_CONTRAST) {
            c0 = aug_blend(mean, c0, f); c1 = aug_blend(mean, c1, f); c2 = aug_blend(mean, c2, f);
        } else if (op == NPS_AUG_SATURATION) {
            const int l = aug_luma(c0, c1, c2);
            c0 = aug_blend(l, c0, f); c1 = aug_blend(l, c1, f); c2 = aug_blend(l, c2, f);
        } else {
            const int hs = (int)((double)f * 255.0);              // np.uint8(hue_factor * 255): truncated towards zero, then modulo 256
            aug_hue(c0, c1, c2, hs & 255);
        }
    }
}

__device__ __forceinline__ int aug_contrast_pos(const nopesac_aug_row& row) {
    int pos = 0;
#pragma unroll
    for (int k = 0; k < NPS_AUG_OPS; ++k) pos = row.order[k] == NPS_AUG_CONTRAST ? k : pos;
    return pos;
}

__device__ __forceinline__ uint32_t aug_wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// Contrast pre-pass: the integer luma sum of the image as it stands when contrast runs - the pointwise operations ahead of contrast in
// the row's order are recomputed per pixel.  grid (NPS_AUG_PARTIALS, n); workgroup b of image i leaves ONE partial in ws[i][b], which
// the fused pass sums in index order: integers, the same bits on every run.  Rows without jitter leave at once.
__global__ __launch_bounds__(256) void aug_luma_partials_kernel(const uint8_t* __restrict__ src, long long src_stride, int H, int W,
                                                                const nopesac_aug_row* __restrict__ rows, uint32_t* __restrict__ ws) {
    const nopesac_aug_row row = rows[blockIdx.y];
    if (!(row.flags & NPS_AUG_JITTER)) return;
    const uint8_t* s = src + (long long)blockIdx.y * src_stride;
    const int pos = aug_contrast_pos(row);
    const int npix = H * W;
    uint32_t sum = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += NPS_AUG_PARTIALS * 256) {
        int c0 = s[3ll * i], c1 = s[3ll * i + 1], c2 = s[3ll * i + 2];
        aug_jitter(row, 0, pos, 0, c0, c1, c2);
        sum += (uint32_t)aug_luma(c0, c1, c2);
    }
    __shared__ uint32_t part[4];
    sum = aug_wave_sum_u32(sum);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.y * NPS_AUG_PARTIALS + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// jitter in the row's order, then grey: everything ahead of the blur, on one pixel
__device__ __forceinline__ void aug_point(const nopesac_aug_row& row, int mean, int& c0, int& c1, int& c2) {
    if (row.flags & NPS_AUG_JITTER) aug_jitter(row, 0, NPS_AUG_OPS, mean, c0, c1, c2);
    if (row.flags & NPS_AUG_GREY) c0 = c1 = c2 = aug_luma(c0, c1, c2);
}

__device__ __forceinline__ void aug_store(int c0, int c1, int c2, long long img, int y, int x, int H, int W, uint8_t* __restrict__ chw,
                                          float* __restrict__ nhwc, const float (&mean)[3], const float (&stdv)[3]) {
    if (chw) {
        uint8_t* o = chw + ((img * 3 * H + y) * W + x);
        o[0] = (uint8_t)c0; o[(long long)H * W] = (uint8_t)c1; o[2ll * H * W] = (uint8_t)c2;
    }
    if (nhwc)
        reinterpret_cast<float4*>(nhwc)[(img * H + y) * W + x] =
            make_float4(((float)c0 - mean[0]) / stdv[0], ((float)c1 - mean[1]) / stdv[1], ((float)c2 - mean[2]) / stdv[2], 0.f);
}

// One box pass at tile position (la along the axis, word index p): taps at image coordinates clamped to [0, N) - the replication
// happens at the IMAGE border in every pass - then to the tile, whose outer ring is not valid after the pass and is never read for
// a centre pixel (a pass reaches radius + 1 <= 2 pixels, three passes per axis NPS_AUG_APRON).  Pixels are packed words c0 | c1 << 8 | c2 << 16.
template <int R>
__device__ __forceinline__ uint32_t aug_box_at(const uint32_t* __restrict__ in, int p, int step, int la, int a0, int N, uint32_t ww, uint32_t fw) {
    uint32_t n0 = 0, n1 = 0, n2 = 0, f0 = 0, f1 = 0, f2 = 0;
#pragma unroll
    for (int d = -R - 1; d <= R + 1; ++d) {
        const int g = min(max(a0 + la + d, 0), N - 1);
        const int t = min(max(g - a0, 0), AUG_R - 1);
        const uint32_t w = in[p + (t - la) * step];
        if (d == -R - 1 || d == R + 1) { f0 += w & 255; f1 += (w >> 8) & 255; f2 += (w >> 16) & 255; }
        else { n0 += w & 255; n1 += (w >> 8) & 255; n2 += (w >> 16) & 255; }
    }
    const uint32_t o0 = (n0 * ww + f0 * fw + (1u << 23)) >> 24, o1 = (n1 * ww + f1 * fw + (1u << 23)) >> 24, o2 = (n2 * ww + f2 * fw + (1u << 23)) >> 24;
    return (o0 & 255) | ((o1 & 255) << 8) | ((o2 & 255) << 16);
}

// The fused pass: grid (tiles, n), one NPS_AUG_TILE^2 tile of one image per workgroup, every decision on the row uniform per workgroup.
// Loads always come from addresses clamped into the image (the border replication of the blur wants exactly that), stores are
// predicated: no guarded load anywhere.
__global__ __launch_bounds__(256) void aug_fused_kernel(const uint8_t* __restrict__ src, long long src_stride, int H, int W, int tiles_x,
                                                        const nopesac_aug_row* __restrict__ rows, const uint32_t* __restrict__ ws,
                                                        uint8_t* __restrict__ chw, float* __restrict__ nhwc, const float* __restrict__ mean3,
                                                        const float* __restrict__ std3) {
    __shared__ uint32_t buf[2][AUG_R * AUG_R];
    const long long img = blockIdx.y;
    const nopesac_aug_row row = rows[img];
    const uint8_t* s = src + img * src_stride;
    const int x0 = (int)(blockIdx.x % tiles_x) * AUG_T, y0 = (int)(blockIdx.x / tiles_x) * AUG_T;
    float mean[3] = {0.f, 0.f, 0.f}, stdv[3] = {1.f, 1.f, 1.f};
    if (nhwc) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { mean[c] = mean3[c]; stdv[c] = std3[c]; }
    }
    int lmean = 0;
    if (row.flags & NPS_AUG_JITTER) {           // int(mean(L) + 0.5) = (2 sum + count) / (2 count) in integers
        const uint32_t sum = aug_wave_sum_u32(ws[img * NPS_AUG_PARTIALS + (threadIdx.x & 63)]);
        const unsigned long long count = (unsigned long long)H * W;
        lmean = (int)((2ull * sum + count) / (2ull * count));
    }
    if (!(row.flags & NPS_AUG_BLUR)) {
        for (int p = threadIdx.x; p < AUG_T * AUG_T; p += 256) {
            const int x = x0 + (p % AUG_T), y = y0 + (p / AUG_T);
            const uint8_t* px = s + ((long long)min(y, H - 1) * W + min(x, W - 1)) * 3;
            int c0 = px[0], c1 = px[1], c2 = px[2];
            aug_point(row, lmean, c0, c1, c2);
            if (x < W && y < H) aug_store(c0, c1, c2, img, y, x, H, W, chw, nhwc, mean, stdv);
        }
        return;
    }
    const AugBox box = aug_box(row.sigma);
    const int ax0 = x0 - AUG_A, ay0 = y0 - AUG_A;
    for (int p = threadIdx.x; p < AUG_R * AUG_R; p += 256) {        // pointwise operations recomputed on the apron
        const int x = min(max(ax0 + (p % AUG_R), 0), W - 1), y = min(max(ay0 + (p / AUG_R), 0), H - 1);
        const uint8_t* px = s + ((long long)y * W + x) * 3;
        int c0 = px[0], c1 = px[1], c2 = px[2];
        aug_point(row, lmean, c0, c1, c2);
        buf[0][p] = (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16);
    }
    __syncthreads();
    int cur = 0;
    for (int pass = 0; pass < 6; ++pass) {                          // three along rows, then three along columns, each quantised
        const bool horiz = pass < 3;
        const uint32_t* in = buf[cur];
        uint32_t* out = buf[cur ^ 1];
        const int cols = horiz ? AUG_R : AUG_T, c0 = horiz ? 0 : AUG_A;       // the column passes serve the centre columns only
        for (int q = threadIdx.x; q < cols * AUG_R; q += 256) {
            const int lx = c0 + q % cols, ly = q / cols, p = ly * AUG_R + lx;
            const int la = horiz ? lx : ly, a0 = horiz ? ax0 : ay0, N = horiz ? W : H, step = horiz ? 1 : AUG_R;
            out[p] = box.radius == 0 ? aug_box_at<0>(in, p, step, la, a0, N, box.ww, box.fw) : aug_box_at<1>(in, p, step, la, a0, N, box.ww, box.fw);
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int p = threadIdx.x; p < AUG_T * AUG_T; p += 256) {
        const int lx = p % AUG_T, ly = p / AUG_T, x = x0 + lx, y = y0 + ly;
        const uint32_t w = buf[cur][(ly + AUG_A) * AUG_R + lx + AUG_A];
        if (x < W && y < H) aug_store((int)(w & 255), (int)((w >> 8) & 255), (int)((w >> 16) & 255), img, y, x, H, W, chw, nhwc, mean, stdv);
    }
}

}  // namespace nps

static int64_t aug_workspace_bytes(int n, int H, int W) { return (n > 0 && H > 0 && W > 0) ? (int64_t)n * NPS_AUG_PARTIALS * 4 : 0; }

extern "C" int nopesac_augment_workspace_bytes(int n, int H, int W, int64_t* bytes) {
    NPS_CHECK_ARG(bytes, "augment_workspace_bytes: null result pointer");
    *bytes = aug_workspace_bytes(n, H, W);
    return 0;
}

extern "C" int nopesac_augment_u8(const uint8_t* src, int n, int64_t src_stride, int H, int W, int C, const nopesac_aug_row* rows_host,
                                  const nopesac_aug_row* rows_dev, uint8_t* chw_out, float* nhwc_out, const float* mean, const float* stdv,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace nps;
    NPS_CHECK_ARG(C == 3, "augment: C = %d, three channels expected", C);
    NPS_CHECK_ARG(src && rows_host && rows_dev && (chw_out || nhwc_out) && n > 0 && n <= 65535 && H > 0 && W > 0, "augment: bad args");
    NPS_CHECK_ARG((long long)H * W <= 16843009ll, "augment: %d x %d: the luma sum of the contrast pre-pass would not fit 32 bits", H, W);
    NPS_CHECK_ARG(src_stride >= (int64_t)H * W * 3, "augment: src_stride %lld below one image", (long long)src_stride);
    NPS_CHECK_ARG(!nhwc_out || (mean && stdv && ((uintptr_t)nhwc_out & 15) == 0), "augment: the normalised output needs mean and std and 16-byte alignment");
    NPS_CHECK_ARG(workspace && workspace_bytes >= aug_workspace_bytes(n, H, W), "augment: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)aug_workspace_bytes(n, H, W));
    for (int i = 0; i < n; ++i) {
        const nopesac_aug_row& r = rows_host[i];
        NPS_CHECK_ARG(!(r.flags & ~(NPS_AUG_JITTER | NPS_AUG_GREY | NPS_AUG_BLUR)), "augment: row %d: unknown flags %d", i, r.flags);
        if (r.flags & NPS_AUG_JITTER) {
            int seen = 0;
            for (int k = 0; k < NPS_AUG_OPS; ++k)
                if (r.order[k] >= 0 && r.order[k] < NPS_AUG_OPS) seen |= 1 << r.order[k];
            NPS_CHECK_ARG(seen == (1 << NPS_AUG_OPS) - 1, "augment: row %d: order is not a permutation of 0-3", i);
            for (int k = 0; k < NPS_AUG_OPS; ++k) NPS_CHECK_ARG(r.factor[k] == r.factor[k], "augment: row %d: factor %d is not a number", i, k);
            NPS_CHECK_ARG(r.factor[NPS_AUG_HUE] >= -0.5f && r.factor[NPS_AUG_HUE] <= 0.5f, "augment: row %d: hue factor outside [-0.5, 0.5]", i);
        }
        if (r.flags & NPS_AUG_BLUR) {
            NPS_CHECK_ARG(r.sigma > 0.f && r.sigma <= (float)NPS_AUG_MAX_SIGMA, "augment: row %d: sigma %g outside (0, %d]", i, (double)r.sigma,
                          NPS_AUG_MAX_SIGMA);
            NPS_CHECK_ARG(3 * (aug_box(r.sigma).radius + 1) <= NPS_AUG_APRON, "augment: row %d: sigma %g reaches past the apron", i, (double)r.sigma);
        }
    }
    const int tiles_x = (W + NPS_AUG_TILE - 1) / NPS_AUG_TILE, tiles_y = (H + NPS_AUG_TILE - 1) / NPS_AUG_TILE;
    hipLaunchKernelGGL(aug_luma_partials_kernel, dim3(NPS_AUG_PARTIALS, (unsigned)n), dim3(256), 0, (hipStream_t)stream, src, (long long)src_stride, H, W,
                       rows_dev, (uint32_t*)workspace);
    hipLaunchKernelGGL(aug_fused_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), 0, (hipStream_t)stream, src, (long long)src_stride,
                       H, W, tiles_x, rows_dev, (const uint32_t*)workspace, chw_out, nhwc_out, mean, stdv);
    NPS_LAUNCH_RET();
}
