// What conv_igemm_p8_kernel (conv_p8.hip, 256x256 tiles) and conv_igemm_p8n_kernel (conv_p8n.hip, 256x128 tiles) share: the XCD-aware
// walk over tiles, the per-tile row table, the K-tile cursor, the pixel-half LDS-DMA and the buffer descriptors.  Each kernel keeps its
// LDS layout, weight staging, phase schedule with its counted vmcnt, work-unit logic and epilogues (docs/kernels.md, "The two 256-row
// conv kernels").  Not a public header.
#pragma once
#include "conv_common.h"

namespace nps {

template <int K>
struct IC { static constexpr int value = K; };      // integral constant handed to a generic lambda: a compile-time loop index

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned P8_OOB = 0xFFFFFF00u;              // a voffset past every descriptor: the load returns zeros, the store is dropped

// ---- this workgroup's tiles: XCD x (= blockIdx % 8: private L2) owns a contiguous run of the launch's `units`, its workgroups walk the
//      run with stride = workgroups on that XCD, so the 32 CUs of an XCD always work on 32 neighbouring tiles (shared halo rows)
struct P8TileWalk {
    int xcd, slot, run_begin, run_end, stride;
    __device__ __forceinline__ explicit P8TileWalk(int units) {
        const int nx = (int)gridDim.x < 8 ? (int)gridDim.x : 8;     // XCDs that host workgroups of this grid
        xcd = blockIdx.x % 8; slot = blockIdx.x / 8;
        const int tq = units / nx, tr = units % nx;
        run_begin = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
        run_end = run_begin + tq + (xcd < tr ? 1 : 0);
        stride = ((int)gridDim.x - xcd + 7) / 8;
    }
};

// ---- descriptors.  x starts one padding row + column early, so that a row's pixel offset (ih0 + pad, iw0 + pad) is never negative
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p8_x_rsrc(const ConvParams& p) {
    const long long padb = ((long long)p.pad * p.W + p.pad) * p.x_cs * 2;
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x - padb), 0, (int)(((long long)p.B * p.H * p.W * p.x_cs) * 2 + padb), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p8_w_rsrc(const ConvParams& p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)((long long)p.N * p.K * 2), 0x00020000);
}
// bf16 rows of N channels, pixel stride cs, ending with row M - 1: rows >= M of the last tile read zeros / are dropped (`on` false: empty)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p8_rows_rsrc(const void* base, const ConvParams& p, long long cs, bool on = true) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, on ? (int)((((long long)p.M - 1) * cs + p.N) * 2) : 0, 0x00020000);
}

// exact a / d, a % d by float reciprocal + one-step fix-up (a < 2^23)
__device__ __forceinline__ void p8_divmod(int a, int d, float rcp, int& q, int& r) {
    q = (int)((float)a * rcp);
    r = a - __mul24(q, d);
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
}

// ---- wave-uniform cursor of the NEXT K-tile to stage (K-tiles are staged strictly in order).
// K order: p.force == 0: tap-major (all channels of tap 0, then tap 1 ...: the natural order of the weight rows);
//          p.force == 1: CHANNEL-major (the KH*KW taps of channels 0-63, then of channels 64-127 ...): the pixels a workgroup
//          re-reads for the nine taps of one 64-channel slice are ONE 128-byte line each, so the slice stays in the XCD's L2
//          between the taps (tap-major streams all Cin channels of the tile's pixels nine times: L2 hit rate 76 %).
// The two tapoff steps are members, computed once: written out in advance() the compiler recomputed them (s_sub + s_mul) at each of the
// K loop's advance sites, and the tap-major 3x3 layers measured 1-2 % slower (profiles/conv_p8_shared_header.txt).
template <int BK>
struct P8KCursor {
    int tap, kw, c0;
    unsigned tapoff, k0b;                  // byte offsets of the tap inside x / of the K-tile inside a weight row
    unsigned kw_step, kh_step;             // tapoff steps: to the next tap of a row / on top of that, from a row's last tap to the next row's first
    __device__ __forceinline__ explicit P8KCursor(const ConvParams& p)
        : kw_step((unsigned)p.x_cs * 2u), kh_step((unsigned)(p.W - p.KW) * (unsigned)p.x_cs * 2u) {}
    __device__ __forceinline__ void reset(int c_begin) {       // first tap of channel c_begin (0, or a split-K slice's first channel)
        tap = 0; kw = 0; c0 = c_begin; tapoff = 0u; k0b = (unsigned)c_begin * 2u;
    }
    __device__ __forceinline__ void advance(const ConvParams& p) {
        if (p.force == 0) {
            k0b += BK * 2;
            c0 += BK;
            if (c0 >= p.Cin) {
                c0 = 0; ++tap; ++kw;
                tapoff += kw_step;
                if (kw == p.KW) { kw = 0; tapoff += kh_step; }
            }
        } else {
            ++tap; ++kw;
            k0b += (unsigned)p.Cin * 2u;
            tapoff += kw_step;
            if (kw == p.KW) { kw = 0; tapoff += kh_step; }
            if (tap == p.KH * p.KW) {
                tap = 0; kw = 0; tapoff = 0u;
                c0 += BK;
                k0b = (unsigned)c0 * 2u;
            }
        }
    }
    __device__ __forceinline__ void set_cursor(const ConvParams& p, int kt) {     // stream-K: -> K-tile kt of the tile (wave-uniform integer math)
        const int ntaps = p.KH * p.KW;
        int t, c;
        if (p.force == 0) { const int per = p.Cin / BK; t = kt / per; c = (kt - t * per) * BK; }
        else { const int cs = kt / ntaps; t = kt - cs * ntaps; c = cs * BK; }
        const int kh = t / p.KW;
        tap = t; kw = t - kh * p.KW; c0 = c;
        tapoff = (unsigned)(kh * p.W + kw) * (unsigned)p.x_cs * 2u;
        k0b = (unsigned)(t * p.Cin + c) * 2u;
    }
};

// ---- the BM = 256 pixel rows of a tile.  One 1-KB DMA = 8 tile rows x ROWB = 128 B, lane -> row (lane >> 3), physical 16-byte slot
// (lane & 7); pixel-half piece h (pixel half mi = h of BOTH wave rows): DMA j of wave w fills rows j*128 + h*64 + w*8 .. +7.
// Every tile row is addressed by 8 lanes (its eight 16-byte chunks) of 4 different DMAs, so the row -> (image, oh, ow) -> byte offset +
// tap-validity mask computation is done ONCE per row by threads 0..255 into a 2 KB LDS table at TAB_OFF, and every lane then picks up
// its four rows (first version: each lane did it 4 times - ~900 instructions per wave with 32-bit integer divisions, 64-bit products and
// a 9-tap loop: 5-6 k cycles per tile):
//   * row -> (image, oh, ow) by p8_divmod (exact for M < 2^23)
//   * every product is a 24-bit multiply (v_mul_u32_u24): pixel indices, channel strides and K are < 2^24 and every byte offset
//     < 2^31 (checked by the launcher)
//   * tap mask = row-validity bits x column-validity bits; out-of-image taps and rows >= M (mask 0) read zeros through the bounds check
template <int BM, int ROWB, int TAB_OFF>
struct P8Rows {
    static_assert(BM == 256 && ROWB == 128, "two pixel halves of two 64-row DMA groups, 128-byte rows");
    unsigned coff[2][2], voff[2][2], mask[2][2];    // [piece h][DMA j]: swizzled chunk offset (per-lane constant) / + row offset / tap mask
    float rcp_rpb, rcp_ow;
    __device__ __forceinline__ void init(const ConvParams& p, int wave, int lane) {
        rcp_rpb = 1.0f / (float)p.rows_per_b; rcp_ow = 1.0f / (float)p.OW;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pr = j * 128 + h * 64 + wave * 8 + (lane >> 3);
                coff[h][j] = (unsigned)((lane & 7) ^ ((pr >> 1) & 7)) * 16u;
            }
    }
    // workgroup-collective (contains a barrier): the table of the tile whose first row is m0, then this lane's four rows
    __device__ __forceinline__ void set_tile(unsigned char* lds, const ConvParams& p, int m0, int tid, int wave, int lane) {
        uint2* rowtab = reinterpret_cast<uint2*>(lds + TAB_OFF);           // [BM] {byte offset of the row's pixel, tap mask}
        if (tid < BM) {
            const int m = m0 + tid;
            uint2 e = make_uint2(0u, 0u);
            if (m < p.M) {
                int b, rem, oh, ow;
                p8_divmod(m, p.rows_per_b, rcp_rpb, b, rem);
                p8_divmod(rem, p.OW, rcp_ow, oh, ow);
                const int ih0 = __mul24(oh, p.stride) - p.pad, iw0 = __mul24(ow, p.stride) - p.pad;
                const unsigned pix = __umul24(__umul24((unsigned)b, (unsigned)p.H) + (unsigned)(ih0 + p.pad), (unsigned)p.W) + (unsigned)(iw0 + p.pad);
                unsigned colbits = 0u;
                for (int kw = 0; kw < p.KW; ++kw) colbits |= ((unsigned)(iw0 + kw) < (unsigned)p.W ? 1u : 0u) << kw;
                unsigned mk = 0u;
                for (int kh = 0; kh < p.KH; ++kh)
                    if ((unsigned)(ih0 + kh) < (unsigned)p.H) mk |= colbits << __mul24(kh, p.KW);
                e = make_uint2(__umul24(pix, (unsigned)p.x_cs) * 2u, mk);
            }
            rowtab[tid] = e;
        }
        NPS_LDS_SYNC();
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint2 e = rowtab[j * 128 + h * 64 + wave * 8 + (lane >> 3)];
                voff[h][j] = e.x + coff[h][j];
                mask[h][j] = e.y;
            }
    }
    // pixel-half piece h of the cursor's K-tile -> the A rows of the K-tile buffer `buf`
    template <int BK>
    __device__ __forceinline__ void stage_a(const __amdgpu_buffer_rsrc_t& xsrc, unsigned char* buf, int h, int wave, const P8KCursor<BK>& cur) const {
        const unsigned soff = cur.tapoff + (unsigned)cur.c0 * 2u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned vo = ((mask[h][j] >> cur.tap) & 1u) ? voff[h][j] : P8_OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrc, (lptr_t)(buf + (j * 128 + h * 64 + wave * 8) * ROWB), 16, vo, soff, 0, 0);
        }
    }
};

}  // namespace nps
