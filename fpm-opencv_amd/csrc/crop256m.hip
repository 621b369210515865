// crop256m.hip -- objCrop = IDFT2(objF) / L^2 every iteration (fpmMain.cpp:481)
// for L = 256*M, M in {2, 3, 4} (the fused path's L = Np * resImprovementFactor
// with Np = 256).  objF = fftShift(spec), spec being the centred spectrum the
// solver stores (fpm_state.hpp).
//
// One L-point transform per 16-lane group, entirely in registers:
//   x[i], i = M*m + c  (c < M, m < 256):  Y_c = DFT256(x[M*m + c])      (M four-step 256s)
//   X[k' + 256 p] = sum_c W_L^{c k'} W_M^{c p} Y_c[k']                  (radix-M combine)
// Lane t holds, for every c, the sub-sequence elements m = t + 16 j (j < 16);
// after each 256-point four-step it holds Y_c[t + 16 r] (r < 16), so the
// radix-M combine is lane-local.  The fftShift of objF is free: rolling the
// row index is a different source row, rolling the element index by L/2 =
// 8*16*M is the register relabel j -> j + 8.
//
// Pass 1 (rows): spec rows -> objcrop rows, direct global loads/stores
//   (lane t reads x[M t + c + 16 M j]: each (c, j) covers 16*M contiguous
//   complex per group; it writes X[t + 16 r + 256 p]: 128 contiguous bytes).
// Pass 2 (columns, in place): a block stages a strip of G columns x L rows
//   through LDS (rows of G*8 contiguous bytes), each group transforms one
//   column in registers, scales by 1/L^2 and the strip is written back.
// HBM: at most 2 x 2 x 8 L^2 bytes per patch per iteration; only the live band
// of the spectrum (fpm_state.hpp) is read in pass 1 and re-read in pass 2.
//
// crop256m_kernels at the end is this family's row of the objCrop plan
// (plan_objcrop / launch_objcrop, objcrop.hip).
#include <hip/hip_runtime.h>

#include "crop_common.hpp"
#include "dft16.hpp"
#include "dftL.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

namespace {

// pass 1: row IDFTs of fftShift(spec) over the live rows [sy0, sy1] only
// (fpm_state.hpp: every other spec row is exactly zero, so its objF row's
// IDFT is zero; pass 2 treats those rows as zero instead of reading them),
// loading only the live columns [sx0, sx1].  grid (ceil((sy1-sy0+1) / G), B),
// block 16 G
template <int M, int G>
__global__ void __launch_bounds__(16 * G) k_crop_rows(const float2 *__restrict__ spec, float2 *__restrict__ out,
                                                      const float2 *__restrict__ tw_L, int sy0, int sy1, int sx0,
                                                      int sx1) {
    constexpr int L = 256 * M;
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *twL = sm;                  // L
    float2 *scr_all = sm + L;          // G exchange tiles
    const int g = threadIdx.x >> 4, t = threadIdx.x & 15;
    const int xrd = exch_rbase(t);
    float2 *scr = scr_all + g * XTILE;
    float2 wt[16];
    load_twiddles(twL, tw_L, L, M, wt, t);
    const int b = blockIdx.y, srow = sy0 + blockIdx.x * G + g;
    const bool live = srow <= sy1;     // group-uniform; no block barrier follows
    const int row = srow + L / 2 < L ? srow + L / 2 : srow - L / 2;     // objF row = spec row + L/2
    const float2 *src = spec + (size_t)b * L * L + (size_t)(live ? srow : sy1) * L;
    float2 x[M][16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
#pragma unroll
        for (int c = 0; c < M; ++c) {  // element roll by L/2
            const int sc = M * (t + 16 * j) + c;
            x[c][(j + 8) & 15] = in_band(sc, sx0, sx1) ? src[sc] : make_float2(0.f, 0.f);
        }
    dftL_regs<M, true>(x, scr, wt, twL, t, xrd);
    if (!live) return;
    float2 *dst = out + (size_t)b * L * L + (size_t)row * L;
#pragma unroll
    for (int p = 0; p < M; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[t + 16 * r + 256 * p] = x[p][r];
}

// pass 2: column IDFTs in place, scaled 1/L^2.  grid (L / G, B), block 16 G.
// The strip goes through LDS in two halves of L/2 rows: element i of a column
// is in half i / (L/2), i.e. register j / 8 on input (i = M (t + 16 j) + c) and
// the compile-time set r + 16 p < 8 M on output (k = t + 16 r + 256 p), so a
// half-size strip (58 KB at L = 768) lets two blocks share a CU and overlap
// one block's HBM phase with the other's transform.
// Rows of the intermediate outside the live band (objF row i <-> spec row
// i + L/2 mod L) were not written by pass 1 and are read as zero.
template <int M, int G>
__global__ void __launch_bounds__(16 * G) k_crop_cols(float2 *__restrict__ io, const float2 *__restrict__ tw_L,
                                                      float scale, int sy0, int sy1) {
    constexpr int L = 256 * M, H = L / 2;
    constexpr int SP = G + 1;          // strip row pitch (complex)
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *twL = sm;                  // L
    float2 *strip = sm + L;            // H x SP
    float2 *scr_all = strip;           // G exchange tiles, inside the strip: used
                                       // only while every column is in registers
    const int g = threadIdx.x >> 4, t = threadIdx.x & 15;
    const int xrd = exch_rbase(t);
    float2 *scr = scr_all + g * XTILE;
    float2 wt[16];
    load_twiddles(twL, tw_L, L, M, wt, t);
    const int b = blockIdx.y, c0 = blockIdx.x * G;
    float2 *base = io + (size_t)b * L * L + c0;
    constexpr int NTH = 16 * G;
    float2 x[M][16];
    constexpr int G2 = G / 2;
    // Both halves' strip loads are issued before the first barrier (twice
    // the bytes in flight per block), parked in registers until their half's
    // LDS round: objCrop 0.636 -> 0.584 ms per step at the metric config
    // (same box, profiles/r03_ab/crop_preload_ab.txt).  L = 1024 would need
    // 257 VGPRs for it and keeps the per-half loads.
    constexpr bool PRELOAD = M <= 3;
    constexpr int NLD = PRELOAD ? (H * G2 + NTH - 1) / NTH : 1;
    float4 qh[2][NLD];
    if constexpr (PRELOAD) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ya = max(sy0 - (1 - h) * H, 0), yb = min(sy1 - (1 - h) * H, H - 1);
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int idx = ya * G2 + threadIdx.x + k * NTH;
                if (idx < (yb + 1) * G2) {
                    const int y = idx / G2, cc = 2 * (idx - y * G2);
                    qh[h][k] = *(const float4 *)(base + (size_t)(y + h * H) * L + cc);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // objF row y + h H is spec row y + (1 - h) H: the live rows of this
        // half are the contiguous range [ya, yb]
        const int ya = max(sy0 - (1 - h) * H, 0), yb = min(sy1 - (1 - h) * H, H - 1);
        if constexpr (PRELOAD) {
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int idx = ya * G2 + threadIdx.x + k * NTH;
                if (idx < (yb + 1) * G2) {
                    const int y = idx / G2, cc = 2 * (idx - y * G2);
                    strip[y * SP + cc] = make_float2(qh[h][k].x, qh[h][k].y);
                    strip[y * SP + cc + 1] = make_float2(qh[h][k].z, qh[h][k].w);
                }
            }
        } else {
            // strip load: consecutive threads take consecutive column pairs of a row
            // (16-byte loads: twice the bytes in flight per load instruction)
#pragma unroll 4  // strip load/store loop: loads in flight per thread
            for (int idx = ya * G2 + threadIdx.x; idx < (yb + 1) * G2; idx += NTH) {
                const int y = idx / G2, cc = 2 * (idx - y * G2);
                const float4 q = *(const float4 *)(base + (size_t)(y + h * H) * L + cc);
                strip[y * SP + cc] = make_float2(q.x, q.y);
                strip[y * SP + cc + 1] = make_float2(q.z, q.w);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 8 * h; j < 8 * h + 8; ++j)
#pragma unroll
            for (int c = 0; c < M; ++c) {
                const int y = M * (t + 16 * j) + c - h * H;
                x[c][j] = (y >= ya && y <= yb) ? strip[y * SP + g] : make_float2(0.f, 0.f);  // ya > yb: none
            }
        __syncthreads();
    }
    dftL_regs<M, true>(x, scr, wt, twL, t, xrd);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();  // exchange tiles / previous half's reads are done
#pragma unroll
        for (int p = 0; p < M; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r + 16 * p < 8 * M) == (h == 0))
                    strip[(t + 16 * r + 256 * p - h * H) * SP + g] = cscale(x[p][r], scale);
        __syncthreads();
#pragma unroll 4  // strip load/store loop: loads in flight per thread
        for (int idx = threadIdx.x; idx < H * G / 2; idx += NTH) {
            const int y = idx / (G / 2), cc = 2 * (idx - y * (G / 2));
            const float2 p0 = strip[y * SP + cc], p1 = strip[y * SP + cc + 1];
            // the output is not re-read: non-temporal stores (0.584 -> 0.569 ms
            // per step at L 768; the 600-point pass measured 1 % slower with them)
            __builtin_nontemporal_store((f32x4_nt){p0.x, p0.y, p1.x, p1.y}, (f32x4_nt *)(base + (size_t)(y + h * H) * L + cc));
        }
    }
}

constexpr int kCropG = 16;   // columns per strip: 128-byte row segments
constexpr int kCropGR = 4;   // rows per block in the row pass

template <int M>
CropPair pair256m() {
    constexpr int L = 256 * M, GR = kCropGR, G = kCropG;
    // the exchange tiles alias the half strip: allocate the larger of the two
    constexpr size_t strip = (size_t)L / 2 * (G + 1) > (size_t)G * XTILE ? (size_t)L / 2 * (G + 1) : (size_t)G * XTILE;
    return {crop_kernel((const void *)k_crop_rows<M, GR>, 16 * GR, (size_t)(L + GR * XTILE) * sizeof(float2), GR),
            crop_kernel((const void *)k_crop_cols<M, G>, 16 * G, (L + strip) * sizeof(float2), G)};
}

}  // namespace

CropPair crop256m_kernels(int L) {
    switch (L) {
        case 512: return pair256m<2>();
        case 768: return pair256m<3>();
        case 1024: return pair256m<4>();
        default: return CropPair{};
    }
}

}  // namespace fpm
