// crop600.hip -- objCrop's register transform for L = 600 (= 200 x 3); the
// passes and the live band are those of crop256m.hip, crop600_kernels at the
// end is this family's row of the objCrop plan (objcrop.hip).
#include <hip/hip_runtime.h>

#include "crop_common.hpp"
#include "dft16.hpp"
#include "dft200.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

namespace {

// ------------------------------------------------------------ L = 600 (= 200 x 3)
// BASELINE config 3 (Np 200, resImprovementFactor 3).  One 600-point transform
// per 10-lane group (dft200.hpp, six groups per wave, lanes 60..63 idle):
//   x[i], i = 3 m + c (c < 3, m < 200): Y_c = DFT200(x[3 m + c]), lane l
//   holding m = l + 10 k (k < 20); then the lane-local radix-3 combine
//   X[k' + 200 p] = sum_c W600^{c k'} W3^{c p} Y_c[k'],  k' = l + 10 k.
// fftShift: the element roll by L/2 = 300 = 3 * 100 is the register relabel
// k -> k + 10 (mod 20); the row roll is the source row, as for L = 256 M.
namespace c600 {
constexpr int L = 600, H = 300, GPW = 6;

// x[c][k] = element 3 (l + 10 k) + c; on return x[p][k] = X[l + 10 k + 200 p]
template <bool INV>
__device__ __forceinline__ void dft600_regs(float2 (&x)[3][20], float2 *tile, const float2 *tw2, const float2 *twL,
                                            int l, int xrd) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dft200<INV, false>(x[c], tile, tw2, l, xrd);
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        const int kp = l + 10 * k;
        float2 z[3];
        z[0] = x[0][k];
        const float2 w1 = twL[kp], w2 = twL[2 * kp];
        z[1] = pout(INV ? pmulc(pin(x[1][k]), pin(w1)) : pmul(pin(x[1][k]), pin(w1)));
        z[2] = pout(INV ? pmulc(pin(x[2][k]), pin(w2)) : pmul(pin(x[2][k]), pin(w2)));
        dft3<INV>(z);
#pragma unroll
        for (int p = 0; p < 3; ++p) x[p][k] = z[p];
    }
}

// W600 table and the four-step table tw2[m1][l] = W200^{l m1} = W600^{3 l m1}
__device__ __forceinline__ void load_tw600(float2 *twL, float2 *tw2, const float2 *__restrict__ tw_L) {
    for (int i = threadIdx.x; i < L; i += blockDim.x) twL[i] = tw_L[i];
    for (int i = threadIdx.x; i < 200; i += blockDim.x) tw2[i] = tw_L[(3 * (i / 10) * (i % 10)) % L];
    __syncthreads();
}

// pass 1: row IDFTs of the live spectrum rows (see k_crop_rows).  grid
// (ceil(nlive / (6 W)), B), block 64 W
template <int W>
__global__ void __launch_bounds__(64 * W) k_crop_rows600(const float2 *__restrict__ spec, float2 *__restrict__ out,
                                                         const float2 *__restrict__ tw_L, int sy0, int sy1, int sx0,
                                                         int sx1) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *twL = sm, *tw2 = sm + L, *tiles = tw2 + 200;  // 6 W exchange tiles of 100 + a dummy
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gw = lane / 10;
    const bool act = gw < GPW;
    const int l = act ? lane - 10 * gw : 0, g = w * GPW + (act ? gw : 0);
    // lanes 60..63 run the transform too (no divergence); their exchange goes
    // to a dummy tile so it cannot race with group 0's
    float2 *tile = tiles + (act ? g : GPW * W) * 100;
    const int xrd = opaque_i(l * kXP10);
    load_tw600(twL, tw2, tw_L);
    const int b = blockIdx.y, srow = sy0 + blockIdx.x * GPW * W + g;
    const bool live = act && srow <= sy1;
    const int row = srow + H < L ? srow + H : srow - H;  // objF row = spec row + L/2
    const float2 *src = spec + (size_t)b * L * L + (size_t)(srow <= sy1 ? srow : sy1) * L;
    float2 x[3][20];
#pragma unroll
    for (int k = 0; k < 20; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // element roll by L/2: register k -> k + 10
            const int sc = 3 * (l + 10 * k) + c;
            x[c][(k + 10) % 20] = in_band(sc, sx0, sx1) ? src[sc] : make_float2(0.f, 0.f);
        }
    dft600_regs<true>(x, tile, tw2, twL, l, xrd);
    if (!live) return;
    float2 *dst = out + (size_t)b * L * L + (size_t)row * L;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < 20; ++k) dst[l + 10 * k + 200 * p] = x[p][k];
}

// pass 2: column IDFTs in place, scaled 1/L^2, one strip of G = 6 W columns
// per block staged through LDS in NH pieces of L / NH rows (see k_crop_cols).
// Piece h holds input registers k in [h K, (h + 1) K), K = 20 / NH (element
// 3 (l + 10 k) + c, 3 l + c < 30, never straddles a piece boundary of a
// multiple of 30 rows) and the output registers whose rows 10 k + 200 p + l
// (l < 10) fall in it.  The strip moves as 16-byte loads and stores (two
// columns per thread); the loads of piece h + 2 are issued as soon as piece h
// has left its registers, so two pieces are in flight while the block works
// (round 3's version loaded piece by piece with 8-byte loads: 2.4 TB/s, SQ
// wait_any 0.65 of wave cycles).  W 4 / NH 2: 24-column strips (192-byte row
// segments, 64-byte aligned), 59 KB pieces, both pieces' loads in flight from
// the start (round 5: NH 4 -> 2 took config 3's objCrop from 0.448 to 0.345
// ms per step; NH 1, a 600-row strip and one block per CU, 0.45 ms;
// profiles/r05_ab/crop600_pieces_ab.txt).
// grid (ceil(L / G), B), block 64 W
template <int W, int NH>
__global__ void __launch_bounds__(64 * W) k_crop_cols600(float2 *__restrict__ io, const float2 *__restrict__ tw_L,
                                                         float scale, int sy0, int sy1) {
    constexpr int G = GPW * W, SP = G + 1, HH = L / NH, K = 20 / NH, G2 = G / 2;
    static_assert(L % NH == 0 && HH % 30 == 0 && 20 % NH == 0, "pieces of whole 30-row runs");
    static_assert(L % G == 0 && G % 2 == 0, "whole strips of column pairs");
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *twL = sm, *tw2 = sm + L, *strip = tw2 + 200;  // HH x SP
    float2 *tiles = strip;  // exchange tiles inside the strip: used only while every column is in registers
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gw = lane / 10;
    const bool act = gw < GPW;
    const int l = act ? lane - 10 * gw : 0, g = w * GPW + (act ? gw : 0);
    float2 *tile = tiles + (act ? g : G) * 100;  // lanes 60..63: dummy tile (see k_crop_rows600)
    const int xrd = opaque_i(l * kXP10);
    load_tw600(twL, tw2, tw_L);
    const int b = blockIdx.y, c0 = blockIdx.x * G;
    float2 *base = io + (size_t)b * L * L + c0;
    constexpr int NTH = 64 * W, NLD = (HH * G2 + NTH - 1) / NTH;
    // objF row y (0 <= y < L) is spec row (y + H) mod L: the live rows of
    // piece h, [h HH, (h+1) HH), form the contiguous range [ya, yb] relative
    // to the piece (HH divides H, so a piece never wraps)
    auto live = [&](int h, int &ya, int &yb) {
        const int s0 = h * HH >= H ? h * HH - H : h * HH + H;  // spec row of the piece's first row
        ya = max(sy0 - s0, 0);
        yb = min(sy1 - s0, HH - 1);
    };
    float4 q[2][NLD];
    auto issue = [&](int h) {
        int ya, yb;
        live(h, ya, yb);
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = ya * G2 + threadIdx.x + k * NTH;
            if (idx < (yb + 1) * G2) {
                const int y = idx / G2, cc = 2 * (idx - y * G2);
                q[h & 1][k] = *(const float4 *)(base + (size_t)(y + h * HH) * L + cc);
            }
        }
    };
    issue(0);
    issue(1);
    float2 x[3][20];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        int ya, yb;
        live(h, ya, yb);
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = ya * G2 + threadIdx.x + k * NTH;
            if (idx < (yb + 1) * G2) {
                const int y = idx / G2, cc = 2 * (idx - y * G2);
                strip[y * SP + cc] = make_float2(q[h & 1][k].x, q[h & 1][k].y);
                strip[y * SP + cc + 1] = make_float2(q[h & 1][k].z, q[h & 1][k].w);
            }
        }
        if (h + 2 < NH) issue(h + 2);
        __syncthreads();
#pragma unroll
        for (int k = K * h; k < K * h + K; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int y = 3 * (l + 10 * k) + c - h * HH;
                x[c][k] = (act && y >= ya && y <= yb) ? strip[y * SP + g] : make_float2(0.f, 0.f);
            }
        __syncthreads();
    }
    dft600_regs<true>(x, tile, tw2, twL, l, xrd);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        __syncthreads();  // exchange tiles / previous piece's reads are done
        if (act) {
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int k = 0; k < 20; ++k)
                    if ((10 * k + 200 * p) / HH == h)
                        strip[(l + 10 * k + 200 * p - h * HH) * SP + g] = cscale(x[p][k], scale);
        }
        __syncthreads();
#pragma unroll 4
        for (int idx = threadIdx.x; idx < HH * G2; idx += NTH) {
            const int y = idx / G2, cc = 2 * (idx - y * G2);
            const float2 p0 = strip[y * SP + cc], p1 = strip[y * SP + cc + 1];
            *(float4 *)(base + (size_t)(y + h * HH) * L + cc) = make_float4(p0.x, p0.y, p1.x, p1.y);
        }
    }
}

// L 600: row pass 12 rows per block (2 waves; 6 rows: 0.345 -> 0.336 ms
// per step), column pass 24-column strips in two pieces
constexpr int WR = 2, WC = 4, NHC = 2;
}  // namespace c600

}  // namespace

CropPair crop600_kernels() {
    using namespace c600;
    constexpr int GC = GPW * WC;
    constexpr size_t strip = (size_t)(L / NHC) * (GC + 1) > (size_t)(GC + 1) * 100 ? (size_t)(L / NHC) * (GC + 1)
                                                                                  : (size_t)(GC + 1) * 100;
    return {crop_kernel((const void *)k_crop_rows600<WR>, 64 * WR,
                        (size_t)(L + 200 + (GPW * WR + 1) * 100) * sizeof(float2), GPW * WR),
            crop_kernel((const void *)k_crop_cols600<WC, NHC>, 64 * WC, (L + 200 + strip) * sizeof(float2), GC)};
}

}  // namespace fpm
