// residual.hip -- the data-fidelity residual of the current state
// (fpm_residual, fpm_hip.h): for the LED at position i of order[]
//     E[i] = sum_yx (|psi_i(y,x)| - sqrt(I_i(y,x)))^2,   S[i] = sum_yx I_i
// with psi_i = ifft2(ifftshift(window_i(O)) P) / Np^2, the reference's
// ObjcropP (fpmMain.cpp:358-365), evaluated without any update.  This is the
// first third of an LED step (general.hip K1 and the first half of K2), and
// unlike the update loop every LED is independent: one launch covers a batch
// of nl LEDs x all B patches (blockIdx.z, or the leading factor of the 1-D
// grids, is the LED of the batch), so a few large patches still fill the chip.
// Nothing here writes the state: the kernels read the spectrum, the pupil and
// the stack, and write only the context's residual scratch.
//
//   rows  k_res_rows_tiled / k_res_rows     O P on the disk, row IDFTs of the
//         k_res_rows256                      box rows, T[nl][B][nb][Np] stored
//   cols  k_res_cols_wave / _tiled /        box rows of T, column IDFT,
//         k_res_cols, k_res_cols256          (|psi| - sqrt(I))^2 and I summed
//                                            into one partial per block
//   fold  k_res_fold                        a (LED, patch)'s partials added in
//                                            index order
// The LDS pair (any Np = 2^a 3^b 5^c) follows general.hip's tiled and
// wave-private-column kernels and their one-sequence-per-block fallback; the
// register pair (Np 256, fp32 spectrum, the stack in the g = 16 column
// layout) follows np256.hip's R1 / C
// without the commit, the amplitude replacement, the forward transform and
// the write-back.
//
// The stack is read where it lies (DevState::meas_g): pixel (y, x) of an image
// is at y Np + x in the C-ABI layout (g = 0) and at
// x Np + (y mod g)(Np / g) + y / g in the column layouts (g = 16, 10, 9, or Np:
// transposed), as in k_init_amp (init.hip).
//
// Summation is deterministic: lanes accumulate squared differences in fp32
// and the intensities as integers, waves and blocks reduce in double and
// 64-bit integers in a fixed order, each block writes one partial, and the
// fold adds them in index order -- no atomics, and a (LED, patch)'s value does
// not depend on the batch it ran in.
#include <algorithm>

#include "dftL.hpp"
#include "fft_inplace.hpp"
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

namespace {

// (|psi| - sqrt(I))^2 of one pixel added to acc: v = the unscaled IDFT value,
// psi = v / Np^2 (the reference's ifft2 scaling), no eps.  I is exact and
// sqrt(I) is not, so where |psi| < sqrt(I) / 2 the square is expanded around
// I, |psi| (|psi| - 2 sqrt(I)) + I: the term is >= I / 4 there, so both
// forms keep fp32 relative accuracy, and a pixel the model leaves exactly
// dark (a window off the spectrum's support) contributes exactly I -- such a
// lane's fp32 sum is a sum of integers below 2^24, so E = S to the bit.
__device__ __forceinline__ float res_add(float acc, float2 v, float inv_n2, unsigned I) {
    const float a = sqrtf(cabs2(v)) * inv_n2, fi = (float)I, s = sqrtf(fi);
    const float d = a - s;
    return acc + (2.0f * a < s ? __builtin_fmaf(a, a - 2.0f * s, fi) : d * d);
}

// centre of LED position i0 + z's sub-aperture and its stack index
__device__ __forceinline__ StepArgs res_led(const ResArgs &ra, int z, int np) {
    StepArgs sa;
    sa.led = ra.order[ra.i0 + z];
    sa.xc = ra.x0[sa.led] + np / 2;
    sa.yc = ra.y0[sa.led] + np / 2;
    return sa;
}

// The block's sums as one partial: lanes -> wave in double / u64 (xor
// butterfly, a fixed association), waves -> block in wave order by thread 0.
// Every thread of the block must call it.
template <int NW>
__device__ __forceinline__ void res_block_partial(float acc, unsigned isum, const ResArgs &ra, size_t slot) {
    __shared__ double dred[NW];
    __shared__ unsigned long long ured[NW];
    double d = (double)acc;
    unsigned long long u = isum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        d += __shfl_xor(d, o);
        u += __shfl_xor(u, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        dred[w] = d;
        ured[w] = u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NW; ++i) {
            d += dred[i];
            u += ured[i];
        }
        ra.perr[slot] = d;
        ra.pref[slot] = u;
    }
}

// ---- LDS pair: one sequence per block ------------------------------------------
// general.hip's k_gather_rowifft for a batch.  grid (nb, B, nl), block 256,
// LDS 2 Np complex
__global__ void __launch_bounds__(256) k_res_rows(DevState st, ResArgs ra, FftPlan pl,
                                                  const float2 *__restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int row = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const StepArgs sa = res_led(ra, z, np);
    float2 *bufa = smem, *bufb = smem + np;
    // st.pupil is the committed pupil: fpm_run ends every iteration with the
    // pupil commit (launch_pupil_commit after the last LED on the register paths)
    const float2 *pup = st.pupil + (size_t)b * nb * nb;
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = make_float2(0.f, 0.f);
    __syncthreads();
    const int yrow = sa.yc + row - r;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {
        if (st.disk[row * nb + j]) {
            const int kx = j - r;
            const float2 o = spec_ld(st, b, (size_t)yrow * st.L + sa.xc + kx);  // :358-362
            bufa[kx < 0 ? kx + np : kx] = cmul(o, pup[row * nb + j]);          // :364
        }
    }
    __syncthreads();
    float2 *res = stockham<true>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);  // :365 (rows)
    float2 *T = ra.T + (((size_t)z * st.B + b) * nb + row) * np;
    for (int i = threadIdx.x; i < np; i += blockDim.x) T[i] = res[i];
}

// One column per block.  grid (Np, B, nl), block 256, LDS 2 Np complex
__global__ void __launch_bounds__(256) k_res_cols(DevState st, ResArgs ra, FftPlan pl,
                                                  const float2 *__restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, g = st.meas_g;
    const int x = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int led = ra.order[ra.i0 + z];
    float2 *bufa = smem, *bufb = smem + np;
    const float2 *T = ra.T + ((size_t)z * st.B + b) * nb * np;
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int j = threadIdx.x; j < nb; j += blockDim.x) bufa[j - r < 0 ? j - r + np : j - r] = T[(size_t)j * np + x];
    __syncthreads();
    const float2 *res = stockham<true>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);  // :365 (columns)
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    const uint16_t *I = st.meas + ((size_t)led * st.mB + b) * np * np;
    float acc = 0.f;
    unsigned isum = 0;
    if (g) {  // uniform: the stored column x is contiguous, position p holds row (p mod (Np/g)) g + p / (Np/g)
        const int npg = np / g;
        const float rnpg = 1.0f / (float)npg;
        for (int p = threadIdx.x; p < np; p += blockDim.x) {
            const int t = udiv(p, npg, rnpg), m = p - t * npg;
            const unsigned iv = I[(size_t)x * np + p];
            acc = res_add(acc, res[m * g + t], inv_n2, iv);
            isum += iv;
        }
    } else {
        for (int y = threadIdx.x; y < np; y += blockDim.x) {
            const unsigned iv = I[(size_t)y * np + x];
            acc = res_add(acc, res[y], inv_n2, iv);
            isum += iv;
        }
    }
    res_block_partial<4>(acc, isum, ra, ((size_t)z * st.B + b) * ra.nblk + x);
}

// ---- LDS pair: tiled -----------------------------------------------------------
// general.hip's k_gather_rowifft_tiled for a batch: C = 2^lc box rows per block
// in one row-major LDS tile (row_pitch) with the twiddles beside it.
// grid (ceil(nb / C), B, nl), block NT
template <int NT, int E>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(E <= 16 ? 4 : 1)))
k_res_rows_tiled(DevState st, ResArgs ra, FftPlan pl, const float2 *__restrict__ tw, int lc) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, C = 1 << lc, lss = row_pitch(np, lc);
    const int j0 = blockIdx.x << lc, b = blockIdx.y, z = blockIdx.z;
    const StepArgs sa = res_led(ra, z, np);
    const int cs = min(C, nb - j0);
    float2 *tile = smem, *stw = smem + (size_t)C * lss;
    // the committed pupil (k_res_rows)
    const float2 *pup = st.pupil + (size_t)b * nb * nb;
    for (int i = threadIdx.x; i < np; i += NT) stw[i] = tw[i];
    for (int i = threadIdx.x; i < C * lss; i += NT) tile[i] = make_float2(0.f, 0.f);
    __syncthreads();
    const float rnb = 1.0f / (float)nb;
    for (int idx = threadIdx.x; idx < cs * nb; idx += NT) {
        const int c = udiv(idx, nb, rnb), j = idx - c * nb, row = j0 + c;
        if (!st.disk[row * nb + j]) continue;
        const int kx = j - r;
        const float2 o = spec_ld(st, b, (size_t)(sa.yc + row - r) * st.L + sa.xc + kx);  // :358-362
        tile[c * lss + (kx < 0 ? kx + np : kx)] = cmul(o, pup[row * nb + j]);            // :364
    }
    __syncthreads();
    tile_transform_ex<true, NT, E>(tile, pl, lc, lss, 1, stw);                              // :365 (rows)
    float2 *T = ra.T + (((size_t)z * st.B + b) * nb + j0) * np;
    const float rnp = 1.0f / (float)np;
    for (int idx = threadIdx.x; idx < cs * np; idx += NT) {
        const int c = udiv(idx, np, rnp), i = idx - c * np;
        T[(size_t)c * np + i] = tile[c * lss + i];
    }
}

// general.hip's k_colpass_tiled up to the column IDFT, then the residual sums:
// C = 2^lc adjacent columns per block, the box rows of T read as C*8-byte row
// segments.  The stack is read as C*2-byte row segments in the C-ABI layout
// and as the 2 Np contiguous bytes of each column in the column layouts.
// grid (ceil(Np / C), B, nl), block NT
template <int NT, int E>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(E <= 16 ? 4 : 1)))
k_res_cols_tiled(DevState st, ResArgs ra, FftPlan pl, const float2 *__restrict__ tw, int lc) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, C = 1 << lc, cm = C - 1, g = st.meas_g;
    const int x0 = blockIdx.x << lc, b = blockIdx.y, z = blockIdx.z;
    const int led = ra.order[ra.i0 + z];
    const int cs = min(C, np - x0);            // columns present in this tile
    float2 *tile = smem;                       // np * C
    float2 *stw = smem + (size_t)np * C;       // np twiddles
    const float2 *T = ra.T + ((size_t)z * st.B + b) * nb * np;
    for (int i = threadIdx.x; i < np; i += NT) stw[i] = tw[i];
    for (int i = threadIdx.x; i < np * C; i += NT) tile[i] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
        const int j = idx >> lc, c = idx & cm;
        const int i = j - r < 0 ? j - r + np : j - r;
        if (c < cs) tile[i * C + c] = T[(size_t)j * np + x0 + c];
    }
    __syncthreads();
    tile_transform<true, NT, E>(tile, pl, lc, stw);                                         // :365 (columns)
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    const uint16_t *I = st.meas + ((size_t)led * st.mB + b) * np * np;
    float acc = 0.f;
    unsigned isum = 0;
    // rows in natural order, the tile's C columns across adjacent lanes (no
    // LDS bank conflict); in a column layout row y of column x lies at
    // x Np + (y mod g)(Np / g) + y / g, so the block still reads each of its
    // columns' 2 Np bytes exactly once.  (Walking a stored column in memory
    // order instead would put a wave's 64 LDS reads 2^lc g rows apart, all in
    // one bank.)
    const int npg = g ? np / g : 1;
    const float rg = 1.0f / (float)(g ? g : 1);
    for (int idx = threadIdx.x; idx < np * C; idx += NT) {
        const int y = idx >> lc, c = idx & cm;
        if (c >= cs) continue;
        const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
        const unsigned iv = g ? I[(size_t)(x0 + c) * np + t * npg + m] : I[(size_t)y * np + x0 + c];
        acc = res_add(acc, tile[idx], inv_n2, iv);
        isum += iv;
    }
    res_block_partial<NT / 64>(acc, isum, ra, ((size_t)z * st.B + b) * ra.nblk + blockIdx.x);
}

// general.hip's k_colpass_wave up to the column IDFT, then the residual sums:
// every wave owns CW whole columns of the block's C = NW*CW-column tile
// (column-major, pitch P), so the radix passes synchronise the wave only.  A
// lane's measurement values (rows lane + 64 q of its wave's columns) are
// loaded before the transform, so their latency hides behind it.
// grid (ceil(Np / (NW*CW)), B, nl), block 64*NW, LDS (NW*CW*P + Np) complex
template <int NW, int CW>
__global__ void __launch_bounds__(64 * NW)
k_res_cols_wave(DevState st, ResArgs ra, FftPlan pl, const float2 *__restrict__ tw, int P) {
    constexpr int NT = 64 * NW, C = NW * CW, NQY = 16 / CW, LPC = 64 / CW;
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, g = st.meas_g;
    const int x0 = blockIdx.x * C, b = blockIdx.y, z = blockIdx.z;
    const int led = ra.order[ra.i0 + z];
    const int cs = min(C, np - x0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float2 *stw = smem + (size_t)C * P;
    float2 *wb = smem + (size_t)w * CW * P;
    float2 *cb = wb + (lane / LPC) * P;  // this lane's column in the radix passes
    const int l = lane % LPC;
    const float2 *T = ra.T + ((size_t)z * st.B + b) * nb * np;
    // this lane's measurement values, every load issued before the first use
    // (clamped in-bounds, masked afterwards); in a column layout row y of
    // column x lies at x Np + (y mod g)(Np / g) + y / g
    const uint16_t *I = st.meas + ((size_t)led * st.mB + b) * np * np;
    const int npg = g ? np / g : 1;
    const float rg = 1.0f / (float)(g ? g : 1);
    unsigned iv[NQY * CW];
#pragma unroll
    for (int q = 0; q < NQY; ++q) {
        const int y = min(lane + 64 * q, np - 1);
        const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const int x = x0 + min(w * CW + c, cs - 1);
            iv[q * CW + c] = g ? I[(size_t)x * np + t * npg + m] : I[(size_t)y * np + x];
        }
    }
    for (int i = threadIdx.x; i < np; i += NT) stw[i] = tw[i];
    // every tile element written once: box rows from T, zeros elsewhere
    const float rC = 1.0f / (float)C;
    for (int idx = threadIdx.x; idx < np * C; idx += NT) {
        const int i = udiv(idx, C, rC), c = idx - i * C;
        const int ky = i < np / 2 ? i : i - np, j = ky + r;
        float2 v = make_float2(0.f, 0.f);
        if (c < cs && j >= 0 && j < nb) v = T[(size_t)j * np + x0 + c];
        smem[c * P + i] = v;
    }
    __syncthreads();
    wave_transform<true, LPC>(cb, pl, stw, l);                                             // :365 (columns)
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    float acc = 0.f;
    unsigned isum = 0;
#pragma unroll
    for (int q = 0; q < NQY; ++q) {
        const int y = lane + 64 * q;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (y >= np || w * CW + c >= cs) continue;
            acc = res_add(acc, wb[c * P + y], inv_n2, iv[q * CW + c]);
            isum += iv[q * CW + c];
        }
    }
    res_block_partial<NW>(acc, isum, ra, ((size_t)z * st.B + b) * ra.nblk + blockIdx.x);
}

// ---- register pair: Np 256, fp32 spectrum, g = 16 ------------------------------
namespace r256 {
constexpr int N = 256, H = N / 2;
constexpr int WPB = 4;            // waves per block
constexpr int NT = 64 * WPB;
constexpr int GPB = 4 * WPB;      // 16-lane groups per block: rows or columns per block
constexpr int SP = GPB + 1;       // strip row pitch (complex)
static_assert(NT == N, "one twiddle per thread");
}  // namespace r256

__device__ __forceinline__ int fold256(int k) { return k < r256::H ? k : k - r256::N; }  // signed frequency

// block -> (LED z of the batch, patch b, sub-block) of a 1-D grid of
// nl * nsub * xcd_patches(B) blocks, patch b on XCD b mod 8 as np256.hip's
// xcd_block places it (nsub * xcd_patches(B) is a multiple of 8, so the LED
// does not move the XCD): a (LED, patch)'s T is written and read back through
// one XCD's L2.  false for the padding blocks of patches b >= B.
__host__ __device__ __forceinline__ int xcd_patches(int B) { return (B + 7) & ~7; }
__device__ __forceinline__ bool res_xcd_block(int nsub, int B, int &z, int &b, int &sub) {
    const int per = nsub * xcd_patches(B);
    const int id = blockIdx.x;
    z = id / per;
    const int k = (id - z * per) >> 3, q = k / nsub;
    b = (id & 7) + 8 * q;
    sub = k - q * nsub;
    return b < B;
}

// np256.hip's R1 without the commit: a group per support-box row.
// grid (nl * ceil(nb / GPB) * xcd_patches(B)), block NT, LDS (N + GPB XTILE_H) complex
__global__ void __launch_bounds__(r256::NT) k_res_rows256(DevState st, ResArgs ra, const float2 *__restrict__ tw) {
    using namespace r256;
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int g = threadIdx.x >> 4, t = threadIdx.x & 15, xrd = exch_rbase_half(t);
    const int r = st.r, nb = st.nb;
    int z, b, sub;
    if (!res_xcd_block((nb + GPB - 1) / GPB, st.B, z, b, sub)) return;  // block-uniform
    const StepArgs sa = res_led(ra, z, N);
    const int row = sub * GPB + g;
    const float2 twv = tw[threadIdx.x];
    float2 *twL = sm;
    float2 *wt = sm + N + g * XTILE_H;
    const int rowc = row < nb ? row : nb - 1;  // groups past the box: in-bounds loads, discarded
    const int ky = rowc - r, w2 = r * r - ky * ky;
    // the committed pupil (k_res_rows)
    const float2 *pup = st.pupil + ((size_t)b * nb + rowc) * nb + r;  // indexed by kx
    const float2 *sp = st.spec + (size_t)b * st.L * st.L + (size_t)(sa.yc + ky) * st.L + sa.xc;  // + kx (:358-362)
    // every load of the row issued before the first use (unconditional: a
    // lane off the disk reads the row's centre pixel and masks it)
    float2 pv[16], ov[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int kx = fold256(t + 16 * j);
        const int kc = kx * kx <= w2 ? kx : 0;
        pv[j] = pup[kc];
        ov[j] = sp[kc];
    }
    sm[threadIdx.x] = twv;
    __syncthreads();
    if (row >= nb) return;  // group-uniform; no block barrier follows
    float2 x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int kx = fold256(t + 16 * j);
        x[j] = kx * kx <= w2 ? cmul(ov[j], pv[j]) : make_float2(0.f, 0.f);  // :364
    }
    float2 y[16];
    dft256_full<true, true>(x, y, wt, LdsTw{twL, t, 1}, t, xrd);  // :365 (rows); y[k] = X[t + 16 k]
    float2 *T = ra.T + (((size_t)z * st.B + b) * nb + row) * N + t;
#pragma unroll
    for (int k = 0; k < 16; ++k) T[16 * k] = y[k];
}

// np256.hip's C up to the column IDFT, then the residual sums: a block per 16
// adjacent columns (a group each).
// grid (nl * (N / GPB) * xcd_patches(B)), block NT, LDS (N + max(nb SP, GPB XTILE_H)) complex
__global__ void __launch_bounds__(r256::NT) k_res_cols256(DevState st, ResArgs ra, const float2 *__restrict__ tw) {
    using namespace r256;
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int g = threadIdx.x >> 4, t = threadIdx.x & 15, xrd = exch_rbase_half(t);
    const int r = st.r, nb = st.nb;
    int z, b, sub;
    if (!res_xcd_block(N / GPB, st.B, z, b, sub)) return;  // block-uniform
    const int led = ra.order[ra.i0 + z];
    const int x0 = sub * GPB;
    const float2 twv = tw[threadIdx.x];
    float2 *twL = sm;
    float2 *strip = sm + N;              // nb x SP (box rows only); the group tiles
    float2 *wt = strip + g * XTILE_H;    // alias it while every column is in registers
    const float2 *T = ra.T + ((size_t)z * st.B + b) * nb * N + x0;
    // this group's measurement column, rows t + 16 m (meas_layout g = 16:
    // stored[x Np + 16 t + m] = I[t + 16 m][x]), two 16-byte loads per lane
    const uint4 *Ic = (const uint4 *)(st.meas + (((size_t)led * st.mB + b) * N + x0 + g) * N + 16 * t);
    const uint4 ia = Ic[0], ib = Ic[1];
    // the box rows of the strip: 128-byte row segments, every load of a
    // thread issued before its LDS stores (clamped, masked)
    constexpr int KMAX = N * GPB / NT;  // nb <= N rows
    const int tot = nb * GPB;
    float2 tv[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int idx = min((int)threadIdx.x + NT * k, tot - 1);
        if (NT * k < tot) tv[k] = T[(size_t)(idx / GPB) * N + (idx % GPB)];  // uniform guard
    }
    sm[threadIdx.x] = twv;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int idx = (int)threadIdx.x + NT * k;
        if (NT * k < tot && idx < tot) strip[(idx / GPB) * SP + (idx % GPB)] = tv[k];
    }
    __syncthreads();
    // FFT row i of a column is box row i + r (i <= r) or i - N + r (i >= N - r);
    // every other row is zero (:364)
    auto boxrow = [&](int i) { return i <= r ? i + r : (i >= N - r ? i - N + r : -1); };
    float2 v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int j = boxrow(t + 16 * m);
        v[m] = j >= 0 ? strip[j * SP + g] : make_float2(0.f, 0.f);
    }
    __syncthreads();  // the strip is the groups' exchange space from here
    float2 y[16];
    dft256_full<true, true>(v, y, wt, LdsTw{twL, t, 1}, t, xrd);  // :365 (columns); y[m] = row t + 16 m
    const float inv_n2 = 1.0f / ((float)N * (float)N);
    const unsigned iw[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
    float acc = 0.f;
    unsigned isum = 0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const unsigned iv = (iw[m >> 1] >> (16 * (m & 1))) & 0xffffu;
        acc = res_add(acc, y[m], inv_n2, iv);
        isum += iv;
    }
    res_block_partial<WPB>(acc, isum, ra, ((size_t)z * st.B + b) * ra.nblk + sub);
}

// ---- fold ----------------------------------------------------------------------
// a thread per (LED of the batch, patch): its nblk partials in index order
__global__ void __launch_bounds__(256) k_res_fold(ResArgs ra, int nl, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nl * B) return;
    const double *pe = ra.perr + (size_t)i * ra.nblk;
    const unsigned long long *pr = ra.pref + (size_t)i * ra.nblk;
    double e = 0.0;
    unsigned long long s = 0;
    for (int k = 0; k < ra.nblk; ++k) {
        e += pe[k];
        s += pr[k];
    }
    const size_t o = (size_t)ra.i0 * B + i;  // [n_order][B]
    ra.err[o] = e;
    ra.ref[o] = (double)s;  // exact: S < 2^16 Np^2 < 2^53
}

}  // namespace

// ---- the plan and the launchers --------------------------------------------------
ResidualPlan plan_residual(const DevState &st, const FftPlan &pl, int n_order, int meas_g, bool fp16,
                           const Switches &sw) {
    using namespace r256;
    ResidualPlan p{};
    p.pl = pl;
    const int np = st.np, nb = st.nb, B = st.B;
    // the register pair wherever the stack lies in the g = 16 column layout
    // (the Np 256 fused kernels and the Np 256 register general path)
    const bool lds_only = sw.res_lds || sw.res_one_seq;
    p.kind = np == N && meas_g == 16 && !fp16 && st.r >= 1 && st.r < H && !lds_only ? ResidualPlan::Reg256
                                                                                     : ResidualPlan::Lds;
    if (p.kind == ResidualPlan::Reg256) {
        const int Bp = xcd_patches(B);
        p.rows = StepKernel{(const void *)k_res_rows256, dim3(((nb + GPB - 1) / GPB) * Bp), dim3(NT),
                            (size_t)(N + GPB * XTILE_H) * sizeof(float2), 0};
        p.cols = StepKernel{(const void *)k_res_cols256, dim3((N / GPB) * Bp), dim3(NT),
                            (size_t)(N + std::max(nb * SP, GPB * XTILE_H)) * sizeof(float2), 0};
        p.nblk = N / GPB;
    } else {
        const size_t lds = 2 * (size_t)np * sizeof(float2);  // of the one-sequence kernels
        // up to 16 box rows / 16 columns per block, as many as fit the in-place
        // transform (general.hip trades them for blocks when a few large
        // patches leave the chip short; here the batch supplies the blocks)
        // (FPM_RES_ONE_SEQ=1: the fallback of sizes where not even two fit, at any size)
        int lr = sw.res_one_seq ? 0 : 4;
        while (lr > 0 && !fft_fits(pl, lr, 256)) --lr;
        if (lr > 0) {
            const bool r16 = fft_fits(pl, lr, 256, 16);
            p.rows = StepKernel{r16 ? (const void *)k_res_rows_tiled<256, 16> : (const void *)k_res_rows_tiled<256, 24>,
                                dim3((nb + (1 << lr) - 1) >> lr, B), dim3(256),
                                ((size_t)row_pitch(np, lr) * (1 << lr) + np) * sizeof(float2), lr};
        } else {
            p.rows = StepKernel{(const void *)k_res_rows, dim3(nb, B), dim3(256), lds, 0};
        }
        int lc = sw.res_one_seq ? 0 : 4;
        while (lc > 0 && !fft_fits(pl, lc)) --lc;
        // wave-private columns where a wave holds at least two (Np <= 512: 4
        // waves x 4 or 2 columns), as general.hip's K2; FPM_NO_WAVE_COLS=1: tiled
        const int cw = colw_cw(pl);
        if (cw > 1 && !sw.no_wave_cols && !sw.res_one_seq) {
            const int P = colw_pitch(np), C = 4 * cw;
            p.cols = StepKernel{cw == 4 ? (const void *)k_res_cols_wave<4, 4> : (const void *)k_res_cols_wave<4, 2>,
                                dim3((np + C - 1) / C, B), dim3(256), ((size_t)C * P + np) * sizeof(float2), P};
        } else if (lc > 0) {
            p.cols = StepKernel{nullptr, dim3((np + (1 << lc) - 1) >> lc, B), dim3(256),
                                ((size_t)np * (1 << lc) + np) * sizeof(float2), lc};
            if (fft_fits(pl, lc, 256, 16)) {
                p.cols.fn = (const void *)k_res_cols_tiled<256, 16>;
            } else if (fft_fits(pl, lc, 256)) {
                p.cols.fn = (const void *)k_res_cols_tiled<256, 24>;
            } else {
                p.cols.block = dim3(kFftThreads);
                p.cols.fn = fft_fits(pl, lc, kFftThreads, 16) ? (const void *)k_res_cols_tiled<kFftThreads, 16>
                                                              : (const void *)k_res_cols_tiled<kFftThreads, 24>;
            }
        } else {
            p.cols = StepKernel{(const void *)k_res_cols, dim3(np, B), dim3(256), lds, 0};
        }
        p.nblk = (int)p.cols.grid.x;
    }
    // LEDs per launch: as many as the scratch cap holds (FPM_RES_BATCH=n forces n)
    p.t_led = (size_t)B * nb * np;
    const size_t fit = kResidualScratchBytes / (p.t_led * sizeof(float2));
    p.nl = sw.res_batch > 0 ? sw.res_batch : (int)std::min<size_t>(std::max<size_t>(fit, 1), 65535);
    p.nl = std::max(1, std::min({p.nl, n_order, 65535}));
    return p;
}

hipError_t prepare_residual(const ResidualPlan &p) {
    // beyond the 64 KB a launch may take by default (Np 1024 and up, tiled columns)
    for (const StepKernel *k : {&p.rows, &p.cols})
        if (k->lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k->lds);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t launch_residual_batch(const ResidualPlan &p, const DevState &st, const ResArgs &ra_in, int nl,
                                 const float2 *tw, hipStream_t s) {
    DevState sv = st;
    ResArgs ra = ra_in;
    ra.nblk = p.nblk;
    FftPlan pl = p.pl;
    for (const StepKernel *k : {&p.rows, &p.cols}) {
        dim3 grid = k->grid;
        int arg = k->arg;
        hipError_t e;
        if (p.kind == ResidualPlan::Reg256) {
            grid.x *= nl;
            void *args[] = {&sv, &ra, &tw};
            e = hipLaunchKernel(k->fn, grid, k->block, args, k->lds, s);
        } else {
            grid.z = nl;
            void *args[] = {&sv, &ra, &pl, &tw, &arg};  // the one-sequence kernels take the first four
            e = hipLaunchKernel(k->fn, grid, k->block, args, k->lds, s);
        }
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_res_fold, dim3((nl * st.B + 255) / 256), dim3(256), 0, s, ra, nl, st.B);
    return hipGetLastError();
}

}  // namespace fpm
