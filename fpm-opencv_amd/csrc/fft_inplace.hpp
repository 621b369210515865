// fft_inplace.hpp -- one radix pass of the in-place, register-lifted LDS
// transform and its capacity rules, shared by the batched transform
// (fft_batch.hip), the tiled step kernels of the general path (general.hip) and
// the residual sweep (residual.hip), with the tile transforms built from it.
//
// The transform runs IN PLACE over one LDS buffer: every pass lifts all of a
// thread's butterflies into registers, barriers, and stores (<= E complex
// values per thread), so C*n can reach E*blockDim without a ping-pong buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_lds.hpp"

namespace fpm {

constexpr int kFftThreads = 512;
constexpr int kFftRegElems = 24;
// complex values a radix-R in-place pass can lift into registers across the block
inline int fft_pass_capacity(int R, int nt = kFftThreads, int e = kFftRegElems) { return e / R * R * nt; }

// C = 2^lc sequences of pl.n fit the in-place transform's register budget
inline bool fft_fits(const FftPlan &pl, int lc, int nt = kFftThreads, int e = kFftRegElems) {
    for (int i = 0; i < pl.nstages; ++i)
        if ((pl.n << lc) > fft_pass_capacity(pl.radix[i], nt, e)) return false;
    return true;
}

template <int R, bool INV, int NT = kFftThreads, int E = kFftRegElems>
__device__ __forceinline__ void fft_inplace_pass(float2 *buf, int n, int lc, int lss, int les, int Ns,
                                                 const float2 *__restrict__ tw) {
    constexpr int Q = E / R;
    const int nR = n / R, total = nR << lc, tmul = n / (Ns * R);
    const bool pow2 = (Ns & (Ns - 1)) == 0;
    const int lNs = 31 - __builtin_clz(Ns);
    const float rNs = 1.0f / (float)Ns;
    float2 v[Q][R];
    int dst[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int jj = threadIdx.x + q * NT;
        if (jj < total) {
            const int sq = jj & ((1 << lc) - 1), j = jj >> lc;
            const float2 *src = buf + sq * lss;
#pragma unroll
            for (int r = 0; r < R; ++r) v[q][r] = src[(j + r * nR) * les];
            const int jq = pow2 ? (j >> lNs) : udiv(j, Ns, rNs);
            const int k = j - jq * Ns;
            if (Ns > 1) {
                const int ts = tmul * k;
#pragma unroll
                for (int r = 1; r < R; ++r) {
                    float2 w = tw[r * ts];
                    if (INV) w.y = -w.y;
                    v[q][r] = cmul(v[q][r], w);
                }
            }
            if (R == 2) dft2<INV>(v[q]);
            if (R == 3) dft3<INV>(v[q]);
            if (R == 4) dft4<INV>(v[q]);
            if (R == 5) dft5<INV>(v[q]);
            if (R == 8) dft8<INV>(v[q]);
            dst[q] = sq * lss + (jq * Ns * R + k) * les;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int jj = threadIdx.x + q * NT;
        if (jj < total) {
#pragma unroll
            for (int r = 0; r < R; ++r) buf[dst[q] + r * Ns * les] = v[q][r];
        }
    }
    __syncthreads();
}

// ---- tiled transforms -----------------------------------------------------------
// runs the plan's passes in place over a C = 2^lc column tile (element i of
// column c at buf[i*C + c]); every thread of the block must call it
template <bool INV, int NT, int E>
__device__ __forceinline__ void tile_transform(float2 *buf, const FftPlan &pl, int lc, const float2 *stw) {
    int Ns = 1;
    for (int st = 0; st < pl.nstages; ++st) {
        const int R = pl.radix[st];
        switch (R) {
            case 8: fft_inplace_pass<8, INV, NT, E>(buf, pl.n, lc, 1, 1 << lc, Ns, stw); break;
            case 4: fft_inplace_pass<4, INV, NT, E>(buf, pl.n, lc, 1, 1 << lc, Ns, stw); break;
            case 2: fft_inplace_pass<2, INV, NT, E>(buf, pl.n, lc, 1, 1 << lc, Ns, stw); break;
            case 3: fft_inplace_pass<3, INV, NT, E>(buf, pl.n, lc, 1, 1 << lc, Ns, stw); break;
            default: fft_inplace_pass<5, INV, NT, E>(buf, pl.n, lc, 1, 1 << lc, Ns, stw); break;
        }
        Ns *= R;
    }
}

// the plan's passes in place over C = 2^lc sequences with arbitrary strides
// (row tiles: lss = n + 1, les = 1)
template <bool INV, int NT, int E>
__device__ __forceinline__ void tile_transform_ex(float2 *buf, const FftPlan &pl, int lc, int lss, int les,
                                                  const float2 *stw) {
    // radices smallest first, as in wave_transform: the stride-R writes of
    // the Ns = 1 pass then spread over the banks
    int Ns = 1;
    for (int st = pl.nstages - 1; st >= 0; --st) {
        const int R = pl.radix[st];
        switch (R) {
            case 8: fft_inplace_pass<8, INV, NT, E>(buf, pl.n, lc, lss, les, Ns, stw); break;
            case 4: fft_inplace_pass<4, INV, NT, E>(buf, pl.n, lc, lss, les, Ns, stw); break;
            case 2: fft_inplace_pass<2, INV, NT, E>(buf, pl.n, lc, lss, les, Ns, stw); break;
            case 3: fft_inplace_pass<3, INV, NT, E>(buf, pl.n, lc, lss, les, Ns, stw); break;
            default: fft_inplace_pass<5, INV, NT, E>(buf, pl.n, lc, lss, les, Ns, stw); break;
        }
        Ns *= R;
    }
}

// Row pitch of a C = 2^lc row tile: >= Np + 1 and = 32/C (mod 32), so the C
// rows a 32-lane read group touches (32/C consecutive elements each) are
// 64/C banks apart and cover the 64 banks once (Np + 1 put the C rows 2 banks
// apart: 2-4 way conflicts on every pass read).
__host__ __device__ inline int row_pitch(int np, int lc) {
    const int m = lc >= 5 ? 1 : 32 >> lc;
    int p = np + 1;
    while ((p & 31) != (m & 31)) ++p;
    return p;
}

// ---- wave-private columns (general.hip k_colpass_wave) ----
constexpr int kWaveElems = 16;  // register elements per lane in a wave pass

// one radix-R Stockham pass over the lane's column `cb` (lanes l, l + LPC,
// ... of the column's butterflies: l = lane % LPC)
template <int R, bool INV, int LPC>
__device__ __forceinline__ void wave_pass(float2 *cb, int n, int Ns, const float2 *__restrict__ tw, int l) {
    constexpr int Q = kWaveElems / R;
    const int nR = n / R, tmul = n / (Ns * R);
    const bool pow2 = (Ns & (Ns - 1)) == 0;
    const int lNs = 31 - __builtin_clz(Ns);
    const float rNs = 1.0f / (float)Ns;
    float2 v[Q][R];
    int base[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = l + LPC * q;
        base[q] = -1;
        if (j < nR) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[q][r] = cb[j + r * nR];
            const int jq = pow2 ? (j >> lNs) : udiv(j, Ns, rNs);
            const int k = j - jq * Ns;
            if (Ns > 1) {
                const int ts = tmul * k;
#pragma unroll
                for (int r = 1; r < R; ++r) {
                    float2 w = tw[r * ts];
                    if (INV) w.y = -w.y;
                    v[q][r] = cmul(v[q][r], w);
                }
            }
            if (R == 2) dft2<INV>(v[q]);
            if (R == 3) dft3<INV>(v[q]);
            if (R == 4) dft4<INV>(v[q]);
            if (R == 5) dft5<INV>(v[q]);
            if (R == 8) dft8<INV>(v[q]);
            base[q] = jq * Ns * R + k;
        }
    }
    wave_sync();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (base[q] >= 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) cb[base[q] + r * Ns] = v[q][r];
        }
    }
    wave_sync();
}

// The plan's radices run in reverse (smallest first: 200 = 5*5*8), so the
// stride-R writes of the Ns = 1 pass come from a radix whose stride spreads
// over the banks (a radix-8 first pass is a 4-way conflict on every write).
template <bool INV, int LPC>
__device__ __forceinline__ void wave_transform(float2 *cb, const FftPlan &pl, const float2 *stw, int l) {
    int Ns = 1;
    for (int s = pl.nstages - 1; s >= 0; --s) {
        const int R = pl.radix[s];
        switch (R) {
            case 8: wave_pass<8, INV, LPC>(cb, pl.n, Ns, stw, l); break;
            case 4: wave_pass<4, INV, LPC>(cb, pl.n, Ns, stw, l); break;
            case 2: wave_pass<2, INV, LPC>(cb, pl.n, Ns, stw, l); break;
            case 3: wave_pass<3, INV, LPC>(cb, pl.n, Ns, stw, l); break;
            default: wave_pass<5, INV, LPC>(cb, pl.n, Ns, stw, l); break;
        }
        Ns *= R;
    }
}

// column pitch of the tile: Np rounded to 2 mod 4, so the C columns of the
// coalesced load/store land in distinct banks and every column is 16-byte
// aligned
inline int colw_pitch(int np) {
    int p = np;
    while ((p & 3) != 2) ++p;
    return p;
}

// columns per wave of k_colpass_wave for this plan: the largest CW in {4,2,1}
// for which 64/CW lanes hold a column's butterflies in every radix pass
// (kWaveElems values per lane);
// 0 when even one column does not fit
inline int colw_cw(const FftPlan &pl) {
    for (int cw = 4; cw >= 1; cw >>= 1) {
        bool ok = true;
        for (int i = 0; i < pl.nstages; ++i) {
            const int R = pl.radix[i];
            const int lpc = 64 / cw;
            if ((pl.n / R + lpc - 1) / lpc > kWaveElems / R) ok = false;
        }
        if (ok) return cw;
    }
    return 0;
}

}  // namespace fpm
