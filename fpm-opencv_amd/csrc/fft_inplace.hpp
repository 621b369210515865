// fft_inplace.hpp -- one radix pass of the in-place, register-lifted LDS
// transform and its capacity rules, shared by the batched transform
// (fft_batch.hip) and the tiled step kernels of the general path (general.hip).
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

}  // namespace fpm
