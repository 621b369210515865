// fft_batch.hip -- batched 1-D transforms of any length 2^a 3^b 5^c, in place
// over one LDS tile per block (fft_inplace.hpp): fpm_init's fft2
// (fpmMain.cpp:325) and objCrop for every L without a register kernel
// (objcrop.hip).
#include <algorithm>

#include "fft_inplace.hpp"
#include "launch.hpp"

namespace fpm {

// Batched 1-D transforms of `nseq` sequences of length pl.n per patch.
// element i of sequence s of patch b:
//   in [b*in_bs + ((s+sroll)%nseq)*in_ss + ((i+iroll)%n)*in_es]
//   out[b*out_bs + s*out_ss + i*out_es] = scale * DFT(in)[i]
// A block owns C = 2^lc consecutive sequences.  When the sequences are
// columns (in_es != 1) consecutive threads read consecutive sequences, so a
// wave touches 16 rows x C*8 contiguous bytes; the LDS tile is then
// sequence-interleaved (lss 1, les C).  For rows it is row-major with one pad
// element per row (lss n+1, les 1) so the butterflies of C sequences hit
// distinct banks.
template <bool INV>
__global__ void __launch_bounds__(kFftThreads) k_fft_batch(const float2 *in, float2 *out, FftPlan pl,
                                                           const float2 *__restrict__ tw, int lc, int nseq,
                                                           size_t in_bs, int in_ss, int in_es, size_t out_bs,
                                                           int out_ss, int out_es, int sroll, int iroll,
                                                           float scale, const __half2 *in16, float in16_scale,
                                                           FftBand band) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int n = pl.n, C = 1 << lc, cm = C - 1;
    const int s0 = blockIdx.x << lc, b = blockIdx.y;
    const int cs = min(C, nseq - s0);
    const bool colmajor = in_es != 1;
    const int lss = colmajor ? 1 : n + 1, les = colmajor ? C : 1;
    const float rn = 1.0f / (float)n;
    in += (size_t)b * in_bs;
    if (in16) in16 += (size_t)b * in_bs;
    out += (size_t)b * out_bs;
    const int tot = n << lc;
    // twiddle table in LDS after the tile (a global read per butterfly put an
    // L1 round trip on every pass's critical path)
    float2 *stw = smem + (size_t)C * (n + 1);
    for (int i = threadIdx.x; i < n; i += kFftThreads) stw[i] = tw[i];
    // all of a thread's loads are issued before any LDS store so their
    // latencies overlap (a rolled loop waits for each one in turn)
    float2 v[kFftRegElems];
    int at[kFftRegElems];
#pragma unroll
    for (int q = 0; q < kFftRegElems; ++q) {
        const int idx = threadIdx.x + q * kFftThreads;
        v[q] = make_float2(0.f, 0.f);
        at[q] = -1;
        if (idx < tot) {
            int sq, i;
            if (colmajor) { sq = idx & cm; i = idx >> lc; }
            else { sq = udiv(idx, n, rn); i = idx - sq * n; }
            at[q] = sq * lss + i * les;
            int gs = s0 + sq + sroll, gi = i + iroll;
            if (gs >= nseq) gs -= nseq;
            if (gi >= n) gi -= n;
            int eb = gi + band.eroll;
            if (eb >= n) eb -= n;
            // outside the band the input is exactly zero: skip the load
            if (sq < cs && gs >= band.qlo && gs <= band.qhi && eb >= band.elo && eb <= band.ehi) {
                const size_t ii = (size_t)gs * in_ss + (size_t)gi * in_es;
                if (in16) {  // fp16-stored spectrum (config 5): widen, undo the storage scale
                    const float2 f = __half22float2(in16[ii]);
                    v[q] = make_float2(f.x * in16_scale, f.y * in16_scale);
                } else {
                    v[q] = in[ii];
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kFftRegElems; ++q)
        if (at[q] >= 0) smem[at[q]] = v[q];
    __syncthreads();
    int Ns = 1;
    for (int st = 0; st < pl.nstages; ++st) {
        const int R = pl.radix[st];
        switch (R) {
            case 8: fft_inplace_pass<8, INV>(smem, n, lc, lss, les, Ns, stw); break;
            case 4: fft_inplace_pass<4, INV>(smem, n, lc, lss, les, Ns, stw); break;
            case 2: fft_inplace_pass<2, INV>(smem, n, lc, lss, les, Ns, stw); break;
            case 3: fft_inplace_pass<3, INV>(smem, n, lc, lss, les, Ns, stw); break;
            default: fft_inplace_pass<5, INV>(smem, n, lc, lss, les, Ns, stw); break;
        }
        Ns *= R;
    }
    const bool ocol = out_es != 1;
    for (int idx = threadIdx.x; idx < tot; idx += kFftThreads) {
        int sq, i;
        if (ocol) { sq = idx & cm; i = idx >> lc; }
        else { sq = udiv(idx, n, rn); i = idx - sq * n; }
        if (sq < cs) out[(size_t)(s0 + sq) * out_ss + (size_t)i * out_es] = cscale(smem[sq * lss + i * les], scale);
    }
}

// largest C = 2^lc with C*n complex values in registers across the block
// (kFftRegElems per thread; radix-5 passes hold 20) and at most 16 sequences
static int fft_log2_seq_per_block(const FftPlan &pl) {
    int cap = kFftRegElems * kFftThreads;
    for (int i = 0; i < pl.nstages; ++i) cap = std::min(cap, fft_pass_capacity(pl.radix[i]));
    int lc = 0;
    while (lc < 4 && (pl.n << (lc + 1)) <= cap) ++lc;
    return (pl.n << lc) <= cap ? lc : -1;
}

int fft_max_len() { return fft_pass_capacity(5); }  // the smallest of the radix-2/3/4/5 capacities

StepKernel fft_batch_kernel(const FftPlan &pl, bool inverse) {
    StepKernel k{};
    const int lc = fft_log2_seq_per_block(pl);
    if (lc < 0) return k;
    k.fn = inverse ? (const void *)k_fft_batch<true> : (const void *)k_fft_batch<false>;
    k.block = dim3(kFftThreads);
    // row-major tiles carry one pad element per sequence
    k.lds = (((size_t)1 << lc) * (pl.n + 1) + pl.n) * sizeof(float2);  // tile + twiddles
    k.arg = lc;
    return k;
}

hipError_t launch_fft_batch(bool inverse, const float2 *in, float2 *out, const FftPlan &pl, const float2 *tw,
                            int nseq, int B, size_t in_bs, int in_ss, int in_es, size_t out_bs, int out_ss,
                            int out_es, int sroll, int iroll, float scale, hipStream_t s, const __half2 *in16,
                            float in16_scale, FftBand band) {
    const StepKernel k = fft_batch_kernel(pl, inverse);
    if (!k.fn) return hipErrorInvalidValue;
    const int lc = k.arg, C = 1 << lc;
    const size_t lds = k.lds;
    dim3 grid((nseq + C - 1) / C, B);
    hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (inverse)
        hipLaunchKernelGGL(k_fft_batch<true>, grid, dim3(kFftThreads), lds, s, in, out, pl, tw, lc, nseq, in_bs,
                           in_ss, in_es, out_bs, out_ss, out_es, sroll, iroll, scale, in16, in16_scale, band);
    else
        hipLaunchKernelGGL(k_fft_batch<false>, grid, dim3(kFftThreads), lds, s, in, out, pl, tw, lc, nseq, in_bs,
                           in_ss, in_es, out_bs, out_ss, out_es, sroll, iroll, scale, in16, in16_scale, band);
    return hipGetLastError();
}

}  // namespace fpm
