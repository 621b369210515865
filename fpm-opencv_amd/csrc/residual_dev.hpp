// residual_dev.hpp -- what the LED step's kernels need to run as the residual
// sweep's (fpm_residual, residual.hip).  general.hip's K1 / K2 and np256.hip's
// C are templates over their argument struct: StepArgs is the update step of
// one LED, ResArgs a batch of (LED, window) entries whose tail sums
// (|psi| - sqrt(I))^2 and I into one partial per block instead of replacing
// the amplitude.  The overloads below give both the same front half; the
// sums are the ResArgs instances' tail.
#pragma once
#include <type_traits>

#include "cpk.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"
#include "np256_layout.hpp"

namespace fpm {

template <class A>
constexpr bool kIsRes = std::is_same<A, ResArgs>::value;

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

// The LED a block works on: the step's own, or entry i0 + z of the batch's
// list (stack index and centre of its window, launch.hpp ResEntry) in one load
__device__ __forceinline__ StepArgs res_led(const StepArgs &sa, int, int) { return sa; }
__device__ __forceinline__ StepArgs res_led(const ResArgs &ra, int z, int) {
    const int4 e = *reinterpret_cast<const int4 *>(ra.ent + ra.i0 + z);
    StepArgs sa;
    sa.led = e.x;
    sa.xc = e.y;
    sa.yc = e.z;
    return sa;
}

// Box row `row` of patch b in T: the state's [B][nb][Np], or the sweep's
// [nl][B][nb][Np] at LED z
__device__ __forceinline__ float2 *res_T(const DevState &st, const StepArgs &, int, int b, int row, int np) {
    return st.T + ((size_t)b * st.nb + row) * np;
}
__device__ __forceinline__ float2 *res_T(const DevState &st, const ResArgs &ra, int z, int b, int row, int np) {
    return ra.T + (((size_t)z * st.B + b) * st.nb + row) * np;
}

// The block's sums as one partial: lanes -> wave in double / u64 (xor
// butterfly, a fixed association), waves -> block in wave order by thread 0.
// Every thread of the block must call it.  kResPartialLds: its __shared__ bytes.
template <int NW>
constexpr size_t kResPartialLds = NW * (sizeof(double) + sizeof(unsigned long long));
template <int NW>
__device__ __forceinline__ void res_block_partial(float acc, unsigned isum, const ResArgs &ra, size_t slot) {
    __shared__ double dred[NW];
    __shared__ unsigned long long ured[NW];
    static_assert(sizeof dred + sizeof ured == kResPartialLds<NW>, "the create-time LDS check counts these arrays");
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

// block -> (LED z of the batch, patch b, sub-block) of a 1-D grid of
// nl * nsub * xcd_patches(B) blocks, patch b on XCD b mod 8 as xcd_block
// places it (nsub * xcd_patches(B) is a multiple of 8, so the LED does not
// move the XCD): a (LED, patch)'s T is written and read back through one
// XCD's L2.  false for the padding blocks of patches b >= B.
__device__ __forceinline__ bool res_xcd_block(int nsub, int B, int &z, int &b, int &sub) {
    const int per = nsub * xcd_patches(B);
    const int id = blockIdx.x;
    z = id / per;
    const int k = (id - z * per) >> 3, q = k / nsub;
    b = (id & 7) + 8 * q;
    sub = k - q * nsub;
    return b < B;
}

}  // namespace fpm
