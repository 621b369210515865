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
#include "fpm_hip.h"
#include "fpm_state.hpp"
#include "launch.hpp"
#include "np256_layout.hpp"

namespace fpm {

// GainResArgs and MomArgs (launch.hpp) are the same batch with another tail:
// the squared difference under the LED's gain, and the raw moments
// sum |psi|^2 and sum |psi| sqrt(I) (fpm_moments).  Everything before the tail
// is the ResArgs instance's, and the ResArgs instance -- what a context
// without gains launches -- has the tail it always had.
template <class A>
constexpr bool kIsMom = std::is_same<A, MomArgs>::value;
template <class A>
constexpr bool kIsGainRes = std::is_same<A, GainResArgs>::value;
// PredArgs (fpm_predict) shares the front half too and has no sums: its tail
// stores every pixel (pred_value, pred_store below).
template <class A>
constexpr bool kIsPred = std::is_same<A, PredArgs>::value;
// GradArgs (fpm_gradient) shares the front half and the gained sums, and goes
// on where the sweep stops: its tail is the update step's shape (grad_rho below
// in place of the amplitude replacement, then the forward column transform).
template <class A>
constexpr bool kIsGrad = std::is_same<A, GradArgs>::value;
template <class A>
constexpr bool kIsRes = std::is_same<A, ResArgs>::value || kIsGainRes<A> || kIsMom<A> || kIsPred<A> || kIsGrad<A>;

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
// The same under the LED's gain g (g2 = g g): (|psi| - g sqrt(I))^2, expanded
// around g2 I where |psi| < g sqrt(I) / 2.  With g = 1.0f both products are
// exact and the value is res_add's to the bit: the empty asm keeps the two
// products opaque, so nothing below fuses them into a multiply-add and the
// rest is res_add's own expression, contracted as the compiler contracts that
// (fused, the Np 90 / 200 / 2700 sweeps rounded differently from res_add).
__device__ __forceinline__ float res_add_gain(float acc, float2 v, float inv_n2, unsigned I, float g, float g2) {
    const float a = sqrtf(cabs2(v)) * inv_n2, fi = (float)I;
    float s = g * sqrtf(fi), gi = g2 * fi;
    asm("" : "+v"(s), "+v"(gi));
    const float d = a - s;
    return acc + (2.0f * a < s ? __builtin_fmaf(a, a - 2.0f * s, gi) : d * d);
}

// A lane's sums over its pixels, the tail of every column kernel's sweep
// instance.  ResArgs: e = sum (|psi| - sqrt(I))^2; GainResArgs: the same under
// the LED's gain.  MomArgs: q = sum |psi|^2 and c = sum |psi| sqrt(I), each
// product formed in fp32 and accumulated as e is; raw, the gain table does not
// enter.  s = sum I as an integer in all three.
// The gain a column kernel's tail needs, loaded at the top of the kernel (the
// scalar load's latency runs under the column transform): the LED's for the
// gained residual, none for the ungained one, the update step (its gain enters
// at the update) or the moments.
template <class A>
__device__ __forceinline__ float res_gain(const DevState &st, int led, int b) {
    if constexpr (kIsGainRes<A> || kIsPred<A> || kIsGrad<A>) return led_gain(st, led, b);
    else return 1.0f;
}

// ---- fpm_predict's tail: one pixel of the predicted image instead of a sum.
// The kind is uniform over the launch, so each switch is a scalar branch.
//   AMPLITUDE  |psi|, raw: the gain does not enter (as fpm_moments)
//   COUNTS     what the camera would record, rint((|psi| / g)^2) saturated at
//              65535 (half to even; an integer below 2^16, exact as a float)
//   DIFF       |psi| - g sqrt(I); the product kept opaque as in res_add_gain,
//              so g = 1.0f is bit for bit the ungained difference
// I is read by DIFF alone: the callers load it under the same uniform branch.
__device__ __forceinline__ bool pred_reads_stack(const PredArgs &pa) { return pa.kind == FPM_PREDICT_DIFF; }
__device__ __forceinline__ float pred_value(const PredArgs &pa, float2 v, float inv_n2, float g, unsigned I) {
    const float a = sqrtf(cabs2(v)) * inv_n2;
    if (pa.kind == FPM_PREDICT_COUNTS) {
        const float q = a / g;
        return fminf(rintf(q * q), 65535.0f);
    }
    if (pa.kind == FPM_PREDICT_DIFF) {
        float s = g * sqrtf((float)I);
        asm("" : "+v"(s));
        return a - s;
    }
    return a;
}
// the image of entry i0 + z and patch b in out, as an element offset, and the
// store of pixel off of out: 2 bytes for the counts, else 4
__device__ __forceinline__ size_t pred_image(const PredArgs &pa, int z, int B, int b, int np) {
    return ((size_t)(pa.i0 + z - pa.o0) * B + b) * np * np;
}
__device__ __forceinline__ void pred_store(const PredArgs &pa, size_t off, float val) {
    if (pa.kind == FPM_PREDICT_COUNTS) static_cast<uint16_t *>(pa.out)[off] = (uint16_t)val;
    else static_cast<float *>(pa.out)[off] = val;
}

// ---- fpm_gradient's tail: one pixel of rho = psi - g sqrt(I) psi / |psi|, the
// residual field whose forward transform is the gradient's R (gradient.hip).
// v = the unscaled IDFT value, psi = v / Np^2, no eps; written psi (a - s) / a
// with a = |psi| as the sums form it and s = g sqrt(I) kept opaque as in
// res_add_gain, so g = 1.0f gives the bits of no gain.  0 where |psi| = 0: a
// window off the spectrum's support leaves rho exactly zero.
__device__ __forceinline__ float2 grad_rho(float2 v, float inv_n2, unsigned I, float g) {
    const float a = sqrtf(cabs2(v)) * inv_n2;
    float s = g * sqrtf((float)I);
    asm("" : "+v"(s));
    const float f = a > 0.f ? (a - s) / a * inv_n2 : 0.f;
    return make_float2(v.x * f, v.y * f);
}

template <class A>
struct ResAcc {
    float e = 0.f, g, g2;
    unsigned s = 0;
    __device__ __forceinline__ explicit ResAcc(float gain) : g(gain), g2(gain * gain) {}
    __device__ __forceinline__ void add(float2 v, float inv_n2, unsigned I) {
        if constexpr (kIsGainRes<A> || kIsGrad<A>) e = res_add_gain(e, v, inv_n2, I, g, g2);
        else e = res_add(e, v, inv_n2, I);
        s += I;
    }
};
template <>
struct ResAcc<MomArgs> {
    float q = 0.f, c = 0.f;
    unsigned s = 0;
    __device__ __forceinline__ explicit ResAcc(float) {}
    __device__ __forceinline__ void add(float2 v, float inv_n2, unsigned I) {
        const float a = sqrtf(cabs2(v)) * inv_n2;
        q += a * a;
        c += a * sqrtf((float)I);
        s += I;
    }
};

// The LED a block works on: the step's own, or entry i0 + z of the batch's
// list (stack index and centre of its window, launch.hpp ResEntry) in one load
__device__ __forceinline__ StepArgs res_led(const StepArgs &sa, int, int) { return sa; }
__device__ __forceinline__ StepArgs res_led(const ResArgs &ra, int z, int) {  // (a MomArgs is a ResArgs)
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
// Every thread of the block must call it.  kResPartialLds: its __shared__ bytes,
// the same for both tails (the moments' second sum goes through the same
// arrays after a barrier), so one launch shape serves both instances.
template <int NW>
constexpr size_t kResPartialLds = NW * (sizeof(double) + sizeof(unsigned long long));
template <int NW, class A>
__device__ __forceinline__ void res_block_partial(const ResAcc<A> &acc, const A &ra, size_t slot) {
    __shared__ double dred[NW];
    __shared__ unsigned long long ured[NW];
    static_assert(sizeof dred + sizeof ured == kResPartialLds<NW>, "the create-time LDS check counts these arrays");
    double d, d2 = 0.0;
    if constexpr (kIsMom<A>) {
        d = (double)acc.q;
        d2 = (double)acc.c;
    } else {
        d = (double)acc.e;
    }
    unsigned long long u = acc.s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        d += __shfl_xor(d, o);
        u += __shfl_xor(u, o);
        if constexpr (kIsMom<A>) d2 += __shfl_xor(d2, o);
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
    if constexpr (kIsMom<A>) {  // the cross sums, same order, through dred again
        __syncthreads();
        if (lane == 0) dred[w] = d2;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < NW; ++i) d2 += dred[i];
            ra.pcross[slot] = d2;
        }
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
