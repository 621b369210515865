// update.hpp -- the per-pixel arithmetic of an LED step: the object update and
// pupil numerator of the fused LED-update kernels (slot_update) and of the
// general path (general_update), and the general path's amplitude replacement.
#pragma once
#include <hip/hip_runtime.h>

#include "cpk.hpp"
#include "fft_lds.hpp"
#include "fpm_state.hpp"

namespace fpm {

// Object update and pupil numerator of one support pixel (fpmMain.cpp:405-471),
// packed FP32: with D = Objfup - ObjfcropP (:409),
//   O' = O + D conj(P) |P| / ((|P|^2 + d2 + i d2im) max|P|)      (:406-419,433)
//   num = D conj(O) |O| / (|O|^2 + d1 + i d1im)  (/ max|objF| at the commit)
// The complex reciprocal is taken scale-safely: with a = |X|^2 + delta and
// q = c / a, 1 / ((a + ic) m) = (1 - iq) / (a (1 + q^2) m), so no intermediate
// exceeds a (the form (a - ic) / ((a^2 + c^2) m) squares a = |O|^2 + d1, i.e.
// |O|^4, which overflows fp32 once |O| reaches ~3e9).  The real factor |P|
// (|O|) is folded into the coefficient.  The object and the pupil coefficient
// are computed side by side: every transcendental is followed by the other
// chain's independent one instead of its own use (a trans-use hazard wait
// state each time in the chained order), and never more than two in a row
// (four in a row measured slower).  Every fused kernel
// calls this one function; tests/test_gpu_update_coef.py pins it through
// fpm_debug_slot_update up to |O|^2 + delta1 = 1e30.
// GAIN, g: the LED's gain (fused_gain): the measured amplitude is g sqrt(I),
// and the transform after the amplitude replacement is linear, so Objfup = g f
// and D = g f - ObjfcropP, one packed multiply-add in place of the subtraction
// (g = 1.0f: g f is exact, the same bits).  Compile time, because the scalar
// costs the fused kernels registers they do not have (DESIGN.md section 4.6:
// 0.3 - 3.5 % of a launch): a context whose gains are all ones launches the
// GAIN = false instances, which are the kernels as they were.
template <bool GAIN>
__device__ __forceinline__ float2 slot_update(float2 f, float2 o, float2 p, float pm, float g, const DevState &st,
                                              float2 &num, float &oa) {
    const pf2 po = pin(o), pp = pin(p);
    const float pa2 = cabs2(p), oa2 = cabs2(o);
    const float pa = __builtin_amdgcn_sqrtf(pa2);
    oa = __builtin_amdgcn_sqrtf(oa2);
    pf2 D;
    if constexpr (GAIN) D = pin(f) * g - pmul(po, pp);
    else D = pin(f) - pmul(po, pp);
    const float ap = __builtin_fmaf(pa, pa, st.delta2), ao = __builtin_fmaf(oa, oa, st.delta1);
    const float rp = __builtin_amdgcn_rcpf(ap), ro = __builtin_amdgcn_rcpf(ao);
    const pf2 dp = pmulc(D, pp), dq = pmulc(D, po);
    const float qp = st.d2_im * rp, qo = st.d1_im * ro;
    const float xp = __builtin_fmaf(qp, qp, 1.0f) * pm, xo = __builtin_fmaf(qo, qo, 1.0f) * 1.0f;
    const float sp0 = __builtin_amdgcn_rcpf(xp), so0 = __builtin_amdgcn_rcpf(xo);
    const float fp = rp * pa, fo = ro * oa;
    const float sp = sp0 * fp, so = so0 * fo;
    num = pout(pmul(dq, (pf2){so, -qo * so}));
    return pout(po + pmul(dp, (pf2){sp, -qp * sp}));
}

// The same update in the general path (general.hip, np1024.hip, np256.hip),
// with IEEE divisions (upd_coef_div): F = Objfup (:394), o = the pre-update
// Objfcrop (:361); GAIN, g: the LED's gain (Objfup = g F, as in slot_update: a
// compile-time variant here too, config 5 measured 0.2 % either side of the
// parent with the factor at run time).  Returns O', writes the pupil numerator to num.
template <bool GAIN>
__device__ __forceinline__ float2 general_update(float2 F, float2 o, float2 p, float pm, float g, const DevState &st,
                                                 float2 &num) {
    const float2 D = csub(GAIN ? cscale(F, g) : F, cmul(o, p));  // Objfup - ObjfcropP (:409,463)
    // object update (:406-419,433): D |P| P* / ((|P|^2 + d2) max|P|)
    const float pa = cmag(p);
    const float2 dpc = cmul(cmul(D, cscale(cconj(p), pa)), upd_coef_div(pa * pa + st.delta2, st.d2_im, pm));
    // pupil numerator (:459-464,469): D |O| O* / (|O|^2 + d1); max|objF| at the commit
    const float oa = cmag(o);
    num = cmul(cmul(D, cscale(cconj(o), oa)), upd_coef_div(oa * oa + st.delta1, st.d1_im, 1.0f));
    return cadd(o, dpc);
}

// Amplitude replacement of one pixel (fpmMain.cpp:378-393): v = the unscaled
// IDFT value, psi = v / Np^2, I the measured intensity;
// psi' = sqrt(I) psi / |psi + eps| (eps on Re and Im)
__device__ __forceinline__ float2 amp_replace(float2 v, float inv_n2, uint16_t I, const DevState &st) {
    const float2 psi = cscale(v, inv_n2);
    const float a = sqrtf((float)I);
    const float tre = psi.x + st.eps, tim = psi.y + st.eps_im;
    const float mag = sqrtf(tre * tre + tim * tim);
    const float sc = a / mag;
    return make_float2(psi.x * sc, psi.y * sc);
}

}  // namespace fpm
