// fused256.hpp -- register 256-point DFT building blocks of the Np 256 fused
// LED-update kernel (fpm_fused.hip): support-pruned 16-point DFTs, the
// four-step exchange variants and the twiddle holders.  Layout and pruning:
// see the fpm_fused.hip header.
#pragma once
#include <hip/hip_runtime.h>

#include "cpk.hpp"
#include "dft16.hpp"

namespace fpm {

// The register 16-point DFTs below compute in packed FP32 (cpk.hpp): every
// complex add/sub is one v_pk_add_f32, every twiddle multiply two VOP3P ops.
// Arrays are float2 at the interfaces (LDS and global memory) and pf2 inside;
// the conversions are bit casts of the same VGPR pairs.
template <int N>
__device__ __forceinline__ void to_pk(const float2 (&a)[N], pf2 (&p)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = pin(a[i]);
}
template <int N>
__device__ __forceinline__ void from_pk(const pf2 (&p)[N], float2 (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = pout(p[i]);
}

// 16-point DFT whose input is zero except v[0,1,2,13,14,15]
template <bool INV>
__device__ __forceinline__ void pdft16_in6(const pf2 (&in)[16], pf2 (&r)[16]) {
    // stage 1, butterfly k1 over positions (k1, k1+4, k1+8, k1+12)
    const pf2 a0 = in[0], b1 = in[1], b13 = in[13], c2 = in[2], c14 = in[14], d15 = in[15];
    pf2 v[16];
    // k1 = 0: (a0,0,0,0)
    v[0] = a0; v[4] = a0; v[8] = a0; v[12] = a0;
    // k1 = 1: (b1,0,0,b13): U[m] = b1 + b13 W4^{3m};  W4^3 = conj(W4) = -W4
    v[1] = b1 + b13;
    v[5] = psub_w4<INV>(b1, b13);
    v[9] = b1 - b13;
    v[13] = padd_w4<INV>(b1, b13);
    v[2] = c2 + c14;
    v[6] = psub_w4<INV>(c2, c14);
    v[10] = c2 - c14;
    v[14] = padd_w4<INV>(c2, c14);
    // k1 = 3: (0,0,0,d15): U[m] = d15 W4^{3m}
    const pf2 z = {0.f, 0.f};
    v[3] = d15;
    v[7] = psub_w4<INV>(z, d15);
    v[11] = -d15;
    v[15] = padd_w4<INV>(z, d15);
    pmid_tw<INV>(v);
    pstage2<INV>(v);
#pragma unroll
    for (int m = 0; m < 16; ++m) r[m] = v[4 * (m & 3) + (m >> 2)];
}

// 16-point DFT returning only outputs m in {0,1,2,13,14,15} as o[0..5]
template <bool INV>
__device__ __forceinline__ void pdft16_out6(pf2 (&v)[16], pf2 (&o)[6]) {
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) pbf4<INV>(v[k1], v[k1 + 4], v[k1 + 8], v[k1 + 12]);
    pmid_tw<INV>(v);
    // stage 2 over k1 for fixed m1 (positions 4 m1 + k1): y0 = sum, y3 = (a0-a2) - W4(a1-a3);
    // m1 = 2 carries the W16^4 twiddle of position 10 (a2 -> W4 a2)
    o[0] = (v[0] + v[2]) + (v[1] + v[3]);                          // m = 0  (m1 0, m2 0)
    o[1] = (v[4] + v[6]) + (v[5] + v[7]);                          // m = 1  (m1 1, m2 0)
    o[2] = padd_w4<INV>(v[8], v[10]) + (v[9] + v[11]);             // m = 2
    o[3] = psub_w4<INV>(v[4] - v[6], v[5] - v[7]);                 // m = 13 (m1 1, m2 3)
    o[4] = psub_w4<INV>(psub_w4<INV>(v[8], v[10]), v[9] - v[11]);  // m = 14
    o[5] = psub_w4<INV>(v[12] - v[14], v[13] - v[15]);             // m = 15
}

// first radix-4 butterfly of a 16-point DFT with one non-zero input a in
// position Q of (k1, k1+4, k1+8, k1+12): a -> (a, W4^Q a, W4^2Q a, W4^3Q a)
template <bool INV, int Q>
__device__ __forceinline__ void pbf4_one(pf2 a, pf2 &y0, pf2 &y1, pf2 &y2, pf2 &y3) {
    const pf2 z = {0.f, 0.f};
    if constexpr (Q == 0) {
        y0 = a; y1 = a; y2 = a; y3 = a;
    } else if constexpr (Q == 1) {   // pbf4 of (0, a, 0, 0)
        y0 = a; y1 = padd_w4<INV>(z, a); y2 = -a; y3 = psub_w4<INV>(z, a);
    } else if constexpr (Q == 2) {   // (0, 0, a, 0)
        y0 = a; y1 = -a; y2 = a; y3 = -a;
    } else {                         // (0, 0, 0, a)
        y0 = a; y1 = psub_w4<INV>(z, a); y2 = -a; y3 = padd_w4<INV>(z, a);
    }
}

// 16-point DFT whose input is zero outside v[4Q .. 4Q+3] (one quarter of a
// row, split mode with four workgroups per patch): the first radix-4 stage
// sees one non-zero input per butterfly
template <bool INV, int Q>
__device__ __forceinline__ void pdft16_inquarter(pf2 (&v)[16], pf2 (&r)[16]) {
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
        const pf2 a = v[k1 + 4 * Q];
        pbf4_one<INV, Q>(a, v[k1], v[k1 + 4], v[k1 + 8], v[k1 + 12]);
    }
    pmid_tw<INV>(v);
    pstage2<INV>(v);
#pragma unroll
    for (int m = 0; m < 16; ++m) r[m] = v[4 * (m & 3) + (m >> 2)];
}

// Four-step twiddles W256^{m t} (m = 0..15) of lane t, held in 32 VGPRs for a
// whole pass: a table read per use serialised on LDS latency at two waves per
// SIMD.
struct Tw {
    float2 w[16];
    __device__ __forceinline__ void load(const float2 *tw2, int t) {
#pragma unroll
        for (int m = 0; m < 16; ++m) w[m] = tw2[m * 16 + t];
    }
    __device__ __forceinline__ float2 operator[](int m) const { return w[m]; }
};

// ---------------------------------------------- the exchange, spread out
// exchange16 (dft16.hpp) issues its sixteen row stores and eight reads as one
// burst behind the last twiddle: the wave queues behind its own burst at LDS
// issue and then sits through the round trip.  fpm_fused.hip asks the
// transforms below for the spread form instead (template flag SPREAD, the
// pair transforms always): the exchange in its two parts (exch_put /
// exch_get, dft16.hpp), every row store right behind the twiddle block that
// finishes it (twiddle_put) and the reads in the order their consumer's first
// butterflies need them.  The flag defaults to the exchange16 form, which the
// distributed kernel (fused_dist.hip) keeps: its schedule was tuned around
// that form and the spread one has not been measured there.  The values and
// the tile slots are the same in both forms, so results do not depend on it.
// FPM_XSPREAD=0 builds fpm_fused.hip on the exchange16 form too, for same-box
// A/B runs.  Measured: DESIGN.md 4.1 "Exchange bursts".
#ifndef FPM_XSPREAD
#define FPM_XSPREAD 1
#endif
constexpr bool kXSpread = FPM_XSPREAD != 0;  // what fpm_fused.hip passes as SPREAD

// py[m] *= w[m] (CONJ: by conj(w[m])) for m in [M0, M1) in blocks split the
// way ptw_range (cpk.hpp) splits them, every block's rows stored to tile row
// row0 + m right behind it
template <bool CONJ, int M0, int M1>
__device__ __forceinline__ void twiddle_put(pf2 *py, const pf2 *w, float2 *scr, int t, int row0 = 0) {
    constexpr int n = M1 - M0, nb = (n + 4) / 5;
    static_assert(n >= 3, "every block holds 3..5 twiddles (ptw_block)");
#pragma unroll
    for (int b = 0, i = M0; b < nb; ++b) {
        const int len = (n - (i - M0)) / (nb - b);  // 3..5 for n >= 3
        if (len == 5) ptw_block<CONJ, 5>(&py[i], &w[i]);
        else if (len == 4) ptw_block<CONJ, 4>(&py[i], &w[i]);
        else ptw_block<CONJ, 3>(&py[i], &w[i]);
#pragma unroll
        for (int m = i; m < i + len; ++m) exch_put(scr, t, row0 + m, pout(py[m]));
        i += len;
    }
}

// the four-step exchange behind a transform's fifteen twiddles: y[m] = py[m]
// wt[m] (CONJ: conj) through the tile, z[j] = y_of_lane_j[t] out
template <bool CONJ, bool SPREAD, class TW>
__device__ __forceinline__ void twiddle_exchange(pf2 (&py)[16], const TW &wt, float2 *scr, int t, int xrd,
                                                 float2 (&z)[16]) {
    if constexpr (SPREAD) {
        pf2 w[16];
#pragma unroll
        for (int m = 1; m < 16; ++m) w[m] = pin(wt[m]);
        w[0] = w[1];
        exch_put(scr, t, 0, pout(py[0]));  // no twiddle
        twiddle_put<CONJ, 1, 16>(py, w, scr, t);
        exch_get(scr, xrd, z);
    } else {
        ptwiddle15<CONJ>(py, wt);
        float2 y[16];
        from_pk(py, y);
        exchange16(scr, t, xrd, y, z);
    }
}

// inverse 256-point DFT (unscaled), input v[k] = X[t + 16 k] (only the six
// SK registers may be non-zero), output r[m2] = x[t + 16 m2]
template <bool SPREAD = false, class TW>
__device__ __forceinline__ void idft256_in6(float2 (&v)[16], float2 (&r)[16], float2 *scr, const TW &wt, int t,
                                            int xrd) {
    pf2 pv[16], py[16];
    to_pk(v, pv);
    pdft16_in6<true>(pv, py);
    twiddle_exchange<true, SPREAD>(py, wt, scr, t, xrd, v);
    to_pk(v, pv);
    pdft16<true>(pv, py);
    from_pk(py, r);
}

// forward 256-point DFT, input v[n2] = x[t + 16 n2], output o[s] = X[t + 16 SK[s]]
template <bool SPREAD = false, class TW>
__device__ __forceinline__ void dft256_out6(float2 (&v)[16], float2 (&o)[6], float2 *scr, const TW &wt, int t,
                                            int xrd) {
    pf2 pv[16], py[16], po[6];
    to_pk(v, pv);
    pdft16<false>(pv, py);
    twiddle_exchange<false, SPREAD>(py, wt, scr, t, xrd, v);
    to_pk(v, pv);
    pdft16_out6<false>(pv, po);
    from_pk(po, o);
}

// forward 256-point DFT of quarter P of a row (x = t + 16 n2, n2 in
// [4P, 4P+4), zero elsewhere), output o[s] = X[t + 16 SK[s]]
template <int NPARTS, int P, class TW>
__device__ __forceinline__ void dft256_inpart_out6(float2 (&v)[16], float2 (&o)[6], float2 *scr, const TW &wt,
                                                   int t, int xrd) {
    static_assert(NPARTS == 4, "four column parts (two halves run as row pairs, below)");
    pf2 pv[16], py[16], po[6];
    to_pk(v, pv);
    pdft16_inquarter<false, P>(pv, py);
    ptwiddle15<false>(py, wt);
    float2 y[16];
    from_pk(py, y);
    exchange16(scr, t, xrd, y, v);
    to_pk(v, pv);
    pdft16_out6<false>(pv, po);
    from_pk(po, o);
}

// pruned forward row DFT of column part h (block-uniform, 0 <= h < NPARTS):
// input row[16 m'] = x[t + 16 (h MPP + m')], m' < MPP = 16 / NPARTS, output
// o[s] = the part's contribution to X[t + 16 SK[s]].  One unrolled branch per
// part keeps every register index static.
template <int NPARTS, class TW, int HH = 0>
__device__ __forceinline__ void row_dft_part(const float2 *row, float2 (&v)[16], float2 (&o)[6], float2 *scr,
                                             const TW &wt, int t, int xrd, int h) {
    constexpr int MPP = 16 / NPARTS;
    if constexpr (HH < NPARTS) {
        if (HH == h) {
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = make_float2(0.f, 0.f);
#pragma unroll
            for (int m = 0; m < MPP; ++m) v[HH * MPP + m] = row[16 * m];
            dft256_inpart_out6<NPARTS, HH>(v, o, scr, wt, t, xrd);
        } else {
            row_dft_part<NPARTS, TW, HH + 1>(row, v, o, scr, wt, t, xrd, h);
        }
    }
}

// ------------------------------------------------------------- row pairs
// Blocks of the kernel with two column halves (fpm_fused.hip, NPARTS == 2):
// the halves are cut on the LOW digit of the column, x = x1 + 16 x2 with half
// H = x1 in [8H, 8H+8), so one four-step transform serves both FFT rows of a
// group.  Spectral index k = kb + 16 ka; lane = low digit, register = high.
//   inverse: lane kb forms, per row, the 8 stage-1 outputs x1 of the half
//     (in-6, out-half DFT16 over ka), times W256^{-x1 kb}, into tile position
//     8 j + (x1 - 8H); after the exchange lane t' holds the 16 kb of (row
//     t' >> 3, x1 = 8H + (t' & 7)) and one dense DFT16 gives its 16 x2.
//   forward: the mirror image; lane t' runs the dense DFT16 over x2, twiddles
//     by W256^{x1 kb}, and after the exchange lane kb forms per row an
//     in-half, out-6 DFT16 over x1.
// tests/test_rowpair_model.py restates both with these index maps.

// radix-4 butterfly returning outputs 2H and 2H+1 only; W2: a2 carries the
// W16^4 mid twiddle (pbf4_w2)
template <bool INV, int H, bool W2>
__device__ __forceinline__ void pbf4_half(pf2 a0, pf2 a1, pf2 a2, pf2 a3, pf2 &lo, pf2 &hi) {
    const pf2 s02 = W2 ? padd_w4<INV>(a0, a2) : a0 + a2, d02 = W2 ? psub_w4<INV>(a0, a2) : a0 - a2;
    const pf2 s13 = a1 + a3, e13 = a1 - a3;
    if constexpr (H == 0) {
        lo = s02 + s13;
        hi = padd_w4<INV>(d02, e13);
    } else {
        lo = s02 - s13;
        hi = psub_w4<INV>(d02, e13);
    }
}

// 16-point DFT of an input that is zero except in[s] at position SK[s],
// returning the outputs m in [8H, 8H+8) as r[m - 8H]
template <bool INV, int H>
__device__ __forceinline__ void pdft16_in6_outhalf(const pf2 (&in)[6], pf2 (&r)[8]) {
    const pf2 a0 = in[0], b1 = in[1], c2 = in[2], b13 = in[3], c14 = in[4], d15 = in[5];
    const pf2 z = {0.f, 0.f};
    pf2 v[16];  // stage 1 as pdft16_in6
    v[0] = a0; v[4] = a0; v[8] = a0; v[12] = a0;
    v[1] = b1 + b13;
    v[5] = psub_w4<INV>(b1, b13);
    v[9] = b1 - b13;
    v[13] = padd_w4<INV>(b1, b13);
    v[2] = c2 + c14;
    v[6] = psub_w4<INV>(c2, c14);
    v[10] = c2 - c14;
    v[14] = padd_w4<INV>(c2, c14);
    v[3] = d15;
    v[7] = psub_w4<INV>(z, d15);
    v[11] = -d15;
    v[15] = padd_w4<INV>(z, d15);
    pmid_tw<INV>(v);
    // stage 2 over k1 for fixed m1: outputs m = m1 + 4 m2, m2 in {2H, 2H+1}
    pbf4_half<INV, H, false>(v[0], v[1], v[2], v[3], r[0], r[4]);
    pbf4_half<INV, H, false>(v[4], v[5], v[6], v[7], r[1], r[5]);
    pbf4_half<INV, H, true>(v[8], v[9], v[10], v[11], r[2], r[6]);
    pbf4_half<INV, H, false>(v[12], v[13], v[14], v[15], r[3], r[7]);
}

// 16-point DFT of an input that is zero outside positions 8H .. 8H+7 (in[i] at
// 8H + i), returning the outputs m in SK as o[0..5]
template <bool INV, int H>
__device__ __forceinline__ void pdft16_inhalf_out6(const pf2 (&in)[8], pf2 (&o)[6]) {
    pf2 v[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {  // stage 1: two of a butterfly's four inputs
        const pf2 a = in[k1], b = in[k1 + 4];
        if (H == 0) {  // (a, b, 0, 0)
            v[k1] = a + b;
            v[k1 + 4] = padd_w4<INV>(a, b);
            v[k1 + 8] = a - b;
            v[k1 + 12] = psub_w4<INV>(a, b);
        } else {       // (0, 0, a, b): W4^2 = -1, W4^3 = -W4
            v[k1] = a + b;
            v[k1 + 4] = -padd_w4<INV>(a, b);
            v[k1 + 8] = a - b;
            v[k1 + 12] = -psub_w4<INV>(a, b);
        }
    }
    pmid_tw<INV>(v);
    // stage 2 as pdft16_out6
    o[0] = (v[0] + v[2]) + (v[1] + v[3]);
    o[1] = (v[4] + v[6]) + (v[5] + v[7]);
    o[2] = padd_w4<INV>(v[8], v[10]) + (v[9] + v[11]);
    o[3] = psub_w4<INV>(v[4] - v[6], v[5] - v[7]);
    o[4] = psub_w4<INV>(psub_w4<INV>(v[8], v[10]), v[9] - v[11]);
    o[5] = psub_w4<INV>(v[12] - v[14], v[13] - v[15]);
}

// stage 1 of the paired inverse transform for half H: X[j][s] = X_j[t + 16 SK[s]]
// of rows j = 0, 1 -> y[8 j + i] = W256^{-(8H+i) t} sum_ka X_j[t + 16 ka] W16^{-(8H+i) ka}
// (wt: the lane's W256^{m t}; x1 = 0 has no twiddle)
template <int H, class TW>
__device__ __forceinline__ void idft256_pair_stage1(const float2 (&X)[2][6], pf2 (&py)[16], const TW &wt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        pf2 in[6], o[8];
        to_pk(X[j], in);
        pdft16_in6_outhalf<true, H>(in, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) py[8 * j + i] = o[i];
    }
    pf2 w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = pin(wt[8 * H + i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if constexpr (H == 0) {
            ptw_block<true, 4>(&py[8 * j + 1], &w[1]);
            ptw_block<true, 3>(&py[8 * j + 5], &w[5]);
        } else {
            ptw_block<true, 4>(&py[8 * j], &w[0]);
            ptw_block<true, 4>(&py[8 * j + 4], &w[4]);
        }
    }
}
// the same with every twiddle block's rows stored to the exchange tile right
// behind it (twiddle_put; the same blocks as above), one row after the other
template <int H, class TW>
__device__ __forceinline__ void idft256_pair_stage1_put(const float2 (&X)[2][6], const TW &wt, float2 *scr, int t) {
    pf2 w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = pin(wt[8 * H + i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        pf2 in[6], o[8];
        to_pk(X[j], in);
        pdft16_in6_outhalf<true, H>(in, o);
        if constexpr (H == 0) {
            exch_put(scr, t, 8 * j, pout(o[0]));  // x1 = 0: no twiddle
            twiddle_put<true, 1, 5>(o, w, scr, t, 8 * j);
            twiddle_put<true, 5, 8>(o, w, scr, t, 8 * j);
        } else {
            twiddle_put<true, 0, 4>(o, w, scr, t, 8 * j);
            twiddle_put<true, 4, 8>(o, w, scr, t, 8 * j);
        }
    }
}

// inverse 256-point DFTs (unscaled) of the two rows of a group, column half h
// (block-uniform): input X[j][s] = X_j[t + 16 SK[s]], output r[x2] =
// x_j[x1 + 16 x2] for j = t >> 3, x1 = 8 h + (t & 7).  One unrolled branch
// per half keeps every register index static.
template <class TW>
__device__ __forceinline__ void idft256_pair_in6(const float2 (&X)[2][6], float2 (&v)[16], float2 (&r)[16], float2 *scr,
                                                 const TW &wt, int t, int xrd, int h) {
    pf2 pv[16], py[16];
    if constexpr (kXSpread) {
        if (h == 0) idft256_pair_stage1_put<0>(X, wt, scr, t);
        else idft256_pair_stage1_put<1>(X, wt, scr, t);
        exch_get(scr, xrd, v);
    } else {
        if (h == 0) idft256_pair_stage1<0>(X, py, wt);
        else idft256_pair_stage1<1>(X, py, wt);
        float2 y[16];
        from_pk(py, y);
        exchange16(scr, t, xrd, y, v);
    }
    to_pk(v, pv);
    pdft16<true>(pv, py);
    from_pk(py, r);
}

// forward 256-point DFTs of column half h of the two rows of a group: input
// v[x2] = x_j[x1 + 16 x2] for j = t >> 3, x1 = 8 h + (t & 7), output o[j][s] =
// the half's contribution to X_j[t + 16 SK[s]].  wx: W256^{m x1}, m = 0..15
// (the twiddle set of the lane's x1, not of t).
template <class TW>
__device__ __forceinline__ void dft256_pair_out6(float2 (&v)[16], float2 (&o)[2][6], float2 *scr, const TW &wx, int t,
                                                 int xrd, int h) {
    pf2 pv[16], py[16];
    to_pk(v, pv);
    pdft16<false>(pv, py);
    twiddle_exchange<false, kXSpread>(py, wx, scr, t, xrd, v);
    to_pk(v, pv);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        pf2 in[8], po[6];
#pragma unroll
        for (int i = 0; i < 8; ++i) in[i] = pv[8 * j + i];
        if (h == 0) pdft16_inhalf_out6<false, 0>(in, po);
        else pdft16_inhalf_out6<false, 1>(in, po);
        from_pk(po, o[j]);
    }
}

}  // namespace fpm
