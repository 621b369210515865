// gradient.hip -- the gradient of the data-fidelity cost (fpm_gradient,
// fpm_hip.h).  For a list of entries (an LED's image and where its window
// sits) and every patch, with psi_i = ifft2(ifftshift(W_i) P) / Np^2 as the
// residual sweep forms it,
//     f      = sum_i sum_yx (|psi_i| - g_i sqrt(I_i))^2
//     rho_i  = psi_i - g_i sqrt(I_i) psi_i / |psi_i|        (0 where |psi_i| = 0)
//     R_i    = fft2(rho_i) / Np^2
//     G_O[window_i] += 2 conj(P) R_i          G_P += 2 conj(W_i) R_i
// G = df/dRe(z) + i df/dIm(z), twice the Wirtinger derivative df/dconj(z).
//
// With D = Objfup - ObjfcropP of an LED step (update.hpp), -2 conj(P) D / Np^2
// is that step's gradient, so a batch of nl entries runs through the LED
// step's three transform passes on the sweep's plan and scratch:
//   rows in     the sweep's row kernel, unchanged (k_gather_rowifft*, k_res_rows256)
//   columns     the sweep's column kernel with the GradArgs tail
//               (residual_dev.hpp): column IDFT, the sums E / S and rho in one
//               walk, forward column transform, the nb box rows back to T
//   fold        the sweep's (k_res_fold): E and S of the same pass
//   rows out    here: forward row transform of the nb box rows of T, the
//               disk's columns scaled 1 / Np^2 into R [nl][B][nb][nb]
//                 k_grad_rows     one row per block, ping-pong Stockham: every
//                                 size the LDS ladder accepts
//                 k_grad_rows256  a 16-lane group per row on the Np 256 register
//                                 transform: np256.hip's R2 without its update,
//                                 tile maxima and commit
//   accumulate  here, in gather form, so no two threads write one element and
//               nothing is atomic:
//                 k_grad_acc_obj    a thread per spectrum pixel p of the batch's
//                                   bounding box walks the batch's entries in
//                                   list order and adds 2 conj(P[k]) R_z[k],
//                                   k = p - c_z, where k is on the disk
//                                 k_grad_acc_pupil  a thread per disk pixel k adds
//                                   2 conj(O[c_z + k]) R_z[k]
//               The running fp32 value is loaded from the output, the terms are
//               added one by one in list order, and it is stored again: the
//               sequence of additions an element sees is the list's, however
//               the list was cut into launches.  The un-centred (objF) and
//               centred (pupil) index is formed at the store.
// The outputs are cleared by the caller before the first batch, so every
// element outside the entries' disks (the support) is exactly +0.
#include <algorithm>

#include "cpk.hpp"
#include "dftL.hpp"
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"
#include "np256_layout.hpp"
#include "residual_dev.hpp"

namespace fpm {

namespace {

constexpr int kAccThreads = 256, kAccX = 64, kAccY = kAccThreads / kAccX;

// R of (entry z of the batch, patch b): [nb][nb], the disk only
__device__ __forceinline__ size_t grad_R(const DevState &st, int z, int b) {
    return ((size_t)z * st.B + b) * st.nb * st.nb;
}

// ---- rows out: LDS, one box row per block ------------------------------------------
// grid (nb, B, nl), block 256, LDS 2 Np complex
__global__ void __launch_bounds__(256) k_grad_rows(DevState st, GradArgs a, FftPlan pl,
                                                   const float2 *__restrict__ tw, float2 *__restrict__ R) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int row = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    float2 *bufa = smem, *bufb = smem + np;
    const float2 *T = res_T(st, a, z, b, row, np);
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = T[i];
    __syncthreads();
    const float2 *res = stockham<false>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    float2 *Rr = R + grad_R(st, z, b) + (size_t)row * nb;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {
        if (!st.disk[row * nb + j]) continue;
        const int kx = j - r;
        Rr[j] = cscale(res[kx < 0 ? kx + np : kx], inv_n2);
    }
}

// ---- rows out: the Np 256 register transform ------------------------------------------
// grid (nl * ceil(nb / GPB) * xcd_patches(B)), block NT, LDS (N + GPB XTILE_H) complex
__global__ void __launch_bounds__(n256::NT) k_grad_rows256(DevState st, GradArgs a, const float2 *__restrict__ tw,
                                                          float2 *__restrict__ R) {
    using namespace n256;
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int g = threadIdx.x >> 4, t = threadIdx.x & 15, xrd = exch_rbase_half(t);
    const int r = st.r, nb = st.nb;
    int z, b, sub;
    if (!res_xcd_block((nb + GPB - 1) / GPB, st.B, z, b, sub)) return;  // block-uniform
    const int row = sub * GPB + g;
    const float2 twv = tw[threadIdx.x];
    float2 *twL = sm;
    float2 *wt = sm + N + g * XTILE_H;
    const int rowc = row < nb ? row : nb - 1;  // groups past the box: in-bounds loads, discarded
    const float2 *Tr = res_T(st, a, z, b, rowc, N) + t;
    float2 x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = Tr[16 * j];
    sm[threadIdx.x] = twv;
    __syncthreads();
    if (row >= nb) return;  // group-uniform; no block barrier follows
    float2 F[16];
    dft256_full<false, true>(x, F, wt, LdsTw{twL, t, 1}, t, xrd);  // F[k] = X[t + 16 k]
    const int ky = row - r, w2 = r * r - ky * ky;
    const float inv_n2 = 1.0f / ((float)N * (float)N);
    float2 *Rr = R + grad_R(st, z, b) + (size_t)row * nb + r;  // indexed by kx
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int kx = fold256(t + 16 * k);
        if (kx * kx <= w2) Rr[kx] = cscale(F[k], inv_n2);
    }
}

// ---- accumulate ---------------------------------------------------------------------
// acc += 2 conj(c) v
__device__ __forceinline__ float2 grad_add(float2 acc, float2 c, float2 v) {
    acc.x += 2.0f * (c.x * v.x + c.y * v.y);
    acc.y += 2.0f * (c.x * v.y - c.y * v.x);
    return acc;
}

// grid (ceil(bw / 64), ceil(bh / 4), B), block 256: pixel (by0 + .., bx0 + ..)
// of the centred spectrum, stored at its un-centred place (L is even)
__global__ void __launch_bounds__(kAccThreads) k_grad_acc_obj(DevState st, GradAcc q) {
    const int L = st.L, h = L / 2, r = st.r, nb = st.nb, b = blockIdx.z;
    const int dx = blockIdx.x * kAccX + (threadIdx.x & (kAccX - 1)), dy = blockIdx.y * kAccY + threadIdx.x / kAccX;
    const int x = q.bx0 + dx, y = q.by0 + dy;
    if (dx >= q.bw || dy >= q.bh || x < 0 || y < 0 || x >= L || y >= L) return;
    const float2 *pup = st.pupil + (size_t)b * nb * nb;
    float2 *out = q.gO + ((size_t)b * L + (y < h ? y + h : y - h)) * L + (x < h ? x + h : x - h);
    float2 acc = make_float2(0.f, 0.f);
    bool hit = false;
    for (int z = 0; z < q.nl; ++z) {
        const int4 e = *reinterpret_cast<const int4 *>(q.ent + q.i0 + z);  // (led, xc, yc)
        const int kx = x - e.y, ky = y - e.z;
        if (kx * kx + ky * ky > r * r) continue;
        if (!hit) acc = *out;
        hit = true;
        const int idx = (ky + r) * nb + kx + r;
        acc = grad_add(acc, pup[idx], q.R[grad_R(st, z, b) + idx]);
    }
    if (hit) *out = acc;
}

// grid (ceil(nb^2 / 256), B), block 256: box pixel k, stored at its centred place
__global__ void __launch_bounds__(kAccThreads) k_grad_acc_pupil(DevState st, GradAcc q) {
    const int L = st.L, np = st.np, r = st.r, nb = st.nb, b = blockIdx.y;
    const int idx = blockIdx.x * kAccThreads + threadIdx.x;
    if (idx >= nb * nb || !st.disk[idx]) return;
    const int row = idx / nb, ky = row - r, kx = idx - row * nb - r;
    float2 *out = q.gP + ((size_t)b * np + np / 2 + ky) * np + np / 2 + kx;
    float2 acc = *out;
    for (int z = 0; z < q.nl; ++z) {
        const int4 e = *reinterpret_cast<const int4 *>(q.ent + q.i0 + z);
        const float2 o = spec_ld(st, b, (size_t)(e.z + ky) * L + e.y + kx);
        acc = grad_add(acc, o, q.R[grad_R(st, z, b) + idx]);
    }
    *out = acc;
}

}  // namespace

// ---- the plan and the launcher --------------------------------------------------------
// the rows-out launch of one LED's grid beside the sweep's plan (plan_residual)
void plan_gradient_rows(ResidualPlan &p, const DevState &st) {
    using namespace n256;
    if (p.kind == ResidualPlan::Reg256)
        p.grad_rows = StepKernel{(const void *)k_grad_rows256, dim3(row_blocks(st.nb) * xcd_patches(st.B)), dim3(NT),
                                 lds_rows(), 0, 0};
    else
        p.grad_rows = StepKernel{(const void *)k_grad_rows, dim3(st.nb, st.B), dim3(256),
                                 2 * (size_t)st.np * sizeof(float2), 0, 0};
}

hipError_t launch_gradient_batch(const ResidualPlan &p, const DevState &st, const MomArgs &ra, const GradAcc &acc_in,
                                 int nl, const float2 *tw, hipStream_t s) {
    // rows in, the columns with the gradient's tail, the fold of E and S
    hipError_t e = launch_residual_batch(p, st, ra, ResTail::Grad, nl, tw, s);
    if (e != hipSuccess) return e;
    GradArgs ga{};
    static_cast<ResArgs &>(ga) = static_cast<const ResArgs &>(ra);
    GradAcc q = acc_in;
    q.ent = ra.ent;
    q.i0 = ra.i0;
    q.nl = nl;
    DevState sv = st;
    FftPlan pl = p.pl;
    float2 *R = const_cast<float2 *>(q.R);
    const StepKernel &k = p.grad_rows;
    if (p.kind == ResidualPlan::Reg256) {
        void *args[] = {&sv, &ga, &tw, &R};
        e = hipLaunchKernel(k.fn, dim3(k.grid.x * nl), k.block, args, k.lds, s);
    } else {
        void *args[] = {&sv, &ga, &pl, &tw, &R};
        e = hipLaunchKernel(k.fn, dim3(k.grid.x, k.grid.y, nl), k.block, args, k.lds, s);
    }
    if (e != hipSuccess) return e;
    if (q.gO && q.bw > 0 && q.bh > 0)
        hipLaunchKernelGGL(k_grad_acc_obj, dim3((q.bw + kAccX - 1) / kAccX, (q.bh + kAccY - 1) / kAccY, st.B),
                           dim3(kAccThreads), 0, s, st, q);
    if (q.gP)
        hipLaunchKernelGGL(k_grad_acc_pupil, dim3((st.nb * st.nb + kAccThreads - 1) / kAccThreads, st.B),
                           dim3(kAccThreads), 0, s, st, q);
    return hipGetLastError();
}

}  // namespace fpm
