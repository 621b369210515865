// residual.hip -- the data-fidelity residual of the current state
// (fpm_residual, fpm_residual_at, fpm_hip.h): for the LED at position i of
// order[] -- or, for any entry of a list, that LED's image with its window
// wherever the entry puts it --
//     E[i] = sum_yx (|psi_i(y,x)| - sqrt(I_i(y,x)))^2,   S[i] = sum_yx I_i
// with psi_i = ifft2(ifftshift(window_i(O)) P) / Np^2, the reference's
// ObjcropP (fpmMain.cpp:358-365), evaluated without any update.  This is the
// first third of an LED step, so its kernels ARE the step's: general.hip's
// K1 / K2 (every generation) and np256.hip's C are templates over their
// argument struct, and the sweep launches their ResArgs instances
// (residual_dev.hpp: the LED and its window from the entry list, T of the batch, and the sums as
// K2's tail in place of amplitude replacement, forward transform and
// write-back).  Unlike the update loop every LED is independent: one launch
// covers a batch of nl LEDs x all B patches (blockIdx.z, or the leading factor
// of the 1-D grids, is the LED of the batch), so a few large patches still
// fill the chip.  Nothing here writes the state: the kernels read the
// spectrum, the pupil and the stack, and write only the context's residual
// scratch.
//
// The column kernels have three tails (residual_dev.hpp): ResArgs, the sums
// above; GainResArgs, E under the LED gains, E = sum (|psi| - g sqrt(I))^2,
// launched when some gain is not 1 (fpm_set_gains); MomArgs, the raw moments
// Q = sum |psi|^2 and C = sum |psi| sqrt(I) beside S (fpm_moments).  One launch
// shape, one row kernel and one fold serve all three.  A fourth, PredArgs
// (fpm_predict), sums nothing: it stores |psi|, the counts a camera would
// record or |psi| - g sqrt(I) of every pixel, the kind a uniform runtime
// switch of the one instance, and reads the stack for the last kind only; it
// shares the launch shape and the row kernel and has no fold
// (launch_predict_batch).
//
// What is left in this file:
//   k_res_rows256   the register pair's row kernel (Np 256, fp32 spectrum, the
//                   stack in the g = 16 column layout): np256.hip's R1 without
//                   the commit, so all sixteen loads of a lane are issued at
//                   once instead of half rows around the pupil stores
//   k_res_fold      a (LED, patch)'s partials added in index order
//   plan_residual   register or LDS pair (the ladder is plan_lds_ladder's,
//                   general.hip), LEDs per launch; the launcher
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
#include "fpm_state.hpp"
#include "launch.hpp"
#include "np256_layout.hpp"
#include "residual_dev.hpp"

namespace fpm {

namespace {

// ---- register pair: the row kernel ------------------------------------------------
// np256.hip's R1 without the commit: a group per support-box row.
// grid (nl * ceil(nb / GPB) * xcd_patches(B)), block NT, LDS (N + GPB XTILE_H) complex
__global__ void __launch_bounds__(n256::NT) k_res_rows256(DevState st, ResArgs ra, const float2 *__restrict__ tw) {
    using namespace n256;
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
    // st.pupil is the committed pupil: fpm_run ends every iteration with the
    // pupil commit (launch_pupil_commit after the last LED on the register paths)
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

// ---- fold ----------------------------------------------------------------------
// a thread per (LED of the batch, patch): its nblk partials in index order
__global__ void __launch_bounds__(256) k_res_fold(MomArgs ra, int nl, int B) {
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
    const size_t o = (size_t)ra.i0 * B + i;  // [n][B], by entry index
    if (ra.pcross) {  // fpm_moments: the cross sums the same way
        const double *pc = ra.pcross + (size_t)i * ra.nblk;
        double c = 0.0;
        for (int k = 0; k < ra.nblk; ++k) c += pc[k];
        ra.cross[o] = c;
    }
    ra.err[o] = e;
    ra.ref[o] = (double)s;  // exact: S < 2^16 Np^2 < 2^53
}

}  // namespace

// ---- the plan and the launchers --------------------------------------------------
ResidualPlan plan_residual(const DevState &st, const FftPlan &pl, int n_order, int meas_g, bool fp16,
                           const Switches &sw) {
    using namespace n256;
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
        p.rows = StepKernel{(const void *)k_res_rows256, dim3(row_blocks(nb) * Bp), dim3(NT), lds_rows(), 0};
        p.cols = StepKernel{residual_cols256_kernel(ResTail::Plain), dim3(kColBlocks * Bp), dim3(NT), lds_cols(nb), 0};
        p.cols_gain = p.cols_mom = p.cols_pred = p.cols;
        p.cols_gain.fn = residual_cols256_kernel(ResTail::Gain);
        p.cols_mom.fn = residual_cols256_kernel(ResTail::Moments);
        p.cols_pred.fn = residual_cols256_kernel(ResTail::Predict);
        p.cols_grad = p.cols;
        p.cols_grad.fn = residual_cols256_kernel(ResTail::Grad);
        p.nblk = kColBlocks;
    } else {
        p.ladder = plan_lds_ladder(pl, np, nb, B, sw, false);
        residual_lds_kernels(p.ladder, p.rows, p.cols, p.cols_gain, p.cols_mom, p.cols_pred);
        gradient_lds_cols_kernel(p.ladder, p.cols_grad);
        p.nblk = (int)p.cols.grid.x;
    }
    // LEDs per launch: as many as the scratch cap holds (FPM_RES_BATCH=n forces n)
    p.t_led = (size_t)B * nb * np;
    const size_t fit = kResidualScratchBytes / (p.t_led * sizeof(float2));
    p.nl = sw.res_batch > 0 ? sw.res_batch : (int)std::min<size_t>(std::max<size_t>(fit, 1), 65535);
    p.nl = std::max(1, std::min({p.nl, n_order, 65535}));
    plan_gradient_rows(p, st);
    return p;
}

hipError_t launch_residual_batch(const ResidualPlan &p, const DevState &st, const MomArgs &ra_in, ResTail tail, int nl,
                                 const float2 *tw, hipStream_t s) {
    MomArgs ra = ra_in;
    ra.nblk = p.nblk;
    const StepKernel *cols = tail == ResTail::Moments ? &p.cols_mom
                             : tail == ResTail::Gain  ? &p.cols_gain
                             : tail == ResTail::Grad  ? &p.cols_grad
                                                      : &p.cols;
    for (const StepKernel *k : {&p.rows, cols}) {
        // every instance but the moments' takes the ResArgs base (the leading bytes of ra)
        const bool mom = k == &p.cols_mom;
        hipError_t e;
        if (p.kind == ResidualPlan::Reg256) {  // the register kernels take no FftPlan
            DevState sv = st;
            void *args[] = {&sv, &ra, &tw};
            e = hipLaunchKernel(k->fn, dim3(k->grid.x * nl), k->block, args, k->lds, s);
        } else {
            e = mom ? launch_step_kernel(*k, st, ra, p.pl, tw, s, nl)
                    : launch_step_kernel(*k, st, static_cast<const ResArgs &>(ra), p.pl, tw, s, nl);
        }
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_res_fold, dim3((nl * st.B + 255) / 256), dim3(256), 0, s, ra, nl, st.B);
    return hipGetLastError();
}

// fpm_predict: the sweep's row kernel, then the column kernel whose tail stores
// the pixels.  No partials and no fold.
hipError_t launch_predict_batch(const ResidualPlan &p, const DevState &st, const PredArgs &pa_in, int nl,
                                const float2 *tw, hipStream_t s) {
    PredArgs pa = pa_in;
    pa.nblk = p.nblk;
    hipError_t e;
    if (p.kind == ResidualPlan::Reg256) {  // the register kernels take no FftPlan
        DevState sv = st;
        void *rargs[] = {&sv, static_cast<ResArgs *>(&pa), &tw}, *cargs[] = {&sv, &pa, &tw};
        e = hipLaunchKernel(p.rows.fn, dim3(p.rows.grid.x * nl), p.rows.block, rargs, p.rows.lds, s);
        if (e != hipSuccess) return e;
        return hipLaunchKernel(p.cols_pred.fn, dim3(p.cols_pred.grid.x * nl), p.cols_pred.block, cargs,
                               p.cols_pred.lds, s);
    }
    e = launch_step_kernel(p.rows, st, static_cast<const ResArgs &>(pa), p.pl, tw, s, nl);
    if (e != hipSuccess) return e;
    return launch_step_kernel(p.cols_pred, st, pa, p.pl, tw, s, nl);
}

}  // namespace fpm
