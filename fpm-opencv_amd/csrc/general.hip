// general.hip -- the general (any Np = 2^a 3^b 5^c, any pupil radius) path of
// the per-LED update, fpmMain.cpp:348-476, as batched kernels per LED step.
// Every launch covers all B patches of the context (or of its patch group).
//
//   K1 k_gather_rowifft   sub-aperture gather x pupil, row IDFTs over the
//                         support box rows          (fpmMain.cpp:358-365)
//   K2 k_colpass          column IDFT, amplitude replacement, column DFT,
//                         only the box rows kept   (fpmMain.cpp:365-394)
//   K3 k_rowfft_update    row DFT of the box rows, object update written to
//                         the centred spectrum, pupil-update numerator
//                                                   (fpmMain.cpp:394-447,457-464)
//   K4 k_tile_rows        tile maxima of |spec| under the ROI and the maxima
//                         of those tile rows                (fpmMain.cpp:460,467)
//   K5 k_pupil_commit     exact max|objF| from the row maxima, P += num/max * S
//                         on a slice of the support box, partial max|P| for
//                         the next LED                       (fpmMain.cpp:459-475,415)
// K4 and K5 spread one patch over many workgroups, so a context with a few
// large patches (config 5: Np 1024, L 4096) still fills the chip.
//
// K1-K3 exist in three generations: one sequence per block (ping-pong
// Stockham, any size that fits LDS), tiled (several rows / columns per block,
// in place: fft_inplace.hpp) and, for K2, wave-private columns.  Np 1024 and
// Np 256 replace them by register kernels (np1024.hip, np256.hip).  Which of
// these a context runs depends on nothing but its sizes, so plan_general_step
// decides it once and launch_general_step only launches.
//
// K1 and K2 (every generation) are templates over their argument struct:
// StepArgs is the update step of one LED, ResArgs the residual sweep
// (fpm_residual, residual.hip) over a batch of LEDs of order[], which is K1
// and K2 up to the column IDFT with the residual sums as K2's tail.  The few
// lines that differ stand under if constexpr or behind residual_dev.hpp's
// overloads (res_led, res_T); the StepArgs instances are instruction for
// instruction what the kernels were before they became templates
// (tools/cmp_asm.py --pair).  PredArgs (fpm_predict) is the sweep with K2's
// tail storing the pixels instead of summing them.  plan_lds_ladder picks the generation and the
// launch shapes for both.
//
// Pruning: P vanishes outside the support disk, so the inverse transform has
// nonzero input only on the (2r+1)^2 box and only the box outputs of the
// forward transform are ever used.  Row passes therefore run on nb = 2r+1 rows,
// not Np.
#include <algorithm>

#include "fft_inplace.hpp"
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"
#include "residual_dev.hpp"
#include "update.hpp"

namespace fpm {

// ---- K1 ---------------------------------------------------------------------
// grid (nb, B), block 256, LDS 2*Np float2.  Here and in K2, every generation:
// A = ResArgs adds the grid's z, the LED of the sweep's batch.
// kLds...: the kernel's own __shared__ bytes, which a launch needs on top of
// its dynamic LDS (plan_context checks the sum against the device's limit).
// A static_assert ties each to the array it counts, and fpm_debug_get_ladder
// compares them with what the compiled kernels report (tests/test_gpu_ladder.py).
constexpr size_t kLdsGatherRowifft = 0;
template <class A>
__global__ void __launch_bounds__(256) k_gather_rowifft(DevState st, A a, FftPlan pl,
                                                        const float2 *__restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int row = blockIdx.x, b = blockIdx.y, z = kIsRes<A> ? blockIdx.z : 0;
    const StepArgs sa = res_led(a, z, np);
    const int ky = row - r;
    float2 *bufa = smem, *bufb = smem + np;
    const float2 *pup = st.pupil + (size_t)b * nb * nb;
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = make_float2(0.f, 0.f);
    __syncthreads();
    const int yrow = sa.yc + ky;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {
        if (st.disk[row * nb + j]) {
            const int kx = j - r;
            float2 o = spec_ld(st, b, (size_t)yrow * st.L + sa.xc + kx);
            float2 p = pup[row * nb + j];
            // (one index in two forms: each instance keeps the instructions it had,
            // and the sweep's compare-and-add is 20 fewer than the %)
            if constexpr (kIsRes<A>) bufa[kx < 0 ? kx + np : kx] = cmul(o, p);
            else bufa[(kx + np) % np] = cmul(o, p);
        }
    }
    __syncthreads();
    float2 *res = stockham<true>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);
    float2 *T = res_T(st, a, z, b, row, np);
    for (int i = threadIdx.x; i < np; i += blockDim.x) T[i] = res[i];
}

// ---- K2 ---------------------------------------------------------------------
// grid (Np, B), block 256, LDS 2*Np float2. One column per block.
template <class A>
constexpr size_t kLdsColpass = kIsRes<A> && !kIsPred<A> ? kResPartialLds<4> : 0;  // res_block_partial
template <class A>
__global__ void __launch_bounds__(256) k_colpass(DevState st, A a, FftPlan pl,
                                                 const float2 *__restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int x = blockIdx.x, b = blockIdx.y, z = kIsRes<A> ? blockIdx.z : 0;
    const StepArgs sa = res_led(a, z, np);
    [[maybe_unused]] const float rg_led = res_gain<A>(st, sa.led, b);
    float2 *bufa = smem, *bufb = smem + np;
    float2 *T = res_T(st, a, z, b, 0, np);
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {  // (the index as in K1)
        if constexpr (kIsRes<A>) bufa[j - r < 0 ? j - r + np : j - r] = T[(size_t)j * np + x];
        else bufa[(j - r + np) % np] = T[(size_t)j * np + x];
    }
    __syncthreads();
    float2 *res = stockham<true>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);
    float2 *oth = (res == bufa) ? bufb : bufa;
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    const uint16_t *I = st.meas + ((size_t)sa.led * st.mB + b) * np * np;
    if constexpr (kIsPred<A>) {
        // fpm_predict: the column's pixels stored at stride Np (the fallback of
        // sizes where not even two columns fit a block); the stack is read by
        // DIFF alone, where it lies
        const int g = st.meas_g, npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        const bool rd = pred_reads_stack(a);  // uniform
        const size_t o = pred_image(a, z, st.B, b, np) + x;
        for (int y = threadIdx.x; y < np; y += blockDim.x) {
            unsigned iv = 0;
            if (rd) {
                const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
                iv = g ? I[(size_t)x * np + t * npg + m] : I[(size_t)y * np + x];
            }
            pred_store(a, o + (size_t)y * np, pred_value(a, res[y], inv_n2, rg_led, iv));
        }
    } else if constexpr (kIsGrad<A>) {
        // fpm_gradient: the sums and rho in one walk (the stack where it lies),
        // then the step's tail: forward column transform, box rows back to T
        const int g = st.meas_g, npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        ResAcc<A> acc(rg_led);
        for (int y = threadIdx.x; y < np; y += blockDim.x) {
            const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
            const unsigned iv = g ? I[(size_t)x * np + t * npg + m] : I[(size_t)y * np + x];
            acc.add(res[y], inv_n2, iv);
            res[y] = grad_rho(res[y], inv_n2, iv, rg_led);
        }
        __syncthreads();
        res = stockham<false>(res, oth, 1, pl, tw, threadIdx.x, blockDim.x);
        for (int j = threadIdx.x; j < nb; j += blockDim.x) T[(size_t)j * np + x] = res[j - r < 0 ? j - r + np : j - r];
        res_block_partial<4>(acc, a, ((size_t)z * st.B + b) * a.nblk + x);
    } else if constexpr (kIsRes<A>) {
        const int g = st.meas_g;
        ResAcc<A> acc(rg_led);
        if (g) {  // uniform: the stored column x is contiguous, position p holds row (p mod (Np/g)) g + p / (Np/g)
            const int npg = np / g;
            const float rnpg = 1.0f / (float)npg;
            for (int p = threadIdx.x; p < np; p += blockDim.x) {
                const int t = udiv(p, npg, rnpg), m = p - t * npg;
                const unsigned iv = I[(size_t)x * np + p];
                acc.add(res[m * g + t], inv_n2, iv);
            }
        } else {
            for (int y = threadIdx.x; y < np; y += blockDim.x) {
                const unsigned iv = I[(size_t)y * np + x];
                acc.add(res[y], inv_n2, iv);
            }
        }
        res_block_partial<4>(acc, a, ((size_t)z * st.B + b) * a.nblk + x);
    } else {
        for (int y = threadIdx.x; y < np; y += blockDim.x) res[y] = amp_replace(res[y], inv_n2, I[(size_t)y * np + x], st);
        __syncthreads();
        res = stockham<false>(res, oth, 1, pl, tw, threadIdx.x, blockDim.x);
        for (int j = threadIdx.x; j < nb; j += blockDim.x) T[(size_t)j * np + x] = res[(j - r + np) % np];
    }
}

// ---- K3 ---------------------------------------------------------------------
// grid (nb, B), block 256, LDS 2*Np float2
constexpr size_t kLdsRowfftUpdate = 4 * sizeof(float);  // red
template <bool GAIN>
__global__ void __launch_bounds__(256) k_rowfft_update(DevState st, StepArgs sa, FftPlan pl,
                                                       const float2 *__restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int row = blockIdx.x, b = blockIdx.y;
    const int ky = row - r;
    const float gl = fused_gain<GAIN>(st, sa.led, b);
    float2 *bufa = smem, *bufb = smem + np;
    const float2 *T = st.T + ((size_t)b * nb + row) * np;
    for (int i = threadIdx.x; i < np; i += blockDim.x) bufa[i] = T[i];
    __syncthreads();
    float2 *res = stockham<false>(bufa, bufb, 1, pl, tw, threadIdx.x, blockDim.x);
    float2 *pup = st.pupil + (size_t)b * nb * nb;
    float2 *dP = st.dP + (size_t)b * nb * nb;
    // max|P| of the previous commit: the block reads the npart partial maxima
    // in parallel (a serial scalar-load chain cost ~30 us at npart ~ 100)
    __shared__ float red[4];
    static_assert(sizeof red == kLdsRowfftUpdate, "the create-time LDS check counts this array");
    float pm = 0.f;
    for (int i = threadIdx.x; i < st.npart; i += blockDim.x) pm = fmaxf(pm, st.pmax[b * st.npart + i]);
    pm = block_max_nonneg(pm, red);
    const int yrow = sa.yc + ky;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {
        if (!st.disk[row * nb + j]) continue;
        const int kx = j - r;
        const size_t si = (size_t)yrow * st.L + sa.xc + kx;
        const float2 o = spec_ld(st, b, si);     // pre-update Objfcrop (:361)
        const float2 p = pup[row * nb + j];
        const float2 F = res[(kx + np) % np];    // Objfup (:394)
        float2 num;
        spec_st(st, b, si, general_update<GAIN>(F, o, p, pm, gl, st, num));
        dP[row * nb + j] = num;
    }
}

// ---- K4 ---------------------------------------------------------------------
// grid (ROI tile rows, B), block 256 or 1024: one tile row of the ROI box per block.
// Each wave refreshes whole 16x16 tiles (4 pixels per lane, no barrier),
// issuing every load of its tiles before the first reduction; the row's other
// (unchanged) tile maxima are loaded first and folded in with one block max.
// Block size: one wave per ROI tile column up to 16 waves (1024 threads for
// config 5's 42-tile rows; 256 for config 3's 4-5 tiles, where 16 mostly
// idle waves per block only added latency).
template <int kRowThreads>
__global__ void __launch_bounds__(kRowThreads) k_tile_rows(DevState st, StepArgs sa) {
    constexpr int NW = kRowThreads / 64, MT = 5;  // tiles a wave refreshes at once
    __shared__ float red[NW];
    const int r = st.r, L = st.L, ntx = st.ntx;
    const int b = blockIdx.y;
    const int ty = (sa.yc - r) / kTile + blockIdx.x;
    const int tx0 = (sa.xc - r) / kTile, tx1 = (sa.xc + r) / kTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float *tmax = st.tmax + (size_t)b * st.nty * ntx + (size_t)ty * ntx;
    // the row's unchanged tile maxima first: their loads overlap the refresh
    float mx = 0.f;
    for (int tx = threadIdx.x; tx < ntx; tx += kRowThreads)
        if (tx < tx0 || tx > tx1) mx = fmaxf(mx, tmax[tx]);
    // the ROI tiles: every load of a wave's (up to MT) tiles before the first
    // reduction -- one memory latency instead of one per tile
    // (unconditional loads of clamped in-bounds pixels, masked after all of
    // them: a masked spec_ld, widening fp16 where it loaded, waited for each
    // of its loads in turn -- 20 memory round trips per wave)
    auto pix = [&](int base, int i, int j, bool &ok) {  // pixel j of tile i: its index, ok = inside the ROI row
        const int tx = base + i * NW, p = lane + 64 * j;
        const int y = ty * kTile + (p >> 4), x = min(tx, tx1) * kTile + (p & 15);
        ok = tx <= tx1 && y < L && x < L;
        return ok ? (size_t)y * L + x : (size_t)0;
    };
    for (int base = tx0 + w; base <= tx1; base += MT * NW) {
        float m[MT];
        if (st.spec16) {  // uniform
            const __half2 *sp = st.spec16 + (size_t)b * L * L;
            __half2 hv[MT][4];
            bool ok[MT][4];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) hv[i][j] = sp[pix(base, i, j, ok[i][j])];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                m[i] = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float2 f = __half22float2(hv[i][j]);
                    const float a = cmag(make_float2(f.x * st.hinv, f.y * st.hinv));  // spec_ld's widening
                    m[i] = fmaxf(m[i], ok[i][j] ? a : 0.f);
                }
            }
        } else {
            const float2 *sp = st.spec + (size_t)b * L * L;
            float2 ov[MT][4];
            bool ok[MT][4];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) ov[i][j] = sp[pix(base, i, j, ok[i][j])];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                m[i] = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) m[i] = fmaxf(m[i], ok[i][j] ? cmag(ov[i][j]) : 0.f);
            }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int tx = base + i * NW;
            if (tx > tx1) break;  // wave-uniform
            const float t = wave_max_nonneg(m[i]);
            if (lane == 0) tmax[tx] = t;
            mx = fmaxf(mx, t);
        }
    }
    mx = block_max_nonneg(mx, red);
    if (threadIdx.x == 0) st.rmax[(size_t)b * st.nty + ty] = mx;
}

// ---- K5 ---------------------------------------------------------------------
// grid (npart, B), block 256: global max|objF| (fpmMain.cpp:467) from the nty
// row maxima, then P += num / max * S (fpmMain.cpp:470-475) on this block's
// slice of the support box and its partial max|P| for the next LED (:415).
constexpr int kCommitThreads = 256;
constexpr int kCommitPx = 1024;  // support-box pixels per K5 block (a multiple of kCommitThreads)
__global__ void __launch_bounds__(kCommitThreads) k_pupil_commit(DevState st) {
    __shared__ float red[kCommitThreads / 64];
    const int nb = st.nb, b = blockIdx.y, part = blockIdx.x;
    const float *rmax = st.rmax + (size_t)b * st.nty;
    const int n = nb * nb, chunk = (n + st.npart - 1) / st.npart;
    const int i0 = part * chunk, i1 = min(n, i0 + chunk);
    float2 *pup = st.pupil + (size_t)b * nb * nb;
    const float2 *dP = st.dP + (size_t)b * nb * nb;
    // this thread's pixels (chunk <= kCommitPx) are loaded before the max
    // reduction, so their latency overlaps the rmax round trip
    constexpr int KP = kCommitPx / kCommitThreads;
    float2 pv[KP], dv[KP];
    bool on[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int i = i0 + threadIdx.x + k * kCommitThreads;
        on[k] = i < i1 && st.disk[i];
        pv[k] = on[k] ? pup[i] : make_float2(0.f, 0.f);
        dv[k] = on[k] ? dP[i] : make_float2(0.f, 0.f);
    }
    float m = 0.f;
    for (int i = threadIdx.x; i < st.nty; i += kCommitThreads) m = fmaxf(m, rmax[i]);
    const float omax = block_max_nonneg(m, red);
    float pm = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (!on[k]) continue;
        float2 p = pv[k];
        p.x += dv[k].x / omax;
        p.y += dv[k].y / omax;
        pup[i0 + threadIdx.x + k * kCommitThreads] = p;
        pm = fmaxf(pm, cmag(p));
    }
    pm = block_max_nonneg(pm, red);
    if (threadIdx.x == 0) st.pmax[b * st.npart + part] = pm;
}

int pupil_parts(int nb) { return std::max(1, (nb * nb + kCommitPx - 1) / kCommitPx); }

// ---- K1 / K3 (tiled) ------------------------------------------------------------
// C = 2^lc box rows per block in one row-major LDS tile (pitch Np + 1) with
// the twiddles beside it: the row transforms of a block run together, in
// place, instead of one 256-thread block per row with global twiddle reads.
// grid (ceil(nb / C), B), block NT.
constexpr size_t kLdsGatherRowifftTiled = 0;
template <int NT>
constexpr size_t kLdsRowfftUpdateTiled = NT / 64 * sizeof(float);  // red
template <int NT, int E, class A>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(E <= 16 ? 4 : 1))) k_gather_rowifft_tiled(DevState st, A a, FftPlan pl,
                                                             const float2 *__restrict__ tw, int lc) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, C = 1 << lc, lss = row_pitch(np, lc);
    const int j0 = blockIdx.x << lc, b = blockIdx.y, z = kIsRes<A> ? blockIdx.z : 0;
    const StepArgs sa = res_led(a, z, np);
    const int cs = min(C, nb - j0);
    float2 *tile = smem, *stw = smem + (size_t)C * lss;
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
    tile_transform_ex<true, NT, E>(tile, pl, lc, lss, 1, stw);                              // :365
    float2 *T = res_T(st, a, z, b, j0, np);
    const float rnp = 1.0f / (float)np;
    for (int idx = threadIdx.x; idx < cs * np; idx += NT) {
        const int c = udiv(idx, np, rnp), i = idx - c * np;
        T[(size_t)c * np + i] = tile[c * lss + i];
    }
}

template <int NT, int E, bool GAIN>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(E <= 16 ? 4 : 1))) k_rowfft_update_tiled(DevState st, StepArgs sa, FftPlan pl,
                                                            const float2 *__restrict__ tw, int lc) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    __shared__ float red[NT / 64];
    static_assert(sizeof red == kLdsRowfftUpdateTiled<NT>, "the create-time LDS check counts this array");
    const int np = st.np, r = st.r, nb = st.nb, C = 1 << lc, lss = row_pitch(np, lc);
    const int j0 = blockIdx.x << lc, b = blockIdx.y;
    const int cs = min(C, nb - j0);
    const float gl = fused_gain<GAIN>(st, sa.led, b);
    float2 *tile = smem, *stw = smem + (size_t)C * lss;
    for (int i = threadIdx.x; i < np; i += NT) stw[i] = tw[i];
    const float2 *T = st.T + ((size_t)b * nb + j0) * np;
    const float rnp = 1.0f / (float)np;
    for (int idx = threadIdx.x; idx < C * np; idx += NT) {
        const int c = udiv(idx, np, rnp), i = idx - c * np;
        tile[c * lss + i] = c < cs ? T[(size_t)c * np + i] : make_float2(0.f, 0.f);
    }
    // max|P| of the previous commit from its npart partial maxima
    float pm = 0.f;
    for (int i = threadIdx.x; i < st.npart; i += NT) pm = fmaxf(pm, st.pmax[b * st.npart + i]);
    pm = block_max_nonneg(pm, red);  // its barriers also publish the tile
    tile_transform_ex<false, NT, E>(tile, pl, lc, lss, 1, stw);                             // :394
    float2 *pup = st.pupil + (size_t)b * nb * nb;
    float2 *dP = st.dP + (size_t)b * nb * nb;
    const float rnb = 1.0f / (float)nb;
    for (int idx = threadIdx.x; idx < cs * nb; idx += NT) {
        const int c = udiv(idx, nb, rnb), j = idx - c * nb, row = j0 + c;
        if (!st.disk[row * nb + j]) continue;
        const int kx = j - r;
        const size_t si = (size_t)(sa.yc + row - r) * st.L + sa.xc + kx;
        const float2 o = spec_ld(st, b, si);                    // pre-update Objfcrop (:361)
        const float2 p = pup[row * nb + j];
        const float2 F = tile[c * lss + (kx < 0 ? kx + np : kx)];  // Objfup (:394)
        float2 num;
        spec_st(st, b, si, general_update<GAIN>(F, o, p, pm, gl, st, num));
        dP[row * nb + j] = num;
    }
}

// ---- K2 (tiled) ---------------------------------------------------------------
// The column pass for C = 2^lc adjacent columns per block: the box rows of T
// are read as C*8-byte row segments (coalesced), the column IDFT, amplitude
// replacement and column DFT run in place in one LDS tile, and only the box
// rows are written back.  The last tile may be partial (Np not a multiple of
// C: its missing columns are zero and never stored).  grid (ceil(Np / C), B),
// block NT (256 when the tile fits its register-lifted passes, so a 16 x 200
// tile keeps every wave busy instead of idling half of a 512-thread block).
template <int NT, class A>
constexpr size_t kLdsColpassTiled = kIsRes<A> && !kIsPred<A> ? kResPartialLds<NT / 64> : 0;  // res_block_partial
template <int NT, int E, class A>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(E <= 16 ? 4 : 1))) k_colpass_tiled(DevState st, A a, FftPlan pl,
                                                      const float2 *__restrict__ tw, int lc) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb, C = 1 << lc, cm = C - 1;
    const int x0 = blockIdx.x << lc, b = blockIdx.y, z = kIsRes<A> ? blockIdx.z : 0;
    const StepArgs sa = res_led(a, z, np);
    [[maybe_unused]] const float rg_led = res_gain<A>(st, sa.led, b);
    const int cs = min(C, np - x0);            // columns present in this tile
    float2 *tile = smem;                       // np * C
    float2 *stw = smem + (size_t)np * C;       // np twiddles
    float2 *T = res_T(st, a, z, b, 0, np);
    for (int i = threadIdx.x; i < np; i += NT) stw[i] = tw[i];
    for (int i = threadIdx.x; i < np * C; i += NT) tile[i] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
        const int j = idx >> lc, c = idx & cm;
        const int i = j - r < 0 ? j - r + np : j - r;
        if (c < cs) tile[i * C + c] = T[(size_t)j * np + x0 + c];
    }
    __syncthreads();
    tile_transform<true, NT, E>(tile, pl, lc, stw);
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    const uint16_t *I = st.meas + ((size_t)sa.led * st.mB + b) * np * np;
    if constexpr (kIsPred<A>) {
        // fpm_predict: the sums' walk below (rows in natural order, the tile's C
        // columns across adjacent lanes), each row's columns stored as one
        // segment of C elements; the stack is read by DIFF alone
        const int g = st.meas_g, npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        const bool rd = pred_reads_stack(a);  // uniform
        const size_t o = pred_image(a, z, st.B, b, np) + x0;
        for (int idx = threadIdx.x; idx < np * C; idx += NT) {
            const int y = idx >> lc, c = idx & cm;
            if (c >= cs) continue;
            unsigned iv = 0;
            if (rd) {
                const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
                iv = g ? I[(size_t)(x0 + c) * np + t * npg + m] : I[(size_t)y * np + x0 + c];
            }
            pred_store(a, o + (size_t)y * np + c, pred_value(a, tile[idx], inv_n2, rg_led, iv));
        }
    } else if constexpr (kIsGrad<A>) {
        // fpm_gradient: the sums' walk below with rho written in place, then the
        // step's tail (forward column transform, box rows back to T)
        const int g = st.meas_g, npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        ResAcc<A> acc(rg_led);
        for (int idx = threadIdx.x; idx < np * C; idx += NT) {
            const int y = idx >> lc, c = idx & cm;
            if (c >= cs) continue;
            const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
            const unsigned iv = g ? I[(size_t)(x0 + c) * np + t * npg + m] : I[(size_t)y * np + x0 + c];
            acc.add(tile[idx], inv_n2, iv);
            tile[idx] = grad_rho(tile[idx], inv_n2, iv, rg_led);
        }
        __syncthreads();
        tile_transform<false, NT, E>(tile, pl, lc, stw);
        for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
            const int j = idx >> lc, c = idx & cm;
            const int i = j - r < 0 ? j - r + np : j - r;
            if (c < cs) T[(size_t)j * np + x0 + c] = tile[i * C + c];
        }
        res_block_partial<NT / 64>(acc, a, ((size_t)z * st.B + b) * a.nblk + blockIdx.x);
    } else if constexpr (kIsRes<A>) {
        // rows in natural order, the tile's C columns across adjacent lanes (no
        // LDS bank conflict).  The stack is read as C*2-byte row segments in
        // the C-ABI layout; in a column layout row y of column x lies at
        // x Np + (y mod g)(Np / g) + y / g, so the block still reads each of its
        // columns' 2 Np bytes exactly once.  (Walking a stored column in memory
        // order instead would put a wave's 64 LDS reads 2^lc g rows apart, all in
        // one bank.)
        const int g = st.meas_g;
        ResAcc<A> acc(rg_led);
        const int npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        for (int idx = threadIdx.x; idx < np * C; idx += NT) {
            const int y = idx >> lc, c = idx & cm;
            if (c >= cs) continue;
            const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
            const unsigned iv = g ? I[(size_t)(x0 + c) * np + t * npg + m] : I[(size_t)y * np + x0 + c];
            acc.add(tile[idx], inv_n2, iv);
        }
        res_block_partial<NT / 64>(acc, a, ((size_t)z * st.B + b) * a.nblk + blockIdx.x);
    } else {
        for (int idx = threadIdx.x; idx < np * C; idx += NT) {
            const int y = idx >> lc, c = idx & cm;
            if (c >= cs) continue;
            tile[idx] = amp_replace(tile[idx], inv_n2, I[(size_t)y * np + x0 + c], st);
        }
        __syncthreads();
        tile_transform<false, NT, E>(tile, pl, lc, stw);
        for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
            const int j = idx >> lc, c = idx & cm;
            const int i = j - r < 0 ? j - r + np : j - r;
            if (c < cs) T[(size_t)j * np + x0 + c] = tile[i * C + c];
        }
    }
}

// ---- K2 (wave-private columns) ----------------------------------------------------
// Same column pass, but every wave owns CW whole columns of the block's
// C = NW*CW-column tile, so the radix passes synchronise the wave only
// (wave_sync) instead of the whole block: two block barriers per launch
// (after the coalesced tile load, before the coalesced store) instead of two
// per radix pass.  Within a wave, 64/CW consecutive lanes serve one column
// (column-major, pitch P), so a lane's column and its base address are fixed
// for the whole transform and every butterfly element is an immediate offset
// from it.  The measurement values a lane needs for amplitude replacement
// (rows lane + 64q of its wave's columns) are loaded into registers before
// the inverse transform, so their latency hides behind it.
// grid (ceil(Np / (NW*CW)), B), block 64*NW, LDS (NW*CW*pitch + Np) float2
template <int NW, class A>
constexpr size_t kLdsColpassWave = kIsRes<A> && !kIsPred<A> ? kResPartialLds<NW> : 0;  // res_block_partial
template <int NW, int CW, class A>
__global__ void __launch_bounds__(64 * NW)
k_colpass_wave(DevState st, A a, FftPlan pl, const float2 *__restrict__ tw, int P) {
    constexpr int NT = 64 * NW, C = NW * CW, NQY = 16 / CW;
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int np = st.np, r = st.r, nb = st.nb;
    const int x0 = blockIdx.x * C, b = blockIdx.y, z = kIsRes<A> ? blockIdx.z : 0;
    const StepArgs sa = res_led(a, z, np);
    [[maybe_unused]] const float rg_led = res_gain<A>(st, sa.led, b);
    const int cs = min(C, np - x0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int LPC = 64 / CW;
    float2 *stw = smem + (size_t)C * P;
    float2 *wb = smem + (size_t)w * CW * P;
    float2 *cb = wb + (lane / LPC) * P;  // this lane's column in the radix passes
    const int l = lane % LPC;
    float2 *T = res_T(st, a, z, b, 0, np);
    // this lane's measurement values: rows lane + 64q of the wave's columns
    const uint16_t *I = st.meas + ((size_t)sa.led * st.mB + b) * np * np;
    [[maybe_unused]] typename std::conditional<kIsRes<A>, unsigned, uint16_t>::type iv[NQY * CW];
    if constexpr (kIsPred<A>) {
        // fpm_predict reads the stack in its tail, for DIFF alone, in the order it stores
    } else if constexpr (kIsRes<A>) {
        // the sweep reads the stack where it lies: every load issued before the
        // first use (clamped in-bounds, masked afterwards); in a column layout
        // row y of column x lies at x Np + (y mod g)(Np / g) + y / g
        const int g = st.meas_g;
        const int npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
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
    } else {
#pragma unroll
        for (int q = 0; q < NQY; ++q) {
            const int y = lane + 64 * q;
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                const int x = w * CW + c;
                iv[q * CW + c] = (y < np && x < cs) ? I[(size_t)y * np + x0 + x] : (uint16_t)0;
            }
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
    wave_transform<true, LPC>(cb, pl, stw, l);
    const float inv_n2 = 1.0f / ((float)np * (float)np);
    if constexpr (kIsPred<A>) {
        // fpm_predict: the block's tile walked as the step's write-back walks
        // it, rows in natural order with the C columns across adjacent lanes, so
        // each row's columns leave as one segment of C elements
        __syncthreads();
        const int g = st.meas_g, npg = g ? np / g : 1;
        const float rg = 1.0f / (float)(g ? g : 1);
        const bool rd = pred_reads_stack(a);  // uniform
        const size_t o = pred_image(a, z, st.B, b, np) + x0;
        for (int idx = threadIdx.x; idx < np * C; idx += NT) {
            const int y = udiv(idx, C, rC), c = idx - y * C;
            if (c >= cs) continue;
            unsigned iv1 = 0;
            if (rd) {
                const int m = udiv(y, g ? g : 1, rg), t = y - m * g;  // g > 0: y = t + g m
                iv1 = g ? I[(size_t)(x0 + c) * np + t * npg + m] : I[(size_t)y * np + x0 + c];
            }
            pred_store(a, o + (size_t)y * np + c, pred_value(a, smem[c * P + y], inv_n2, rg_led, iv1));
        }
    } else if constexpr (kIsGrad<A>) {
        // fpm_gradient: the sums and rho on the lane's own pixels, then the step's
        // tail (wave-private forward transform, coalesced write-back of the box rows)
        ResAcc<A> acc(rg_led);
#pragma unroll
        for (int q = 0; q < NQY; ++q) {
            const int y = lane + 64 * q;
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (y >= np || w * CW + c >= cs) continue;
                float2 *e = wb + c * P + y;
                acc.add(*e, inv_n2, iv[q * CW + c]);
                *e = grad_rho(*e, inv_n2, iv[q * CW + c], rg_led);
            }
        }
        wave_sync();
        wave_transform<false, LPC>(cb, pl, stw, l);
        __syncthreads();
        for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
            const int j = udiv(idx, C, rC), c = idx - j * C;
            const int i = j - r < 0 ? j - r + np : j - r;
            if (c < cs) T[(size_t)j * np + x0 + c] = smem[c * P + i];
        }
        res_block_partial<NW>(acc, a, ((size_t)z * st.B + b) * a.nblk + blockIdx.x);
    } else if constexpr (kIsRes<A>) {
        ResAcc<A> acc(rg_led);
#pragma unroll
        for (int q = 0; q < NQY; ++q) {
            const int y = lane + 64 * q;
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (y >= np || w * CW + c >= cs) continue;
                acc.add(wb[c * P + y], inv_n2, iv[q * CW + c]);
            }
        }
        res_block_partial<NW>(acc, a, ((size_t)z * st.B + b) * a.nblk + blockIdx.x);
    } else {
#pragma unroll
        for (int q = 0; q < NQY; ++q) {
            const int y = lane + 64 * q;
            if (y >= np) continue;
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                float2 *e = wb + c * P + y;
                *e = amp_replace(*e, inv_n2, iv[q * CW + c], st);
            }
        }
        wave_sync();
        wave_transform<false, LPC>(cb, pl, stw, l);
        __syncthreads();
        for (int idx = threadIdx.x; idx < nb * C; idx += NT) {
            const int j = udiv(idx, C, rC), c = idx - j * C;
            const int i = j - r < 0 ? j - r + np : j - r;
            if (c < cs) T[(size_t)j * np + x0 + c] = smem[c * P + i];
        }
    }
}

// ---- the plan and the step launcher -------------------------------------------
// Which generation of K1 / K3 and of K2 a size runs, with the launch shapes:
// decided here for the update step and for the residual sweep alike.
// step: the update step, which trades tile size for block count when a few
// large patches would leave the chip short of blocks (the sweep gets its
// blocks from the batch).  FPM_ONE_SEQ forces the one-sequence kernels on the
// step, FPM_RES_ONE_SEQ on the sweep.
LdsLadder plan_lds_ladder(const FftPlan &pl, int np, int nb, int B, const Switches &sw, bool step) {
    LdsLadder l{};
    const bool one_seq = step ? sw.one_seq : sw.res_one_seq;  // the fallback of sizes where not even two fit, at any size
    const size_t lds = 2 * (size_t)np * sizeof(float2);  // of the one-sequence kernels
    // row kernels: up to 16 box rows per block (one row per block when not
    // even 2 rows fit a 256-thread tile)
    int lr = one_seq ? 0 : 4;
    while (lr > 0 && !fft_fits(pl, lr, 256)) --lr;
    auto rblk = [&](int k) { return ((nb + (1 << k) - 1) >> k) * B; };
    while (step && lr > 1 && rblk(lr) < 512) --lr;
    if (lr > 0) {
        // 16 register elements per thread when the tile allows (fewer VGPRs, more
        // waves per SIMD to hide the LDS round trips of each pass), else 24
        l.row_e = fft_fits(pl, lr, 256, 16) ? 16 : 24;
        l.rows = StepKernel{nullptr, dim3((nb + (1 << lr) - 1) >> lr, B), dim3(256),
                            ((size_t)row_pitch(np, lr) * (1 << lr) + np) * sizeof(float2), lr};
    } else {
        l.rows = StepKernel{nullptr, dim3(nb, B), dim3(256), lds, 0};
    }
    // tiled column pass: up to 16 columns per block while the tile fits the
    // in-place register-lifted transform (the step: down to 4 for blocks);
    // one column per block when not even 2 columns fit
    int lc = one_seq ? 0 : 4;
    while (lc > 0 && !fft_fits(pl, lc)) --lc;
    auto cblk = [&](int k) { return ((np + (1 << k) - 1) >> k) * B; };
    while (step && lc > 2 && cblk(lc) < 512) --lc;
    const int cw = colw_cw(pl);
    if (cw > 1 && !sw.no_wave_cols && !one_seq) {
        // wave-private columns where a wave holds at least two (Np <= 512):
        // 4 waves x CW columns; FPM_NO_WAVE_COLS=1: tiled
        const int P = colw_pitch(np), C = 4 * cw;
        l.cw = cw;
        l.cols = StepKernel{nullptr, dim3((np + C - 1) / C, B), dim3(256), ((size_t)C * P + np) * sizeof(float2), P};
    } else if (lc > 0) {
        // 256 threads when the tile fits their register-lifted passes, else 512
        const int nt = fft_fits(pl, lc, 256) ? 256 : kFftThreads;
        l.col_e = fft_fits(pl, lc, nt, 16) ? 16 : 24;
        l.cols = StepKernel{nullptr, dim3((np + (1 << lc) - 1) >> lc, B), dim3(nt),
                            ((size_t)np * (1 << lc) + np) * sizeof(float2), lc};
    } else {
        l.cols = StepKernel{nullptr, dim3(np, B), dim3(256), lds, 0};
    }
    return l;
}

// the ladder's K1 / K2 for the update step (A = StepArgs) or the sweep (ResArgs)
template <class A>
static void pick_lds_kernels(const LdsLadder &l, StepKernel &rows, StepKernel &cols) {
    if constexpr (!kIsMom<A> && !kIsGainRes<A> && !kIsPred<A> && !kIsGrad<A>) {  // the row kernels have no tail: every sweep launches the ResArgs ones
        rows = l.rows;
        rows.fn = l.row_e == 16 ? (const void *)k_gather_rowifft_tiled<256, 16, A>
                  : l.row_e     ? (const void *)k_gather_rowifft_tiled<256, 24, A>
                                : (const void *)k_gather_rowifft<A>;
        rows.lds_static = l.row_e ? kLdsGatherRowifftTiled : kLdsGatherRowifft;
    }
    cols = l.cols;
    const bool e16 = l.col_e == 16;
    if (l.cw) {
        cols.fn = l.cw == 4 ? (const void *)k_colpass_wave<4, 4, A> : (const void *)k_colpass_wave<4, 2, A>;
        cols.lds_static = kLdsColpassWave<4, A>;
    } else if (!l.col_e) {
        cols.fn = (const void *)k_colpass<A>;
        cols.lds_static = kLdsColpass<A>;
    } else if (cols.block.x == 256) {
        cols.fn = e16 ? (const void *)k_colpass_tiled<256, 16, A> : (const void *)k_colpass_tiled<256, 24, A>;
        cols.lds_static = kLdsColpassTiled<256, A>;
    } else {
        cols.fn = e16 ? (const void *)k_colpass_tiled<kFftThreads, 16, A>
                      : (const void *)k_colpass_tiled<kFftThreads, 24, A>;
        cols.lds_static = kLdsColpassTiled<kFftThreads, A>;
    }
}

GeneralPlan plan_general_step(const DevState &st, GeneralPlan::Kind kind, const FftPlan &pl, const Switches &sw) {
    GeneralPlan p{};
    p.pl = pl;
    // Np 1024: register-resident row/column transforms (np1024.hip); Np 256
    // beyond the fused kernels' radius: np256.hip, whose K4 runs inside its R2;
    // the context's plan decides which (plan_context, create.cpp)
    p.kind = kind;
    if (p.kind != GeneralPlan::Lds) return p;
    const LdsLadder l = plan_lds_ladder(pl, st.np, st.nb, st.B, sw, true);
    p.ladder = l;
    pick_lds_kernels<StepArgs>(l, p.k1, p.k2);
    p.k3 = l.rows;
    p.k3.fn = l.row_e == 16 ? (const void *)k_rowfft_update_tiled<256, 16, false>
              : l.row_e     ? (const void *)k_rowfft_update_tiled<256, 24, false>
                            : (const void *)k_rowfft_update<false>;
    p.k3.lds_static = l.row_e ? kLdsRowfftUpdateTiled<256> : kLdsRowfftUpdate;
    p.k3_gain = p.k3;
    p.k3_gain.fn = l.row_e == 16 ? (const void *)k_rowfft_update_tiled<256, 16, true>
                   : l.row_e     ? (const void *)k_rowfft_update_tiled<256, 24, true>
                                 : (const void *)k_rowfft_update<true>;
    return p;
}

void residual_lds_kernels(const LdsLadder &l, StepKernel &rows, StepKernel &cols, StepKernel &cols_gain,
                          StepKernel &cols_mom, StepKernel &cols_pred) {
    pick_lds_kernels<GainResArgs>(l, rows, cols_gain);  // (rows untouched by these three)
    pick_lds_kernels<MomArgs>(l, rows, cols_mom);
    pick_lds_kernels<PredArgs>(l, rows, cols_pred);
    pick_lds_kernels<ResArgs>(l, rows, cols);
}

// fpm_gradient's column kernel of the rung: the launch shape of the sweep's
void gradient_lds_cols_kernel(const LdsLadder &l, StepKernel &cols_grad) {
    StepKernel rows{};  // (untouched)
    pick_lds_kernels<GradArgs>(l, rows, cols_grad);
}

hipError_t launch_general_step(const GeneralPlan &plan, const DevState &st, int led, int x0, int y0,
                               const float2 *tw, bool first, bool gains, hipStream_t s) {
    StepArgs sa;
    sa.led = led;
    sa.xc = x0 + st.np / 2;
    sa.yc = y0 + st.np / 2;
    if (plan.kind == GeneralPlan::Reg1024) {
        const hipError_t e = launch_np1024_rows_cols(st, sa, tw, !first, gains, s);
        if (e != hipSuccess) return e;
    } else if (plan.kind == GeneralPlan::Reg256) {
        return launch_np256_rows_cols(st, sa, tw, !first, gains, s);  // K4 inside, K5 folded
    } else {
        // a refused launch would leave T stale under K4 / K5: the first error ends the step
        for (const StepKernel *k : {&plan.k1, &plan.k2, gains ? &plan.k3_gain : &plan.k3}) {
            const hipError_t e = launch_step_kernel(*k, st, sa, plan.pl, tw, s);
            if (e != hipSuccess) return e;
        }
    }
    // K4's block size follows the LED's ROI tile columns
    const int nrow = (sa.yc + st.r) / kTile - (sa.yc - st.r) / kTile + 1;
    const int ncol = (sa.xc + st.r) / kTile - (sa.xc - st.r) / kTile + 1;
    if (ncol > 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tile_rows<1024>), dim3(nrow, st.B), dim3(1024), 0, s, st, sa);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tile_rows<256>), dim3(nrow, st.B), dim3(256), 0, s, st, sa);
    return plan.commit_folded() ? hipGetLastError() : launch_pupil_commit(st, s);
}

hipError_t launch_pupil_commit(const DevState &st, hipStream_t s) {
    hipLaunchKernelGGL(k_pupil_commit, dim3(st.npart, st.B), dim3(kCommitThreads), 0, s, st);
    return hipGetLastError();
}

}  // namespace fpm
