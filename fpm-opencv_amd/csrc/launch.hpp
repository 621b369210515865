// launch.hpp -- every host function of the .hip files that the extern "C"
// boundary (ctx.hpp and the .cpp files) or another .hip file calls, and the
// host structs they exchange.
// Included by ctx.hpp and by each file that defines or calls one of them, so a
// signature that drifts is a compile error and not a link-time surprise.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "fused_host.hpp"

namespace fpm {

// ---- the environment switches, read once per context (read_switches, create.cpp)
struct Switches {
    bool no_s90, no_reg1024, no_reg256, t32;  // FPM_NO_S90, FPM_NO_REG1024, FPM_NO_REG256, FPM_T32
    bool stamps, no_graph;                    // FPM_STAMPS, FPM_NO_GRAPH
    bool no_wave_cols, no_crop4k;             // FPM_NO_WAVE_COLS, FPM_NO_CROP4K
    bool s90_dense, mr_dense;                 // FPM_S90_DENSE, FPM_MR_DENSE
    bool no_split, no_dist;                   // FPM_NO_SPLIT, FPM_NO_DIST
    bool no_ledtab;                           // FPM_NO_LEDTAB: the fused kernels read the global LED tables
    int patch_groups, split, dist;            // FPM_PATCH_GROUPS, FPM_SPLIT, FPM_DIST: the value (>= 0), -1 = unset
    bool res_lds;                             // FPM_RES_LDS: the residual's LDS kernel pair where the register pair applies
    bool res_one_seq;                         // FPM_RES_ONE_SEQ: the LDS pair's one-sequence-per-block kernels at any size
    int res_batch;                            // FPM_RES_BATCH: LEDs per residual launch (> 0), else from the scratch cap
    bool one_seq;                             // FPM_ONE_SEQ: the update step's one-sequence-per-block kernels at any size
};

// ---- general path: the LED step (general.hip)
// One launch of the LDS step kernels (K1 / K2 / K3): every kernel takes
// (DevState, StepArgs, FftPlan, twiddles) and the tiled / wave ones one int more.
struct StepKernel {
    const void *fn;
    dim3 grid, block;
    size_t lds;  // dynamic LDS bytes
    int arg;     // rows per block lr, columns per block lc (both log2) or the column pitch P
    size_t lds_static;  // the kernel's own __shared__ bytes (the constants beside the kernels, general.hip)
    size_t lds_total() const { return lds + lds_static; }
};
// One launch of an LDS step kernel for the update step (A = StepArgs) or for
// nl LEDs of the residual sweep (ResArgs: blockIdx.z is the LED of the batch)
template <class A>
inline hipError_t launch_step_kernel(const StepKernel &k, DevState st, A a, FftPlan pl, const float2 *tw,
                                     hipStream_t s, int nl = 1) {
    int arg = k.arg;
    void *args[] = {&st, &a, &pl, &tw, &arg};  // the one-sequence kernels take the first four
    return hipLaunchKernel(k.fn, dim3(k.grid.x, k.grid.y, nl), k.block, args, k.lds, s);
}
// Once per context, before the first launch: a kernel that asks for more than
// the 64 KB of dynamic LDS a launch may take by default is allowed all the
// device offers (lds_limit less the kernel's own).  Never this context's own
// byte count: the attribute belongs to the kernel, and a later context with a
// smaller tile must not lower it under a live one that needs more.
inline hipError_t allow_large_lds(std::initializer_list<const StepKernel *> ks, size_t lds_limit) {
    for (const StepKernel *k : ks)
        if (k->lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(lds_limit - k->lds_static));
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}
// Which generation of the LDS row (K1 / K3) and column (K2) kernels a size
// runs, and their launch shapes (plan_lds_ladder, general.hip)
struct LdsLadder {
    StepKernel rows, cols;  // fn unset
    int row_e;              // tiled rows: register elements per thread (16 / 24); 0: one row per block
    int cw;                 // wave-private columns per wave (4 / 2); 0: tiled, or one column per block
    int col_e;              // tiled columns: register elements per thread (16 / 24); 0 otherwise
};
LdsLadder plan_lds_ladder(const FftPlan &pl, int np, int nb, int B, const Switches &sw, bool step);
// What launch_general_step launches for a context (a patch group): nothing in
// it depends on the LED, so fpm_create makes it once (plan_general_step).
struct GeneralPlan {
    // np1024.hip / np256.hip register kernels, or K1-K3 below; chosen with the
    // rest of the context (plan_context, create.cpp), since the stack's layout
    // and the scratch buffers follow it
    enum Kind { Reg1024, Reg256, Lds } kind;
    FftPlan pl;                               // of Np
    StepKernel k1, k2, k3;                    // Lds only
    StepKernel k3_gain;                       // k3's GAIN instance: what a context with gains launches
    LdsLadder ladder;                         // Lds only: the rung k1-k3 were picked from
    // the register row / column kernels fold the pupil commit into the next
    // LED's row IDFT (launch_pupil_commit after the iteration's last LED)
    bool commit_folded() const { return kind != Lds; }
};
GeneralPlan plan_general_step(const DevState &st, GeneralPlan::Kind kind, const FftPlan &pl, const Switches &sw);
// first: the iteration's first LED (register kernels: no pupil commit pending);
// gains: some LED gain is not 1, the update kernels' GAIN instances
hipError_t launch_general_step(const GeneralPlan &plan, const DevState &st, int led, int x0, int y0,
                               const float2 *tw, bool first, bool gains, hipStream_t s);
hipError_t launch_pupil_commit(const DevState &st, hipStream_t s);
int pupil_parts(int nb);
// Np 1024 / Np 256 register row/column kernels of the general path (np1024.hip, np256.hip)
bool np1024_supported(int np, int r);
bool np256_supported(int np, int r, int L, bool fp16);
hipError_t launch_np1024_rows_cols(const DevState &st, const StepArgs &sa, const float2 *tw, bool commit,
                                   bool gains, hipStream_t s);
hipError_t launch_np256_rows_cols(const DevState &st, const StepArgs &sa, const float2 *tw, bool commit,
                                  bool gains, hipStream_t s);

// ---- the data-fidelity residual of the current state (residual.hip)
// Scratch cap of a residual sweep: T of one launch's LEDs, [nl][B][nb][Np]
// complex.  256 MB is the size of the chip's last-level cache, so what the row
// kernel writes the column kernel can still find on the die, and at the metric
// geometry (256 patches, r 33: 35 MB per LED) it holds 7 LEDs = 9 000 row and
// 28 000 column blocks, tens of rounds of workgroups: a larger batch adds
// memory and no parallelism.
constexpr size_t kResidualScratchBytes = (size_t)256 << 20;
// One entry of a residual launch's list: the image and where its sub-aperture
// window sits, resolved on the host (order[pos], crop + offset + Np / 2) so a
// block finds its LED with a single 16-byte load.
struct alignas(16) ResEntry {
    int led;     // stack index
    int xc, yc;  // centre of the window in the centred spectrum
    int pad;
};
static_assert(sizeof(ResEntry) == 16, "res_led reads an entry as one int4");
// What a residual launch reads besides the state: the entry list (fpm_residual:
// the context's identity list, one entry per position of order[];
// fpm_residual_at: the caller's probes) and the context's residual scratch.
struct ResArgs {
    const ResEntry *ent;
    int i0;                    // index in ent[] of the batch's first entry
    float2 *T;                 // [nl][B][nb][Np] row-transform scratch
    double *perr;              // [nl][B][nblk] one partial of E per column block
    unsigned long long *pref;  //                and of S
    double *err, *ref;         // [n][B] the folded sums, by entry index
    int nblk;
};
// The same batch with another tail of the column kernels (residual_dev.hpp),
// each a type of its own so the tail is chosen at compile time and the
// ResArgs instances stay the code they were:
//   GainResArgs  the residual under a gain table that is not all ones,
//                E = sum (|psi| - g sqrt(I))^2 (fpm_set_gains)
//   MomArgs      fpm_moments: perr / err hold Q = sum |psi|^2, pcross / cross
//                C = sum |psi| sqrt(I) (null in a residual launch)
//   PredArgs     fpm_predict: no sums at all, the tail stores every pixel of
//                the image, out[entry - o0][patch][y][x] (perr .. nblk unused)
//   GradArgs     fpm_gradient: the gained sums as GainResArgs', then rho in
//                place of the amplitude replacement and the forward column
//                transform, the box rows kept back in T (the step's tail)
struct GainResArgs : ResArgs {};
struct GradArgs : ResArgs {};
struct MomArgs : ResArgs {
    double *pcross, *cross;
};
struct PredArgs : ResArgs {
    void *out;      // [n][B][Np][Np] float (amplitude, diff) or uint16_t (counts)
    unsigned kind;  // FPM_PREDICT_AMPLITUDE / _COUNTS / _DIFF: uniform over the launch
    int o0;         // the entry index out's first row belongs to
};
// Which kernel pair a context's sweep launches and how many LEDs at a time;
// decided with the rest of the context (plan_context: no HIP call).
struct ResidualPlan {
    enum Kind { Reg256, Lds } kind;
    FftPlan pl;                // of Np
    StepKernel rows, cols;     // one LED's grid: the launch multiplies it by the batch
    StepKernel cols_gain;      // cols with the gained residual's tail and with the moments' (fpm_moments):
    StepKernel cols_mom;       //   the same launch shape
    StepKernel cols_pred;      // cols with the pixel-storing tail (fpm_predict): no fold follows it
    StepKernel cols_grad;      // cols with fpm_gradient's tail (sums, rho, forward column transform)
    StepKernel grad_rows;      // fpm_gradient's rows out (gradient.hip): one LED's grid, as rows
    LdsLadder ladder;         // Lds only: the rung rows / cols were picked from
    int nblk;                  // column blocks = partials per (LED, patch)
    int nl;                    // LEDs per launch
    size_t t_led;              // complex elements of T per LED
};
ResidualPlan plan_residual(const DevState &st, const FftPlan &pl, int n_order, int meas_g, bool fp16,
                           const Switches &sw);
// the sweep's kernels are the step's, instantiated for ResArgs: the ladder's
// K1 / K2 (general.hip) and the Np 256 register column kernel (np256.hip)
enum class ResTail { Plain, Gain, Moments, Predict, Grad };
void residual_lds_kernels(const LdsLadder &l, StepKernel &rows, StepKernel &cols, StepKernel &cols_gain,
                          StepKernel &cols_mom, StepKernel &cols_pred);
const void *residual_cols256_kernel(ResTail tail);
void gradient_lds_cols_kernel(const LdsLadder &l, StepKernel &cols_grad);
// rows, columns and fold of the nl entries ra.ent[ra.i0 ...] with the column
// kernel of `tail` (Moments: ra.pcross / ra.cross set, both folds)
hipError_t launch_residual_batch(const ResidualPlan &p, const DevState &st, const MomArgs &ra, ResTail tail, int nl,
                                 const float2 *tw, hipStream_t s);
// rows and the pixel-storing columns of the nl entries pa.ent[pa.i0 ...]: entry
// i's images go to pa.out's row i - pa.o0 (fpm_predict)
hipError_t launch_predict_batch(const ResidualPlan &p, const DevState &st, const PredArgs &pa, int nl,
                                const float2 *tw, hipStream_t s);

// ---- fpm_gradient (gradient.hip)
// What the rows-out and accumulate kernels of a batch need besides the sweep's
// arguments: R [nl][B][nb][nb] scratch, the outputs (device memory, cleared
// before the list's first batch; either null) and the bounding box, in the
// centred spectrum, of the support boxes of the batch's windows.
struct GradAcc {
    const ResEntry *ent;  // set by the launcher from the batch: the list,
    int i0, nl;           //   its first entry and the number of entries
    const float2 *R;
    float2 *gO;           // [B][L][L] un-centred (fpm_download's objF layout)
    float2 *gP;           // [B][Np][Np] centred (fpm_download's pupil layout)
    int bx0, by0, bw, bh;
};
// the rows-out launch for the plan's kind (called by plan_residual)
void plan_gradient_rows(ResidualPlan &p, const DevState &st);
// rows in, columns with the GradArgs tail and the fold of E / S (ra as
// launch_residual_batch's), rows out, then the accumulation of the batch's nl
// entries into acc.gO / acc.gP in list order
hipError_t launch_gradient_batch(const ResidualPlan &p, const DevState &st, const MomArgs &ra, const GradAcc &acc,
                                 int nl, const float2 *tw, hipStream_t s);

// ---- batched transform of any length 2^a 3^b 5^c (fft_batch.hip)
// Input band: sequences gs outside [qlo, qhi] and elements gi with
// (gi + eroll) mod n outside [elo, ehi] are known to be exactly zero and are
// not read (objCrop over the spectrum's live band, fpm_state.hpp); the default
// covers everything.
struct FftBand {
    int qlo = 0, qhi = 0x7fffffff, elo = 0, ehi = 0x7fffffff, eroll = 0;
};
int fft_max_len();
// The launch of k_fft_batch for a length: fn (null when not even one sequence
// fits a block), the block, the dynamic LDS of the tile and the twiddles and
// arg = lc, log2 of the sequences per block.  What launch_fft_batch launches
// and what plan_objcrop records.
StepKernel fft_batch_kernel(const FftPlan &pl, bool inverse);
hipError_t launch_fft_batch(bool inverse, const float2 *in, float2 *out, const FftPlan &pl, const float2 *tw,
                            int nseq, int B, size_t in_bs, int in_ss, int in_es, size_t out_bs, int out_ss,
                            int out_es, int sroll, int iroll, float scale, hipStream_t s,
                            const __half2 *in16 = nullptr, float in16_scale = 1.f, FftBand band = FftBand());

// ---- fpm_init (init.hip)
hipError_t launch_init(const DevState &st, int init_led, float2 *scratch, const FftPlan &pl_np,
                       const float2 *tw_np, hipStream_t s);
// rmax from tmax (general path): k_row_max_all for a state that did not come from launch_init
hipError_t launch_row_max_all(const DevState &st, hipStream_t s);

// ---- fpm_set_state / fpm_download_state_device (state.hip)
// Device scratch of the check pass: the lowest linear index, in the caller's
// layout, of an offender in the spectrum ([0]) and in the pupil ([1]), ~0 =
// none; behind it max|P S| of each patch, float [B].
struct StateCheck {
    unsigned long long first[2];
};
inline float *state_check_pmax(StateCheck *c) { return reinterpret_cast<float *>(c + 1); }
inline size_t state_check_bytes(int B) { return sizeof(StateCheck) + (size_t)B * sizeof(float); }
// objF [B][L][L] un-centred, pupil [B][Np][Np] (pupil_shared: [Np][Np]) centred,
// both device memory, either null.  check writes chk only; place installs what
// check accepted (the spectrum with its tile / row maxima and clean dirty
// words, the pupil times the disk with chk's maxima as pmax); out is the
// inverse copy.  fused: max|P| as the fused kernels round it.
hipError_t launch_state_check(const DevState &st, const float2 *objF, const float2 *pupil, bool pupil_shared,
                              bool fused, StateCheck *chk, hipStream_t s);
hipError_t launch_state_place(const DevState &st, const float2 *objF, const float2 *pupil, bool pupil_shared,
                              const StateCheck *chk, hipStream_t s);
hipError_t launch_state_out(const DevState &st, float2 *objF, float2 *pupil, hipStream_t s);

// ---- fpm_stitch / fpm_stitch_tiles (stitch.hip)
// gy x gx tiles of L x L at strides (sy, sx) and the H x W field they cover
struct StitchGeom {
    int gy, gx, L, sy, sx, H, W;
};
// Workgroups per neighbour pair of the pair-sum pass: what a left/right and an
// up/down region need, and the larger of the two (>= 1), the pitch of partials
struct StitchParts {
    int lr, ud, parts;
};
StitchParts stitch_pair_parts(const StitchGeom &g);
// (c_re, c_im, a, b) of every neighbour pair (stitch_solve.hpp: StitchPairSums,
// pair order) into sums [pairs][4]; partials [pairs][parts][4] is scratch
hipError_t launch_stitch_pairs(const StitchGeom &g, const float2 *tiles, double *partials, double *sums,
                               hipStream_t s);
// field [H][W] = sum_t w_t factors[t] T[t]; factors [gy*gx] or null = all ones.
// stitch_blend_vector: the launch takes the 16-byte path
bool stitch_blend_vector(const StitchGeom &g, const float2 *tiles, const float2 *field);
hipError_t launch_stitch_blend(const StitchGeom &g, const float2 *tiles, const float2 *factors, float2 *field,
                               hipStream_t s);

// ---- fpm_refocus (refocus.hip)
// The angular-spectrum multiply of one plane: scratch [B][L][L] (centred, fp32)
// = spec_ld(st, b, .) H(zl[b * zstride]) over the live band of st; nothing
// outside the band is written.  zl is device memory, zstride 0 (one z for
// every patch) or 1.
hipError_t launch_refocus_mul(const DevState &st, const double *zl, int zstride, double fl, float2 *scratch,
                              hipStream_t s);
// Row strips (= partials) per patch of the sums pass at this L and margin
int refocus_sum_blocks(int L, int margin);
// The focus sums of one plane [B][L][L] over [margin, L - margin)^2: per-block
// partials [B][blocks][3], then the fold in block order into sum_a[b],
// sum_a2[b], sum_g[b] (device memory, [B] each)
hipError_t launch_refocus_sums(const float2 *plane, int B, int L, int margin, double *partials, double *sum_a,
                               double *sum_a2, double *sum_g, hipStream_t s);

// ---- objCrop (objcrop.hip; kernels: crop256m.hip, crop600.hip, crop360.hip, crop4k.hip, fft_batch.hip)
// The two launches of a register family, one table row per family file.  Every
// row kernel takes (spec, out, tw, sy0, sy1, sx0, sx1) and every column kernel
// (io, tw, scale, sy0, sy1); arg = rows per block / columns per strip.  The
// grids follow the live band, which fpm_set_crops and fpm_debug_objcrop
// change, so they are computed at launch.
struct CropPair {
    StepKernel rows, cols;  // grid unset
};
inline StepKernel crop_kernel(const void *fn, int threads, size_t lds, int per_block, size_t lds_static = 0) {
    return StepKernel{fn, dim3(), dim3(threads), lds, per_block, lds_static};
}
CropPair crop256m_kernels(int L);  // L = 512 / 768 / 1024; any other L: fn null
CropPair crop600_kernels();
CropPair crop360_kernels();
// The three passes of the six-step L 4096 transform, in launch order; arg =
// columns (cols1, cols2) / rows per block
struct Crop4kKernels {
    StepKernel cols1, cols2, rows;  // grid unset
};
Crop4kKernels crop4k_kernels();
// What launch_objcrop launches for a context; decided with the rest of the
// context (plan_context: no HIP call).
struct ObjcropPlan {
    // register transforms of L = 256 M, 600 and 360; the six-step L 4096
    // passes; the batched transform (fft_batch.hip)
    enum Kind { Regs256M, Regs600, Regs360, SixStep4k, Batched } kind;
    StepKernel rows, cols;  // grid unset; Batched: k_fft_batch, arg = sequences per block C (fn null: L does not fit)
    StepKernel cols2;       // SixStep4k only: the in-place second column pass (cols is the first)
    FftPlan pl;             // Batched only: of L
    bool regs() const { return kind == Regs256M || kind == Regs600 || kind == Regs360; }
    // the pass that runs first: the six-step transform starts with its columns
    const StepKernel &first() const { return kind == SixStep4k ? cols : rows; }
};
ObjcropPlan plan_objcrop(int L, bool fp16, const FftPlan &pl_L, const Switches &sw);
// hipErrorInvalidValue when the live band of st is not 0 <= lo <= hi < L
hipError_t launch_objcrop(const ObjcropPlan &plan, const DevState &st, float2 *out, const float2 *tw_L,
                          hipStream_t s);

// ---- Np 256 fused kernel: one workgroup per patch and split mode (fpm_fused.hip)
int fused_threads(int np, int r, int L, const DevState &st);
size_t fused_T_elems(int np, int r, int B);
size_t fused_xch_elems(int B, int ks);
size_t fused_flag_words(int B, int ks);
int fused_split_parts(int nt, int B, int n_cu, const Switches &sw);
hipError_t launch_fused_iteration(const DevState &st, const FusedLaunch &in, int ks, float2 *xch, int *flags,
                                  int stall_led, hipStream_t s);
// ---- distributed mode of the Np 256 kernel (fused_dist.hip)
size_t fused_dist_elems(int B, int ks);
int fused_dist_parts(int B, int n_cu, int r, int L, const Switches &sw);
hipError_t launch_fused_dist(const DevState &st, const FusedLaunch &in, int ks, float2 *area, int *flags,
                             int stall_led, unsigned tag_base, hipStream_t s);
// ---- Np 200 fused kernel (fused_mr.hip)
bool fused_mr_supported(int np, int r, const DevState &st);
hipError_t launch_fused_mr_iteration(const DevState &st, const FusedLaunch &in, hipStream_t s);
// ---- Np 90 fused kernel (fused_s90.hip)
bool fused_s90_supported(int np, int r, const DevState &st);
hipError_t launch_fused_s90_iteration(const DevState &st, const FusedLaunch &in, hipStream_t s);
// ---- small-patch fused kernel (fused_small.hip, Np <= 96)
bool fused_small_supported(int np, int r, const DevState &st);
hipError_t launch_fused_small_iteration(const DevState &st, const FusedLaunch &in, const FftPlan &pl,
                                        hipStream_t s);

// ---- measurement preprocessing and the fused kernels' in-place layout (preprocess.hip)
hipError_t meas_layout(uint16_t *meas, int np, int g, size_t nimg, bool fwd, hipStream_t s);
bool meas_layout_copy(const uint16_t *src, uint16_t *dst, int np, int g, size_t nimg, hipStream_t s,
                      hipError_t *err);
hipError_t launch_preprocess_frame(const uint16_t *frame, int width, int np, int B, const int *px0_dev,
                                   const int *py0_dev, int bk1x, int bk1y, int bk2x, int bk2y, double bg_threshold,
                                   double dark_mult, bool darkfield, unsigned long long *sums, uint16_t *out,
                                   int16_t *bg_out_dev, hipStream_t s);

}  // namespace fpm
