/*
 * fpm_hip.h -- C ABI of the MI355X-native FPM solver (libfpm_hip.so).
 *
 * Drop-in boundary for the reference's hot path
 *     void runFPM(FPM_Dataset *dataset);      fpmMain.h:119, fpmMain.cpp:274-498
 * which is called once from main after loadFPMDataset (fpmMain.cpp:590-591).
 * FPM_Dataset is a C++ class full of cv::UMat, so the ABI flattens exactly the
 * fields runFPM reads into plain integers, doubles and
 * pointers; the outputs runFPM writes (objF, objCrop, pupil, pupilSupport) are
 * copied out by fpm_download.  No torch or OpenCV types cross this boundary.
 *
 * Conventions
 *   - complex arrays are interleaved float32 pairs (re, im), row-major;
 *   - "stack index" = position of an LED image in the uploaded stack
 *     (the reference indexes imageStack by LED number; the host front-end maps
 *     LED numbers to stack indices, fpm_host.h);
 *   - every call returns FPM_OK (0) or a negative errno-style code, and
 *     fpm_last_error() describes the most recent failure on this thread;
 *   - the caller owns host buffers, the library owns device buffers;
 *   - one context per GPU; a context is not shared between threads.
 */
#ifndef FPM_HIP_H
#define FPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  Round 4 (4): fpm_info gained threads_per_wg,
 * readable only through fpm_get_info_sized.  Round 6 (5): fpm_get_info writes
 * only the ABI-3 struct size (path .. fused_kernel) -- under ABI 4 it wrote
 * the whole struct, so a caller reading threads_per_wg from it must move to
 * fpm_get_info_sized; fpm_get_clock added; fpm_run refuses a capturing
 * stream.  (6): fpm_residual added.  fpm_abi_version() reports the library's
 * revision.  Entry points appended since then change nothing a revision-6
 * caller sees, so the revision stands and each addition has a feature macro:
 * FPM_HAS_LED_CALIBRATION = fpm_residual_at, fpm_set_crops, fpm_get_crops;
 * FPM_HAS_LED_GAINS = fpm_set_gains, fpm_get_gains, fpm_moments;
 * FPM_HAS_STATE = fpm_set_state, fpm_download_state_device;
 * FPM_HAS_STITCH = fpm_stitch_tiles, fpm_stitch;
 * FPM_HAS_PREDICT = fpm_predict;
 * FPM_HAS_REFOCUS = fpm_refocus;
 * FPM_HAS_GRADIENT = fpm_gradient. */
#define FPM_ABI_VERSION   6
#define FPM_HAS_PREDICT 1
#define FPM_HAS_REFOCUS 1
#define FPM_HAS_GRADIENT 1
#define FPM_HAS_LED_CALIBRATION 1
#define FPM_HAS_LED_GAINS 1
#define FPM_HAS_STATE 1
#define FPM_HAS_STITCH 1

#define FPM_OK            0
#define FPM_ERR_INVAL   (-22)   /* bad argument / unsupported geometry      */
#define FPM_ERR_NOMEM   (-12)   /* device or host allocation failed          */
#define FPM_ERR_DEVICE   (-5)   /* HIP runtime / kernel launch failure       */
#define FPM_ERR_STATE   (-71)   /* call out of order (e.g. run before init)  */
#define FPM_ERR_NODEV   (-19)   /* no usable gfx950 device                   */

/* Solver path selection (fpm_problem.path). */
#define FPM_PATH_AUTO     0     /* fused per-patch kernel when it applies    */
#define FPM_PATH_GENERAL  1     /* 4 kernels per LED step, any Np / radius   */
#define FPM_PATH_FUSED    2     /* one persistent launch per iteration       */

/*
 * Raw sensor frames for fpm_upload_frames: the loader preprocessing of
 * loadFPMDataset (fpmMain.cpp:124-144) on the device, for n_patch patches
 * cut from each full frame:
 *   Image  = frame[patch_y0 + y][patch_x0 + x]                 (:124-125)
 *   Image  = saturate(rint(Image / darkfield_exp_multiplier))  when darkfield[i]
 *            and the multiplier != 1                            (:128-129)
 *   bg     = (mean(bk1 window) + mean(bk2 window)) / 2 of the UNDIVIDED
 *            frame, clamped to bg_threshold, rounded to int16   (:131-140)
 *   Image  = saturate(Image - bg)                               (:143-144)
 * Background windows are Np x Np and shared by all patches of a frame; they
 * may coincide with each other and with a patch.  The divide rounds half to
 * even (5 / 2 -> 2, 7 / 2 -> 4) and saturates at 65535 (a multiplier below 1);
 * bg rounds half away from zero (999.5 -> 1000, -7.5 -> -8); the subtraction
 * saturates at 0 and, with a negative bg_threshold, at 65535.  darkfield[i] is
 * read as a flag: any nonzero value divides.  The window sums are exact at
 * every Np (64-bit).  All of this is pinned bit for bit against the oracle's
 * restatement, on every stack layout a context can have
 * (tests/preprocess_cases.py).  Out of contract: a background above 32767,
 * where the reference's (int16_t)round(bg) is undefined.
 */
typedef struct fpm_frames {
    int32_t height, width;        /* full frame size                              */
    const int32_t *patch_x0;      /* [n_patch] cropX of each patch (column)       */
    const int32_t *patch_y0;      /* [n_patch] cropY of each patch (row)          */
    int32_t bk1_x, bk1_y;         /* bk1cropX / bk1cropY                          */
    int32_t bk2_x, bk2_y;         /* bk2cropX / bk2cropY                          */
    double  bg_threshold;         /* bgThresh (JSON asInt)                        */
    double  darkfield_exp_multiplier;  /* darkfieldExpMultiplier                  */
    const uint8_t *darkfield;     /* [n_stack] 1 where illumination NA > objective NA */
} fpm_frames;

/* fpm_problem.flags */
#define FPM_FLAG_OBJCROP_LAST_ONLY 1u  /* compute objCrop only after the last
                                          iteration of fpm_run (the reference
                                          recomputes it every iteration,
                                          fpmMain.cpp:481; default keeps that) */
#define FPM_FLAG_SPEC_FP16         2u  /* store the high-resolution spectrum as
                                          fp16 (scaled by a power of two), compute
                                          in fp32: BASELINE config 5 ("fp16
                                          storage / fp32 accumulate"); general
                                          path only.  The reference keeps
                                          CV_64FC2 objF (fpmMain.h:92) */
#define FPM_FLAG_SCALAR_RE_ONLY    4u  /* legacy semantics for the reference's
                                          cv::add / cv::multiply(UMat CV_64FC2,
                                          double) at fpmMain.cpp:390,417-418,
                                          469-470: the scalar touches the real
                                          channel only.  Default (flag clear) is
                                          OpenCV's published behaviour: a double
                                          becomes a 1x1 array that arithm_op's
                                          convertAndUnrollScalar replicates into
                                          EVERY channel, so eps is added to Re and
                                          Im and the update denominators are
                                          complex, ((|P|^2+d2) + i d2) max|P| and
                                          ((|O|^2+d1) + i d1) max|objF| (DESIGN.md
                                          section 2) */

/*
 * Problem description: the FPM_Dataset fields runFPM reads
 * (fpmMain.h:43-101, read at fpmMain.cpp:290-481).
 */
typedef struct fpm_problem {
    int32_t np;            /* Np: ROI size (cropSizeX, fpmMain.cpp:519); even    */
    int32_t nlarge;        /* Nlarge == Mlarge == Np*resImprovementFactor (:564) */
    int32_t n_stack;       /* images in the uploaded stack                       */
    int32_t n_order;       /* ledUsedCount: LEDs processed per iteration (:348)  */
    const int32_t *order;  /* [n_order] stack indices in processing order:
                              sortedIndicies[0..ledUsedCount) (fpmMain.cpp:350)  */
    const int32_t *crop_x0;/* [n_stack] cropXStart in the centred spectrum (:157) */
    const int32_t *crop_y0;/* [n_stack] cropYStart (:163)                        */
    int32_t na_radius;     /* naRadius = ceil(objNA*ps_eff*Np/lambda) (:305)     */
    int32_t init_pos;      /* position in order[] of the init image; the
                              reference uses sortedIndicies.at(1) (:319) -> 1    */
    double  delta1;        /* pupil-update regulariser, JSON asInt (:567)         */
    double  delta2;        /* object-update regulariser, JSON asInt (:568); > 0  */
    double  eps;           /* amplitude-replacement eps, float 1e-10 (fpmMain.h:99) */
    int32_t n_patch;       /* independent patches batched on this device (>= 1) */
    int32_t path;          /* FPM_PATH_*                                          */
    uint32_t flags;        /* FPM_FLAG_*                                          */
} fpm_problem;

typedef struct fpm_ctx fpm_ctx;

/* fpm_info.fused_kernel: the LED-update kernel fpm_run launches */
#define FPM_KERNEL_GENERAL      0  /* general path: 4-5 launches per LED          */
#define FPM_KERNEL_FUSED_NP256  1  /* k_fused_iteration (Np 256, r <= 34)          */
#define FPM_KERNEL_FUSED_NP200  2  /* k_fused_mr (Np 200)                          */
#define FPM_KERNEL_FUSED_SMALL  3  /* k_fused_small (Np <= 96)                     */
#define FPM_KERNEL_FUSED_NP256_DIST 4  /* k_fused_dist (Np 256, every phase distributed
                                          over wg_per_patch workgroups; small batches) */
#define FPM_KERNEL_FUSED_NP90   5  /* k_fused_s90 (Np 90: register 9 x 10 transforms) */

/* Which path the context runs and its per-launch geometry. */
typedef struct fpm_info {
    int32_t path;          /* FPM_PATH_GENERAL or FPM_PATH_FUSED */
    int32_t box;           /* 2*na_radius+1: side of the pupil box             */
    int32_t support_px;    /* pixels in the pupil support disk                  */
    int32_t device;
    size_t  device_bytes;  /* device memory owned by the context               */
    int32_t wg_per_patch;  /* fused Np 256 path: workgroups per patch (1, or 2 /
                              4 / 8 in split or distributed mode when
                              wg_per_patch * n_patch <= CUs)                   */
    int32_t fused_kernel;  /* FPM_KERNEL_*                                      */
    int32_t threads_per_wg;/* threads per workgroup of the LED-update kernel (ABI 4) */
} fpm_info;

/* bytes of the ABI-3 struct, fields path .. fused_kernel: what fpm_get_info writes */
#define FPM_INFO_V3_SIZE  (offsetof(fpm_info, fused_kernel) + sizeof(int32_t))

/* Per-kernel timing of the most recent fpm_run, from HIP events recorded on
 * the stream the kernels were launched on.  fpm_run clears it (and the
 * fpm_clock below) once its arguments are accepted, so after a run that was
 * refused (a capturing stream) or failed every field is zero: never the values
 * of an earlier run. */
typedef struct fpm_timing {
    double run_ms;         /* whole fpm_run, event to event                    */
    double led_ms;         /* LED-update kernels only (all iterations)         */
    double led_launch_ms;  /* average duration of one LED-update launch        */
    int32_t led_launches;  /* number of LED-update launches measured           */
    double objcrop_ms;     /* per-iteration objCrop IDFT kernels               */
} fpm_timing;

/* Create a context on `device`; validates geometry, allocates device state. */
int  fpm_create(const fpm_problem *prob, int device, fpm_ctx **out);
void fpm_destroy(fpm_ctx *ctx);

/* Upload the measurement stack, uint16 [n_stack][n_patch][Np][Np]
 * (LED-major: every LED step reads one contiguous slab). Host pointer. */
int  fpm_upload_stack(fpm_ctx *ctx, const uint16_t *meas);
/* Same, from device memory on the context's device (no PCIe round trip). */
int  fpm_upload_stack_device(fpm_ctx *ctx, const uint16_t *meas_dev);

/* Upload raw frames [n_stack][height][width] (host memory, or device memory on
 * the context's device when frames_on_device != 0) and build the measurement
 * stack on the GPU (fpm_frames above).  bg_val, when not NULL, receives the
 * per-image background [n_stack] (FPMImage::bg_val, fpmMain.h:33). */
int  fpm_upload_frames(fpm_ctx *ctx, const fpm_frames *frames, const uint16_t *data,
                       int frames_on_device, int16_t *bg_val);

/* Copy the measurement stack [n_stack][n_patch][Np][Np] back to the host. */
int  fpm_download_stack(fpm_ctx *ctx, uint16_t *meas);

/* fpmMain.cpp:302-343: pupil = support disk, spectrum from order[init_pos]. */
int  fpm_init(fpm_ctx *ctx);

/* fpmMain.cpp:345-482: `iters` sequential passes over order[], each followed
 * by the objCrop IDFT (fpmMain.cpp:481) unless FPM_FLAG_OBJCROP_LAST_ONLY.
 * Enqueued on the context stream; returns when the work has completed
 * (per-kernel HIP-event timings are then available from fpm_get_timing).
 * Blocking, so it cannot be recorded into a graph: on a stream that is being
 * captured it returns FPM_ERR_INVAL before enqueuing anything (the capture
 * stays valid).  The split / distributed modes also need every workgroup of
 * a grid resident at once, which a replayed graph could not guarantee
 * beside other co-resident grids. */
int  fpm_run(fpm_ctx *ctx, int iters);

/* Data-fidelity residual of the current state (read-only: spectrum, pupil,
 * maxima, objCrop and the stack are left bit for bit as they were).
 *   err [n_order][n_patch]  E = sum_yx (|psi| - g sqrt(I))^2, psi = ifft2(window * P)
 *                           scaled 1/Np^2 like the reference's ifft2; no eps;
 *                           g the image's gain (fpm_set_gains; 1 by default)
 *   ref [n_order][n_patch]  S = sum_yx I  (exact)
 * Row i is order[i]'s LED.  Either pointer may be NULL, not both.
 * elapsed_ms (may be NULL): event-to-event time of the sweep on the run stream.
 * Blocking.  FPM_ERR_STATE before fpm_init; FPM_ERR_INVAL on a capturing
 * stream, before anything is enqueued (as fpm_run).  fpm_timing and fpm_clock
 * of the last fpm_run are not touched.  The first call allocates the sweep's
 * scratch (at most 256 MB of row transforms unless one LED's exceed that;
 * counted in fpm_info.device_bytes from then on).  Two calls on the same
 * state return the same bits. */
int  fpm_residual(fpm_ctx *ctx, double *err, double *ref, double *elapsed_ms);

/* The residual of the current state with windows moved: LED position
 * calibration's search.  Entry k gives E (and S) for the image of order[pos]
 * with its sub-aperture window at (crop_x0 + dx, crop_y0 + dy) instead of
 * (crop_x0, crop_y0).
 *   err, ref [n][n_patch]   as fpm_residual's, row k = probes[k]; either may
 *                           be NULL, not both
 * The contract of fpm_residual: read-only, blocking, deterministic;
 * FPM_ERR_STATE before fpm_init; FPM_ERR_INVAL on a capturing stream.  Every
 * entry is validated on the host before the first launch: FPM_ERR_INVAL,
 * naming the entry, when n < 1, when pos is outside [0, n_order), or when a
 * window leaves the spectrum (0 <= crop + d <= Nlarge - Np must hold in x and
 * y: fpm_create's rule).  A window may leave the live band of the spectrum:
 * it reads the stored zeros there.  An entry's value depends on the state and
 * on that entry alone (not on its neighbours in the list, the batch it ran
 * in or FPM_RES_BATCH), and (pos, 0, 0) returns the bits of fpm_residual's row
 * pos.  Entries run in list order, so keep an LED's candidates adjacent: its
 * image is then read while cached.  n is not limited: lists longer than
 * n_order run in pieces through the same scratch. */
typedef struct fpm_probe {
    int32_t pos;           /* position in order[]                               */
    int32_t dx, dy;        /* offset of the window from the crop table's        */
} fpm_probe;
int  fpm_residual_at(fpm_ctx *ctx, const fpm_probe *probes, int n, double *err, double *ref,
                     double *elapsed_ms);

/* Replace the crop table ([n_stack] each, validated as by fpm_create) of a
 * live context; spectrum, pupil, stack and everything the caller holds stay
 * valid.  Legal before and after fpm_init and between fpm_run calls; blocking
 * (waits for the run stream); FPM_ERR_INVAL on a capturing stream.  The new
 * table must plan the context fpm_create planned (same kernels, launch shapes
 * and LDS fits, judged with the live band grown to hold the old and the new
 * windows); otherwise FPM_ERR_INVAL with the reason, and the context is
 * unchanged: create a new one for such a table.  fpm_get_crops copies the
 * table in use. */
int  fpm_set_crops(fpm_ctx *ctx, const int32_t *crop_x0, const int32_t *crop_y0);
int  fpm_get_crops(const fpm_ctx *ctx, int32_t *crop_x0, int32_t *crop_y0);

/* LED gains: a per-image amplitude factor g [n_stack][n_patch] (float32,
 * LED-major like the stack, all ones by default) for LEDs whose brightness or
 * exposure differs from the nominal one.  Every consumer of a measured
 * amplitude uses g sqrt(I) in place of sqrt(I): fpm_init's initial spectrum,
 * the amplitude replacement of every LED step (psi' = g sqrt(I) psi / |psi + eps|,
 * eps untouched) and E of fpm_residual / fpm_residual_at; S stays the raw sum.
 * A gain of 1.0f is bit for bit no gain.
 * fpm_set_gains: every value finite and > 0, and under FPM_FLAG_SPEC_FP16
 * 256 g < 65504 (the headroom of the fp16 spectrum); otherwise FPM_ERR_INVAL
 * naming the first bad index, the context unchanged.  NULL = all ones.  Legal
 * before and after fpm_init and between fpm_run calls; blocking (waits for
 * the run stream); FPM_ERR_INVAL on a capturing stream.  Spectrum, pupil,
 * maxima and stack are untouched.  fpm_get_gains copies the table in use. */
int  fpm_set_gains(fpm_ctx *ctx, const float *gain);
int  fpm_get_gains(const fpm_ctx *ctx, float *gain);

/* The sums a gain is estimated from, of the current state:
 *   model [n][n_patch]  Q = sum_yx |psi|^2
 *   cross [n][n_patch]  C = sum_yx |psi| sqrt(I)
 *   ref   [n][n_patch]  S = sum_yx I  (exact)
 * with psi as fpm_residual's.  Raw: the gain table does not enter, so for any g
 *   E(g) = Q - 2 g C + g^2 S,   argmin_g E = C / S,   min_g E = Q - C^2 / S.
 * probes == NULL: the context's own list (n is ignored; row i is order[i]'s
 * LED, as fpm_residual's); otherwise fpm_residual_at's entries, validation and
 * row order, so the best window under an unknown brightness is the entry that
 * minimises Q - C^2 / S.  Any output pointer may be NULL, not all of them.
 * The contract of fpm_residual_at: read-only, blocking, deterministic (an
 * entry's bits depend on the state and that entry alone); FPM_ERR_STATE before
 * fpm_init; FPM_ERR_INVAL on a capturing stream before anything is enqueued.
 * It runs the residual sweep's kernels and scratch plus two buffers of sums of
 * its own, allocated by its first call. */
int  fpm_moments(fpm_ctx *ctx, const fpm_probe *probes, int n, double *model, double *cross,
                 double *ref, double *elapsed_ms);

/* The forward model's images of the current state: what each LED should have
 * produced, psi = ifft2(window * P) with psi as fpm_residual's (scaled 1/Np^2,
 * no eps), per pixel.  flags = exactly one kind, optionally | FPM_PREDICT_DEVICE:
 *   AMPLITUDE  float32  |psi|, raw: the gain table does not enter (as fpm_moments)
 *   COUNTS     uint16   the image the camera would record,
 *                       sat_u16(rint((|psi| / g)^2)): half to even, saturated at
 *                       65535, g the image's gain (fpm_set_gains)
 *   DIFF       float32  |psi| - g sqrt(I), the signed per-pixel mismatch
 * A gain of 1.0f is bit for bit no gain.
 *   out [n][n_patch][Np][Np]  pixel (y, x) at y*Np + x whatever layout the
 *                             context keeps its stack in; host memory, or with
 *                             FPM_PREDICT_DEVICE memory of the context's device
 * probes == NULL: the context's own list (n is ignored; n = n_order and row i
 * is order[i]'s LED, so COUNTS scattered from position i to stack index
 * order[i] is fpm_upload_stack's layout); otherwise fpm_residual_at's entries,
 * validation, messages and row order.  n is not limited.
 * The contract of fpm_residual_at: read-only (spectrum, pupil, maxima,
 * objCrop, stack, gains, crops, fpm_timing and fpm_clock are left bit for
 * bit), blocking, deterministic (an entry's bytes depend on the state and on
 * that entry alone, not on the batch, FPM_RES_BATCH or its neighbours);
 * FPM_ERR_INVAL on a capturing stream before anything is enqueued, on a NULL
 * out, on more than one kind and on an unknown flag bit; FPM_ERR_STATE before
 * a state exists.  AMPLITUDE and COUNTS need no stack and never read it: they
 * are legal on a context initialised by fpm_set_state alone (simulation).
 * DIFF returns FPM_ERR_STATE "no stack uploaded" there.
 * It runs the residual sweep's kernels and scratch.  With a device out the
 * kernels store straight into the caller's memory; with a host out each
 * launch's batch goes through a staging buffer of nl * n_patch * Np^2 4-byte
 * elements (nl = LEDs per launch), allocated by the first such call and
 * counted in fpm_info.device_bytes from then on.
 * elapsed_ms (may be NULL): event to event over the kernels; the staging
 * copies to the host are outside it. */
#define FPM_PREDICT_AMPLITUDE 0u
#define FPM_PREDICT_COUNTS    1u
#define FPM_PREDICT_DIFF      2u
#define FPM_PREDICT_DEVICE    4u
int  fpm_predict(fpm_ctx *ctx, const fpm_probe *probes, int n, uint32_t flags, void *out,
                 double *elapsed_ms);

/* The gradient of the data-fidelity cost of the current state.  For a list of
 * entries and every patch, with psi exactly as fpm_residual's,
 *   psi_i = ifft2(ifftshift(W_i) P)       scaled 1/Np^2, no eps
 *   W_i   = the entry's Np x Np window of O = fftshift(objF)
 *   P     = ifftshift(pupil support)
 *   f     = sum_i sum_yx (|psi_i| - g_i sqrt(I_i))^2 = sum_i E_i of fpm_residual_at
 * the outputs are G = df/dRe(z) + i df/dIm(z), so that df = sum Re(conj(G) dz):
 * the convention of PyTorch's complex leaves, twice the Wirtinger derivative
 * df/dconj(z).  With
 *   rho_i = psi_i - g_i sqrt(I_i) psi_i / |psi_i|    (0 where |psi_i| = 0)
 *   R_i   = fft2(rho_i) / Np^2
 *   G_O[window_i] += 2 fftshift(conj(P) R_i)        grad_objF  = ifftshift(G_O)
 *   G_P           += 2 conj(ifftshift(W_i)) R_i     grad_pupil = fftshift(G_P) support
 *   grad_objF  [n_patch][L][L][2]    un-centred, fpm_download's objF layout
 *   grad_pupil [n_patch][Np][Np][2]  centred, fpm_download's pupil layout
 *   err, ref   [n][n_patch]          E and S of the same entries (fpm_residual_at's),
 *                                    from the same pass; either may be NULL
 * The gradients are host memory, or with FPM_GRAD_DEVICE memory of the
 * context's device; either may be NULL, not both.  They are fp32 on every
 * context (FPM_FLAG_SPEC_FP16 included).
 * probes == NULL: the context's own list (n is ignored), as fpm_predict;
 * otherwise fpm_residual_at's entries, validation, messages and row order: a
 * moved window gives the gradient with that window, and a list may name an LED
 * more than once (each entry counts once).
 * Every element of an output is written: exactly zero outside the union of the
 * entries' support disks (grad_objF) and outside the support (grad_pupil).  An
 * entry whose window misses the spectrum's support (psi = 0) adds exactly
 * nothing.  A gain table of ones returns the bits of no table.
 * Deterministic without floating-point atomics: entries are added in list
 * order, each element by one thread, so the bits depend on the state and the
 * list alone -- not on FPM_RES_BATCH, on how the list was cut into launches or
 * on an earlier call.
 * One use: objF -= Np^2 grad_objF / (2 M), M_k = sum_i |P(k - c_i)|^2 (c_i the
 * window's position) where M > 0, majorises the cost: with the pupil held fixed
 * it never increases f.  The same holds for the pupil with the object fixed
 * and M_k = sum_i |O(c_i + k)|^2.  A spectrum given to fpm_set_state must stay
 * zero outside the live band; the gradient of the context's own list is.
 * The contract of fpm_predict: read-only (spectrum, pupil, maxima, objCrop,
 * stack, gains, crops, fpm_timing and fpm_clock are left bit for bit),
 * blocking; FPM_ERR_INVAL on a capturing stream before anything is enqueued, on
 * an unknown flag bit and on both gradient pointers NULL; FPM_ERR_STATE before
 * a state exists or with no stack uploaded.
 * It runs the residual sweep's kernels and scratch plus R of one launch's
 * entries (nl n_patch (2r+1)^2 complex), allocated by the first call; a host
 * output goes through a device copy of its own size, allocated by the first
 * call that asks for it; with a device pointer the accumulation goes straight
 * into the caller's memory.  All of it is counted in fpm_info.device_bytes.
 * elapsed_ms (may be NULL): event to event over the kernels; the copies of the
 * gradients to the host are outside it. */
#define FPM_GRAD_DEVICE 1u   /* grad_objF / grad_pupil are memory of the context's device */
int  fpm_gradient(fpm_ctx *ctx, const fpm_probe *probes, int n, uint32_t flags,
                  float *grad_objF, float *grad_pupil, double *err, double *ref,
                  double *elapsed_ms);

/* Digital refocusing: the recovered field propagated to other z planes by the
 * angular-spectrum method, and the sums a focus measure is made of, without
 * the spectrum leaving the device.  The arguments are dimensionless, as
 * fpm_problem is:
 *   zl [nz]   z / lambda, the signed distance in wavelengths; with
 *             FPM_REFOCUS_Z_PER_PATCH [nz][n_patch], every patch its own
 *   fl        lambda / (L ps), the normalised frequency of one spectrum bin
 *             (ps the high-resolution pixel size, fpm_host's ps)
 * Plane.  With objF as fpm_download returns it (un-centred) and signed bin
 * indices ky, kx in [-L/2, L/2):
 *   s   = fl^2 (kx^2 + ky^2)
 *   H   = exp(+i 2 pi zl sqrt(1 - s)) for s <= 1, 0 for s > 1 (evanescent)
 *   u_z = IDFT2(objF H) / L^2        (objCrop's transform and scale)
 * The phase is taken in double: c = zl sqrt(1 - s) is reduced to c - rint(c)
 * and the fp32 sine and cosine of that fraction of a turn are used, so H is
 * correct to fp32 rounding for every accepted zl.  A plane whose zl entries are
 * all exactly 0 is the transform of the stored spectrum itself: the bits of
 * fpm_download's objCrop (its evanescent bins included).
 *   planes [nz][n_patch][L][L][2]  host memory, or with FPM_REFOCUS_DEVICE
 *                                  memory of the context's device, clear of
 *                                  the context's own buffers; may be NULL
 * Focus sums, per plane and patch over the interior R = [margin, L - margin)^2
 * (a propagated field wraps around its border), a the fp32 magnitude of u_z:
 *   sum_a  [nz][n_patch]  sum_R a
 *   sum_a2 [nz][n_patch]  sum_R a^2
 *   sum_g  [nz][n_patch]  sum (a(y,x+1) - a(y,x))^2 + sum (a(y+1,x) - a(y,x))^2
 *                         over the pairs that lie wholly in R
 * Differences and squares are formed and accumulated in double in a fixed
 * order (per-block partials, then a fold; no floating-point atomics).  Any of
 * the three may be NULL.  With N = |R|, m = sum_a / N, v = sum_a2 / N - m^2:
 * normalised variance v / m^2, Tamura coefficient sqrt(sqrt(v) / m), gradient
 * energy sum_g / sum_a2; which one suits a sample is the caller's choice.
 * Accuracy: a carries fp32 rounding (relative e of about 1e-7), so sum_a and
 * sum_a2 are good to that, but sum_g is a sum of differences: its relative
 * error is about 2 e sqrt(sum_a2 / sum_g), which grows without bound as the
 * interior becomes flat (1e-6 at sum_g / sum_a2 = 1e-2, 1e-5 at 1e-4).
 * With planes == NULL only the sums are produced (the autofocus sweep: nothing
 * leaves the device but 3 nz n_patch doubles).
 * The contract of fpm_predict: read-only (spectrum, pupil, maxima, stack,
 * gains, crops, fpm_timing and fpm_clock are left bit for bit; what
 * fpm_download returns afterwards is unchanged: the objCrop buffer serves as
 * the plane staging and is recomputed lazily, as after fpm_set_state),
 * blocking, deterministic: a plane's bytes and sums depend on the state and on
 * that plane's zl alone, not on its neighbours in the list or on nz.
 * FPM_ERR_STATE before a state exists (a context that only had fpm_set_state is
 * legal); FPM_ERR_INVAL on a capturing stream before anything is enqueued, and,
 * naming the argument, on a NULL zl, nz < 1, a zl that is not finite or with
 * |zl| > 1e6 (naming its index; beyond that the double reduction no longer
 * gives an fp32-exact phase), fl not finite or <= 0, margin < 0 or
 * 2 margin > L - 2, an unknown flag bit, every output NULL.
 * With a device `planes` the transform stores straight into the caller's
 * memory; with a host pointer each plane is copied out after its kernels.
 * elapsed_ms (may be NULL): event to event over the kernels; the host copies
 * are outside it.  The first call allocates the scratch ([n_patch][L][L] fp32
 * complex for objF H, the partial and folded sums; counted in
 * fpm_info.device_bytes from then on). */
#define FPM_REFOCUS_DEVICE      1u  /* planes is device memory on the context's device */
#define FPM_REFOCUS_Z_PER_PATCH 2u  /* zl is [nz][n_patch] instead of [nz] */
int  fpm_refocus(fpm_ctx *ctx, const double *zl, int nz, double fl, int margin, uint32_t flags,
                 float *planes, double *sum_a, double *sum_a2, double *sum_g, double *elapsed_ms);

/* Wait for all work on the context stream. */
int  fpm_synchronize(fpm_ctx *ctx);

/* Copy results to host (any pointer may be NULL):
 *   objF    [n_patch][L][L][2]   un-centred spectrum, like dataset->objF
 *   objCrop [n_patch][L][L][2]   IDFT(objF)/L^2 (fpmMain.cpp:481)
 *   pupil   [n_patch][Np][Np][2] centred pupil (fpmMain.cpp:496)
 *   support [n_patch][Np][Np]    un-centred pupilSupport (real part, 0/1)  */
int  fpm_download(fpm_ctx *ctx, float *objF, float *objCrop, float *pupil,
                  float *support);

/* Device-to-device copy of objCrop [n_patch][L][L][2] into caller memory on
 * the context's device (for the multi-GPU gather). */
int  fpm_download_objcrop_device(fpm_ctx *ctx, float *dst_dev);

/* Install a solver state: warm start from a converged patch's pupil, resume
 * from a checkpoint, or evaluate a hypothetical state with fpm_residual.
 * Layouts are fpm_download's:
 *   objF  [n_patch][L][L][2]    un-centred spectrum
 *   pupil [n_patch][Np][Np][2]  centred pupil; FPM_STATE_PUPIL_SHARED: one
 *                               [Np][Np][2] array used for every patch
 * Host pointers, or with FPM_STATE_DEVICE both in device memory on the
 * context's device (read in place).
 * Call order.  Either pointer may be NULL = keep what the context has; not
 * both.  With both given the call is legal on any created context (no stack
 * uploaded, after a debug objCrop call, after a split-mode abort) and makes it
 * initialised: it replaces fpm_init.  With one NULL the context must be
 * initialised already, else FPM_ERR_STATE.  fpm_run, fpm_residual and their
 * kin return FPM_ERR_STATE while no stack is uploaded; a later stack upload
 * clears the state, as it always did.
 * Pupil.  Stored is pupil * S, S the support disk: values outside the disk are
 * ignored (the reference masks with pupilSupport, fpmMain.cpp:312,472).  Every
 * value inside the disk must be finite, and max|P S| of every patch > 0
 * (fpm_init's is 1; 0 would be 0/0 in the object update).
 * Spectrum.  Every value finite; every element outside the context's live
 * band (the rows and columns the support boxes of the init placement and of
 * the used LEDs cover in the centred spectrum) exactly zero, anything inside
 * it accepted; under FPM_FLAG_SPEC_FP16 |component| * hscale < 65504
 * (hscale = 2^-ceil(log2 Np^2)).
 * Any violation returns FPM_ERR_INVAL; the message names the array and the
 * first offender in linear order as (patch, y, x) of the caller's layout.
 * After a refused call the context is as it was: spectrum, pupil, maxima and
 * the initialised flag bit for bit (objCrop may be recomputed lazily).
 * Blocking; FPM_ERR_INVAL on a capturing stream before anything is enqueued.
 * Gains, crops, the stack, fpm_timing and fpm_clock are untouched; objCrop is
 * recomputed by the next fpm_download / fpm_run, as after fpm_init.  The
 * carried maxima are rebuilt exactly from the stored values (under fp16
 * storage: after its rounding), so a run resumed from a downloaded state
 * continues as the run it came from.  The first call allocates a few bytes of
 * check scratch (counted in fpm_info.device_bytes from then on). */
#define FPM_STATE_DEVICE        1u  /* objF / pupil point to device memory on the context's device */
#define FPM_STATE_PUPIL_SHARED  2u  /* pupil is one [Np][Np] array used for every patch */
int  fpm_set_state(fpm_ctx *ctx, const float *objF, const float *pupil, uint32_t flags);

/* The inverse: the un-centred fp32 spectrum [n_patch][L][L][2] (an fp16
 * spectrum dequantised as fpm_download does) and the centred pupil
 * [n_patch][Np][Np][2] into caller memory on the context's device.  Read-only
 * and blocking.  Either pointer may be NULL, not both.  FPM_ERR_STATE before a
 * state exists; FPM_ERR_INVAL on a capturing stream. */
int  fpm_download_state_device(fpm_ctx *ctx, float *objF_dev, float *pupil_dev);

/* Stitch a regular grid of overlapping tiles into one field: neighbours are
 * brought to a common phase (and scale) from the pixels they share, then
 * feathered together.  Every patch of a patch-wise reconstruction is its own
 * phase-retrieval problem, defined up to a complex constant, and carries FFT
 * wrap-around error along its border; side by side the tiles show seams.
 * Geometry.  Tiles T[t], t = i*gx + j, each tile x tile (= L) complex, tile
 * (i, j) at rows [i*stride_y, i*stride_y + L), columns [j*stride_x, ...).  The
 * field is H x W, H = (gy-1)*stride_y + L, W = (gx-1)*stride_x + L.  Strides
 * lie in [ceil(L/2), L], so a pixel is under at most two tiles per axis.
 * Weights.  w = wy(i, y) wx(j, x); along an axis with overlap V = L - stride
 * and local coordinate u: (u+1)/(V+1) for u < V when the tile has a lower
 * neighbour, (L-u)/(V+1) for u >= stride when it has an upper one, else 1.
 * The weights over a pixel sum to 1: nothing is divided.
 * Factors.  f[0] = 1; the others in raster order from the left and the upper
 * neighbour n.  Over the pixels a pair (n, t) shares, unweighted:
 *   c = sum T[n] conj(T[t]),  a = sum |T[n]|^2,  b = sum |T[t]|^2
 *   z = sum_n f[n] c,  num = sum_n |f[n]|^2 a,  den = sum_n b
 *   FPM_STITCH_ALIGN_PHASE    f[t] = z / |z|
 *   FPM_STITCH_ALIGN_COMPLEX  f[t] = (z / |z|) sqrt(num / den)
 *   neither flag              every f = 1, the sums are not computed
 *   z == 0 or den == 0        f[t] = 1
 * The sums are accumulated in double on the GPU in a fixed order (no
 * floating-point atomics), the solve runs in double on the host.
 * Field.  out(y, x) = sum_t w_t f32(f[t]) T[t] over the covering tiles in
 * ascending t, in fp32.  A pixel under one tile whose factor is exactly 1 is a
 * copy of that tile's bits, so strides of L without alignment are pure
 * placement.  Two calls return the same bits.
 *   tiles   [gy*gx][L][L][2]
 *   field   [H][W][2]; must not overlap tiles
 *   factors [gy*gx][2] double (re, im), host memory; may be NULL
 * Host pointers are staged through device scratch the call allocates and
 * frees; with FPM_STITCH_DEVICE tiles and field are device memory on `device`,
 * the tiles are read in place and nothing crosses PCIe but the pair sums and
 * the factors.  hip_stream: the hipStream_t the work is enqueued on (NULL = the
 * null stream).  Blocking.  The call makes `device` the calling thread's
 * current device (hipSetDevice) and leaves it so, as every call on a context
 * does for the context's device.  elapsed_ms (may be NULL): event-to-event time of
 * the kernels (pair sums + blend; not the copies or the solve).
 * FPM_ERR_INVAL, the message naming the field at fault: a NULL grid, tiles or
 * field; gy or gx < 1; tile < 2; a stride outside [ceil(L/2), L]; both align
 * flags, or an unknown flag; a capturing stream (before anything is enqueued);
 * a grid past what the launches index (tile > 32768, more than 16384 tiles or
 * 262140 field rows). */
typedef struct fpm_stitch_grid {
    int32_t gy, gx;        /* tiles per column / per row, tile t = i*gx + j          */
    int32_t tile;          /* L                                                       */
    int32_t stride_y, stride_x;   /* ceil(L/2) .. L                                   */
} fpm_stitch_grid;
#define FPM_STITCH_ALIGN_PHASE   1u
#define FPM_STITCH_ALIGN_COMPLEX 2u   /* phase and scale; excludes ALIGN_PHASE        */
#define FPM_STITCH_DEVICE        4u   /* tiles / field are device memory on `device`  */
int  fpm_stitch_tiles(int device, const float *tiles, const fpm_stitch_grid *g, uint32_t flags,
                      float *field, double *factors, void *hip_stream, double *elapsed_ms);

/* The same for the context's own objCrop tiles (refreshed first, as
 * fpm_download does), on the run stream: gy*gx == n_patch and tile == nlarge,
 * else FPM_ERR_INVAL.  FPM_STITCH_DEVICE then describes `field` only (device
 * memory on the context's device, clear of the context's own buffers: a
 * field that overlaps the objCrop tiles is FPM_ERR_INVAL).  Read-only on the context: spectrum, pupil,
 * maxima, fpm_timing and fpm_clock are untouched, and nothing it allocates
 * stays in fpm_info.device_bytes.  Blocking.  FPM_ERR_STATE before a state
 * exists; FPM_ERR_INVAL on a capturing stream, before anything is enqueued. */
int  fpm_stitch(fpm_ctx *ctx, const fpm_stitch_grid *g, uint32_t flags, float *field,
                double *factors, double *elapsed_ms);

/* Use a caller-provided hipStream_t (NULL = the context's own stream). */
int  fpm_set_stream(fpm_ctx *ctx, void *hip_stream);

/* fpm_get_info is frozen at the ABI-3 layout: it writes FPM_INFO_V3_SIZE
 * bytes (path .. fused_kernel) and never a later field, so a binary built
 * against the ABI-3 header, whose struct is that size, stays safe.  Fields
 * appended since (threads_per_wg, ABI 4) are read with fpm_get_info_sized,
 * which writes only the first info_size bytes: pass sizeof(fpm_info) of the
 * header the caller was built with (fields are only ever appended). */
int  fpm_get_info(const fpm_ctx *ctx, fpm_info *info);
int  fpm_get_info_sized(const fpm_ctx *ctx, fpm_info *info, size_t info_size);
int  fpm_get_timing(const fpm_ctx *ctx, fpm_timing *timing);

/* Clock of the LED-update launches of the most recent fpm_run (fused path;
 * ABI 5): block 0 of every launch reads the shader-cycle counter (s_memtime)
 * and the constant-rate real-time counter (s_memrealtime) at entry and after
 * its last LED, so clock_mhz = cycles / real time is the shader clock the
 * kernel actually ran at and cycles_per_launch its length in cycles, which a
 * slower clock does not change (MI355X_MICROARCH.md, DVFS).  launches = 0 on
 * the general path, which has no probe, and after an fpm_run that was refused
 * or failed (see fpm_timing). */
typedef struct fpm_clock {
    double clock_mhz;          /* mean shader clock over the probed launches   */
    double cycles_per_launch;  /* block 0's shader cycles per launch           */
    double ms_per_launch;      /* block 0's real time per launch               */
    int32_t launches;          /* launches probed                              */
} fpm_clock;
int  fpm_get_clock(const fpm_ctx *ctx, fpm_clock *clock);

/* One-shot equivalent of runFPM for n_patch patches: create, upload, init,
 * run, download, destroy.  Blocking. */
int  fpm_runFPM(const fpm_problem *prob, int device, const uint16_t *meas,
                int iters, float *objF, float *objCrop, float *pupil,
                float *support);

/* Description of the most recent error on the calling thread. */
const char *fpm_last_error(void);

/* Library build identification (also proves the .so loaded). */
const char *fpm_version(void);
/* FPM_ABI_VERSION the library was built with; a caller compiled against a
 * newer header than the library refuses to run. */
int fpm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FPM_HIP_H */
