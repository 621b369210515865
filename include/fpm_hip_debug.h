/* fpm_hip_debug.h -- test-only entry points of libfpm_hip.so (not part of the
 * drop-in boundary include/fpm_hip.h): device helpers exposed so the tests can
 * pin them on extreme inputs no valid stack reaches, a fault injector for
 * the multi-workgroup handoffs, and read-backs of what a context planned and
 * of the maxima it carries between LED steps. */
#ifndef FPM_HIP_DEBUG_H
#define FPM_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fpm_ctx fpm_ctx;

/* The object update and pupil numerator of n support pixels exactly as every
 * fused kernel evaluates them (update.hpp slot_update, fpmMain.cpp:405-471):
 * with D = f - o p,
 *   nv  = o + D conj(p) |p| / ((|p|^2 + delta2 + i d2_im) pm)
 *   num = D conj(o) |o| / ((|o|^2 + delta1 + i d1_im))
 *   oa  = |o|
 * f, o, p, nv, num are interleaved complex [n][2]; pm, oa are [n].  Runs on the
 * current HIP device; returns 0 or an FPM_ERR_* code. */
int fpm_debug_slot_update(const float *f, const float *o, const float *p, const float *pm, int n, float delta1,
                          float delta2, float d1_im, float d2_im, float *nv, float *num, float *oa);

/* The general path's update coefficient f / ((a + i c) m) (fpm_state.hpp
 * upd_coef_div, called by update.hpp general_update) for n host inputs; out[2k], out[2k+1]
 * = real, imaginary part. */
int fpm_debug_update_coef(const float *a, const float *c, const float *m, const float *f, float *out, int n);

/* Split / distributed mode fault injection: from LED position `led` of every
 * later fpm_run on, the last workgroup of each patch stops publishing its
 * handoffs, so its partners time out (~1 s) and fpm_run must report
 * FPM_ERR_DEVICE; -1 switches it off. */
int fpm_debug_set_stall(fpm_ctx *ctx, int led);

/* What plan_context decided and fpm_info does not report (any pointer may be
 * NULL): meas_g = the stack's layout on the device (0 C-ABI, g > 0 the column
 * layout with g-lane groups, Np transposed); general_kind = the general path's
 * step kernels (0 Np 1024 register, 1 Np 256 register, 2 LDS; -1 on a fused
 * context); residual_kind = fpm_residual's kernel pair (0 register, 1 LDS). */
int fpm_debug_get_plan(const fpm_ctx *ctx, int *meas_g, int *general_kind, int *residual_kind);

/* The live band of the centred spectrum the context planned (fpm_state.hpp),
 * inclusive: band[4] = sy0, sy1, sx0, sx1.  Outside it the spectrum is exactly
 * zero, and the state entry point of fpm_hip.h refuses a spectrum that is not;
 * the crop-table entry point can grow it. */
int fpm_debug_get_band(const fpm_ctx *ctx, int band[4]);

/* The max|objF| / max|P| bookkeeping a context carries from one LED step and
 * one launch to the next (fpm_state.hpp), read back after synchronising the
 * context's stream; needs fpm_init.  Read-only: the device state is not
 * touched.  Any pointer may be NULL.
 *   dims[4]             nty, ntx, npart, has_rmax (size the other arrays with a
 *                       first call that passes only dims)
 *   tmax  [B][nty][ntx] max|spec| of each 16 x 16 tile of the centred spectrum
 *   dirty [B][nty][ntx] 1: the tile's tmax is only an upper bound (fused
 *                       kernels; they keep the bits indexed by live-band tile,
 *                       converted here: a tile outside the band is clean, and
 *                       its tmax is the 0 fpm_init wrote)
 *   rmax  [B][nty]      maximum of each tile row (general path: has_rmax = 1;
 *                       FPM_ERR_INVAL when asked of a fused context)
 *   pmax  [B][npart]    partial maxima of |P| */
int fpm_debug_get_maxima(const fpm_ctx *ctx, int *dims, float *tmax, unsigned char *dirty, float *rmax, float *pmax);

/* The rung of the general path's LDS kernel ladder (general.hip: one sequence
 * per block, row / column tiles, wave-private columns) that a size runs, as
 * plan_lds_ladder and pick_lds_kernels decide it, for the row kernels (K1, and
 * K3 in the update step) and the column kernel (K2). */
#define FPM_LADDER_ONE_SEQ 0
#define FPM_LADDER_TILED 1
#define FPM_LADDER_WAVE 2
typedef struct fpm_ladder_kernel {
    int generation;  /* FPM_LADDER_* */
    int tile;        /* tiled: log2 of the rows (lr) / columns (lc) per block; wave: columns per wave (cw); else 0 */
    int threads;     /* per block */
    int e;           /* register elements per thread: tiled 16 / 24, wave 16, one sequence per block 0 */
    int grid_x, grid_y;
    int lds_dynamic; /* bytes the launch asks for */
    int lds_static;  /* bytes of the kernel's own __shared__ arrays (rows of the update step: the larger of K1's and K3's) */
} fpm_ladder_kernel;
typedef struct fpm_ladder {
    fpm_ladder_kernel rows, cols;
} fpm_ladder;

/* The rung for box size nb = 2r+1 and B patches at Np = np, of the update step
 * (step = 1) or of the residual sweep (step = 0); no_wave_cols and one_seq are
 * the switches FPM_NO_WAVE_COLS and FPM_ONE_SEQ (step) / FPM_RES_ONE_SEQ
 * (sweep).  Calls the planner itself and nothing of HIP: needs neither a
 * context nor a device.  FPM_ERR_INVAL when np is not 2^a 3^b 5^c. */
int fpm_debug_plan_ladder(int np, int nb, int B, int step, int no_wave_cols, int one_seq, fpm_ladder *out);

/* The same record of a live context on the general path's LDS kernels: what its
 * update step (residual = 0; patch group 0) or its residual sweep (residual = 1)
 * launches.  FPM_ERR_INVAL on a fused context and on one whose step runs the
 * register kernels (Np 1024, Np 256).  Also compares each launched kernel's
 * static LDS constant with what its compiled code declares: FPM_ERR_STATE if
 * they differ. */
int fpm_debug_get_ladder(const fpm_ctx *ctx, int residual, fpm_ladder *out);

/* What plan_objcrop (objcrop.hip) decides for a spectrum size: the transform
 * objCrop runs and the launches of its row and column passes. */
#define FPM_OBJCROP_REGS_256M 0   /* register transforms of L = 512 / 768 / 1024 (crop256m.hip) */
#define FPM_OBJCROP_REGS_600 1    /* of L 600 (crop600.hip) */
#define FPM_OBJCROP_REGS_360 2    /* of L 360 (crop360.hip) */
#define FPM_OBJCROP_SIX_STEP_4K 3 /* the six-step passes of L 4096 (crop4k.hip) */
#define FPM_OBJCROP_BATCHED 4     /* k_fft_batch (fft_batch.hip) */
typedef struct fpm_objcrop_plan {
    int kind;             /* FPM_OBJCROP_* */
    int per_block;        /* what a block of the first pass holds: rows of the live band (register kinds),
                             sequences C (batched), columns (six-step: its column passes run first) */
    int rows_lds_dynamic; /* bytes the row launch asks for */
    int rows_lds_static;  /* bytes of the row kernel's own __shared__ arrays */
    int cols_lds_dynamic; /* the same of the column launch (six-step: of its first column pass) */
    int cols_lds_static;
} fpm_objcrop_plan;

/* The plan for Nlarge = nlarge, with fp16 spectrum storage (fp16 != 0:
 * FPM_FLAG_SPEC_FP16) and the switch FPM_NO_CROP4K (no_crop4k != 0).  Calls
 * the planner itself and nothing of HIP: needs neither a context nor a device,
 * and does not compare the LDS with any device's limit.  FPM_ERR_INVAL when
 * nlarge is odd, below 4, not 2^a 3^b 5^c or beyond the batched transform. */
int fpm_debug_plan_objcrop(int nlarge, int fp16, int no_crop4k, fpm_objcrop_plan *out);

/* The same record of a live context: what its fpm_run and fpm_debug_objcrop launch. */
int fpm_debug_get_objcrop_plan(const fpm_ctx *ctx, fpm_objcrop_plan *out);

/* objCrop of a given spectrum and live band, through the product's own
 * launch_objcrop with the context's plan (objcrop.hip and the kernel files it
 * names): no kernel and no dispatch of its own.  Legal on any created context; needs neither a stack nor fpm_init.
 *   spec    [B][L][L][2]  the CENTRED spectrum, copied verbatim into the
 *                         context's spectrum buffer (FPM_FLAG_SPEC_FP16: stored
 *                         as half(v * hscale), as every kernel stores it)
 *   band    sy0, sy1, sx0, sx1, inclusive: the live band the kernels are told
 *           (0 <= lo <= hi < L); what spec holds outside it must not matter
 *   objcrop [B][L][L][2]  the result.  The context's objCrop buffer is filled
 *                         with 0xFF bytes (NaN) before the launch, so an element
 *                         no pass writes, or an intermediate row read although
 *                         no pass wrote it, shows in the result.
 * Blocking.  FPM_ERR_INVAL on a null argument, a band outside the spectrum and
 * a capturing stream.  The context's planned band is kept, its state is not:
 * fpm_run and fpm_download return FPM_ERR_STATE until fpm_init is called. */
int fpm_debug_objcrop(fpm_ctx *ctx, const float *spec, const int band[4], float *objcrop);

#ifdef __cplusplus
}
#endif
#endif
