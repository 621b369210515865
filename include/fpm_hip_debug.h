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

#ifdef __cplusplus
}
#endif
#endif
