// launch.hpp -- every host function of the .hip files that api.cpp calls.
// Included by api.cpp and by each file that defines one of them, so a
// signature that drifts is a compile error and not a link-time surprise.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "fused_host.hpp"

namespace fpm {

// ---- general path (general.hip)
hipError_t launch_general_step(const DevState &st, int led, int x0, int y0, const FftPlan &pl,
                               const float2 *tw, bool first, hipStream_t s);
hipError_t launch_pupil_commit(const DevState &st, hipStream_t s);
int fft_max_len();
int pupil_parts(int nb);
hipError_t launch_init(const DevState &st, int init_led, float2 *scratch, const FftPlan &pl_np,
                       const float2 *tw_np, hipStream_t s);
hipError_t launch_objcrop(const DevState &st, float2 *out, const FftPlan &pl_L, const float2 *tw_L,
                          hipStream_t s);
// Np 1024 / Np 256 register row/column kernels of the general path
// (np1024.hip, np256.hip; both fold the pupil commit into the next LED)
bool np1024_supported(int np, int r);
bool np256_supported(int np, int r, int L, bool fp16);
bool commit_folded(const DevState &st);

// ---- Np 256 fused kernel: one workgroup per patch and split mode (fpm_fused.hip)
int fused_threads(int np, int r, int L, const DevState &st);
size_t fused_T_elems(int np, int r, int B);
size_t fused_xch_elems(int B, int ks);
size_t fused_flag_words(int B, int ks);
int fused_split_parts(int nt, int B, int n_cu);
hipError_t launch_fused_iteration(const DevState &st, const FusedLaunch &in, int ks, float2 *xch, int *flags,
                                  int stall_led, hipStream_t s);
// ---- distributed mode of the Np 256 kernel (fused_dist.hip)
size_t fused_dist_elems(int B, int ks);
int fused_dist_parts(int B, int n_cu, int r, int L);
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
