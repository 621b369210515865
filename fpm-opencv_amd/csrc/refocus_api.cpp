// refocus_api.cpp -- fpm_refocus: the recovered field at other z planes and the
// sums a focus measure is made of (kernels: refocus.hip), as a sequence of
// steps: check the arguments, refuse a capturing stream, make sure the scratch
// exists, and for every plane multiply the spectrum by H into the scratch,
// launch the context's own objCrop on a view whose spectrum is the scratch, and
// reduce the plane.  No objCrop kernel, plan or launch differs from
// fpm_download's; a plane at z = 0 skips the multiply and transforms the stored
// spectrum itself.
// The plane list runs in pieces of kRefocusPiece planes, what the device copy of
// zl and the folded sums hold.  A device `planes` (or none) takes one event
// pair around a piece's kernels; a host `planes` takes every plane from the
// objCrop buffer before the next one overwrites it, so every plane has its own
// pair and the copies lie between the pairs: elapsed_ms is the kernels' in both.
// Read-only: the objCrop buffer, when it served as the staging, is marked stale
// and recomputed by the next fpm_download, as after fpm_set_state (unless the
// plane it holds last is one at z = 0, which is objCrop).
// (The kernels' file is refocus.hip; the two cannot share a basename, Makefile.)
#include <algorithm>
#include <cmath>

#include "ctx.hpp"

using namespace fpm;

namespace {

constexpr int kPiece = fpm_ctx::kRefocusPiece;

// allocated by the first call, counted in fpm_info.device_bytes, released by the destructor
int ensure_scratch(fpm_ctx *c) {
    if (c->rf_ready) return FPM_OK;
    const size_t B = c->st.B, ll = (size_t)c->st.L * c->st.L;
    int rc = FPM_OK;
    // each buffer and event once: a call that failed half way leaves what it
    // got to the next call and to the destructor
    auto get = [&](auto **q, size_t n) {
        if (rc == FPM_OK && !*q) rc = dalloc(c, q, n, false);
    };
    get(&c->rf_zl, kPiece * B);
    get(&c->rf_part, B * refocus_sum_blocks(c->st.L, 0) * 3);
    get(&c->rf_sums, 3 * kPiece * B);
    get(&c->rf_spec, B * ll);
    if (rc) return rc;
    for (auto &e : c->rf_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // the multiply writes the live band only; the rest stays zero for good
    HIP_TRY(hipMemsetAsync(c->rf_spec, 0, B * ll * sizeof(float2), c->stream));
    c->rf_ready = true;
    return FPM_OK;
}

// waits for the stream; adds the time between the two events to *ms
int lap(fpm_ctx *c, double *ms) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, c->rf_ev[0], c->rf_ev[1]));
    *ms += t;
    return FPM_OK;
}

int refocus(fpm_ctx *c, const double *zl, int nz, bool per_patch, double fl, int margin, bool dev, float2 *planes,
            double *sum_a, double *sum_a2, double *sum_g, double *elapsed_ms) {
    int rc = ensure_scratch(c);
    if (rc) return rc;
    const DevState &st = c->st;
    const size_t B = st.B, img = B * st.L * st.L, zc = per_patch ? B : 1;
    const bool sums = sum_a || sum_a2 || sum_g, host = planes && !dev;
    // where a piece's folded sums land: [3][kPiece][B]
    double *const fa = sum_a ? c->rf_sums : nullptr, *const fa2 = sum_a2 ? c->rf_sums + kPiece * B : nullptr,
                 *const fg = sum_g ? c->rf_sums + 2 * kPiece * B : nullptr;
    double ms = 0.0;
    for (int k0 = 0; k0 < nz; k0 += kPiece) {
        const int m = std::min(kPiece, nz - k0);
        // (zl is pageable: the copy has left it when hipMemcpyAsync returns)
        HIP_TRY(hipMemcpyAsync(c->rf_zl, zl + k0 * zc, m * zc * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (!host) HIP_TRY(hipEventRecord(c->rf_ev[0], c->stream));
        for (int i = 0; i < m; ++i) {
            const double *z = zl + (k0 + i) * zc;
            const bool at_zero = std::all_of(z, z + zc, [](double v) { return v == 0.0; });
            if (host) HIP_TRY(hipEventRecord(c->rf_ev[0], c->stream));
            DevState view = st;
            if (!at_zero) {
                HIP_TRY(launch_refocus_mul(st, c->rf_zl + i * zc, per_patch ? 1 : 0, fl, c->rf_spec, c->stream));
                view.spec = c->rf_spec;  // fp32 on every context
                view.spec16 = nullptr;
            }
            float2 *out = dev ? planes + (k0 + i) * img : c->objcrop;
            if (!dev) c->objcrop_valid = false;
            HIP_TRY(launch_objcrop(c->oplan, view, out, c->tw_L, c->stream));
            if (!dev) c->objcrop_valid = at_zero;  // the staging holds this plane; at z = 0 that is objCrop itself
            if (sums)
                HIP_TRY(launch_refocus_sums(out, st.B, st.L, margin, c->rf_part, fa ? fa + i * B : nullptr,
                                            fa2 ? fa2 + i * B : nullptr, fg ? fg + i * B : nullptr, c->stream));
            if (host) {
                HIP_TRY(hipEventRecord(c->rf_ev[1], c->stream));
                HIP_TRY(hipMemcpyAsync(planes + (k0 + i) * img, out, img * sizeof(float2), hipMemcpyDeviceToHost,
                                       c->stream));
                if ((rc = lap(c, &ms))) return rc;
            }
        }
        if (!host) HIP_TRY(hipEventRecord(c->rf_ev[1], c->stream));
        const size_t bytes = m * B * sizeof(double);
        if (sum_a) HIP_TRY(hipMemcpyAsync(sum_a + k0 * B, fa, bytes, hipMemcpyDeviceToHost, c->stream));
        if (sum_a2) HIP_TRY(hipMemcpyAsync(sum_a2 + k0 * B, fa2, bytes, hipMemcpyDeviceToHost, c->stream));
        if (sum_g) HIP_TRY(hipMemcpyAsync(sum_g + k0 * B, fg, bytes, hipMemcpyDeviceToHost, c->stream));
        if (!host) {
            if ((rc = lap(c, &ms))) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    if (elapsed_ms) *elapsed_ms = ms;
    return FPM_OK;
}

}  // namespace

extern "C" int fpm_refocus(fpm_ctx *c, const double *zl, int nz, double fl, int margin, uint32_t flags, float *planes,
                           double *sum_a, double *sum_a2, double *sum_g, double *elapsed_ms) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    const uint32_t known = FPM_REFOCUS_DEVICE | FPM_REFOCUS_Z_PER_PATCH;
    if (flags & ~known) return set_err(FPM_ERR_INVAL, "fpm_refocus: unknown flag bits 0x%x", flags & ~known);
    if (!zl) return set_err(FPM_ERR_INVAL, "fpm_refocus: zl is NULL");
    if (nz < 1) return set_err(FPM_ERR_INVAL, "fpm_refocus: nz=%d < 1", nz);
    if (!std::isfinite(fl) || !(fl > 0.0))
        return set_err(FPM_ERR_INVAL, "fpm_refocus: fl=%g must be finite and > 0", fl);
    const int L = c->st.L;
    if (margin < 0 || 2 * (long long)margin > L - 2)
        return set_err(FPM_ERR_INVAL, "fpm_refocus: margin=%d outside [0, %d] (2 margin <= L - 2, L = %d)", margin,
                       (L - 2) / 2, L);
    if (!planes && !sum_a && !sum_a2 && !sum_g)
        return set_err(FPM_ERR_INVAL, "fpm_refocus: every output pointer is NULL (planes, sum_a, sum_a2, sum_g)");
    const bool per_patch = flags & FPM_REFOCUS_Z_PER_PATCH;
    const size_t zc = per_patch ? c->st.B : 1;
    for (size_t i = 0; i < (size_t)nz * zc; ++i)
        if (!std::isfinite(zl[i]) || std::fabs(zl[i]) > 1e6)
            return set_err(FPM_ERR_INVAL, "fpm_refocus: zl[%zu]=%g must be finite with |zl| <= 1e6", i, zl[i]);
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_refocus before a state exists (fpm_init or fpm_set_state)");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = refuse_capture(c, "fpm_refocus")) return rc;
    // without planes the flag describes nothing: the sums pass reads the staging
    const bool dev = planes && (flags & FPM_REFOCUS_DEVICE);
    return refocus(c, zl, nz, per_patch, fl, margin, dev, (float2 *)planes, sum_a, sum_a2, sum_g, elapsed_ms);
}
