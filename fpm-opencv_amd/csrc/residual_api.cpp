// residual_api.cpp -- fpm_residual: the data-fidelity residual of the current
// state (residual.hip) as a sequence of steps: refuse a capturing stream,
// make sure the scratch exists, launch the LED batches between two events,
// copy the folded sums out, report the event time.  Read-only: nothing of the
// state, the stack or the last run's timing and clock is written.
// (The kernels' file is residual.hip; the two cannot share a basename, Makefile.)
#include <algorithm>
#include <vector>

#include "ctx.hpp"

using namespace fpm;

namespace {

// allocated by the first call, counted in fpm_info.device_bytes, released by the destructor
int ensure_scratch(fpm_ctx *c) {
    if (c->res_ready) return FPM_OK;
    const ResidualPlan &p = c->rplan;
    const size_t part = (size_t)p.nl * c->st.B * p.nblk, out = (size_t)c->prob.n_order * c->st.B;
    // each buffer and event once: a call that failed half way (out of memory)
    // leaves what it got to the next call and to the destructor
    int rc = FPM_OK;
    auto get = [&](auto **q, size_t n) {
        if (rc == FPM_OK && !*q) rc = dalloc(c, q, n, false);
    };
    get(&c->res_perr, part);
    get(&c->res_pref, part);
    get(&c->res_err, out);
    get(&c->res_ref, out);
    get(&c->res_T, (size_t)p.nl * p.t_led);
    if (rc) return rc;
    for (auto &e : c->res_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(allow_large_lds({&p.rows, &p.cols}, c->lds_limit));  // Np 1024 and up, tiled columns
    c->res_ready = true;
    return FPM_OK;
}

}  // namespace

extern "C" int fpm_residual(fpm_ctx *c, double *err, double *ref, double *elapsed_ms) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!err && !ref) return set_err(FPM_ERR_INVAL, "fpm_residual: err and ref are both NULL");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_residual before fpm_init");
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_residual");
    if (rc || (rc = ensure_scratch(c))) return rc;
    const ResidualPlan &p = c->rplan;
    const int n = c->prob.n_order;
    ResArgs ra{c->order_dev, c->x0_dev, c->y0_dev, 0, c->res_T, c->res_perr, c->res_pref, c->res_err, c->res_ref,
               p.nblk};
    HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
    for (int i0 = 0; i0 < n; i0 += p.nl) {
        ra.i0 = i0;
        HIP_TRY(launch_residual_batch(p, c->st, ra, std::min(p.nl, n - i0), c->tw_np, c->stream));
    }
    HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
    const size_t bytes = (size_t)n * c->st.B * sizeof(double);
    if (err) HIP_TRY(hipMemcpyAsync(err, c->res_err, bytes, hipMemcpyDeviceToHost, c->stream));
    if (ref) HIP_TRY(hipMemcpyAsync(ref, c->res_ref, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (elapsed_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->res_ev[0], c->res_ev[1]));
        *elapsed_ms = ms;
    }
    return FPM_OK;
}
