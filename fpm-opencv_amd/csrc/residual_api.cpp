// residual_api.cpp -- fpm_residual, fpm_residual_at, fpm_moments and
// fpm_predict: the data-fidelity residual of the current state, the raw
// moments it is made of, or the predicted images themselves (residual.hip),
// as a sequence of steps: refuse
// a capturing stream, make sure the scratch exists, launch the batches of an
// entry list between two events, copy the folded sums out, report the event
// time.  One path: fpm_residual sweeps the context's identity list (every
// position of order[] with its own window), fpm_residual_at a list the caller
// gives as (position, offset) probes, resolved and validated on the host and
// run in pieces of at most n_order entries, the size of the folded-sum scratch.
// fpm_moments is the same path with the column kernels' moments tail and one
// more pair of sum buffers; it takes either list.
// Read-only: nothing of the state, the stack or the last run's timing and
// clock is written.
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
    get(&c->res_ent, (size_t)c->prob.n_order);
    get(&c->res_T, (size_t)p.nl * p.t_led);
    if (rc) return rc;
    for (auto &e : c->res_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(allow_large_lds({&p.rows, &p.cols, &p.cols_gain}, c->lds_limit));  // Np 1024 and up, tiled columns
    c->res_ready = true;
    return FPM_OK;
}

// fpm_moments' additions to it, by its first call
int ensure_moments_scratch(fpm_ctx *c) {
    int rc = ensure_scratch(c);
    if (rc || c->mom_ready) return rc;
    const ResidualPlan &p = c->rplan;
    if (!c->res_pcross) rc = dalloc(c, &c->res_pcross, (size_t)p.nl * c->st.B * p.nblk, false);
    if (!rc && !c->res_cross) rc = dalloc(c, &c->res_cross, (size_t)c->prob.n_order * c->st.B, false);
    if (rc) return rc;
    HIP_TRY(allow_large_lds({&p.cols_mom}, c->lds_limit));
    c->mom_ready = true;
    return FPM_OK;
}

// the entries ent[0, n) (device, n <= n_order) in list order, nl per launch;
// mom: the moments (Q in the err buffers, C in the cross ones)
int launch_entries(fpm_ctx *c, const ResEntry *ent, int n, bool mom) {
    const ResidualPlan &p = c->rplan;
    MomArgs ra{{ent, 0, c->res_T, c->res_perr, c->res_pref, c->res_err, c->res_ref, p.nblk},
               mom ? c->res_pcross : nullptr, mom ? c->res_cross : nullptr};
    // a context whose gains are all ones launches the residual's ungained instance
    const ResTail tail = mom ? ResTail::Moments : c->gains_unit ? ResTail::Plain : ResTail::Gain;
    for (int i0 = 0; i0 < n; i0 += p.nl) {
        ra.i0 = i0;
        HIP_TRY(launch_residual_batch(p, c->st, ra, tail, std::min(p.nl, n - i0), c->tw_np, c->stream));
    }
    return FPM_OK;
}

// their folded sums [n][B] to err / ref / cross (any may be null)
int copy_sums(fpm_ctx *c, int n, double *err, double *ref, double *cross = nullptr) {
    const size_t bytes = (size_t)n * c->st.B * sizeof(double);
    if (err) HIP_TRY(hipMemcpyAsync(err, c->res_err, bytes, hipMemcpyDeviceToHost, c->stream));
    if (ref) HIP_TRY(hipMemcpyAsync(ref, c->res_ref, bytes, hipMemcpyDeviceToHost, c->stream));
    if (cross) HIP_TRY(hipMemcpyAsync(cross, c->res_cross, bytes, hipMemcpyDeviceToHost, c->stream));
    return FPM_OK;
}

// what every entry point checks before anything is enqueued; need_stack: the
// call compares with the images (everything but fpm_predict's AMPLITUDE and COUNTS)
int admit(fpm_ctx *c, const char *what, bool any_output, bool need_stack = true) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!any_output) return set_err(FPM_ERR_INVAL, "%s: every output pointer is NULL", what);
    if (!c->initialized) return set_err(FPM_ERR_STATE, "%s before fpm_init", what);
    // a state set by fpm_set_state on a context without a stack has no images to compare with
    if (need_stack && !c->uploaded) return set_err(FPM_ERR_STATE, "%s: no stack uploaded", what);
    HIP_TRY(hipSetDevice(c->device));
    return refuse_capture(c, what);
}

int finish(fpm_ctx *c, double *elapsed_ms) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (elapsed_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->res_ev[0], c->res_ev[1]));
        *elapsed_ms = ms;
    }
    return FPM_OK;
}

// the context's identity list: every position of order[] with its own window
int sweep_identity(fpm_ctx *c, bool mom, double *err, double *ref, double *cross, double *elapsed_ms) {
    int rc = mom ? ensure_moments_scratch(c) : ensure_scratch(c);
    if (rc) return rc;
    const int n = c->prob.n_order;
    HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
    if ((rc = launch_entries(c, c->ident_dev, n, mom))) return rc;
    HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
    if ((rc = copy_sums(c, n, err, ref, cross))) return rc;
    return finish(c, elapsed_ms);
}

// a probe list as entries: every one resolved and validated before the first launch
int resolve_probes(const fpm_ctx *c, const char *what, const fpm_probe *probes, int n, std::vector<ResEntry> &ent) {
    if (!probes || n < 1) return set_err(FPM_ERR_INVAL, "%s: %s", what, probes ? "n < 1" : "null probes");
    const int np = c->st.np, L = c->st.L, n_order = c->prob.n_order;
    ent.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        const fpm_probe &q = probes[k];
        if (q.pos < 0 || q.pos >= n_order)
            return set_err(FPM_ERR_INVAL, "%s: entry %d: pos=%d outside order[0, %d)", what, k, q.pos, n_order);
        const int led = c->order[q.pos];
        const long long x = (long long)c->x0[led] + q.dx, y = (long long)c->y0[led] + q.dy;
        if (x < 0 || x > L - np || y < 0 || y > L - np)
            return set_err(FPM_ERR_INVAL, "%s: entry %d: window (%lld,%lld) of LED %d leaves the %dx%d "
                           "spectrum", what, k, x, y, led, L, L);
        ent[k] = ResEntry{led, (int)x + np / 2, (int)y + np / 2, 0};
    }
    return FPM_OK;
}

// a probe list, after admit
int sweep_probes(fpm_ctx *c, const char *what, bool mom, const fpm_probe *probes, int n, double *err, double *ref,
                 double *cross, double *elapsed_ms) {
    std::vector<ResEntry> ent;
    int rc = resolve_probes(c, what, probes, n, ent);
    if (rc) return rc;
    const int n_order = c->prob.n_order;
    if ((rc = mom ? ensure_moments_scratch(c) : ensure_scratch(c))) return rc;
    const size_t B = c->st.B;
    HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
    // pieces of n_order entries, what the entry table and the folded sums
    // hold; everything is ordered on the run stream (ent is pageable: the copy
    // has left it when hipMemcpyAsync returns), so a piece's table and sums
    // are free again when the next one overwrites them
    for (int k0 = 0; k0 < n; k0 += n_order) {
        const int m = std::min(n_order, n - k0);
        HIP_TRY(hipMemcpyAsync(c->res_ent, ent.data() + k0, (size_t)m * sizeof(ResEntry), hipMemcpyHostToDevice,
                               c->stream));
        if ((rc = launch_entries(c, c->res_ent, m, mom)) ||
            (rc = copy_sums(c, m, err ? err + k0 * B : nullptr, ref ? ref + k0 * B : nullptr,
                            cross ? cross + k0 * B : nullptr)))
            return rc;
    }
    HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
    return finish(c, elapsed_ms);
}

// fpm_predict's additions to the sweep's scratch: the staging buffer of one
// launch's images, by the first call with a host output
int ensure_predict_scratch(fpm_ctx *c, bool stage) {
    int rc = ensure_scratch(c);
    if (rc) return rc;
    const ResidualPlan &p = c->rplan;
    if (!c->pred_ready) {
        HIP_TRY(allow_large_lds({&p.cols_pred}, c->lds_limit));
        c->pred_ready = true;
    }
    if (stage && !c->pred_stage)
        rc = dalloc(c, &c->pred_stage, (size_t)p.nl * c->st.B * c->st.np * c->st.np, false);
    return rc;
}

// the images of a list (probes null: the identity list), after admit.  The list
// runs in pieces of n_order entries (the entry table) and each piece nl
// entries per launch, as the sweep's.  A device out takes the kernels' stores
// as they are, one event pair around all launches; a host out takes each
// launch's batch from the staging buffer before the next launch overwrites it,
// so every launch has its own event pair and the copies lie between the pairs:
// elapsed_ms is the kernels' time in both.
int predict(fpm_ctx *c, const fpm_probe *probes, int n, unsigned kind, bool dev, void *out, double *elapsed_ms) {
    std::vector<ResEntry> ent;
    int rc;
    const int n_order = c->prob.n_order;
    if (!probes) n = n_order;
    else if ((rc = resolve_probes(c, "fpm_predict", probes, n, ent))) return rc;
    if ((rc = ensure_predict_scratch(c, !dev))) return rc;
    const ResidualPlan &p = c->rplan;
    const size_t img = (size_t)c->st.B * c->st.np * c->st.np, esz = kind == FPM_PREDICT_COUNTS ? 2 : 4;
    char *const o = static_cast<char *>(out);
    double ms_sum = 0.0;
    if (dev) HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
    for (int k0 = 0; k0 < n; k0 += n_order) {
        const int m = std::min(n_order, n - k0);
        const ResEntry *e = c->ident_dev;
        if (probes) {  // (ent is pageable: the copy has left it when hipMemcpyAsync returns)
            HIP_TRY(hipMemcpyAsync(c->res_ent, ent.data() + k0, (size_t)m * sizeof(ResEntry), hipMemcpyHostToDevice,
                                   c->stream));
            e = c->res_ent;
        }
        for (int i0 = 0; i0 < m; i0 += p.nl) {
            const int nl = std::min(p.nl, m - i0);
            PredArgs pa{};
            pa.ent = e;
            pa.i0 = i0;
            pa.T = c->res_T;
            pa.kind = kind;
            pa.out = dev ? static_cast<void *>(o + (size_t)k0 * img * esz) : static_cast<void *>(c->pred_stage);
            pa.o0 = dev ? 0 : i0;
            if (!dev) HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
            HIP_TRY(launch_predict_batch(p, c->st, pa, nl, c->tw_np, c->stream));
            if (!dev) {
                HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
                HIP_TRY(hipMemcpyAsync(o + (size_t)(k0 + i0) * img * esz, c->pred_stage, (size_t)nl * img * esz,
                                       hipMemcpyDeviceToHost, c->stream));
                double ms = 0.0;
                if ((rc = finish(c, &ms))) return rc;
                ms_sum += ms;
            }
        }
    }
    if (dev) {
        HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
        return finish(c, elapsed_ms);
    }
    if (elapsed_ms) *elapsed_ms = ms_sum;
    return FPM_OK;
}

}  // namespace

namespace fpm {
int sweep_admit(fpm_ctx *c, const char *what) { return admit(c, what, true); }
int sweep_resolve_probes(const fpm_ctx *c, const char *what, const fpm_probe *probes, int n,
                         std::vector<ResEntry> &ent) {
    return resolve_probes(c, what, probes, n, ent);
}
int sweep_ensure_scratch(fpm_ctx *c) { return ensure_scratch(c); }
}  // namespace fpm

extern "C" int fpm_predict(fpm_ctx *c, const fpm_probe *probes, int n, uint32_t flags, void *out,
                           double *elapsed_ms) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    const uint32_t known = FPM_PREDICT_COUNTS | FPM_PREDICT_DIFF | FPM_PREDICT_DEVICE;
    if (flags & ~known) return set_err(FPM_ERR_INVAL, "fpm_predict: unknown flag bits 0x%x", flags & ~known);
    const unsigned kind = flags & (FPM_PREDICT_COUNTS | FPM_PREDICT_DIFF);
    if (kind == (FPM_PREDICT_COUNTS | FPM_PREDICT_DIFF))
        return set_err(FPM_ERR_INVAL, "fpm_predict: flags 0x%x name more than one kind (COUNTS and DIFF)", flags);
    if (!out) return set_err(FPM_ERR_INVAL, "fpm_predict: out is NULL");
    const int rc = admit(c, "fpm_predict", true, kind == FPM_PREDICT_DIFF);
    return rc ? rc : predict(c, probes, n, kind, (flags & FPM_PREDICT_DEVICE) != 0, out, elapsed_ms);
}

extern "C" int fpm_residual(fpm_ctx *c, double *err, double *ref, double *elapsed_ms) {
    const int rc = admit(c, "fpm_residual", err || ref);
    return rc ? rc : sweep_identity(c, false, err, ref, nullptr, elapsed_ms);
}

extern "C" int fpm_residual_at(fpm_ctx *c, const fpm_probe *probes, int n, double *err, double *ref,
                               double *elapsed_ms) {
    const int rc = admit(c, "fpm_residual_at", err || ref);
    return rc ? rc : sweep_probes(c, "fpm_residual_at", false, probes, n, err, ref, nullptr, elapsed_ms);
}

extern "C" int fpm_moments(fpm_ctx *c, const fpm_probe *probes, int n, double *model, double *cross, double *ref,
                           double *elapsed_ms) {
    const int rc = admit(c, "fpm_moments", model || cross || ref);
    if (rc) return rc;
    return probes ? sweep_probes(c, "fpm_moments", true, probes, n, model, ref, cross, elapsed_ms)
                  : sweep_identity(c, true, model, ref, cross, elapsed_ms);
}
