// gradient_api.cpp -- fpm_gradient: the gradient of the data-fidelity cost with
// respect to the spectrum and the pupil (kernels: gradient.hip and the GradArgs
// tail of the sweep's column kernels, residual_dev.hpp).  The sweep's steps
// (residual_api.cpp): refuse what cannot run, resolve the list, make sure the
// scratch exists, clear the outputs, launch the batches in list order between
// two events, copy the folded sums and -- with host outputs -- the gradients
// out, report the event time.  Read-only on the context's state.
#include <algorithm>
#include <vector>

#include "ctx.hpp"

using namespace fpm;

namespace {

// fpm_gradient's additions to the sweep's scratch: R of one batch by the first
// call, the device copy of a host output by the first call that asks for it
int ensure_gradient_scratch(fpm_ctx *c, bool stage_obj, bool stage_pupil) {
    int rc = sweep_ensure_scratch(c);
    if (rc) return rc;
    const ResidualPlan &p = c->rplan;
    const DevState &st = c->st;
    // R is not cleared: the accumulate kernels read exactly the elements the rows-out kernels write, the
    // support disk ky^2 + kx^2 <= r^2 of every box -- st.disk in k_grad_rows / k_grad_acc_pupil, the same
    // inequality spelled out in k_grad_rows256 / k_grad_acc_obj (plan_context builds st.disk from it).  A
    // support mask of another shape must change all four together.
    if (!c->grad_R && (rc = dalloc(c, &c->grad_R, (size_t)p.nl * st.B * st.nb * st.nb, false))) return rc;
    if (!c->grad_ready) {
        HIP_TRY(allow_large_lds({&p.cols_grad, &p.grad_rows}, c->lds_limit));
        c->grad_ready = true;
    }
    if (stage_obj && !c->grad_obj && (rc = dalloc(c, &c->grad_obj, (size_t)st.B * st.L * st.L, false))) return rc;
    if (stage_pupil && !c->grad_pupil && (rc = dalloc(c, &c->grad_pupil, (size_t)st.B * st.np * st.np, false)))
        return rc;
    return FPM_OK;
}

int gradient(fpm_ctx *c, const fpm_probe *probes, int n, bool dev, float *grad_objF, float *grad_pupil, double *err,
             double *ref, double *elapsed_ms) {
    const DevState &st = c->st;
    const int n_order = c->prob.n_order, np = st.np, r = st.r;
    std::vector<ResEntry> ent;
    int rc;
    if (probes) {
        if ((rc = sweep_resolve_probes(c, "fpm_gradient", probes, n, ent))) return rc;
    } else {  // the context's own list, as ident_dev holds it
        n = n_order;
        ent.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const int led = c->order[i];
            ent[i] = ResEntry{led, c->x0[led] + np / 2, c->y0[led] + np / 2, 0};
        }
    }
    if ((rc = ensure_gradient_scratch(c, !dev && grad_objF, !dev && grad_pupil))) return rc;
    const ResidualPlan &p = c->rplan;
    const size_t B = st.B, no = B * st.L * st.L, npu = B * (size_t)np * np;
    float2 *gO = !grad_objF ? nullptr : dev ? reinterpret_cast<float2 *>(grad_objF) : c->grad_obj;
    float2 *gP = !grad_pupil ? nullptr : dev ? reinterpret_cast<float2 *>(grad_pupil) : c->grad_pupil;
    HIP_TRY(hipEventRecord(c->res_ev[0], c->stream));
    // every element is written: +0 wherever no entry's disk (the support) reaches
    if (gO) HIP_TRY(hipMemsetAsync(gO, 0, no * sizeof(float2), c->stream));
    if (gP) HIP_TRY(hipMemsetAsync(gP, 0, npu * sizeof(float2), c->stream));
    // pieces of n_order entries (the entry table and the folded sums), each nl
    // entries per launch, as the sweep's; everything is ordered on the run stream
    for (int k0 = 0; k0 < n; k0 += n_order) {
        const int m = std::min(n_order, n - k0);
        const ResEntry *e = c->ident_dev;
        if (probes) {  // (ent is pageable: the copy has left it when hipMemcpyAsync returns)
            HIP_TRY(hipMemcpyAsync(c->res_ent, ent.data() + k0, (size_t)m * sizeof(ResEntry), hipMemcpyHostToDevice,
                                   c->stream));
            e = c->res_ent;
        }
        MomArgs ra{{e, 0, c->res_T, c->res_perr, c->res_pref, c->res_err, c->res_ref, p.nblk}, nullptr, nullptr};
        for (int i0 = 0; i0 < m; i0 += p.nl) {
            const int nl = std::min(p.nl, m - i0);
            ra.i0 = i0;
            // the batch's bounding box: the support boxes of its windows
            int x0 = st.L, y0 = st.L, x1 = -1, y1 = -1;
            for (int z = 0; z < nl; ++z) {
                const ResEntry &q = ent[(size_t)k0 + i0 + z];
                x0 = std::min(x0, q.xc - r), x1 = std::max(x1, q.xc + r);
                y0 = std::min(y0, q.yc - r), y1 = std::max(y1, q.yc + r);
            }
            x0 = std::max(x0, 0), y0 = std::max(y0, 0);
            x1 = std::min(x1, st.L - 1), y1 = std::min(y1, st.L - 1);
            const GradAcc acc{nullptr, 0, 0, c->grad_R, gO, gP, x0, y0, x1 - x0 + 1, y1 - y0 + 1};
            HIP_TRY(launch_gradient_batch(p, st, ra, acc, nl, c->tw_np, c->stream));
        }
        const size_t bytes = (size_t)m * B * sizeof(double);
        if (err) HIP_TRY(hipMemcpyAsync(err + k0 * B, c->res_err, bytes, hipMemcpyDeviceToHost, c->stream));
        if (ref) HIP_TRY(hipMemcpyAsync(ref + k0 * B, c->res_ref, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(c->res_ev[1], c->stream));
    if (!dev) {
        if (gO) HIP_TRY(hipMemcpyAsync(grad_objF, gO, no * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        if (gP) HIP_TRY(hipMemcpyAsync(grad_pupil, gP, npu * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (elapsed_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->res_ev[0], c->res_ev[1]));
        *elapsed_ms = ms;
    }
    return FPM_OK;
}

}  // namespace

extern "C" int fpm_gradient(fpm_ctx *c, const fpm_probe *probes, int n, uint32_t flags, float *grad_objF,
                            float *grad_pupil, double *err, double *ref, double *elapsed_ms) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (flags & ~FPM_GRAD_DEVICE)
        return set_err(FPM_ERR_INVAL, "fpm_gradient: unknown flag bits 0x%x", flags & ~FPM_GRAD_DEVICE);
    if (!grad_objF && !grad_pupil)
        return set_err(FPM_ERR_INVAL, "fpm_gradient: grad_objF and grad_pupil are both NULL");
    const int rc = sweep_admit(c, "fpm_gradient");
    return rc ? rc : gradient(c, probes, n, (flags & FPM_GRAD_DEVICE) != 0, grad_objF, grad_pupil, err, ref, elapsed_ms);
}
