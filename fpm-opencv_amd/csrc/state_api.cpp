// state_api.cpp -- fpm_set_state and fpm_download_state_device: a solver state
// in from, and out to, the layouts of fpm_download (kernels: state.hip).
#include <cmath>

#include "ctx.hpp"

using namespace fpm;

namespace {

// the check pass's scratch, allocated by the first call (counted in device_bytes from then on)
int ensure_check_scratch(fpm_ctx *c) {
    if (c->state_chk) return FPM_OK;
    unsigned long long *p = nullptr;
    const int rc = dalloc(c, &p, (state_check_bytes(c->st.B) + 7) / 8, false);
    if (rc == FPM_OK) c->state_chk = reinterpret_cast<StateCheck *>(p);
    return rc;
}

// FPM_ERR_INVAL naming the spectrum's first offender, element i of src [B][L][L]
int refuse_spectrum(const fpm_ctx *c, const float2 *src, unsigned long long i) {
    const DevState &st = c->st;
    const int L = st.L;
    float2 v{};
    HIP_TRY(hipMemcpy(&v, src + i, sizeof v, hipMemcpyDeviceToHost));
    const int b = (int)(i / ((size_t)L * L)), y = (int)(i / L % L), x = (int)(i % L);
    if (!std::isfinite(v.x) || !std::isfinite(v.y))
        return set_err(FPM_ERR_INVAL, "fpm_set_state: objF is not finite at (patch %d, y %d, x %d)", b, y, x);
    const int cy = (y + L / 2) % L, cx = (x + L / 2) % L;
    if (cy < st.sy0 || cy > st.sy1 || cx < st.sx0 || cx > st.sx1)
        return set_err(FPM_ERR_INVAL,
                       "fpm_set_state: objF is nonzero at (patch %d, y %d, x %d), outside the live band of the "
                       "context (centred rows [%d, %d], columns [%d, %d]): create a context whose LEDs cover it",
                       b, y, x, st.sy0, st.sy1, st.sx0, st.sx1);
    return set_err(FPM_ERR_INVAL,
                   "fpm_set_state: objF at (patch %d, y %d, x %d) = (%g, %g) leaves the fp16 storage range "
                   "(|component| * %g must stay below 65504)", b, y, x, v.x, v.y, st.hscale);
}

}  // namespace

extern "C" {

int fpm_set_state(fpm_ctx *c, const float *objF, const float *pupil, uint32_t flags) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!objF && !pupil) return set_err(FPM_ERR_INVAL, "fpm_set_state: objF and pupil are both NULL");
    if (flags & ~(FPM_STATE_DEVICE | FPM_STATE_PUPIL_SHARED))
        return set_err(FPM_ERR_INVAL, "fpm_set_state: unknown flags 0x%x", flags);
    if ((!objF || !pupil) && !c->initialized)
        return set_err(FPM_ERR_STATE, "fpm_set_state with %s NULL before a state exists (fpm_init, or both arrays)",
                       objF ? "pupil" : "objF");
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_set_state");
    if (rc || (rc = ensure_check_scratch(c))) return rc;
    const DevState &st = c->st;
    const bool on_device = flags & FPM_STATE_DEVICE, shared = flags & FPM_STATE_PUPIL_SHARED;
    const size_t nspec = (size_t)st.B * st.L * st.L, npup = (size_t)(shared ? 1 : st.B) * st.np * st.np;

    // host arrays are staged on the device: the spectrum in the objCrop buffer
    // (same shape, fpm_init's scratch too), the pupil in a buffer of this call
    const float2 *src_f = (const float2 *)objF, *src_p = (const float2 *)pupil;
    struct Stage {
        void *p = nullptr;
        ~Stage() { (void)hipFree(p); }
    } stage;
    if (objF && !on_device) {
        c->objcrop_valid = false;
        HIP_TRY(hipMemcpyAsync(c->objcrop, objF, nspec * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        src_f = c->objcrop;
    }
    if (pupil && !on_device) {
        if (hipMalloc(&stage.p, npup * sizeof(float2)) != hipSuccess)
            return set_err(FPM_ERR_NOMEM, "fpm_set_state: hipMalloc(%zu) failed", npup * sizeof(float2));
        HIP_TRY(hipMemcpyAsync(stage.p, pupil, npup * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        src_p = (const float2 *)stage.p;
    }

    // check: nothing of the context is written before both arrays are accepted
    HIP_TRY(launch_state_check(st, src_f, src_p, shared, c->fused(), c->state_chk, c->stream));
    std::vector<unsigned long long> h((state_check_bytes(st.B) + 7) / 8);
    HIP_TRY(hipMemcpyAsync(h.data(), c->state_chk, state_check_bytes(st.B), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (objF && h[0] != ~0ull) return refuse_spectrum(c, src_f, h[0]);
    if (pupil) {
        if (h[1] != ~0ull) {
            const size_t i = h[1], np = st.np;
            return set_err(FPM_ERR_INVAL, "fpm_set_state: pupil is not finite at (patch %d, y %d, x %d), inside the support",
                           (int)(i / (np * np)), (int)(i / np % np), (int)(i % np));
        }
        const float *pm = reinterpret_cast<const float *>(h.data() + 2);
        for (int b = 0; b < st.B; ++b)
            if (!(pm[b] > 0.f))
                return set_err(FPM_ERR_INVAL,
                               "fpm_set_state: pupil of patch %d is zero on the whole support (max|P S| must be > 0)", b);
    }

    // place: from here on the context changes
    HIP_TRY(launch_state_place(st, src_f, src_p, shared, c->state_chk, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->initialized = true;
    c->objcrop_valid = false;
    return FPM_OK;
}

int fpm_download_state_device(fpm_ctx *c, float *objF_dev, float *pupil_dev) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!objF_dev && !pupil_dev) return set_err(FPM_ERR_INVAL, "fpm_download_state_device: both pointers are NULL");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_download_state_device before a state exists");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = refuse_capture(c, "fpm_download_state_device")) return rc;
    HIP_TRY(launch_state_out(c->st, (float2 *)objF_dev, (float2 *)pupil_dev, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FPM_OK;
}

}  // extern "C"
