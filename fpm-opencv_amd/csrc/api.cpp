// api.cpp -- the small entry points of the extern "C" boundary of
// libfpm_hip.so (include/fpm_hip.h): the last error, the versions, what a
// context reports about itself (info, timing, clock), the context-based debug
// entries (include/fpm_hip_debug.h) and the one-shot fpm_runFPM.  The boundary mirrors runFPM(FPM_Dataset*)
// (fpmMain.cpp:274-498); the rest of it is in create.cpp, transfer.cpp and
// run.cpp (ctx.hpp).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/fpm_hip_debug.h"
#include "ctx.hpp"

using namespace fpm;

namespace {
thread_local std::string g_err;
}

int fpm::set_err(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// The whole fpm_info of this header (every field of every ABI revision).
static void fill_info(const fpm_ctx *c, fpm_info *info) {
    std::memset(info, 0, sizeof *info);
    info->path = c->fused() ? FPM_PATH_FUSED : FPM_PATH_GENERAL;
    info->box = c->st.nb;
    info->support_px = c->support_px;
    info->device = c->device;
    info->device_bytes = c->bytes;
    info->wg_per_patch = c->split_ks;
    info->fused_kernel = c->row().code;
    info->threads_per_wg = c->row().threads;
}

extern "C" {

const char *fpm_last_error(void) { return g_err.c_str(); }

const char *fpm_version(void) { return "libfpm_hip 0.2 (gfx950, fp32 complex state, optional fp16 spectrum storage)"; }

int fpm_abi_version(void) { return FPM_ABI_VERSION; }

int fpm_get_info_sized(const fpm_ctx *c, fpm_info *info, size_t info_size) {
    if (!c || !info) return set_err(FPM_ERR_INVAL, "null argument");
    if (info_size < FPM_INFO_V3_SIZE)
        return set_err(FPM_ERR_INVAL, "fpm_info of %zu bytes predates every released layout", info_size);
    fpm_info full;
    fill_info(c, &full);
    std::memcpy(info, &full, std::min(info_size, sizeof full));
    return FPM_OK;
}

// Frozen at the ABI-3 layout (FPM_INFO_V3_SIZE bytes, the fields up to
// fused_kernel): a binary built against that header passes a struct of that
// size, so this entry point never writes past it.  Later fields are reported
// through fpm_get_info_sized only.
int fpm_get_info(const fpm_ctx *c, fpm_info *info) {
    if (!c || !info) return set_err(FPM_ERR_INVAL, "null argument");
    fpm_info full;
    fill_info(c, &full);
    std::memcpy(info, &full, FPM_INFO_V3_SIZE);
    return FPM_OK;
}

int fpm_get_timing(const fpm_ctx *c, fpm_timing *t) {
    if (!c || !t) return set_err(FPM_ERR_INVAL, "null argument");
    *t = c->timing;
    return FPM_OK;
}

int fpm_get_clock(const fpm_ctx *c, fpm_clock *clock) {
    if (!c || !clock) return set_err(FPM_ERR_INVAL, "null argument");
    *clock = c->clock;
    return FPM_OK;
}

int fpm_debug_set_stall(fpm_ctx *c, int led) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    c->stall_led = led;
    return FPM_OK;
}

int fpm_debug_get_plan(const fpm_ctx *c, int *meas_g, int *general_kind, int *residual_kind) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (meas_g) *meas_g = c->meas_g;
    if (general_kind) *general_kind = c->fused() ? -1 : (int)c->general_kind;
    if (residual_kind) *residual_kind = (int)c->rplan.kind;
    return FPM_OK;
}

int fpm_debug_get_band(const fpm_ctx *c, int band[4]) {
    if (!c || !band) return set_err(FPM_ERR_INVAL, "null argument");
    band[0] = c->st.sy0;
    band[1] = c->st.sy1;
    band[2] = c->st.sx0;
    band[3] = c->st.sx1;
    return FPM_OK;
}

int fpm_debug_get_maxima(const fpm_ctx *c, int *dims, float *tmax, unsigned char *dirty, float *rmax, float *pmax) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_debug_get_maxima before fpm_init");
    const DevState &st = c->st;
    if (dims) {
        dims[0] = st.nty;
        dims[1] = st.ntx;
        dims[2] = st.npart;
        dims[3] = st.rmax ? 1 : 0;
    }
    if (!tmax && !dirty && !rmax && !pmax) return FPM_OK;
    if (rmax && !st.rmax) return set_err(FPM_ERR_INVAL, "a fused context keeps no tile-row maxima");
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_debug_get_maxima");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t B = st.B, nt = (size_t)st.ntx * st.nty, nw = (nt + 31) / 32;
    if (tmax) HIP_TRY(hipMemcpy(tmax, st.tmax, B * nt * sizeof(float), hipMemcpyDeviceToHost));
    if (rmax) HIP_TRY(hipMemcpy(rmax, st.rmax, B * st.nty * sizeof(float), hipMemcpyDeviceToHost));
    if (pmax) HIP_TRY(hipMemcpy(pmax, st.pmax, B * st.npart * sizeof(float), hipMemcpyDeviceToHost));
    if (dirty) {
        std::vector<unsigned> bits(B * nw);
        HIP_TRY(hipMemcpy(bits.data(), st.tdirty, bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        std::memset(dirty, 0, B * nt);
        // fused: bit k of a patch is band tile k (tilemax.hpp); general: tile k, never set
        const BandArgs band = c->fused() ? band_of(st) : BandArgs{0, 0, st.ntx, (int)nt, 0.f};
        for (size_t b = 0; b < B; ++b)
            for (int k = 0; k < band.nbt; ++k)
                if ((bits[b * nw + (k >> 5)] >> (k & 31)) & 1u)
                    dirty[b * nt + (size_t)(band.bty0 + k / band.nbx) * st.ntx + band.btx0 + k % band.nbx] = 1;
    }
    return FPM_OK;
}

int fpm_debug_objcrop(fpm_ctx *c, const float *spec, const int band[4], float *objcrop) {
    if (!c || !spec || !band || !objcrop) return set_err(FPM_ERR_INVAL, "null argument");
    const int L = c->st.L;
    if (band[0] < 0 || band[0] > band[1] || band[1] >= L || band[2] < 0 || band[2] > band[3] || band[3] >= L)
        return set_err(FPM_ERR_INVAL, "fpm_debug_objcrop: band rows [%d, %d] columns [%d, %d] outside 0 <= lo <= hi < %d",
                       band[0], band[1], band[2], band[3], L);
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_debug_objcrop");
    if (rc) return rc;
    // the spectrum is overwritten: whatever the context held is gone
    c->initialized = false;
    c->objcrop_valid = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the context's state with the caller's band; the planned one stays in c->st
    DevState st = c->st;
    st.sy0 = band[0];
    st.sy1 = band[1];
    st.sx0 = band[2];
    st.sx1 = band[3];
    const size_t ll = (size_t)L * L, n = (size_t)st.B * ll;
    if (st.spec16) {  // as spec_st stores it (fpm_state.hpp)
        const float2 *src = (const float2 *)spec;
        std::vector<__half2> h16(ll);
        for (int b = 0; b < st.B; ++b) {
            for (size_t i = 0; i < ll; ++i) {
                const float2 v = src[b * ll + i];
                h16[i] = __float22half2_rn(make_float2(v.x * st.hscale, v.y * st.hscale));
            }
            HIP_TRY(hipMemcpy(st.spec16 + b * ll, h16.data(), ll * sizeof(__half2), hipMemcpyHostToDevice));
        }
    } else {
        HIP_TRY(hipMemcpy(st.spec, spec, n * sizeof(float2), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(c->objcrop, 0xFF, n * sizeof(float2), c->stream));
    HIP_TRY(launch_objcrop(c->oplan, st, c->objcrop, c->tw_L, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(objcrop, c->objcrop, n * sizeof(float2), hipMemcpyDeviceToHost));
    return FPM_OK;
}

int fpm_runFPM(const fpm_problem *prob, int device, const uint16_t *meas, int iters, float *objF, float *objCrop,
               float *pupil, float *support) {
    fpm_ctx *c = nullptr;
    int rc = fpm_create(prob, device, &c);
    if (rc) return rc;
    if (!(rc = fpm_upload_stack(c, meas)) && !(rc = fpm_init(c)) && !(rc = fpm_run(c, iters)))
        rc = fpm_download(c, objF, objCrop, pupil, support);
    std::string keep = g_err;
    fpm_destroy(c);
    g_err = keep;
    return rc;
}

}  // extern "C"
