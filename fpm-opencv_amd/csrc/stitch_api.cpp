// stitch_api.cpp -- fpm_stitch_tiles and fpm_stitch: overlapping tiles aligned
// and blended into one field (kernels: stitch.hip; the factor solve:
// stitch_solve.hpp).
#include "ctx.hpp"
#include "stitch_solve.hpp"

using namespace fpm;

namespace {

// device scratch and events owned by one call
struct Scratch {
    std::vector<void *> p;
    hipEvent_t ev[4] = {};
    ~Scratch() {
        for (void *q : p) (void)hipFree(q);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <typename T>
    int get(const char *what, T **out, size_t n) {
        void *q = nullptr;
        const size_t nb = n * sizeof(T) > 0 ? n * sizeof(T) : 16;
        if (hipMalloc(&q, nb) != hipSuccess) return set_err(FPM_ERR_NOMEM, "%s: hipMalloc(%zu) failed", what, nb);
        p.push_back(q);
        *out = (T *)q;
        return FPM_OK;
    }
};

// FPM_ERR_INVAL naming the field at fault; otherwise the geometry
int check_grid(const char *what, const fpm_stitch_grid *g, uint32_t flags, StitchGeom *out) {
    if (!g) return set_err(FPM_ERR_INVAL, "%s: grid is NULL", what);
    if (flags & ~(FPM_STITCH_ALIGN_PHASE | FPM_STITCH_ALIGN_COMPLEX | FPM_STITCH_DEVICE))
        return set_err(FPM_ERR_INVAL, "%s: unknown flags 0x%x", what, flags);
    if ((flags & FPM_STITCH_ALIGN_PHASE) && (flags & FPM_STITCH_ALIGN_COMPLEX))
        return set_err(FPM_ERR_INVAL, "%s: flags hold FPM_STITCH_ALIGN_PHASE and FPM_STITCH_ALIGN_COMPLEX: one of them", what);
    if (g->gy < 1) return set_err(FPM_ERR_INVAL, "%s: gy = %d, must be >= 1", what, g->gy);
    if (g->gx < 1) return set_err(FPM_ERR_INVAL, "%s: gx = %d, must be >= 1", what, g->gx);
    if (g->tile < 2 || g->tile > 32768)
        return set_err(FPM_ERR_INVAL, "%s: tile = %d, must be in [2, 32768]", what, g->tile);
    const int L = g->tile, lo = (L + 1) / 2;
    if (g->stride_y < lo || g->stride_y > L)
        return set_err(FPM_ERR_INVAL, "%s: stride_y = %d outside [%d, %d] (ceil(tile / 2) .. tile)", what, g->stride_y, lo, L);
    if (g->stride_x < lo || g->stride_x > L)
        return set_err(FPM_ERR_INVAL, "%s: stride_x = %d outside [%d, %d] (ceil(tile / 2) .. tile)", what, g->stride_x, lo, L);
    // what the launches index with int and their grids hold
    const long long H = (long long)(g->gy - 1) * g->stride_y + L, W = (long long)(g->gx - 1) * g->stride_x + L;
    if ((long long)g->gy * g->gx > 16384)
        return set_err(FPM_ERR_INVAL, "%s: gy*gx = %lld tiles, at most 16384", what, (long long)g->gy * g->gx);
    if (H > 4 * 65535ll)
        return set_err(FPM_ERR_INVAL, "%s: gy = %d gives a field of %lld rows, at most 262140", what, g->gy, H);
    if (W > (1ll << 30)) return set_err(FPM_ERR_INVAL, "%s: gx = %d gives a field of %lld columns", what, g->gx, W);
    *out = StitchGeom{g->gy, g->gx, L, g->stride_y, g->stride_x, (int)H, (int)W};
    return FPM_OK;
}

int align_mode(uint32_t flags) {
    return flags & FPM_STITCH_ALIGN_PHASE ? kStitchAlignPhase : flags & FPM_STITCH_ALIGN_COMPLEX ? kStitchAlignComplex
                                                                                                  : kStitchAlignNone;
}

// tiles and field in device memory: pair sums, host solve, blend.  Blocking on s.
int stitch_device(const char *what, const StitchGeom &g, int mode, const float2 *tiles, float2 *field, double *factors,
                  hipStream_t s, double *elapsed_ms, Scratch &sc) {
    const int nt = g.gy * g.gx, npairs = stitch_pairs(g.gy, g.gx);
    std::vector<double> f(2 * (size_t)nt);
    stitch_solve(g.gy, g.gx, kStitchAlignNone, nullptr, f.data());  // all ones
    float2 *fac_dev = nullptr;
    for (hipEvent_t &e : sc.ev) HIP_TRY(hipEventCreate(&e));
    const bool align = mode != kStitchAlignNone && npairs > 0;
    if (align) {
        double *partials = nullptr, *sums = nullptr;
        int rc = sc.get(what, &partials, (size_t)npairs * stitch_pair_parts(g).parts * 4);
        if (rc || (rc = sc.get(what, &sums, (size_t)npairs * 4)) || (rc = sc.get(what, &fac_dev, nt))) return rc;
        HIP_TRY(hipEventRecord(sc.ev[0], s));
        HIP_TRY(launch_stitch_pairs(g, tiles, partials, sums, s));
        HIP_TRY(hipEventRecord(sc.ev[1], s));
        std::vector<StitchPairSums> h(npairs);
        static_assert(sizeof(StitchPairSums) == 4 * sizeof(double), "sums [pairs][4]");
        HIP_TRY(hipMemcpyAsync(h.data(), sums, (size_t)npairs * sizeof(StitchPairSums), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        stitch_solve(g.gy, g.gx, mode, h.data(), f.data());
        std::vector<float2> f32(nt);
        for (int t = 0; t < nt; ++t) f32[t] = make_float2((float)f[2 * t], (float)f[2 * t + 1]);
        HIP_TRY(hipMemcpyAsync(fac_dev, f32.data(), nt * sizeof(float2), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));  // f32 leaves scope
    }
    HIP_TRY(hipEventRecord(sc.ev[2], s));
    HIP_TRY(launch_stitch_blend(g, tiles, fac_dev, field, s));
    HIP_TRY(hipEventRecord(sc.ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    if (elapsed_ms) {
        float a = 0.f, b = 0.f;
        if (align) HIP_TRY(hipEventElapsedTime(&a, sc.ev[0], sc.ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, sc.ev[2], sc.ev[3]));
        *elapsed_ms = (double)a + (double)b;
    }
    if (factors) std::copy(f.begin(), f.end(), factors);
    return FPM_OK;
}

int refuse_capturing(const char *what, hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return set_err(FPM_ERR_INVAL, "%s on a capturing stream: %s is blocking (fpm_hip.h)", what, what);
    return FPM_OK;
}

// tiles in device memory, field in host or device memory
int stitch_out(const char *what, const StitchGeom &g, uint32_t flags, const float2 *tiles_dev, float *field,
               double *factors, hipStream_t s, double *elapsed_ms, Scratch &sc) {
    const size_t nfield = (size_t)g.H * g.W;
    float2 *field_dev = (float2 *)field;
    if (!(flags & FPM_STITCH_DEVICE))
        if (int rc = sc.get(what, &field_dev, nfield)) return rc;
    if (int rc = stitch_device(what, g, align_mode(flags), tiles_dev, field_dev, factors, s, elapsed_ms, sc)) return rc;
    if (!(flags & FPM_STITCH_DEVICE)) {
        HIP_TRY(hipMemcpyAsync(field, field_dev, nfield * sizeof(float2), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_stitch_tiles(int device, const float *tiles, const fpm_stitch_grid *grid, uint32_t flags, float *field,
                     double *factors, void *hip_stream, double *elapsed_ms) {
    const char *what = "fpm_stitch_tiles";
    StitchGeom g{};
    if (int rc = check_grid(what, grid, flags, &g)) return rc;
    if (!tiles) return set_err(FPM_ERR_INVAL, "%s: tiles is NULL", what);
    if (!field) return set_err(FPM_ERR_INVAL, "%s: field is NULL", what);
    {
        const char *t0 = (const char *)tiles, *f0 = (const char *)field;
        const size_t tb = (size_t)g.gy * g.gx * g.L * g.L * sizeof(float2), fb = (size_t)g.H * g.W * sizeof(float2);
        if (t0 < f0 + fb && f0 < t0 + tb) return set_err(FPM_ERR_INVAL, "%s: field overlaps tiles", what);
    }
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = refuse_capturing(what, s)) return rc;
    Scratch sc;
    const float2 *tiles_dev = (const float2 *)tiles;
    if (!(flags & FPM_STITCH_DEVICE)) {
        const size_t ntiles = (size_t)g.gy * g.gx * g.L * g.L;
        float2 *stage = nullptr;
        if (int rc = sc.get(what, &stage, ntiles)) return rc;
        HIP_TRY(hipMemcpyAsync(stage, tiles, ntiles * sizeof(float2), hipMemcpyHostToDevice, s));
        tiles_dev = stage;
    }
    return stitch_out(what, g, flags, tiles_dev, field, factors, s, elapsed_ms, sc);
}

int fpm_stitch(fpm_ctx *c, const fpm_stitch_grid *grid, uint32_t flags, float *field, double *factors,
               double *elapsed_ms) {
    const char *what = "fpm_stitch";
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    StitchGeom g{};
    if (int rc = check_grid(what, grid, flags, &g)) return rc;
    if (!field) return set_err(FPM_ERR_INVAL, "%s: field is NULL", what);
    if (g.gy * g.gx != c->st.B)
        return set_err(FPM_ERR_INVAL, "%s: gy*gx = %d, the context has n_patch = %d", what, g.gy * g.gx, c->st.B);
    if (g.L != c->st.L) return set_err(FPM_ERR_INVAL, "%s: tile = %d, the context has nlarge = %d", what, g.L, c->st.L);
    if (flags & FPM_STITCH_DEVICE) {  // a device field must be clear of the tiles the call reads
        const char *t0 = (const char *)c->objcrop, *f0 = (const char *)field;
        const size_t tb = (size_t)c->st.B * g.L * g.L * sizeof(float2), fb = (size_t)g.H * g.W * sizeof(float2);
        if (t0 < f0 + fb && f0 < t0 + tb)
            return set_err(FPM_ERR_INVAL, "%s: field overlaps the context's objCrop tiles", what);
    }
    if (!c->initialized) return set_err(FPM_ERR_STATE, "%s before a state exists", what);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = refuse_capture(c, what)) return rc;
    if (int rc = ensure_objcrop(c)) return rc;
    Scratch sc;
    return stitch_out(what, g, flags, c->objcrop, field, factors, c->stream, elapsed_ms, sc);
}

}  // extern "C"
