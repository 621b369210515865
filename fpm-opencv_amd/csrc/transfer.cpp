// transfer.cpp -- the measurement stack in (fpm_upload_stack,
// fpm_upload_stack_device, fpm_upload_frames) and the results out
// (fpm_download, fpm_download_objcrop_device, fpm_download_stack), in the
// reference's conventions (fpmMain.cpp:447, :496).
#include <cstring>

#include "ctx.hpp"

using namespace fpm;

namespace {

// device scratch owned by one fpm_upload_frames call
struct Scratch {
    std::vector<void *> p;
    ~Scratch() {
        for (void *q : p) (void)hipFree(q);
    }
    template <typename T>
    hipError_t get(T **out, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, n * sizeof(T) > 0 ? n * sizeof(T) : 16);
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};

// The stack is in c->meas.  The kernels read it column-major (meas_layout):
// permuted in place here (2 B per pixel) unless the upload already did
int after_upload(fpm_ctx *c, bool permuted = false) {
    if (c->meas_g && !permuted)
        HIP_TRY(meas_layout(c->meas, c->st.np, c->meas_g, stack_images(c), true, c->stream));
    c->st.meas_g = c->meas_g;
    c->uploaded = true;
    c->initialized = false;
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_upload_stack(fpm_ctx *c, const uint16_t *meas) {
    if (!c || !meas) return set_err(FPM_ERR_INVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->meas, meas, stack_elems(c) * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return after_upload(c);
}

int fpm_upload_stack_device(fpm_ctx *c, const uint16_t *meas) {
    if (!c || !meas) return set_err(FPM_ERR_INVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (c->meas_g && meas != c->meas) {
        // the fused layouts of Np 256 / 200: copy and permute in one pass
        hipError_t e = hipSuccess;
        if (meas_layout_copy(meas, c->meas, c->st.np, c->meas_g, stack_images(c), c->stream, &e)) {
            HIP_TRY(e);
            return after_upload(c, true);
        }
    }
    HIP_TRY(hipMemcpyAsync(c->meas, meas, stack_elems(c) * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream));
    return after_upload(c);
}

int fpm_upload_frames(fpm_ctx *c, const fpm_frames *f, const uint16_t *data, int on_device, int16_t *bg_val) {
    if (!c || !f || !data || !f->patch_x0 || !f->patch_y0) return set_err(FPM_ERR_INVAL, "null argument");
    const int np = c->st.np, B = c->st.B, H = f->height, W = f->width, n = c->prob.n_stack;
    if (H < np || W < np) return set_err(FPM_ERR_INVAL, "frame %dx%d smaller than Np=%d", H, W, np);
    auto inside = [&](int x, int y) { return x >= 0 && y >= 0 && x + np <= W && y + np <= H; };
    for (int b = 0; b < B; ++b)
        if (!inside(f->patch_x0[b], f->patch_y0[b]))
            return set_err(FPM_ERR_INVAL, "patch %d window (%d,%d) outside the %dx%d frame", b, f->patch_x0[b],
                           f->patch_y0[b], W, H);
    if (!inside(f->bk1_x, f->bk1_y) || !inside(f->bk2_x, f->bk2_y))
        return set_err(FPM_ERR_INVAL, "background window outside the frame (cv::Rect assertion in the reference)");
    if (!(f->darkfield_exp_multiplier > 0.0)) return set_err(FPM_ERR_INVAL, "darkfieldExpMultiplier must be > 0");
    HIP_TRY(hipSetDevice(c->device));
    Scratch sc;
    int *px0 = nullptr, *py0 = nullptr;
    unsigned long long *sums = nullptr;
    int16_t *bg_dev = nullptr;
    uint16_t *stage = nullptr;
    HIP_TRY(sc.get(&px0, B));
    HIP_TRY(sc.get(&py0, B));
    HIP_TRY(sc.get(&sums, 2 * (size_t)n));
    HIP_TRY(sc.get(&bg_dev, n));
    HIP_TRY(hipMemcpyAsync(px0, f->patch_x0, B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(py0, f->patch_y0, B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const size_t fpx = (size_t)H * W;
    if (!on_device) HIP_TRY(sc.get(&stage, fpx));
    for (int i = 0; i < n; ++i) {
        const uint16_t *frame = data + (size_t)i * fpx;
        if (!on_device) {  // host frames go through one staging buffer (PCIe)
            HIP_TRY(hipMemcpyAsync(stage, frame, fpx * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
            frame = stage;
        }
        HIP_TRY(launch_preprocess_frame(frame, W, np, B, px0, py0, f->bk1_x, f->bk1_y, f->bk2_x, f->bk2_y,
                                        f->bg_threshold, f->darkfield_exp_multiplier,
                                        f->darkfield ? f->darkfield[i] != 0 : false, sums + 2 * i,
                                        c->meas + (size_t)i * B * np * np, bg_dev + i, c->stream));
    }
    if (bg_val) HIP_TRY(hipMemcpyAsync(bg_val, bg_dev, n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // scratch is freed on return
    return after_upload(c);
}

int fpm_download_stack(fpm_ctx *c, uint16_t *meas) {
    if (!c || !meas) return set_err(FPM_ERR_INVAL, "null argument");
    if (!c->uploaded) return set_err(FPM_ERR_STATE, "no stack uploaded");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nimg = stack_images(c);
    // back to the C-ABI layout for the copy, then forward again
    if (c->meas_g) HIP_TRY(meas_layout(c->meas, c->st.np, c->meas_g, nimg, false, c->stream));
    HIP_TRY(hipMemcpyAsync(meas, c->meas, stack_elems(c) * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (c->meas_g) HIP_TRY(meas_layout(c->meas, c->st.np, c->meas_g, nimg, true, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FPM_OK;
}

int fpm_download(fpm_ctx *c, float *objF, float *objCrop, float *pupil, float *support) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_download before fpm_init");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const DevState &st = c->st;
    const int L = st.L, np = st.np, r = st.r, nb = st.nb, B = st.B;
    const size_t ll = (size_t)L * L;
    if (objF) {
        // spec is centred; objF = fftShift(spec) (fpmMain.cpp:447)
        std::vector<float2> h(ll);
        std::vector<__half2> h16(st.spec16 ? ll : 0);
        for (int b = 0; b < B; ++b) {
            if (st.spec16) {
                HIP_TRY(hipMemcpy(h16.data(), st.spec16 + b * ll, ll * sizeof(__half2), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < ll; ++i) {
                    const float2 f = __half22float2(h16[i]);
                    h[i] = make_float2(f.x * st.hinv, f.y * st.hinv);
                }
            } else {
                HIP_TRY(hipMemcpy(h.data(), st.spec + b * ll, ll * sizeof(float2), hipMemcpyDeviceToHost));
            }
            float2 *o = (float2 *)objF + b * ll;
            for (int y = 0; y < L; ++y)
                for (int x = 0; x < L; ++x) o[(size_t)y * L + x] = h[(size_t)((y + L / 2) % L) * L + (x + L / 2) % L];
        }
    }
    if (objCrop) {
        if (int rc = ensure_objcrop(c)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(objCrop, c->objcrop, B * ll * sizeof(float2), hipMemcpyDeviceToHost));
    }
    if (pupil || support) {
        std::vector<float2> h((size_t)B * nb * nb);
        HIP_TRY(hipMemcpy(h.data(), st.pupil, h.size() * sizeof(float2), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            if (pupil) {
                // centred pupil (fftShift at fpmMain.cpp:496): P[Np/2+ky][Np/2+kx]
                float2 *o = (float2 *)pupil + (size_t)b * np * np;
                std::memset(o, 0, sizeof(float2) * np * np);
                for (int i = 0; i < nb; ++i)
                    for (int j = 0; j < nb; ++j) o[(size_t)(np / 2 + i - r) * np + np / 2 + j - r] = h[((size_t)b * nb + i) * nb + j];
            }
            if (support) {
                float *o = support + (size_t)b * np * np;
                std::memset(o, 0, sizeof(float) * np * np);
                for (int i = 0; i < nb; ++i)
                    for (int j = 0; j < nb; ++j) {
                        const int ky = i - r, kx = j - r;
                        if (ky * ky + kx * kx <= r * r) o[(size_t)((ky + np) % np) * np + (kx + np) % np] = 1.f;
                    }
            }
        }
    }
    return FPM_OK;
}

int fpm_download_objcrop_device(fpm_ctx *c, float *dst) {
    if (!c || !dst) return set_err(FPM_ERR_INVAL, "null argument");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "download before fpm_init");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_objcrop(c)) return rc;
    const size_t n = (size_t)c->st.B * c->st.L * c->st.L * sizeof(float2);
    HIP_TRY(hipMemcpyAsync(dst, c->objcrop, n, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FPM_OK;
}

}  // extern "C"
