// objcrop.hip -- objCrop = IDFT2(objF) / L^2 every iteration (fpmMain.cpp:481),
// objF = fftShift(spec): rows of the rolled spectrum, then columns, scaled by
// 1/L^2.  Here are the plan (plan_objcrop, made once per context by
// plan_context), the one launch path (launch_objcrop) and the batched
// fallback; the kernels live one family per file:
//   crop256m.hip  register transforms of L = 256 M, M in {2, 3, 4}
//   crop600.hip   L 600        crop360.hip  L 360
//   crop4k.hip    the six-step 64 x 64 passes of L 4096
//   fft_batch.hip the mixed-radix batched transform: every other L
#include <hip/hip_runtime.h>

#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

// The dispatch: register transforms only without fp16 storage (they load
// float2), L 4096 six-step unless FPM_NO_CROP4K, everything else batched.  No
// HIP call, no device.
ObjcropPlan plan_objcrop(int L, bool fp16, const FftPlan &pl_L, const Switches &sw) {
    ObjcropPlan p{};
    const CropPair regs = fp16       ? CropPair{}
                          : L == 600 ? crop600_kernels()
                          : L == 360 ? crop360_kernels()
                                     : crop256m_kernels(L);
    if (regs.rows.fn) {
        p.kind = L == 600 ? ObjcropPlan::Regs600 : L == 360 ? ObjcropPlan::Regs360 : ObjcropPlan::Regs256M;
        p.rows = regs.rows;
        p.cols = regs.cols;
    } else if (L == 4096 && !sw.no_crop4k) {
        const Crop4kKernels k = crop4k_kernels();
        p.kind = ObjcropPlan::SixStep4k;
        p.cols = k.cols1;
        p.cols2 = k.cols2;
        p.rows = k.rows;
    } else {
        p.kind = ObjcropPlan::Batched;
        p.pl = pl_L;
        p.rows = p.cols = fft_batch_kernel(pl_L, true);
        p.rows.arg = p.cols.arg = 1 << p.rows.arg;  // lc -> C
    }
    return p;
}

namespace {

// rows of the live band, then every column in place
hipError_t launch_regs(const ObjcropPlan &p, const DevState &st, float2 *out, const float2 *tw_L, hipStream_t s) {
    const float2 *spec = st.spec;
    int sy0 = st.sy0, sy1 = st.sy1, sx0 = st.sx0, sx1 = st.sx1;
    float scale = 1.0f / ((float)st.L * (float)st.L);
    const int nrows = sy1 - sy0 + 1, gr = p.rows.arg, gc = p.cols.arg;
    void *ra[] = {&spec, &out, &tw_L, &sy0, &sy1, &sx0, &sx1};
    const hipError_t e = hipLaunchKernel(p.rows.fn, dim3((nrows + gr - 1) / gr, st.B), p.rows.block, ra, p.rows.lds, s);
    if (e != hipSuccess) return e;
    void *ca[] = {&out, &tw_L, &scale, &sy0, &sy1};
    return hipLaunchKernel(p.cols.fn, dim3((st.L + gc - 1) / gc, st.B), p.cols.block, ca, p.cols.lds, s);
}

// the two column passes (one block per 64-row residue and strip), then the rows in place
hipError_t launch_six_step(const ObjcropPlan &p, DevState st, float2 *out, const float2 *tw_L, hipStream_t s) {
    float scale = 1.0f / ((float)st.L * (float)st.L);
    const dim3 grid(st.L / p.cols.arg, 64, st.B);
    void *a1[] = {&st, &out, &tw_L}, *a2[] = {&out, &tw_L}, *a3[] = {&st, &out, &tw_L, &scale};
    hipError_t e = hipLaunchKernel(p.cols.fn, grid, p.cols.block, a1, 0, s);
    if (e != hipSuccess) return e;
    e = hipLaunchKernel(p.cols2.fn, grid, p.cols2.block, a2, 0, s);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(p.rows.fn, dim3(st.L, st.B), p.rows.block, a3, 0, s);
}

hipError_t launch_batched(const ObjcropPlan &p, const DevState &st, float2 *out, const float2 *tw_L, hipStream_t s) {
    const int L = st.L;
    const size_t bs = (size_t)L * L;
    // rows: spec rows (sequences) and columns (elements) outside the live band
    // are zero; columns: objF row i of the intermediate is spec row i + L/2
    FftBand rows, cols;
    rows.qlo = st.sy0;
    rows.qhi = st.sy1;
    rows.elo = st.sx0;
    rows.ehi = st.sx1;
    cols.elo = st.sy0;
    cols.ehi = st.sy1;
    cols.eroll = L / 2;
    hipError_t e = launch_fft_batch(true, st.spec, out, p.pl, tw_L, L, st.B, bs, L, 1, bs, L, 1, L / 2, L / 2, 1.f,
                                    s, st.spec16, st.hinv, rows);
    if (e != hipSuccess) return e;
    return launch_fft_batch(true, out, out, p.pl, tw_L, L, st.B, bs, 1, L, bs, 1, L, 0, 0,
                            1.0f / ((float)L * (float)L), s, nullptr, 1.f, cols);
}

}  // namespace

hipError_t launch_objcrop(const ObjcropPlan &p, const DevState &st, float2 *out, const float2 *tw_L, hipStream_t s) {
    const int L = st.L;
    if (st.sy0 < 0 || st.sy1 >= L || st.sy0 > st.sy1 || st.sx0 < 0 || st.sx1 >= L || st.sx0 > st.sx1)
        return hipErrorInvalidValue;
    if (p.regs()) return launch_regs(p, st, out, tw_L, s);
    if (p.kind == ObjcropPlan::SixStep4k) return launch_six_step(p, st, out, tw_L, s);
    return launch_batched(p, st, out, tw_L, s);
}

}  // namespace fpm
