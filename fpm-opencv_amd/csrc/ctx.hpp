// ctx.hpp -- the context behind the extern "C" boundary of libfpm_hip.so
// (include/fpm_hip.h), shared by the files that implement it:
//   create.cpp    validate, plan, allocate, destroy; fpm_set_crops / fpm_get_crops,
//                 fpm_set_gains / fpm_get_gains
//   transfer.cpp  the stack uploads and the downloads
//   run.cpp       fpm_init, fpm_run, the general path's patch groups and graphs
//   residual_api.cpp  fpm_residual, fpm_residual_at, fpm_moments, fpm_predict (kernels: residual.hip)
//   gradient_api.cpp  fpm_gradient (kernels: gradient.hip and the sweep's column kernels)
//   state_api.cpp fpm_set_state, fpm_download_state_device (kernels: state.hip)
//   refocus_api.cpp fpm_refocus (kernels: refocus.hip; the transform is objCrop's)
//   stitch_api.cpp fpm_stitch_tiles, fpm_stitch (kernels: stitch.hip; solve: stitch_solve.hpp)
//   api.cpp       errors, version, info, timing, clock, fpm_runFPM
// Errors are negative codes plus fpm_last_error(); nothing here ever falls
// back to a CPU path.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/fpm_hip.h"
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

// records the message fpm_last_error() returns (one thread_local string,
// api.cpp) and returns code
int set_err(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fpm::set_err(FPM_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                           \
    } while (0)

#define HIP_RET(x)                                   \
    do {                                             \
        const hipError_t e_ = (x);                   \
        if (e_ != hipSuccess) return e_;             \
    } while (0)

// The LED-update kernel of a context, chosen once by plan_context
// (create.cpp); kKernels has one row per value, in this order.
enum class Kernel { General, Np256, Np256Dist, Np200, Np90, Small };

inline constexpr const char *kStampsFused[kStamps] = {
    "gather", "A:tail+sync", "B:columns", "C:tail+sync", "upd:sync+Opre", "max",        "P",
    "A:rowIDFT", "C:rowDFT", "upd:body",  "B:loop",      "split:Fstores", "split:Fwait"};
inline constexpr const char *kStampsDist[kStamps] = {"gather", "A", "sync1", "B", "sync2", "C", "update", "sync3",
                                                     "merge+Opre", "max", "P", "C:rows(sub)", "sync3:acks(sub)"};

struct KernelRow {
    int code;                   // fpm_info.fused_kernel (FPM_KERNEL_*)
    int threads;                // per workgroup; 0 = the general path's several kernels
    int meas_g;                 // lane-group size of the stack's column layout (meas_layout); -1 = Np
                                // (transposed); the general path's follows its GeneralPlan::Kind
    const char *const *stamps;  // FPM_STAMPS phase names
};
inline constexpr KernelRow kKernels[] = {
    {FPM_KERNEL_GENERAL, 0, 0, nullptr},                    // general.hip, np1024.hip, np256.hip
    {FPM_KERNEL_FUSED_NP256, 512, 16, kStampsFused},        // fpm_fused.hip, one workgroup or split mode
    {FPM_KERNEL_FUSED_NP256_DIST, 512, 16, kStampsDist},    // fused_dist.hip
    {FPM_KERNEL_FUSED_NP200, 768, 10, kStampsFused},        // fused_mr.hip
    {FPM_KERNEL_FUSED_NP90, 1024, 9, kStampsFused},         // fused_s90.hip
    {FPM_KERNEL_FUSED_SMALL, 1024, -1, kStampsFused},       // fused_small.hip
};

}  // namespace fpm

// Everything from `st` down to `ngroups` is decided by plan_context before
// anything is created; the destructor releases whatever was created since.
struct fpm_ctx {
    fpm_problem prob{};
    std::vector<int32_t> order, x0, y0;
    int device = 0;
    size_t lds_limit = 0;           // LDS a workgroup of the device can have (check_device)
    int n_cu = 0;                   // its compute units (check_device): fpm_set_crops plans again with both
    fpm::Switches sw{};             // the environment at fpm_create
    // ---- the plan
    fpm::DevState st{};
    fpm::FftPlan pl_np{}, pl_L{};
    std::vector<uint8_t> disk;      // [nb][nb] support mask
    int support_px = 0;
    fpm::Kernel kernel = fpm::Kernel::General;  // the LED-update kernel
    const fpm::KernelRow &row() const { return fpm::kKernels[(int)kernel]; }
    bool fused() const { return kernel != fpm::Kernel::General; }
    int split_ks = 1;               // split / distributed mode: workgroups per patch (2, 4, 8), else 1
    fpm::GeneralPlan::Kind general_kind = fpm::GeneralPlan::Lds;  // general path: which step kernels
    bool t16 = false;               // general path: the row / column scratch T block-scaled in fp16 (DevState::T16)
    int meas_g = 0;                 // meas holds the column layout of meas_layout with g-lane groups
                                    // once uploaded (kKernels; Np: the Np 1024 general path,
                                    // transposed); 0: C-ABI
    // general path: the patches split into ngroups groups whose LED chains run
    // on concurrent streams (forked from and joined back to the run stream), so
    // one group's launches fill the other's partial last round of workgroups
    int ngroups = 1;
    static constexpr int kMaxGroups = 8;
    fpm::ResidualPlan rplan{};      // fpm_residual: kernel pair and LEDs per launch
    fpm::ObjcropPlan oplan{};       // objCrop: which transform and its launches (plan_objcrop); the crop table
                                    // changes the band its grids follow, never the plan
    // ---- what the context owns
    hipStream_t stream = nullptr;   // the run stream: own_stream or the caller's (fpm_set_stream)
    hipStream_t own_stream = nullptr;
    float2 *tw_np = nullptr, *tw_L = nullptr;
    float2 *objcrop = nullptr;
    uint16_t *meas = nullptr;
    // LED gains [n_stack][B] (fpm_set_gains): the host copy fpm_get_gains returns
    // and the device table the kernels read at every launch (DevState::gain), so
    // a captured graph of the general path never holds a gain by value
    std::vector<float> gain;
    float *gain_dev = nullptr;
    bool gains_unit = true;         // every gain is 1.0f: fpm_residual launches its ungained kernels
    float2 *xch = nullptr;          // split / distributed mode: exchange area
    int *split_flags = nullptr;     //   handoff flags [KS B] + sticky abort flag + XCC ids [KS B]
    int stall_led = -1;             //   fpm_debug_set_stall (tests): the last part stops publishing
    unsigned dist_tags = 0;         //   distributed mode: LEDs launched so far (tile-word tags)
    int *order_dev = nullptr, *x0_dev = nullptr, *y0_dev = nullptr;
    // fpm_residual's entry list: (order[i], window centre of order[i]) for every
    // position i, rebuilt whenever the crop table changes (upload_tables, fpm_set_crops)
    fpm::ResEntry *ident_dev = nullptr;
    uint8_t *disk_dev = nullptr;
    std::vector<void *> allocs;
    size_t bytes = 0;
    bool uploaded = false, initialized = false, objcrop_valid = false;
    std::vector<hipEvent_t> evpool;
    unsigned long long *dbg = nullptr;  // FPM_STAMPS=1: fused-kernel phase cycles
    unsigned long long *clk = nullptr;  // fused kernels' launch clock probe [3] (ClockProbe)
    fpm_clock clock{};                  // of the most recent fpm_run (zero when it was refused or failed)
    fpm_timing timing{};
    // general path: one iteration's 4*n_order launches of each group captured
    // once and replayed as a single graph launch (FPM_NO_GRAPH=1 launches them
    // directly)
    hipGraph_t led_graph[kMaxGroups] = {};
    hipGraphExec_t led_graph_exec[kMaxGroups] = {};
    hipStream_t gstream[kMaxGroups] = {};
    hipEvent_t gfork = nullptr, gjoin[kMaxGroups] = {};
    fpm::GeneralPlan gplan[kMaxGroups] = {};  // what each group's LED step launches (plan_general_step)

    // the residual's scratch, allocated by the first fpm_residual / fpm_residual_at:
    // T of one batch, the per-block partials, the folded [n_order][B] sums, the
    // [n_order] entries of one piece of a probe list, and its two events
    float2 *res_T = nullptr;
    fpm::ResEntry *res_ent = nullptr;
    double *res_perr = nullptr, *res_err = nullptr, *res_ref = nullptr;
    unsigned long long *res_pref = nullptr;
    hipEvent_t res_ev[2] = {};
    bool res_ready = false;         // all of the above exist
    // fpm_moments' own: the per-block partials and the folded sums of C
    double *res_pcross = nullptr, *res_cross = nullptr;
    bool mom_ready = false;
    // fpm_predict's staging buffer of one launch's images [nl][B][Np][Np] (4-byte
    // elements), allocated by its first call with a host output
    uint32_t *pred_stage = nullptr;
    bool pred_ready = false;        // cols_pred may take its LDS (allow_large_lds)
    // fpm_gradient's own: R of one batch [nl][B][nb][nb] by its first call, and the
    // device copies of host outputs ([B][L][L], [B][Np][Np]) by the first call that
    // asks for each
    float2 *grad_R = nullptr, *grad_obj = nullptr, *grad_pupil = nullptr;
    bool grad_ready = false;        // cols_grad / grad_rows may take their LDS (allow_large_lds)
    // fpm_set_state's check scratch, allocated by its first call
    fpm::StateCheck *state_chk = nullptr;
    // fpm_refocus' scratch, allocated by its first call: objF H of one plane
    // [B][L][L] (centred, fp32 on every context; zero outside the live band), the
    // zl of one piece of the plane list [kRefocusPiece][B], the sums pass's
    // partials [B][blocks][3] and the folded sums [3][kRefocusPiece][B], two events
    static constexpr int kRefocusPiece = 64;
    float2 *rf_spec = nullptr;
    double *rf_zl = nullptr, *rf_part = nullptr, *rf_sums = nullptr;
    hipEvent_t rf_ev[2] = {};
    bool rf_ready = false;

    fpm_ctx() = default;
    fpm_ctx(const fpm_ctx &) = delete;
    fpm_ctx &operator=(const fpm_ctx &) = delete;
    ~fpm_ctx();
    // the captured graphs of the general path (the destructor; a capture that failed half way)
    void drop_graphs();
};

namespace fpm {

// images and elements of the measurement stack [n_stack][B][Np][Np]
inline size_t stack_images(const fpm_ctx *c) { return (size_t)c->prob.n_stack * c->st.B; }
inline size_t stack_elems(const fpm_ctx *c) { return stack_images(c) * c->st.np * c->st.np; }

// patch group g = patches [g B / G, (g + 1) B / G)
inline DevState group_view(const fpm_ctx *c, int g) {
    const int G = c->ngroups, B = c->st.B;
    return G == 1 ? c->st : patch_view(c->st, g * B / G, (g + 1) * B / G - g * B / G);
}

// device memory of the context, counted in fpm_info.device_bytes and freed by
// the destructor; zero: cleared as well
template <typename T>
int dalloc(fpm_ctx *c, T **p, size_t count, bool zero) {
    void *q = nullptr;
    const size_t nb = count * sizeof(T);
    hipError_t e = hipMalloc(&q, nb > 0 ? nb : 16);
    if (e != hipSuccess) return set_err(FPM_ERR_NOMEM, "hipMalloc(%zu) failed: %s", nb, hipGetErrorString(e));
    c->allocs.push_back(q);
    c->bytes += nb;
    *p = (T *)q;
    if (zero && hipMemset(q, 0, nb) != hipSuccess) return set_err(FPM_ERR_DEVICE, "memset failed");
    return FPM_OK;
}

// blocking entry points (event waits, read-backs) never run inside a capture:
// FPM_ERR_INVAL for `what` on a capturing stream, before anything is enqueued (run.cpp)
int refuse_capture(const fpm_ctx *c, const char *what);

// the sweep's entry checks, probe resolution and scratch (residual_api.cpp), for
// the entry points in other files that run its kernels (gradient_api.cpp):
// what every call checks before anything is enqueued (a context, a state, a
// stack, no capture); the probes as entries, validated, messages under `what`;
// the scratch and events of the first call
int sweep_admit(fpm_ctx *c, const char *what);
int sweep_resolve_probes(const fpm_ctx *c, const char *what, const fpm_probe *probes, int n,
                         std::vector<ResEntry> &ent);
int sweep_ensure_scratch(fpm_ctx *c);

// the objCrop IDFT of the current spectrum (run.cpp); ensure: only when the
// buffer does not hold it yet
int refresh_objcrop(fpm_ctx *c);
inline int ensure_objcrop(fpm_ctx *c) { return c->objcrop_valid ? FPM_OK : refresh_objcrop(c); }

}  // namespace fpm
