// create.cpp -- fpm_create and fpm_destroy: validate the problem, check the
// device, plan the context (plan_context: every decision, no HIP call), then
// allocate what the plan names and upload the tables.  The context owns what
// it created: its destructor releases it, on fpm_destroy and on every failed
// fpm_create alike.  fpm_set_crops replaces the crop table of a live context:
// it plans the new table the same way and takes it only if the plan is the
// live one's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/fpm_hip_debug.h"
#include "ctx.hpp"
#include "fft_inplace.hpp"

using namespace fpm;

fpm_ctx::~fpm_ctx() {
    drop_graphs();
    for (void *p : allocs) (void)hipFree(p);
    for (auto e : evpool) (void)hipEventDestroy(e);
    for (int g = 0; g < kMaxGroups; ++g) {
        if (gstream[g]) (void)hipStreamDestroy(gstream[g]);
        if (gjoin[g]) (void)hipEventDestroy(gjoin[g]);
    }
    if (gfork) (void)hipEventDestroy(gfork);
    for (auto e : res_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : rf_ev)
        if (e) (void)hipEventDestroy(e);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

void fpm_ctx::drop_graphs() {
    for (int g = 0; g < kMaxGroups; ++g) {
        if (led_graph_exec[g]) (void)hipGraphExecDestroy(led_graph_exec[g]);
        if (led_graph[g]) (void)hipGraphDestroy(led_graph[g]);
        led_graph_exec[g] = nullptr;
        led_graph[g] = nullptr;
    }
}

namespace {

bool make_plan(int n, FftPlan *pl) {
    std::memset(pl, 0, sizeof *pl);
    pl->n = n;
    int m = n, k = 0;
    while (m % 8 == 0) { pl->radix[k++] = 8; m /= 8; }
    while (m % 4 == 0) { pl->radix[k++] = 4; m /= 4; }
    while (m % 2 == 0) { pl->radix[k++] = 2; m /= 2; }
    while (m % 3 == 0) { pl->radix[k++] = 3; m /= 3; }
    while (m % 5 == 0) { pl->radix[k++] = 5; m /= 5; }
    pl->nstages = k;
    return m == 1 && k < 24;
}

// Every environment switch of the library, read once per
// context by fpm_create: a setenv between two runs never changes the kernels
// of a live context.
Switches read_switches() {
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name) {  // the value, clamped at 0; -1 = unset
        const char *e = getenv(name);
        return e ? std::max(0, atoi(e)) : -1;
    };
    Switches sw{};
    sw.no_s90 = on("FPM_NO_S90");
    sw.no_reg1024 = on("FPM_NO_REG1024");
    sw.no_reg256 = on("FPM_NO_REG256");
    sw.t32 = on("FPM_T32");
    sw.stamps = on("FPM_STAMPS");
    sw.no_graph = on("FPM_NO_GRAPH");
    sw.no_wave_cols = on("FPM_NO_WAVE_COLS");
    sw.no_crop4k = on("FPM_NO_CROP4K");
    sw.s90_dense = on("FPM_S90_DENSE");
    sw.mr_dense = on("FPM_MR_DENSE");
    sw.no_split = on("FPM_NO_SPLIT");
    sw.no_dist = on("FPM_NO_DIST");
    sw.no_ledtab = on("FPM_NO_LEDTAB");
    sw.patch_groups = num("FPM_PATCH_GROUPS");
    sw.split = num("FPM_SPLIT");
    sw.dist = num("FPM_DIST");
    sw.res_lds = on("FPM_RES_LDS");
    sw.res_one_seq = on("FPM_RES_ONE_SEQ");
    sw.res_batch = num("FPM_RES_BATCH");
    sw.one_seq = on("FPM_ONE_SEQ");
    return sw;
}

std::vector<float2> twiddles(int n) {
    std::vector<float2> t(n);
    for (int k = 0; k < n; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)n;
        t[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return t;
}

// cv::Rect(cropXStart, cropYStart, Np, Np) must lie inside objF (fpmMain.cpp:361)
int validate_crops(int np, int nlarge, int n_stack, const int32_t *x0, const int32_t *y0) {
    for (int i = 0; i < n_stack; ++i)
        if (x0[i] < 0 || x0[i] > nlarge - np || y0[i] < 0 || y0[i] > nlarge - np)
            return set_err(FPM_ERR_INVAL, "LED %d crop (%d,%d) leaves the %dx%d spectrum", i, x0[i], y0[i], nlarge,
                           nlarge);
    return FPM_OK;
}

int validate(const fpm_problem *p) {
    if (!p) return set_err(FPM_ERR_INVAL, "null problem");
    if (p->np < 4 || (p->np & 1)) return set_err(FPM_ERR_INVAL, "Np=%d must be even and >= 4", p->np);
    if (p->nlarge < p->np || (p->nlarge & 1))
        return set_err(FPM_ERR_INVAL, "Nlarge=%d must be even and >= Np", p->nlarge);
    FftPlan t;
    if (!make_plan(p->np, &t)) return set_err(FPM_ERR_INVAL, "Np=%d is not 2^a 3^b 5^c", p->np);
    if (!make_plan(p->nlarge, &t)) return set_err(FPM_ERR_INVAL, "Nlarge=%d is not 2^a 3^b 5^c", p->nlarge);
    if (p->nlarge > fft_max_len())
        return set_err(FPM_ERR_INVAL, "Nlarge=%d exceeds the batched transform limit %d", p->nlarge, fft_max_len());
    if (p->na_radius < 0 || 2 * p->na_radius + 1 > p->np)
        return set_err(FPM_ERR_INVAL, "naRadius=%d needs 2r+1 <= Np=%d", p->na_radius, p->np);
    if (p->n_stack < 1 || p->n_order < 2)
        return set_err(FPM_ERR_INVAL, "need n_stack>=1 and ledUsedCount>=2 (init uses sortedIndicies.at(1))");
    if (!p->order || !p->crop_x0 || !p->crop_y0) return set_err(FPM_ERR_INVAL, "null order/crop arrays");
    if (p->init_pos < 0 || p->init_pos >= p->n_order) return set_err(FPM_ERR_INVAL, "init_pos out of range");
    if (!(p->delta2 > 0.0))
        return set_err(FPM_ERR_INVAL, "delta2=%g: the reference divides 0/0 outside the support when delta2==0",
                       p->delta2);
    if (!(p->delta1 > 0.0)) return set_err(FPM_ERR_INVAL, "delta1=%g must be > 0", p->delta1);
    if (p->n_patch < 1) return set_err(FPM_ERR_INVAL, "n_patch=%d", p->n_patch);
    for (int i = 0; i < p->n_order; ++i)
        if (p->order[i] < 0 || p->order[i] >= p->n_stack)
            return set_err(FPM_ERR_INVAL, "order[%d]=%d outside the stack", i, p->order[i]);
    return validate_crops(p->np, p->nlarge, p->n_stack, p->crop_x0, p->crop_y0);
}

// a gfx950 device; makes it current and reports its CU count and the LDS a
// workgroup can have
int check_device(int device, int *n_cu, size_t *lds_limit) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_err(FPM_ERR_NODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return set_err(FPM_ERR_NODEV, "device %d of %d", device, ndev);
    hipDeviceProp_t pr;
    HIP_TRY(hipGetDeviceProperties(&pr, device));
    if (std::strncmp(pr.gcnArchName, "gfx950", 6) != 0)
        return set_err(FPM_ERR_NODEV, "device %d is %s, this library is built for gfx950", device, pr.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    *n_cu = pr.multiProcessorCount;
    *lds_limit = std::max(pr.sharedMemPerBlock, pr.maxSharedMemoryPerMultiProcessor);  // one workgroup may take a CU's
    return FPM_OK;
}

// the DevState scalars of the validated problem c->prob; keep: a live
// context's state whose band the new one must contain (fpm_set_crops)
void plan_state(fpm_ctx *c, const DevState *keep) {
    const fpm_problem &p = c->prob;
    const int np = p.np, L = p.nlarge, r = p.na_radius;
    DevState &st = c->st;
    st.np = np;
    st.L = L;
    st.r = r;
    st.nb = 2 * r + 1;
    st.B = st.mB = p.n_patch;
    st.ntx = st.nty = (L + kTile - 1) / kTile;
    st.delta1 = (float)p.delta1;
    st.delta2 = (float)p.delta2;
    st.eps = (float)p.eps;
    // cv::add(UMat CV_64FC2, double) semantics (fpm_hip.h FPM_FLAG_SCALAR_RE_ONLY)
    const bool re_only = (p.flags & FPM_FLAG_SCALAR_RE_ONLY) != 0;
    st.eps_im = re_only ? 0.f : st.eps;
    st.d1_im = re_only ? 0.f : st.delta1;
    st.d2_im = re_only ? 0.f : st.delta2;
    // fp16 storage scale: 2^-ceil(log2 Np^2) (fpm_state.hpp)
    int e2 = 0;
    while ((1ll << e2) < (long long)np * np) ++e2;
    st.hscale = std::ldexp(1.0f, -e2);
    st.hinv = std::ldexp(1.0f, e2);
    // live band of the centred spectrum (fpm_state.hpp): the init placement at
    // L/2 (fpmMain.cpp:332-343) and every used LED's support box (:405-447)
    st.sy0 = st.sx0 = L / 2 - r;
    st.sy1 = st.sx1 = L / 2 + r;
    for (int i = 0; i < p.n_order; ++i) {
        const int led = c->order[i];
        st.sy0 = std::min(st.sy0, c->y0[led] + np / 2 - r);
        st.sy1 = std::max(st.sy1, c->y0[led] + np / 2 + r);
        st.sx0 = std::min(st.sx0, c->x0[led] + np / 2 - r);
        st.sx1 = std::max(st.sx1, c->x0[led] + np / 2 + r);
    }
    st.sy0 = std::max(st.sy0, 0);
    st.sx0 = std::max(st.sx0, 0);
    st.sy1 = std::min(st.sy1, L - 1);
    st.sx1 = std::min(st.sx1, L - 1);
    // never shrunk: what earlier LEDs wrote stays inside the band that objCrop
    // and the maxima scans read
    if (keep) {
        st.sy0 = std::min(st.sy0, keep->sy0);
        st.sx0 = std::min(st.sx0, keep->sx0);
        st.sy1 = std::max(st.sy1, keep->sy1);
        st.sx1 = std::max(st.sx1, keep->sx1);
    }
}

// a planned launch within the LDS a workgroup can have (dynamic plus the kernel's own)
int lds_fits(const fpm_ctx *c, const char *what, const StepKernel &k, size_t lds_limit) {
    if (k.lds_total() <= lds_limit) return FPM_OK;
    return set_err(FPM_ERR_INVAL, "Np=%d r=%d Nlarge=%d: the %s kernel needs %zu B of LDS (%zu dynamic + %zu static), "
                   "the device offers %zu", c->prob.np, c->prob.na_radius, c->prob.nlarge, what, k.lds_total(), k.lds,
                   k.lds_static, lds_limit);
}

// the sweep's LDS pair (the register pair's LDS does not grow with the problem)
int residual_lds_fits(const fpm_ctx *c, size_t lds_limit) {
    if (c->rplan.kind != ResidualPlan::Lds) return FPM_OK;
    int rc = lds_fits(c, "residual row", c->rplan.rows, lds_limit);
    if (!rc) rc = lds_fits(c, "residual column", c->rplan.cols, lds_limit);
    if (!rc) rc = lds_fits(c, "gradient column", c->rplan.cols_grad, lds_limit);
    return rc ? rc : lds_fits(c, "gradient row", c->rplan.grad_rows, lds_limit);
}

// objCrop's launches: only the batched transform's LDS grows with the problem
// (Nlarge 10240: DESIGN.md section 4.7)
int objcrop_lds_fits(const fpm_ctx *c, size_t lds_limit) {
    const ObjcropPlan &p = c->oplan;
    if (!p.rows.fn)
        return set_err(FPM_ERR_INVAL, "Nlarge=%d: not one sequence fits a block of the batched transform",
                       c->prob.nlarge);
    int rc = lds_fits(c, "objCrop row", p.rows, lds_limit);
    if (!rc) rc = lds_fits(c, "objCrop column", p.cols, lds_limit);
    if (!rc && p.kind == ObjcropPlan::SixStep4k) rc = lds_fits(c, "objCrop second column", p.cols2, lds_limit);
    return rc;
}

// the last checks of every plan: the residual sweep's launches, then objCrop's
int sweep_and_objcrop_fit(const fpm_ctx *c, size_t lds_limit) {
    const int rc = residual_lds_fits(c, lds_limit);
    return rc ? rc : objcrop_lds_fits(c, lds_limit);
}

// Everything a context is, decided from the validated problem (c->prob with
// its arrays), the switches (c->sw), the device's CU count and its LDS per
// workgroup before anything is created: no HIP call, no device memory.
// Refuses a fused path that this geometry or fp16 spectrum storage does not
// have, and a size whose planned step, sweep or objCrop kernel needs more LDS
// than the device offers (Np 10240, Nlarge 10240: DESIGN.md section 4.7).
int plan_context(fpm_ctx *c, int n_cu, size_t lds_limit, const DevState *keep = nullptr) {
    const fpm_problem &p = c->prob;
    const Switches &sw = c->sw;
    const int np = p.np, L = p.nlarge, r = p.na_radius, nb = 2 * r + 1, B = p.n_patch;
    DevState &st = c->st;
    plan_state(c, keep);
    make_plan(np, &c->pl_np);
    make_plan(L, &c->pl_L);

    // support disk on the box: Euclidean disk == filled cv::circle (fpmMain.cpp:307)
    c->disk.resize((size_t)nb * nb);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < nb; ++j) {
            const int ky = i - r, kx = j - r;
            c->disk[(size_t)i * nb + j] = (ky * ky + kx * kx <= r * r) ? 1 : 0;
            c->support_px += c->disk[(size_t)i * nb + j];
        }

    const bool fp16 = (p.flags & FPM_FLAG_SPEC_FP16) != 0;
    c->oplan = plan_objcrop(L, fp16, c->pl_L, sw);
    // Np 90 (configs 1 / 2): the register-transform kernel unless FPM_NO_S90=1
    // selects the generic small-patch kernel
    const Kernel fused = fused_threads(np, r, L, st)                                  ? Kernel::Np256
                         : fused_mr_supported(np, r, st)                              ? Kernel::Np200
                         : !sw.no_s90 && fused_s90_supported(np, r, st)               ? Kernel::Np90
                         : fused_small_supported(np, r, st)                           ? Kernel::Small
                                                                                      : Kernel::General;
    if (p.path == FPM_PATH_FUSED && (fp16 || fused == Kernel::General))
        return set_err(FPM_ERR_INVAL, "fused path unsupported for Np=%d r=%d L=%d%s", np, r, L,
                       fp16 ? " with fp16 spectrum storage" : "");
    c->kernel = (p.path == FPM_PATH_GENERAL || fp16) ? Kernel::General : fused;

    if (c->fused()) {
        // small batches: every phase distributed over KS workgroups per patch
        // (fused_dist.hip), else split mode (column parts only), else one
        // workgroup per patch
        if (c->kernel == Kernel::Np256) {
            const int dks = fused_dist_parts(B, n_cu, r, L, sw);
            if (dks > 1) c->kernel = Kernel::Np256Dist;
            c->split_ks = dks > 1 ? dks : fused_split_parts(c->row().threads, B, n_cu, sw);
        }
        st.npart = 1;
        c->meas_g = c->row().meas_g < 0 ? np : c->row().meas_g;
        c->rplan = plan_residual(st, c->pl_np, p.n_order, c->meas_g, fp16, sw);
        return sweep_and_objcrop_fit(c, lds_limit);
    }
    // Np 1024 general path: register row/column kernels reading the stack
    // transposed; Np 256 beyond the fused kernels' radius: register kernels
    // reading the fused column layout (g = 16).  Their row IDFT writes one
    // max|P| partial per box row
    c->general_kind = np1024_supported(np, r) && !sw.no_reg1024           ? GeneralPlan::Reg1024
                      : np256_supported(np, r, L, fp16) && !sw.no_reg256  ? GeneralPlan::Reg256
                                                                          : GeneralPlan::Lds;
    const bool reg = c->general_kind != GeneralPlan::Lds;
    st.npart = reg ? std::max(pupil_parts(nb), nb) : pupil_parts(nb);
    c->meas_g = c->general_kind == GeneralPlan::Reg1024 ? np : c->general_kind == GeneralPlan::Reg256 ? 16 : 0;
    // fp16 spectrum storage on the Np 1024 register kernels: the row /
    // column scratch T block-scaled in fp16 too (half its HBM traffic;
    // FPM_T32=1 keeps it fp32)
    c->t16 = c->general_kind == GeneralPlan::Reg1024 && fp16 && !sw.t32;
    // patch groups on concurrent streams (FPM_PATCH_GROUPS=n overrides):
    // two for the Np 1024 kernels, whose row launches cover a few patches
    // in 1.3 rounds of workgroups (config 5, 8 patches: 65.5 -> 57.5 ms of
    // LED steps per iteration; 3 or 4 groups measured slower, 79 / 77 ms),
    // and for the Np 256 register kernels, whose three short launches per
    // LED then overlap one group's tail with the other's start (dataset_mono
    // at Np 256, 64 patches: 1.18 -> 1.25 M LED-updates/s)
    c->ngroups = sw.patch_groups >= 0 ? sw.patch_groups : (reg ? 2 : 1);
    c->ngroups = std::max(1, std::min({c->ngroups, B, (int)fpm_ctx::kMaxGroups}));
    c->rplan = plan_residual(st, c->pl_np, p.n_order, c->meas_g, fp16, sw);
    // what each patch group's LED step launches: it reads the sizes only
    for (int g = 0; g < c->ngroups; ++g) {
        DevState v = st;
        v.B = (g + 1) * B / c->ngroups - g * B / c->ngroups;
        c->gplan[g] = plan_general_step(v, c->general_kind, c->pl_np, sw);
    }
    int rc = FPM_OK;
    for (int g = 0; !reg && g < c->ngroups; ++g) {  // the register kernels' LDS does not grow with the problem
        const GeneralPlan &gp = c->gplan[g];
        if ((rc = lds_fits(c, "row IDFT", gp.k1, lds_limit)) || (rc = lds_fits(c, "column", gp.k2, lds_limit)) ||
            (rc = lds_fits(c, "row DFT / update", gp.k3, lds_limit)))
            return rc;
    }
    return sweep_and_objcrop_fit(c, lds_limit);
}

// the run stream, the buffers and the patch groups' streams the plan names
int allocate(fpm_ctx *c) {
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
        return set_err(FPM_ERR_DEVICE, "hipStreamCreate failed");
    c->stream = c->own_stream;
    DevState &st = c->st;
    const size_t B = st.B, np = st.np, nb = st.nb, specn = B * st.L * st.L;
    int rc = FPM_OK;  // of the first allocation that failed; the ones after it are skipped
    auto get = [&](auto **p, size_t n, bool zero = false) {
        if (rc == FPM_OK) rc = dalloc(c, p, n, zero);
    };
    if (c->prob.flags & FPM_FLAG_SPEC_FP16) get(&st.spec16, specn);
    else get(&st.spec, specn);
    get(&c->objcrop, specn);
    get(&st.pupil, B * nb * nb);
    get(&st.tmax, B * st.ntx * st.nty);
    get(&st.tdirty, B * ((st.ntx * st.nty + 31) / 32));
    get(&st.pmax, B * st.npart);
    get(&c->disk_dev, c->disk.size());
    get(&c->meas, stack_elems(c));
    get(&c->gain_dev, stack_images(c));
    get(&c->order_dev, c->order.size());
    get(&c->x0_dev, c->x0.size());
    get(&c->y0_dev, c->y0.size());
    get(&c->ident_dev, c->order.size());
    if (c->fused()) {
        get(&st.T, fused_T_elems(st.np, st.r, st.B));
        if (c->split_ks > 1) {
            // distributed mode's tile words start at tag 0, which no LED uses
            get(&c->xch, c->kernel == Kernel::Np256Dist ? fused_dist_elems(st.B, c->split_ks)
                                                        : fused_xch_elems(st.B, c->split_ks), true);
            get(&c->split_flags, fused_flag_words(st.B, c->split_ks), true);
        }
        get(&c->clk, 3, true);
        if (c->sw.stamps) get(&c->dbg, 2 * kStamps, true);
    } else {
        if (c->t16) {
            get(&st.T16, B * nb * np);
            get(&st.tsr, B * nb);
            get(&st.tsc, B * np);
        } else {
            get(&st.T, B * nb * np);
        }
        get(&st.dP, B * nb * nb);
        get(&st.rmax, B * st.nty);
    }
    get(&c->tw_np, np);
    get(&c->tw_L, (size_t)st.L);
    if (rc) return rc;
    st.meas = c->meas;
    st.gain = c->gain_dev;
    st.disk = c->disk_dev;
    st.clk = c->clk;
    for (int g = 1; g < c->ngroups; ++g) {
        if (hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->gjoin[g], hipEventDisableTiming) != hipSuccess)
            return set_err(FPM_ERR_DEVICE, "patch-group stream / event creation failed");
    }
    if (c->ngroups > 1 && hipEventCreateWithFlags(&c->gfork, hipEventDisableTiming) != hipSuccess)
        return set_err(FPM_ERR_DEVICE, "patch-group event creation failed");
    return FPM_OK;
}

template <class V>
bool put(void *dst, const V &v) {
    return hipMemcpy(dst, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice) == hipSuccess;
}

// the crop table and what is derived from it: fpm_residual's entry list
bool upload_crops(fpm_ctx *c) {
    std::vector<ResEntry> ident(c->order.size());
    for (size_t i = 0; i < ident.size(); ++i) {
        const int led = c->order[i];
        ident[i] = ResEntry{led, c->x0[led] + c->st.np / 2, c->y0[led] + c->st.np / 2, 0};
    }
    return put(c->x0_dev, c->x0) && put(c->y0_dev, c->y0) && put(c->ident_dev, ident);
}

int upload_tables(fpm_ctx *c) {
    const auto twn = twiddles(c->st.np), twl = twiddles(c->st.L);
    c->gain.assign(stack_images(c), 1.0f);
    if (!put(c->tw_np, twn) || !put(c->tw_L, twl) || !put(c->disk_dev, c->disk) || !put(c->order_dev, c->order) ||
        !put(c->gain_dev, c->gain) || !upload_crops(c))
        return set_err(FPM_ERR_DEVICE, "table upload failed");
    return FPM_OK;
}

// ---- fpm_set_crops: is the new table's plan the live context's? ---------------------
bool same_kernel(const StepKernel &a, const StepKernel &b) {
    return a.fn == b.fn && a.grid.x == b.grid.x && a.grid.y == b.grid.y && a.grid.z == b.grid.z &&
           a.block.x == b.block.x && a.lds == b.lds && a.arg == b.arg && a.lds_static == b.lds_static;
}

// the first difference between two plans by name, or null: everything
// plan_context decides that a launch or an allocation of the live context relies on
const char *plan_difference(const fpm_ctx *a, const fpm_ctx *b) {
    if (a->kernel != b->kernel) return "the LED-update kernel";
    if (a->split_ks != b->split_ks) return "the workgroups per patch";
    if (a->general_kind != b->general_kind || a->t16 != b->t16) return "the general path's step kernels";
    if (a->meas_g != b->meas_g) return "the stack's device layout";
    if (a->ngroups != b->ngroups) return "the patch groups";
    if (a->st.npart != b->st.npart) return "the pupil-maximum partials";
    const ResidualPlan &p = a->rplan, &q = b->rplan;
    if (p.kind != q.kind || p.nblk != q.nblk || p.nl != q.nl || p.t_led != q.t_led || !same_kernel(p.rows, q.rows) ||
        !same_kernel(p.cols, q.cols) || !same_kernel(p.cols_gain, q.cols_gain) || !same_kernel(p.cols_mom, q.cols_mom) ||
        !same_kernel(p.cols_pred, q.cols_pred) || !same_kernel(p.cols_grad, q.cols_grad) ||
        !same_kernel(p.grad_rows, q.grad_rows))
        return "the residual sweep's plan";
    for (int g = 0; !a->fused() && g < a->ngroups; ++g) {
        const GeneralPlan &u = a->gplan[g], &v = b->gplan[g];
        if (u.kind != v.kind || (u.kind == GeneralPlan::Lds && (!same_kernel(u.k1, v.k1) || !same_kernel(u.k2, v.k2) ||
                                                                 !same_kernel(u.k3, v.k3) ||
                                                                 !same_kernel(u.k3_gain, v.k3_gain))))
            return "the general path's step plan";
    }
    return nullptr;
}

// The fused kernels keep a patch's dirty bits indexed by band tile
// (tilemax.hpp): bit k is tile (bty0 + k / nbx, btx0 + k % nbx).  A band that
// grew renumbers them; tiles newly inside it are clean, and their tmax is the
// 0 fpm_init wrote (the spectrum is zero there).  The stream is idle.
int remap_dirty_bits(fpm_ctx *c, const BandArgs &from, const BandArgs &to) {
    const DevState &st = c->st;
    const size_t nw = ((size_t)st.ntx * st.nty + 31) / 32;
    std::vector<unsigned> old_bits(st.B * nw), bits(st.B * nw, 0u);
    HIP_TRY(hipMemcpy(old_bits.data(), st.tdirty, old_bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < (size_t)st.B; ++b)
        for (int k = 0; k < from.nbt; ++k)
            if ((old_bits[b * nw + (k >> 5)] >> (k & 31)) & 1u) {
                const int ty = from.bty0 + k / from.nbx, tx = from.btx0 + k % from.nbx;
                const int j = (ty - to.bty0) * to.nbx + (tx - to.btx0);
                bits[b * nw + (j >> 5)] |= 1u << (j & 31);
            }
    HIP_TRY(hipMemcpy(st.tdirty, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_create(const fpm_problem *prob, int device, fpm_ctx **out) {
    if (!out) return set_err(FPM_ERR_INVAL, "null out");
    *out = nullptr;
    int rc = validate(prob), n_cu = 0;
    size_t lds_limit = 0;
    if (rc || (rc = check_device(device, &n_cu, &lds_limit))) return rc;

    std::unique_ptr<fpm_ctx> c(new fpm_ctx());
    c->prob = *prob;
    c->device = device;
    c->lds_limit = lds_limit;
    c->n_cu = n_cu;
    c->sw = read_switches();
    c->order.assign(prob->order, prob->order + prob->n_order);
    c->x0.assign(prob->crop_x0, prob->crop_x0 + prob->n_stack);
    c->y0.assign(prob->crop_y0, prob->crop_y0 + prob->n_stack);
    c->prob.order = c->order.data();
    c->prob.crop_x0 = c->x0.data();
    c->prob.crop_y0 = c->y0.data();

    if ((rc = plan_context(c.get(), n_cu, lds_limit)) || (rc = allocate(c.get())) || (rc = upload_tables(c.get())))
        return rc;
    if (!c->fused())
        for (int g = 0; g < c->ngroups && c->general_kind == GeneralPlan::Lds; ++g)
            HIP_TRY(allow_large_lds({&c->gplan[g].k1, &c->gplan[g].k2, &c->gplan[g].k3, &c->gplan[g].k3_gain}, lds_limit));
    // the register column passes of L 1024, 600 and 360; launch_fft_batch sets its own
    if (c->oplan.regs()) HIP_TRY(allow_large_lds({&c->oplan.rows, &c->oplan.cols}, lds_limit));
    *out = c.release();
    return FPM_OK;
}

void fpm_destroy(fpm_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

int fpm_get_crops(const fpm_ctx *c, int32_t *crop_x0, int32_t *crop_y0) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (crop_x0) std::copy(c->x0.begin(), c->x0.end(), crop_x0);
    if (crop_y0) std::copy(c->y0.begin(), c->y0.end(), crop_y0);
    return FPM_OK;
}

int fpm_set_crops(fpm_ctx *c, const int32_t *crop_x0, const int32_t *crop_y0) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!crop_x0 || !crop_y0) return set_err(FPM_ERR_INVAL, "fpm_set_crops: null crop arrays");
    const fpm_problem &p = c->prob;
    int rc = validate_crops(p.np, p.nlarge, p.n_stack, crop_x0, crop_y0);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = refuse_capture(c, "fpm_set_crops"))) return rc;
    // the new table planned on a scratch context that owns nothing (no HIP
    // call), its band grown to hold the live one
    fpm_ctx t;
    t.prob = c->prob;
    t.sw = c->sw;
    t.order = c->order;
    t.x0.assign(crop_x0, crop_x0 + p.n_stack);
    t.y0.assign(crop_y0, crop_y0 + p.n_stack);
    t.prob.order = t.order.data();
    t.prob.crop_x0 = t.x0.data();
    t.prob.crop_y0 = t.y0.data();
    if ((rc = plan_context(&t, c->n_cu, c->lds_limit, &c->st))) {
        const std::string why = fpm_last_error();
        return set_err(rc, "fpm_set_crops: the new table does not fit this context (%s)", why.c_str());
    }
    if (const char *what = plan_difference(c, &t))
        return set_err(FPM_ERR_INVAL, "fpm_set_crops: the new table changes %s this context was created with; "
                       "create a new context for it", what);
    // nothing in flight reads the tables or the band while they change
    HIP_TRY(hipStreamSynchronize(c->stream));
    const BandArgs from = band_of(c->st), to = band_of(t.st);
    const bool renumber = c->fused() && c->initialized &&
                          (from.bty0 != to.bty0 || from.btx0 != to.btx0 || from.nbx != to.nbx || from.nbt != to.nbt);
    if (renumber && (rc = remap_dirty_bits(c, from, to))) return rc;
    std::copy(t.x0.begin(), t.x0.end(), c->x0.begin());  // in place: c->prob points at them
    std::copy(t.y0.begin(), t.y0.end(), c->y0.begin());
    c->st.sy0 = t.st.sy0;
    c->st.sy1 = t.st.sy1;
    c->st.sx0 = t.st.sx0;
    c->st.sx1 = t.st.sx1;
    if (!upload_crops(c)) return set_err(FPM_ERR_DEVICE, "fpm_set_crops: table upload failed");
    c->drop_graphs();  // the general path's graphs hold the old windows: the next fpm_run captures again
    return FPM_OK;
}

int fpm_get_gains(const fpm_ctx *c, float *gain) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!gain) return set_err(FPM_ERR_INVAL, "fpm_get_gains: null gain");
    std::copy(c->gain.begin(), c->gain.end(), gain);
    return FPM_OK;
}

int fpm_set_gains(fpm_ctx *c, const float *gain) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    const size_t n = stack_images(c);
    // fp16 storage holds |objF| hscale <= max sqrt(I) <= 256 (fpm_state.hpp): a
    // gain multiplies the amplitude, so 256 g must stay below the largest half
    const bool fp16 = (c->prob.flags & FPM_FLAG_SPEC_FP16) != 0;
    for (size_t i = 0; gain && i < n; ++i) {
        const float g = gain[i];
        if (!std::isfinite(g) || !(g > 0.f))
            return set_err(FPM_ERR_INVAL, "fpm_set_gains: gain[%zu] (LED %zu, patch %zu) = %g is not finite and > 0", i,
                           i / c->st.B, i % c->st.B, (double)g);
        if (fp16 && !(256.0f * g < 65504.0f))
            return set_err(FPM_ERR_INVAL, "fpm_set_gains: gain[%zu] (LED %zu, patch %zu) = %g: under FPM_FLAG_SPEC_FP16 "
                           "256 g must stay below 65504", i, i / c->st.B, i % c->st.B, (double)g);
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_set_gains");
    if (rc) return rc;
    // nothing in flight reads the table while it changes.  Its address stays, and
    // every kernel (a captured graph's included) loads its gain from it at run
    // time, so the general path's graphs stay valid while the table keeps its kind
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float> g(n, 1.0f);
    if (gain) g.assign(gain, gain + n);
    if (!put(c->gain_dev, g)) return set_err(FPM_ERR_DEVICE, "fpm_set_gains: table upload failed");
    c->gain.swap(g);
    const bool unit = std::all_of(c->gain.begin(), c->gain.end(), [](float v) { return v == 1.0f; });
    // the general path's graphs hold the update kernels of the other kind: the next fpm_run captures again
    if (unit != c->gains_unit) c->drop_graphs();
    c->gains_unit = unit;
    return FPM_OK;
}

int fpm_set_stream(fpm_ctx *c, void *s) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return FPM_OK;
}

// ---- the planner's read-backs (include/fpm_hip_debug.h) ----------------------------
static fpm_ladder_kernel ladder_kernel(const StepKernel &k, int e, int cw, size_t lds_static) {
    fpm_ladder_kernel o;
    o.generation = cw ? FPM_LADDER_WAVE : e ? FPM_LADDER_TILED : FPM_LADDER_ONE_SEQ;
    o.tile = cw ? cw : e ? k.arg : 0;
    o.threads = (int)k.block.x;
    o.e = cw ? kWaveElems : e;
    o.grid_x = (int)k.grid.x;
    o.grid_y = (int)k.grid.y;
    o.lds_dynamic = (int)k.lds;
    o.lds_static = (int)lds_static;
    return o;
}

int fpm_debug_plan_ladder(int np, int nb, int B, int step, int no_wave_cols, int one_seq, fpm_ladder *out) {
    if (!out || np < 2 || nb < 1 || nb > np || B < 1) return set_err(FPM_ERR_INVAL, "fpm_debug_plan_ladder: bad argument");
    FftPlan pl;
    if (!make_plan(np, &pl)) return set_err(FPM_ERR_INVAL, "Np=%d is not 2^a 3^b 5^c", np);
    Switches sw{};
    sw.no_wave_cols = no_wave_cols != 0;
    sw.one_seq = sw.res_one_seq = one_seq != 0;
    DevState st{};
    st.np = np;
    st.nb = nb;
    st.B = B;
    StepKernel rows, cols, cols_gain, cols_mom, cols_pred;
    LdsLadder l;
    size_t row_static;
    if (step) {
        const GeneralPlan p = plan_general_step(st, GeneralPlan::Lds, pl, sw);
        l = p.ladder, rows = p.k1, cols = p.k2;
        row_static = std::max(p.k1.lds_static, p.k3.lds_static);
    } else {
        l = plan_lds_ladder(pl, np, nb, B, sw, false);
        residual_lds_kernels(l, rows, cols, cols_gain, cols_mom, cols_pred);
        row_static = rows.lds_static;
    }
    out->rows = ladder_kernel(rows, l.row_e, 0, row_static);
    out->cols = ladder_kernel(cols, l.col_e, l.cw, cols.lds_static);
    return FPM_OK;
}

static void fill_objcrop_plan(const ObjcropPlan &p, fpm_objcrop_plan *out) {
    out->kind = p.regs() ? (p.kind == ObjcropPlan::Regs256M ? FPM_OBJCROP_REGS_256M
                            : p.kind == ObjcropPlan::Regs600 ? FPM_OBJCROP_REGS_600 : FPM_OBJCROP_REGS_360)
                : p.kind == ObjcropPlan::SixStep4k ? FPM_OBJCROP_SIX_STEP_4K : FPM_OBJCROP_BATCHED;
    out->per_block = p.first().arg;
    out->rows_lds_dynamic = (int)p.rows.lds;
    out->rows_lds_static = (int)p.rows.lds_static;
    out->cols_lds_dynamic = (int)p.cols.lds;
    out->cols_lds_static = (int)p.cols.lds_static;
}

int fpm_debug_plan_objcrop(int nlarge, int fp16, int no_crop4k, fpm_objcrop_plan *out) {
    if (!out || nlarge < 4 || (nlarge & 1)) return set_err(FPM_ERR_INVAL, "fpm_debug_plan_objcrop: bad argument");
    FftPlan pl;
    if (!make_plan(nlarge, &pl)) return set_err(FPM_ERR_INVAL, "Nlarge=%d is not 2^a 3^b 5^c", nlarge);
    if (nlarge > fft_max_len())  // as validate()
        return set_err(FPM_ERR_INVAL, "Nlarge=%d exceeds the batched transform limit %d", nlarge, fft_max_len());
    Switches sw{};
    sw.no_crop4k = no_crop4k != 0;
    fill_objcrop_plan(plan_objcrop(nlarge, fp16 != 0, pl, sw), out);
    return FPM_OK;
}

int fpm_debug_get_objcrop_plan(const fpm_ctx *c, fpm_objcrop_plan *out) {
    if (!c || !out) return set_err(FPM_ERR_INVAL, "null argument");
    fill_objcrop_plan(c->oplan, out);
    return FPM_OK;
}

// the kLds constant of a planned kernel against the __shared__ bytes its code object declares
static int static_lds_matches(const StepKernel &k) {
    hipFuncAttributes a;
    HIP_TRY(hipFuncGetAttributes(&a, k.fn));
    if (a.sharedSizeBytes != k.lds_static)
        return set_err(FPM_ERR_STATE, "a kernel declares %zu B of static LDS, its constant says %zu",
                       (size_t)a.sharedSizeBytes, k.lds_static);
    return FPM_OK;
}

int fpm_debug_get_ladder(const fpm_ctx *c, int residual, fpm_ladder *out) {
    if (!c || !out) return set_err(FPM_ERR_INVAL, "null argument");
    if (c->fused() || c->general_kind != GeneralPlan::Lds)
        return set_err(FPM_ERR_INVAL, "the LED step of this context does not run the LDS kernel ladder");
    if (residual) {
        const ResidualPlan &p = c->rplan;
        if (p.kind != ResidualPlan::Lds) return set_err(FPM_ERR_INVAL, "the residual sweep runs the register pair");
        HIP_TRY(hipSetDevice(c->device));
        int rc = static_lds_matches(p.rows);
        if (rc || (rc = static_lds_matches(p.cols)) || (rc = static_lds_matches(p.cols_gain)) ||
            (rc = static_lds_matches(p.cols_mom)) || (rc = static_lds_matches(p.cols_pred)) ||
            (rc = static_lds_matches(p.cols_grad)) || (rc = static_lds_matches(p.grad_rows)))
            return rc;
        out->rows = ladder_kernel(p.rows, p.ladder.row_e, 0, p.rows.lds_static);
        out->cols = ladder_kernel(p.cols, p.ladder.col_e, p.ladder.cw, p.cols.lds_static);
        return FPM_OK;
    }
    const GeneralPlan &p = c->gplan[0];
    HIP_TRY(hipSetDevice(c->device));
    int rc = static_lds_matches(p.k1);
    if (rc || (rc = static_lds_matches(p.k2)) || (rc = static_lds_matches(p.k3)) ||
        (rc = static_lds_matches(p.k3_gain)))
        return rc;
    out->rows = ladder_kernel(p.k1, p.ladder.row_e, 0, std::max(p.k1.lds_static, p.k3.lds_static));
    out->cols = ladder_kernel(p.k2, p.ladder.col_e, p.ladder.cw, p.k2.lds_static);
    return FPM_OK;
}

}  // extern "C"
