// run.cpp -- fpm_init and fpm_run: the itrCount x ledUsedCount update loop
// and the per-iteration objCrop IDFT (fpmMain.cpp:345-482), as a sequence of
// steps: refuse a capturing stream, launch the iterations between timing
// events, read back the abort word, the event times, the stamps and the clock
// probe.  The general path's patch groups and captured graphs live here too.
#include <cstdio>

#include "ctx.hpp"

using namespace fpm;

int fpm::refresh_objcrop(fpm_ctx *c) {
    HIP_TRY(launch_objcrop(c->oplan, c->st, c->objcrop, c->tw_L, c->stream));
    c->objcrop_valid = true;
    return FPM_OK;
}

int fpm::refuse_capture(const fpm_ctx *c, const char *what) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(c->stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return set_err(FPM_ERR_INVAL, "%s on a capturing stream: %s is blocking and its %s cannot be "
                       "replayed from a graph (fpm_hip.h)",
                       what, what, c->split_ks > 1 ? "co-resident grids" : "launches");
    return FPM_OK;
}

namespace {

// ---- general path: patch groups ------------------------------------------------
// stream of group g when the run stream is s (group 0 runs on s itself)
hipStream_t group_stream(const fpm_ctx *c, int g, hipStream_t s) { return g == 0 ? s : c->gstream[g]; }

// fork the group streams from s / join them back to s
hipError_t fork_groups(fpm_ctx *c, hipStream_t s) {
    if (c->ngroups < 2) return hipSuccess;
    HIP_RET(hipEventRecord(c->gfork, s));
    for (int g = 1; g < c->ngroups; ++g) HIP_RET(hipStreamWaitEvent(c->gstream[g], c->gfork, 0));
    return hipSuccess;
}
hipError_t join_groups(fpm_ctx *c, hipStream_t s) {
    for (int g = 1; g < c->ngroups; ++g) {
        HIP_RET(hipEventRecord(c->gjoin[g], c->gstream[g]));
        HIP_RET(hipStreamWaitEvent(s, c->gjoin[g], 0));
    }
    return hipSuccess;
}

// The LED chains of one iteration of groups [g0, g1), each on its group's
// stream: issued LED by LED across the groups, so that with direct launches
// no group's queue runs ahead
hipError_t launch_led_chains(const fpm_ctx *c, int g0, int g1, hipStream_t s) {
    DevState view[fpm_ctx::kMaxGroups];
    for (int g = g0; g < g1; ++g) view[g] = group_view(c, g);
    for (int i = 0; i < c->prob.n_order; ++i) {
        const int led = c->order[i];
        for (int g = g0; g < g1; ++g)
            HIP_RET(launch_general_step(c->gplan[g], view[g], led, c->x0[led], c->y0[led], c->tw_np, i == 0,
                                        !c->gains_unit, group_stream(c, g, s)));
    }
    // Np 1024 / 256 register kernels: the last LED's pupil commit (the others
    // are folded into the next LED's row IDFT)
    for (int g = g0; g < g1; ++g)
        if (c->gplan[g].commit_folded()) HIP_RET(launch_pupil_commit(view[g], group_stream(c, g, s)));
    return hipSuccess;
}

// The general path issues four launches per LED (~1200 per iteration at 293
// LEDs); every argument is fixed once the context exists, so each group's
// chain of one iteration is captured once (on its own stream) and replayed:
// one graph launch per group per iteration, the groups' graphs on forked streams.
int general_graph(fpm_ctx *c) {
    if (c->led_graph_exec[0]) return FPM_OK;
    for (int g = 0; g < c->ngroups; ++g) {
        hipStream_t cs = group_stream(c, g, c->own_stream);
        HIP_TRY(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        hipError_t e = launch_led_chains(c, g, g + 1, c->own_stream);
        const hipError_t e2 = hipStreamEndCapture(cs, &c->led_graph[g]);
        if (e == hipSuccess) e = e2;
        if (e == hipSuccess) e = hipGraphInstantiate(&c->led_graph_exec[g], c->led_graph[g], nullptr, nullptr, 0);
        if (e != hipSuccess) {
            c->led_graph_exec[g] = nullptr;
            c->drop_graphs();
            return set_err(FPM_ERR_DEVICE, "general-path graph capture: %s", hipGetErrorString(e));
        }
    }
    return FPM_OK;
}

// one iteration of the general path on s: the groups' graphs, or their direct launches
hipError_t launch_general_iteration(fpm_ctx *c, bool use_graph, hipStream_t s) {
    HIP_RET(fork_groups(c, s));
    if (use_graph)
        for (int g = 0; g < c->ngroups; ++g) HIP_RET(hipGraphLaunch(c->led_graph_exec[g], group_stream(c, g, s)));
    else
        HIP_RET(launch_led_chains(c, 0, c->ngroups, s));
    return join_groups(c, s);
}

// ---- the steps of fpm_run ------------------------------------------------------
int grow_event_pool(fpm_ctx *c, size_t need) {
    while (c->evpool.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->evpool.push_back(e);
    }
    return FPM_OK;
}

// all LED updates of one iteration with the context's kernel
int launch_iteration(fpm_ctx *c, const FusedLaunch &in, bool use_graph) {
    switch (c->kernel) {
    case Kernel::Np90: HIP_TRY(launch_fused_s90_iteration(c->st, in, c->stream)); break;
    case Kernel::Small: HIP_TRY(launch_fused_small_iteration(c->st, in, c->pl_np, c->stream)); break;
    case Kernel::Np200: HIP_TRY(launch_fused_mr_iteration(c->st, in, c->stream)); break;
    case Kernel::Np256Dist:
        HIP_TRY(launch_fused_dist(c->st, in, c->split_ks, c->xch, c->split_flags, c->stall_led, c->dist_tags,
                                  c->stream));
        c->dist_tags = (c->dist_tags + (unsigned)c->prob.n_order) & 0x7fffffffu;
        break;
    case Kernel::Np256:
        HIP_TRY(launch_fused_iteration(c->st, in, c->split_ks, c->xch, c->split_flags, c->stall_led, c->stream));
        break;
    case Kernel::General: HIP_TRY(launch_general_iteration(c, use_graph, c->stream)); break;
    }
    return FPM_OK;
}

// A split-mode handoff that timed out in ANY iteration leaves the results
// undefined: the abort word is sticky across launches; report it, clear it,
// and require a fresh fpm_init before the next run
int check_abort_word(fpm_ctx *c) {
    if (!c->split_flags) return FPM_OK;
    int ab = 0;
    int *abw = c->split_flags + (size_t)c->split_ks * c->st.B;
    HIP_TRY(hipMemcpy(&ab, abw, sizeof(int), hipMemcpyDeviceToHost));
    if (!ab) return FPM_OK;
    HIP_TRY(hipMemset(abw, 0, sizeof(int)));
    c->initialized = false;
    c->objcrop_valid = false;
    return set_err(FPM_ERR_DEVICE,
                   "split-mode handoff between the %d workgroups of a patch timed out; results are "
                   "undefined, call fpm_init again", c->split_ks);
}

// ev[0] .. ev[3 iters + 1]: the run's first event, per iteration one before
// the LED updates, one after them and one after the objCrop IDFT, the run's last
int read_timing(fpm_ctx *c, int iters) {
    const hipEvent_t *ev = c->evpool.data();
    double led_ms = 0, crop_ms = 0;
    for (int it = 0; it < iters; ++it) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev[1 + 3 * it], ev[2 + 3 * it]));
        HIP_TRY(hipEventElapsedTime(&b, ev[2 + 3 * it], ev[3 + 3 * it]));
        led_ms += a;
        crop_ms += b;
    }
    float tot = 0;
    HIP_TRY(hipEventElapsedTime(&tot, ev[0], ev[3 * iters + 1]));
    fpm_timing &t = c->timing;
    t.run_ms = tot;
    t.led_ms = led_ms;
    t.objcrop_ms = crop_ms;
    t.led_launches = c->fused() ? iters : iters * c->prob.n_order;
    t.led_launch_ms = t.led_launches ? led_ms / t.led_launches : 0.0;
    return FPM_OK;
}

// FPM_STAMPS=1: the fused kernel's phase cycles of this run to stderr, and cleared
int print_stamps(fpm_ctx *c, int iters) {
    if (!c->dbg) return FPM_OK;
    unsigned long long h[2 * kStamps];
    HIP_TRY(hipMemcpy(h, c->dbg, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->dbg, 0, sizeof h));
    const double steps = (double)iters * c->prob.n_order * c->st.B;
    const char *const *names = c->row().stamps;
    for (int v = 0; v < 2; ++v) {
        fprintf(stderr, "[fpm stamps] cycles per LED step (%s wave view, mean over blocks):", v ? "last" : "first");
        for (int i = 0; i < kStamps; ++i) fprintf(stderr, " %s=%.0f", names[i], h[v * kStamps + i] / steps);
        fprintf(stderr, "\n");
    }
    return FPM_OK;
}

// the fused kernels' clock probe of this run (fpm_get_clock)
int read_clock(fpm_ctx *c) {
    if (!c->clk) return FPM_OK;
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(h, c->clk, sizeof h, hipMemcpyDeviceToHost));
    int khz = 0;  // s_memrealtime rate
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0)
        khz = 100000;
    if (h[2] > 0 && h[1] > 0) {
        const double sec = (double)h[1] / (khz * 1e3);
        c->clock.clock_mhz = (double)h[0] / sec / 1e6;
        c->clock.cycles_per_launch = (double)h[0] / (double)h[2];
        c->clock.ms_per_launch = sec * 1e3 / (double)h[2];
        c->clock.launches = (int32_t)h[2];
    }
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_init(fpm_ctx *c) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!c->uploaded) return set_err(FPM_ERR_STATE, "fpm_init before fpm_upload_stack");
    HIP_TRY(hipSetDevice(c->device));
    const int init_led = c->order[c->prob.init_pos];
    HIP_TRY(launch_init(c->st, init_led, c->objcrop, c->pl_np, c->tw_np, c->stream));
    c->initialized = true;
    c->objcrop_valid = false;
    return FPM_OK;
}

int fpm_run(fpm_ctx *c, int iters) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    if (!c->initialized) return set_err(FPM_ERR_STATE, "fpm_run before fpm_init");
    // initialized used to imply uploaded (fpm_init was the only way in); fpm_set_state
    // installs a state on a context without a stack, which has nothing to run on
    if (!c->uploaded)
        return set_err(FPM_ERR_STATE, "fpm_run: the state came from fpm_set_state and no stack is uploaded "
                       "(fpm_upload_stack, then fpm_set_state again or fpm_init)");
    if (iters < 0) return set_err(FPM_ERR_INVAL, "iters=%d", iters);
    // a run that is refused or fails below reports zeros, not the previous run's values
    c->clock = fpm_clock{};
    c->timing = fpm_timing{};
    HIP_TRY(hipSetDevice(c->device));
    int rc = refuse_capture(c, "fpm_run");
    if (rc) return rc;
    if (c->clk) HIP_TRY(hipMemsetAsync(c->clk, 0, 3 * sizeof(unsigned long long), c->stream));
    // one event pair per iteration around the LED-update launches, one pair
    // around the objCrop IDFT; read back once at the end (fpm_run is blocking)
    const size_t need = 3 * (size_t)iters + 2;
    if ((rc = grow_event_pool(c, need))) return rc;
    const bool use_graph = !c->fused() && iters > 0 && !c->sw.no_graph;
    if (use_graph && (rc = general_graph(c))) return rc;
    const bool last_only = (c->prob.flags & FPM_FLAG_OBJCROP_LAST_ONLY) != 0;
    const FusedLaunch in{c->meas, c->order_dev, c->x0_dev, c->y0_dev, c->prob.n_order, c->tw_np, c->dbg,
                         c->kernel == Kernel::Np90 ? c->sw.s90_dense : c->sw.mr_dense, c->sw.no_ledtab,
                         !c->gains_unit};
    const hipEvent_t *ev = c->evpool.data();
    HIP_TRY(hipEventRecord(ev[0], c->stream));
    for (int it = 0; it < iters; ++it) {
        HIP_TRY(hipEventRecord(ev[1 + 3 * it], c->stream));
        if ((rc = launch_iteration(c, in, use_graph))) return rc;
        HIP_TRY(hipEventRecord(ev[2 + 3 * it], c->stream));
        if ((!last_only || it == iters - 1) && (rc = refresh_objcrop(c))) return rc;
        HIP_TRY(hipEventRecord(ev[3 + 3 * it], c->stream));
    }
    HIP_TRY(hipEventRecord(ev[need - 1], c->stream));
    HIP_TRY(hipEventSynchronize(ev[need - 1]));
    if ((rc = check_abort_word(c)) || (rc = read_timing(c, iters)) || (rc = print_stamps(c, iters))) return rc;
    return read_clock(c);
}

int fpm_synchronize(fpm_ctx *c) {
    if (!c) return set_err(FPM_ERR_INVAL, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FPM_OK;
}

}  // extern "C"
