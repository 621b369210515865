// coresident.cpp -- the process-wide ordering of co-resident grids
// (fused_sync.hpp launch_coresident), used by the launchers of the split and
// distributed modes (fpm_fused.hip, fused_dist.hip).
#include <hip/hip_runtime.h>

#include <mutex>

#include "fused_sync.hpp"

namespace fpm {
// Co-resident grids (split / distributed modes, fused_sync.hpp): the
// occupancy check, then a plain launch ordered after the previous co-resident
// grid of this process on the same device (another context, another stream),
// so two grids that each need every block resident never share the device.
// A capturing stream is refused (hipErrorStreamCaptureUnsupported): an event
// recorded outside the capture cannot be waited on inside it, so a replayed
// graph would carry no such order (fpm_run refuses capture before this).
// Only co-resident grids are ordered against each other; other kernels on
// other streams may still hold CUs, and then the waits' ~1 s timeout reports
// the launch.
hipError_t launch_coresident_raw(const void *fn, int grid, int block, size_t lds, void **args, hipStream_t s) {
    int dev = 0, n_cu = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, lds);
    if (e != hipSuccess) return e;
    if ((long long)per_cu * n_cu < grid) return hipErrorCooperativeLaunchTooLarge;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if ((e = hipStreamIsCapturing(s, &cap)) != hipSuccess) return e;
    if (cap != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
    constexpr int kMaxDev = 64;
    struct Serial {
        std::mutex mu;
        hipEvent_t last = nullptr;  // completion of the device's latest co-resident grid
    };
    static Serial serial[kMaxDev];
    if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
    Serial &sd = serial[dev];
    std::lock_guard<std::mutex> lk(sd.mu);
    if (!sd.last && (e = hipEventCreateWithFlags(&sd.last, hipEventDisableTiming)) != hipSuccess) {
        sd.last = nullptr;
        return e;
    }
    // an event never recorded counts as complete, so the first wait is free
    if ((e = hipStreamWaitEvent(s, sd.last, 0)) != hipSuccess) return e;
    if ((e = hipLaunchKernel(fn, dim3(grid), dim3(block), args, lds, s)) != hipSuccess) return e;
    if (hipEventRecord(sd.last, s) != hipSuccess) {
        // the grid is running but the next co-resident grid could not be
        // ordered after it: drain the stream here instead (the event, never
        // re-recorded, still reads complete), so the launch itself succeeds
        (void)hipStreamSynchronize(s);
    }
    return hipSuccess;
}
}  // namespace fpm
