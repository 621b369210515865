// fused_host.hpp -- host side shared by the launchers of the five fused
// LED-update kernels (fpm_fused.hip, fused_dist.hip, fused_mr.hip,
// fused_s90.hip, fused_small.hip): the LDS capacity, the live band as band
// tiles, the per-launch inputs every launcher takes, and the launch itself.
#pragma once
#include <hip/hip_runtime.h>

#include "fpm_state.hpp"
#include "tilemax.hpp"

namespace fpm {

constexpr size_t kLdsCap = 160 * 1024;  // LDS of a gfx950 workgroup (bytes)

// the live band of the centred spectrum (fpm_state.hpp) lies inside it
inline bool band_valid(const DevState &st) {
    return !(st.sy0 < 0 || st.sy1 >= st.L || st.sy0 > st.sy1 || st.sx0 < 0 || st.sx1 >= st.L || st.sx0 > st.sx1);
}

// band-tile rectangle of the live band (tilemax.hpp)
inline BandArgs band_of(const DevState &st) {
    BandArgs b;
    b.bty0 = st.sy0 / kTile;
    b.btx0 = st.sx0 / kTile;
    b.nbx = st.sx1 / kTile - b.btx0 + 1;
    b.nbt = b.nbx * (st.sy1 / kTile - b.bty0 + 1);
    b.rnbx = 1.0f / (float)b.nbx;
    return b;
}

// what every fused launcher gets from the context besides the DevState
struct FusedLaunch {
    const uint16_t *meas;    // the stack in the kernel's column layout (meas_layout)
    const int *order, *x0, *y0;
    int n_order;
    const float2 *tw;        // exp(-2 pi i k / Np), k < Np
    unsigned long long *dbg; // FPM_STAMPS=1 phase cycles, else null
    bool dense;              // FPM_S90_DENSE=1 / FPM_MR_DENSE=1: the kernel's dense LDS layout
    bool no_ledtab;          // FPM_NO_LEDTAB=1: no LDS LED table, the global tables instead (ledtab.hpp)
    bool gains;              // some LED gain is not 1 (fpm_set_gains): the kernels' GAIN instances
};

// one workgroup-sized dynamic-LDS launch: raise the kernel's limit, launch,
// read the launch error
template <class Args>
inline hipError_t launch_lds(void (*fn)(Args), int grid, int block, size_t lds, Args *a, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    void *args[] = {a};
    (void)hipLaunchKernel((const void *)fn, dim3(grid), dim3(block), args, lds, s);
    return hipGetLastError();
}

}  // namespace fpm
