// init.hip -- fpm_init: the pupil / spectrum initialisation of
// fpmMain.cpp:302-343 and the tile / row maxima of the fresh spectrum.
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

// sqrt of the init image as complex, fpmMain.cpp:319-322. grid (Np, B)
// meas in either layout (DevState::meas_g)
__global__ void k_init_amp(const uint16_t *__restrict__ meas, const float *__restrict__ gain,
                           float2 *__restrict__ out, int np, int B, int led, size_t out_bs, int g) {
    const int y = blockIdx.x, b = blockIdx.y;
    const float gl = gain[(size_t)led * B + b];  // the measured amplitude is g sqrt(I) (fpm_set_gains)
    const uint16_t *I = meas + ((size_t)led * B + b) * np * np;
    float2 *o = out + (size_t)b * out_bs + (size_t)y * np;
    const int col = g ? (y % g) * (np / g) + y / g : 0;  // position of row y inside a stored column
    for (int x = threadIdx.x; x < np; x += blockDim.x) {
        const uint16_t v = g ? I[(size_t)x * np + col] : I[(size_t)y * np + x];
        o[x] = make_float2(gl * sqrtf((float)v), 0.f);
    }
}

// zero the spectrum, place fftShift(fft2(A) * S) at the centre
// (fpmMain.cpp:326-343), P = S, max|P| = 1.  grid (nb, B)
__global__ void k_init_place(DevState st, const float2 *__restrict__ F, size_t f_bs) {
    const int row = blockIdx.x, b = blockIdx.y;
    const int np = st.np, r = st.r, nb = st.nb, L = st.L;
    const int ky = row - r;
    float2 *pup = st.pupil + (size_t)b * nb * nb;
    const float2 *f = F + (size_t)b * f_bs;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) {
        const int kx = j - r;
        const bool in = st.disk[row * nb + j];
        if (in)
            spec_st(st, b, (size_t)(L / 2 + ky) * L + L / 2 + kx, f[(size_t)((ky + np) % np) * np + (kx + np) % np]);
        pup[row * nb + j] = make_float2(in ? 1.f : 0.f, 0.f);
    }
    // max|P0| = 1 (partial maxima other than part 0 were zeroed by launch_init)
    if (row == 0 && threadIdx.x == 0) st.pmax[b * st.npart] = (st.disk[r * nb + r] ? 1.f : 0.f);
}

// tile maxima of |spec| after k_init_place. grid (ntx*nty, B), block 256.
// The spectrum was just zeroed except the init box [L/2 - r, L/2 + r]^2, so a
// tile outside it is 0 without reading it (init read the whole spectrum
// again: 1.2 GB at the metric config)
__global__ void __launch_bounds__(256) k_tile_max_all(DevState st) {
    __shared__ float red[8];
    const int t = blockIdx.x, b = blockIdx.y, L = st.L;
    const int ty = t / st.ntx, tx = t % st.ntx;
    const int lo = L / 2 - st.r, hi = L / 2 + st.r;
    if (ty * kTile > hi || ty * kTile + kTile - 1 < lo || tx * kTile > hi || tx * kTile + kTile - 1 < lo) {
        if (threadIdx.x == 0) st.tmax[(size_t)b * st.nty * st.ntx + t] = 0.f;  // block-uniform
        return;
    }
    const int y = ty * kTile + (threadIdx.x >> 4), x = tx * kTile + (threadIdx.x & 15);
    float m = 0.f;
    if (y < L && x < L) m = cmag(spec_ld(st, b, (size_t)y * L + x));
    m = block_max_nonneg(m, red);
    if (threadIdx.x == 0) st.tmax[(size_t)b * st.nty * st.ntx + t] = m;
}

// row maxima of the tile maxima after init (general path). grid (nty, B)
__global__ void __launch_bounds__(256) k_row_max_all(DevState st) {
    __shared__ float red[4];
    const int ty = blockIdx.x, b = blockIdx.y;
    const float *tm = st.tmax + ((size_t)b * st.nty + ty) * st.ntx;
    float m = 0.f;
    for (int i = threadIdx.x; i < st.ntx; i += 256) m = fmaxf(m, tm[i]);
    m = block_max_nonneg(m, red);
    if (threadIdx.x == 0) st.rmax[(size_t)b * st.nty + ty] = m;
}

hipError_t launch_row_max_all(const DevState &st, hipStream_t s) {
    hipLaunchKernelGGL(k_row_max_all, dim3(st.nty, st.B), dim3(256), 0, s, st);
    return hipGetLastError();
}

hipError_t launch_init(const DevState &st, int init_led, float2 *scratch, const FftPlan &pl_np,
                       const float2 *tw_np, hipStream_t s) {
    const int np = st.np;
    const size_t bs = (size_t)np * np;
    hipLaunchKernelGGL(k_init_amp, dim3(np, st.B), dim3(256), 0, s, st.meas, st.gain, scratch, np, st.B, init_led, bs,
                       st.meas_g);
    // fft2: rows then columns, in place (fpmMain.cpp:325)
    hipError_t e = launch_fft_batch(false, scratch, scratch, pl_np, tw_np, np, st.B, bs, np, 1, bs, np, 1, 0, 0,
                                    1.f, s);
    if (e != hipSuccess) return e;
    e = launch_fft_batch(false, scratch, scratch, pl_np, tw_np, np, st.B, bs, 1, np, bs, 1, np, 0, 0, 1.f, s);
    if (e != hipSuccess) return e;
    e = st.spec16 ? hipMemsetAsync(st.spec16, 0, (size_t)st.B * st.L * st.L * sizeof(__half2), s)
                  : hipMemsetAsync(st.spec, 0, (size_t)st.B * st.L * st.L * sizeof(float2), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(st.pmax, 0, (size_t)st.B * st.npart * sizeof(float), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_init_place, dim3(st.nb, st.B), dim3(256), 0, s, st, (const float2 *)scratch, bs);
    hipLaunchKernelGGL(k_tile_max_all, dim3(st.ntx * st.nty, st.B), dim3(256), 0, s, st);
    if (st.rmax) hipLaunchKernelGGL(k_row_max_all, dim3(st.nty, st.B), dim3(256), 0, s, st);
    e = hipMemsetAsync(st.tdirty, 0, (size_t)st.B * ((st.ntx * st.nty + 31) / 32) * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace fpm
