// state.hip -- fpm_set_state / fpm_download_state_device: install a caller's
// spectrum and pupil as the solver state, with everything the LED-update
// kernels carry beside the two arrays (fpm_state.hpp: the centred layout, the
// fp16 storage scale, the pupil on its support box, tmax / tdirty / rmax /
// pmax), and the inverse copy.  The caller's layouts are fpm_download's:
// objF [B][L][L] un-centred, pupil [B][Np][Np] centred.
//
// Three steps, each its own launches:
//   check   one pass over each incoming array; the first offender in linear
//           order by a 64-bit atomicMin.  Nothing of the context is written.
//   place   un-centred <-> centred is (y + L/2) % L, (x + L/2) % L, its own
//           inverse for even L (fpm_create refuses an odd Nlarge): one kernel
//           template for both directions.  A thread moves V adjacent elements,
//           which stay adjacent inside a half-row: 16-byte accesses (V = 2)
//           where L/2 is even, 8-byte ones (V = 1) otherwise (L 90).
//   maxima  every tile of the live band from the stored spectrum with the step
//           kernels' cmag through spec_ld, so a rebuilt maximum has the bits a
//           run carries; tiles outside the band 0; no tile dirty.
#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

namespace {

constexpr int kStateThreads = 256;

__device__ __forceinline__ bool finite2(float2 v) { return isfinite(v.x) && isfinite(v.y); }

// lowest linear index among the offenders (vector atomic; the slot starts at ~0)
__device__ __forceinline__ void note_first(unsigned long long *slot, size_t i) {
    atomicMin(slot, (unsigned long long)i);
}

// Check of an un-centred spectrum src [B][L][L]: finite, exactly zero outside
// the live band, inside the fp16 range when the context stores fp16.  One
// element pair per thread (L is even, so a pair never leaves its row).
__global__ void __launch_bounds__(kStateThreads) k_state_check_spec(DevState st, const float2 *__restrict__ src,
                                                                   size_t npairs, unsigned long long *first) {
    const size_t p = (size_t)blockIdx.x * kStateThreads + threadIdx.x;
    if (p >= npairs) return;
    const int L = st.L, h = L / 2, rowp = L / 2;
    const size_t row = p / rowp;
    const int x0 = (int)(p - row * rowp) * 2;
    const int y = (int)(row % L);
    const int cy = y < h ? y + h : y - h;
    const bool row_live = cy >= st.sy0 && cy <= st.sy1;
    const float lim = 65504.0f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int x = x0 + k;
        const float2 v = src[2 * p + k];
        const int cx = x < h ? x + h : x - h;
        const bool live = row_live && cx >= st.sx0 && cx <= st.sx1;
        bool bad = !finite2(v) || (!live && (v.x != 0.f || v.y != 0.f));
        if (st.spec16) bad = bad || !(fabsf(v.x) * st.hscale < lim) || !(fabsf(v.y) * st.hscale < lim);
        if (bad) note_first(first, 2 * p + k);
    }
}

// max|P| as the context's LED-update kernels form it: the general path's
// kernels reduce cmag(p), the fused ones take one square root of the largest
// |p|^2 (sqrtf is monotone, so the root of each element reduces to the same bits)
__device__ __forceinline__ float pupil_mag(float2 p, bool fused) { return fused ? sqrtf(cabs2(p)) : cmag(p); }

// Check of a centred pupil src [B or 1][Np][Np] on the support disk, and the
// per-patch max|P S| into pm [B] (zeroed before).  grid (nb, B)
__global__ void __launch_bounds__(kStateThreads) k_state_check_pupil(DevState st, const float2 *__restrict__ src,
                                                                    int shared, int fused,
                                                                    unsigned long long *first, float *pm) {
    __shared__ float red[kStateThreads / 64];
    const int row = blockIdx.x, b = blockIdx.y, np = st.np, nb = st.nb, r = st.r;
    const int sb = shared ? 0 : b;
    const size_t base = ((size_t)sb * np + (np / 2 + row - r)) * np + np / 2 - r;
    float m = 0.f;
    for (int j = threadIdx.x; j < nb; j += kStateThreads) {
        if (!st.disk[row * nb + j]) continue;
        const float2 v = src[base + j];
        if (!finite2(v)) note_first(first, base + j);
        else m = fmaxf(m, pupil_mag(v, fused));
    }
    m = block_max_nonneg(m, red);
    // non-negative floats order as their bit patterns
    if (threadIdx.x == 0 && m > 0.f) atomicMax((unsigned *)pm + b, __float_as_uint(m));
}

// The shift between the caller's un-centred spectrum ext [B][L][L] and the
// context's centred one.  SET: ext -> spec through spec_st's rounding;
// otherwise spec -> ext through spec_ld's widening.  V elements per thread.
template <int V, bool SET>
__global__ void __launch_bounds__(kStateThreads) k_state_shift(DevState st, float2 *__restrict__ ext, size_t nvec) {
    const size_t v = (size_t)blockIdx.x * kStateThreads + threadIdx.x;
    if (v >= nvec) return;
    const int L = st.L, h = L / 2, rowv = L / V;
    const size_t row = v / rowv;
    const int x = (int)(v - row * rowv) * V;
    const int b = (int)(row / L), y = (int)(row - (size_t)b * L);
    const int cy = y < h ? y + h : y - h, cx = x < h ? x + h : x - h;
    const size_t e = v * V, ci = (size_t)cy * L + cx;
    if constexpr (V == 2) {
        if (!st.spec16) {  // uniform: fp32 storage moves 16 bytes as they are
            float4 *in = reinterpret_cast<float4 *>(st.spec + (size_t)b * L * L + ci);
            float4 *out = reinterpret_cast<float4 *>(ext + e);
            if constexpr (SET) *in = *out;
            else *out = *in;
            return;
        }
        if constexpr (SET) {
            const float4 q = *reinterpret_cast<const float4 *>(ext + e);
            spec_st(st, b, ci, make_float2(q.x, q.y));
            spec_st(st, b, ci + 1, make_float2(q.z, q.w));
        } else {
            const float2 u = spec_ld(st, b, ci), w = spec_ld(st, b, ci + 1);
            *reinterpret_cast<float4 *>(ext + e) = make_float4(u.x, u.y, w.x, w.y);
        }
    } else {
        if constexpr (SET) spec_st(st, b, ci, ext[e]);
        else ext[e] = spec_ld(st, b, ci);
    }
}

// Tile maxima of the stored spectrum: the tiles of the live band's tile
// rectangle (what the fused kernels index their dirty bits by, tilemax.hpp)
// from their pixels, every other tile 0 without a read.  grid (ntx nty, B)
__global__ void __launch_bounds__(kStateThreads) k_state_tile_max(DevState st) {
    __shared__ float red[kStateThreads / 64];
    const int t = blockIdx.x, b = blockIdx.y, L = st.L;
    const int ty = t / st.ntx, tx = t % st.ntx;
    float *out = st.tmax + (size_t)b * st.nty * st.ntx + t;
    if (ty < st.sy0 / kTile || ty > st.sy1 / kTile || tx < st.sx0 / kTile || tx > st.sx1 / kTile) {
        if (threadIdx.x == 0) *out = 0.f;  // block-uniform
        return;
    }
    const int y = ty * kTile + (threadIdx.x >> 4), x = tx * kTile + (threadIdx.x & 15);
    float m = 0.f;
    if (y < L && x < L) m = cmag(spec_ld(st, b, (size_t)y * L + x));
    m = block_max_nonneg(m, red);
    if (threadIdx.x == 0) *out = m;
}

// Pupil in: centred src [B or 1][Np][Np] times the support disk onto the
// box; pmax[b][0] = pm[b], the other partials 0.  grid (nb, B)
__global__ void __launch_bounds__(kStateThreads) k_state_pupil_in(DevState st, const float2 *__restrict__ src,
                                                                 int shared, const float *__restrict__ pm) {
    const int row = blockIdx.x, b = blockIdx.y, np = st.np, nb = st.nb, r = st.r;
    const int sb = shared ? 0 : b;
    const size_t base = ((size_t)sb * np + (np / 2 + row - r)) * np + np / 2 - r;
    float2 *pup = st.pupil + ((size_t)b * nb + row) * nb;
    for (int j = threadIdx.x; j < nb; j += kStateThreads)
        pup[j] = st.disk[row * nb + j] ? src[base + j] : make_float2(0.f, 0.f);
    if (row == 0)
        for (int i = threadIdx.x; i < st.npart; i += kStateThreads) st.pmax[(size_t)b * st.npart + i] = i ? 0.f : pm[b];
}

// Pupil out: the box into the centred dst [B][Np][Np], zero around it.  grid (Np, B)
__global__ void __launch_bounds__(kStateThreads) k_state_pupil_out(DevState st, float2 *__restrict__ dst) {
    const int y = blockIdx.x, b = blockIdx.y, np = st.np, nb = st.nb, r = st.r;
    const int i = y - (np / 2 - r);
    const bool row_in = i >= 0 && i < nb;  // block-uniform
    const float2 *pup = st.pupil + ((size_t)b * nb + (row_in ? i : 0)) * nb;
    float2 *o = dst + ((size_t)b * np + y) * np;
    for (int x = threadIdx.x; x < np; x += kStateThreads) {
        const int j = x - (np / 2 - r);
        o[x] = (row_in && j >= 0 && j < nb) ? pup[j] : make_float2(0.f, 0.f);
    }
}

inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + kStateThreads - 1) / kStateThreads)); }

template <bool SET>
void launch_shift(const DevState &st, float2 *ext, hipStream_t s) {
    const size_t n = (size_t)st.B * st.L * st.L;
    // 16-byte accesses need an even half-row and a 16-byte aligned caller array
    if ((st.L / 2) % 2 == 0 && ((uintptr_t)ext & 15) == 0)
        hipLaunchKernelGGL((k_state_shift<2, SET>), blocks_for(n / 2), dim3(kStateThreads), 0, s, st, ext, n / 2);
    else
        hipLaunchKernelGGL((k_state_shift<1, SET>), blocks_for(n), dim3(kStateThreads), 0, s, st, ext, n);
}

}  // namespace

hipError_t launch_state_check(const DevState &st, const float2 *objF, const float2 *pupil, bool pupil_shared,
                              bool fused, StateCheck *chk, hipStream_t s) {
    hipError_t e = hipMemsetAsync(chk->first, 0xFF, sizeof chk->first, s);
    if (e != hipSuccess) return e;
    if (objF) {
        const size_t npairs = (size_t)st.B * st.L * st.L / 2;
        hipLaunchKernelGGL(k_state_check_spec, blocks_for(npairs), dim3(kStateThreads), 0, s, st, objF, npairs,
                           &chk->first[0]);
    }
    if (pupil) {
        e = hipMemsetAsync(state_check_pmax(chk), 0, (size_t)st.B * sizeof(float), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_state_check_pupil, dim3(st.nb, st.B), dim3(kStateThreads), 0, s, st, pupil,
                           (int)pupil_shared, (int)fused, &chk->first[1], state_check_pmax(chk));
    }
    return hipGetLastError();
}

hipError_t launch_state_place(const DevState &st, const float2 *objF, const float2 *pupil, bool pupil_shared,
                              const StateCheck *chk, hipStream_t s) {
    if (objF) {
        launch_shift<true>(st, const_cast<float2 *>(objF), s);
        hipLaunchKernelGGL(k_state_tile_max, dim3(st.ntx * st.nty, st.B), dim3(kStateThreads), 0, s, st);
        hipError_t e =
            hipMemsetAsync(st.tdirty, 0, (size_t)st.B * ((st.ntx * st.nty + 31) / 32) * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        if (st.rmax && (e = launch_row_max_all(st, s)) != hipSuccess) return e;
    }
    if (pupil)
        hipLaunchKernelGGL(k_state_pupil_in, dim3(st.nb, st.B), dim3(kStateThreads), 0, s, st, pupil,
                           (int)pupil_shared, (const float *)state_check_pmax(const_cast<StateCheck *>(chk)));
    return hipGetLastError();
}

hipError_t launch_state_out(const DevState &st, float2 *objF, float2 *pupil, hipStream_t s) {
    if (objF) launch_shift<false>(st, objF, s);
    if (pupil) hipLaunchKernelGGL(k_state_pupil_out, dim3(st.np, st.B), dim3(kStateThreads), 0, s, st, pupil);
    return hipGetLastError();
}

}  // namespace fpm
