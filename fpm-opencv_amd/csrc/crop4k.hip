// crop4k.hip -- objCrop's six-step transform for L = 4096; crop4k_kernels at
// the end is this family's row of the objCrop plan (objcrop.hip).
#include <hip/hip_runtime.h>

#include "fft_lds.hpp"
#include "fpm_state.hpp"
#include "launch.hpp"

namespace fpm {

// ---- objCrop for L = 4096 (config 5) ----------------------------------------
// The batched transform (fft_batch.hip) fits only C = 2 sequences of 4096
// points in a block, so its column pass reads 16-byte column segments (the
// counters: 3x the pass's bytes, 3.6 ms per iteration at config 5).  Here the
// column IDFT runs first, straight from the (read-only) spectrum, as a six-step
// 4096 = 64 x 64 transform whose passes read and write 128-byte row segments
// of 16 adjacent columns; the row IDFT then runs in place, the same 64 x 64
// split inside a block per row (k_crop4k_rows).  With
// n = n1 + 64 n2 and k = k2 + 64 k1 (inverse, W = e^{+2 pi i / 4096}):
//   X[k2 + 64 k1] = sum_n1 W64^{n1 k1} [ W^{n1 k2} sum_n2 x[n1 + 64 n2] W64^{n2 k2} ]
//   pass 1 (block n1): the bracket for all k2, stored at row k2 + 64 n1
//   pass 2 (block k2): reads rows k2 + 64 n1, writes X at rows k2 + 64 k1 --
//                      the same rows, so it runs in place
namespace c4k {
constexpr int L = 4096, CW = 16, NT = 8 * CW;  // 16 columns x 8 lanes per block

// 64-point inverse DFT of the block's 16 columns, 8 lanes per column (8 x 8:
// DFT8 over the lane's values, W64 twiddles, LDS exchange, DFT8): lane (c, j)
// holds x[j + 8 b] in v[b] and returns X[j + 8 q] in v[q].  One barrier; lds
// is used once per launch.
__device__ __forceinline__ void idft64(float2 (&v)[8], float2 *lds, int c, int j, const float2 *__restrict__ tw) {
    dft8<true>(v);  // Z_j[p] = sum_b x[j + 8 b] W8^{b p}
#pragma unroll
    for (int p = 1; p < 8; ++p) v[p] = cmul(v[p], cconj(tw[(64 * j * p) & (L - 1)]));  // W64^{j p}
#pragma unroll
    for (int p = 0; p < 8; ++p) lds[(c * 8 + j) * 9 + p] = v[p];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 8; ++a) v[a] = lds[(c * 8 + a) * 9 + j];  // Z_a[j]
    dft8<true>(v);  // X[j + 8 q] = sum_a Z_a[j] W8^{a q}
}

// pass 1: grid (L / CW, 64 (n1), B); objF row y, column x = spec row / column
// (y + L/2, x + L/2) mod L; zero outside the live band (fpm_state.hpp)
__global__ void __launch_bounds__(NT) k_crop4k_cols1(DevState st, float2 *out, const float2 *__restrict__ tw) {
    __shared__ float2 lds[CW * 8 * 9];
    const int c = threadIdx.x & (CW - 1), j = threadIdx.x / CW;
    const int x = blockIdx.x * CW + c, n1 = blockIdx.y, b = blockIdx.z;
    const int sx = (x + L / 2) & (L - 1);
    const bool live = sx >= st.sx0 && sx <= st.sx1;
    float2 v[8];
    // unconditional loads of clamped indices, masked after all eight (a
    // masked spec_ld widens fp16 where it loads: one round trip per q)
    bool ok[8];
    size_t idx[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int sy = (n1 + 64 * (j + 8 * q) + L / 2) & (L - 1);
        ok[q] = live && sy >= st.sy0 && sy <= st.sy1;
        idx[q] = (size_t)b * L * L + (ok[q] ? (size_t)sy * L + sx : 0);
    }
    if (st.spec16) {  // uniform
        __half2 hv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) hv[q] = st.spec16[idx[q]];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float2 f = __half22float2(hv[q]);
            v[q] = ok[q] ? make_float2(f.x * st.hinv, f.y * st.hinv) : make_float2(0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = st.spec[idx[q]];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = ok[q] ? v[q] : make_float2(0.f, 0.f);
    }
    idft64(v, lds, c, j, tw);
    float2 *o = out + (size_t)b * L * L + x;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k2 = j + 8 * q;
        o[(size_t)(k2 + 64 * n1) * L] = cmul(v[q], cconj(tw[(n1 * k2) & (L - 1)]));  // W^{n1 k2}
    }
}

// pass 2: grid (L / CW, 64 (k2), B), in place on out
__global__ void __launch_bounds__(NT) k_crop4k_cols2(float2 *out, const float2 *__restrict__ tw) {
    __shared__ float2 lds[CW * 8 * 9];
    const int c = threadIdx.x & (CW - 1), j = threadIdx.x / CW;
    const int x = blockIdx.x * CW + c, k2 = blockIdx.y, b = blockIdx.z;
    float2 *o = out + (size_t)b * L * L + x;
    float2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = o[(size_t)(k2 + 64 * (j + 8 * q)) * L];
    idft64(v, lds, c, j, tw);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[(size_t)(k2 + 64 * (j + 8 * q)) * L] = v[q];
}

// rows: grid (L, B), block 512, in place on out: the same 64 x 64 split within
// the row held by the block -- lane (n1, j) runs the DFT64 over n2 for column
// n1 of the row's 64 x 64 matrix x[n1 + 64 n2], the twiddled results are
// transposed through LDS, lane (k2, j) runs the DFT64 over n1; every load and
// store is 512 contiguous bytes per wave.  Elements x with spec column
// (x + L/2) mod L outside the live band are zero and not read.
constexpr int NTR = 512;
__global__ void __launch_bounds__(NTR) k_crop4k_rows(DevState st, float2 *out, const float2 *__restrict__ tw,
                                                      float scale) {
    __shared__ float2 lds[64 * 8 * 9];
    const int i64 = threadIdx.x & 63, j = threadIdx.x >> 6;
    float2 *row = out + ((size_t)blockIdx.y * L + blockIdx.x) * L;
    float2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int x = i64 + 64 * (j + 8 * q), sx = (x + L / 2) & (L - 1);
        v[q] = sx >= st.sx0 && sx <= st.sx1 ? row[x] : make_float2(0.f, 0.f);
    }
    idft64(v, lds, i64, j, tw);  // lane (n1 = i64, j): bracket values for k2 = j + 8 q
    __syncthreads();             // the exchange reads are done: lds is the transpose tile now
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k2 = j + 8 * q;
        lds[i64 * 65 + k2] = cmul(v[q], cconj(tw[(i64 * k2) & (L - 1)]));  // A[n1][k2] W^{n1 k2}
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = lds[(j + 8 * q) * 65 + i64];  // lane (k2 = i64, j): A[j + 8 q][k2]
    __syncthreads();             // before idft64's exchange overwrites lds
    idft64(v, lds, i64, j, tw);  // X[k2 + 64 (j + 8 q)]
#pragma unroll
    for (int q = 0; q < 8; ++q) row[i64 + 64 * (j + 8 * q)] = cscale(v[q], scale);
}
}  // namespace c4k

// cols1 takes (st, out, tw), cols2 (out, tw), rows (st, out, tw, scale); the
// static LDS is each kernel's own lds[] above
Crop4kKernels crop4k_kernels() {
    using namespace c4k;
    constexpr size_t cols_lds = (size_t)CW * 8 * 9 * sizeof(float2), rows_lds = (size_t)64 * 8 * 9 * sizeof(float2);
    return {crop_kernel((const void *)k_crop4k_cols1, NT, 0, CW, cols_lds),
            crop_kernel((const void *)k_crop4k_cols2, NT, 0, CW, cols_lds),
            crop_kernel((const void *)k_crop4k_rows, NTR, 0, 1, rows_lds)};
}

}  // namespace fpm
