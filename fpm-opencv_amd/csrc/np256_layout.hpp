// np256_layout.hpp -- the Np 256 register kernels' block shape, index helpers
// and launch sizes, shared by np256.hip (the LED step's R1 / C / R2) and
// residual.hip (the sweep's row kernel and its plan).
//
// One 256-point transform per 16-lane group, lane t holding elements t + 16 j;
// GPB groups (rows or columns) per block; blocks of patch b on XCD b mod 8.
#pragma once
#include <algorithm>

#include "dftL.hpp"

namespace fpm {

namespace n256 {
constexpr int N = 256, H = N / 2;
constexpr int WPB = 4;            // waves per block
constexpr int NT = 64 * WPB;
constexpr int GPB = 4 * WPB;      // 16-lane groups per block: rows (R1, R2) or columns (C) per block
constexpr int SP = GPB + 1;       // strip row pitch (complex)
static_assert(NT == N, "one twiddle per thread");

// dynamic LDS of the row kernels (R1, R2, k_res_rows256) and of the column kernel C
inline size_t lds_rows() { return (size_t)(N + GPB * XTILE_H) * sizeof(float2); }
inline size_t lds_cols(int nb) { return (size_t)(N + std::max(nb * SP, GPB * XTILE_H)) * sizeof(float2); }
inline int row_blocks(int nb) { return (nb + GPB - 1) / GPB; }  // R1's sub-blocks per patch
constexpr int kColBlocks = N / GPB;                             // C's sub-blocks per patch
}  // namespace n256

__device__ __forceinline__ int fold256(int k) { return k < n256::H ? k : k - n256::N; }  // signed frequency

// FFT row i of a column is box row i + r (i <= r) or i - N + r (i >= N - r);
// every other row is zero (:364): -1
__device__ __forceinline__ int boxrow(int i, int r) {
    return i <= r ? i + r : (i >= n256::N - r ? i - n256::N + r : -1);
}

// block -> (patch b, sub-block) of a 1-D grid of nsub * xcd_patches(B)
// blocks, patch b on XCD b mod 8; false for the padding blocks of patches
// b >= B (B not a multiple of 8), which exit at once.  Against the plain
// b = block / nsub: 1.20-1.22 -> 1.22-1.24 M at dataset_mono Np 256, 64
// patches (profiles/r06_ab/np256_register_path_ab.txt)
__host__ __device__ __forceinline__ int xcd_patches(int B) { return (B + 7) & ~7; }
__device__ __forceinline__ bool xcd_block(int nsub, int B, int &b, int &sub) {
    const int id = blockIdx.x;
    const int k = id >> 3, q = k / nsub;
    b = (id & 7) + 8 * q;
    sub = k - q * nsub;
    return b < B;
}

}  // namespace fpm
