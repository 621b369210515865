// stitch_solve.hpp -- the host half of fpm_stitch's alignment: the complex
// factor of every tile from the sums over the regions neighbouring tiles share
// (fpm_hip.h, fpm_stitch_tiles).  Plain C++, no HIP: the library's boundary
// (stitch_api.cpp) and the stand-alone test driver (tests/shim/stitch_solve_main.cpp)
// include it.
#pragma once
#include <cmath>

namespace fpm {

// Sums over the pixels a neighbour pair (n, t) shares, n the left or the upper
// tile: c = sum T[n] conj(T[t]), a = sum |T[n]|^2, b = sum |T[t]|^2
struct StitchPairSums {
    double c_re, c_im, a, b;
};

enum StitchAlign { kStitchAlignNone = 0, kStitchAlignPhase = 1, kStitchAlignComplex = 2 };

// Pairs of a gy x gx grid: the left/right pairs first, row-major by their right
// tile, then the up/down pairs, row-major by their lower tile.
inline int stitch_pairs_lr(int gy, int gx) { return gy * (gx - 1); }
inline int stitch_pairs(int gy, int gx) { return gy * (gx - 1) + (gy - 1) * gx; }
inline int stitch_pair_left(int gx, int i, int j) { return i * (gx - 1) + (j - 1); }                       // j >= 1
inline int stitch_pair_up(int gy, int gx, int i, int j) { return stitch_pairs_lr(gy, gx) + (i - 1) * gx + j; }  // i >= 1

// f [gy*gx][2] (re, im): f[0] = 1, the others in raster order from the left
// and the upper neighbour, both already placed:
//   z = sum_n f[n] c,  num = sum_n |f[n]|^2 a,  den = sum_n b
//   phase: f = z / |z|;  complex: f = (z / |z|) sqrt(num / den);  z == 0 or den == 0: f = 1
inline void stitch_solve(int gy, int gx, int mode, const StitchPairSums *sums, double *f) {
    for (int i = 0; i < gy; ++i)
        for (int j = 0; j < gx; ++j) {
            const int t = i * gx + j;
            f[2 * t] = 1.0;
            f[2 * t + 1] = 0.0;
            if (t == 0 || mode == kStitchAlignNone) continue;
            double zr = 0, zi = 0, num = 0, den = 0;
            auto add = [&](int n, const StitchPairSums &s) {
                const double fr = f[2 * n], fi = f[2 * n + 1];
                zr += fr * s.c_re - fi * s.c_im;
                zi += fr * s.c_im + fi * s.c_re;
                num += (fr * fr + fi * fi) * s.a;
                den += s.b;
            };
            if (j > 0) add(t - 1, sums[stitch_pair_left(gx, i, j)]);
            if (i > 0) add(t - gx, sums[stitch_pair_up(gy, gx, i, j)]);
            const double az = std::hypot(zr, zi);
            if (az == 0 || den == 0) continue;
            const double scale = mode == kStitchAlignComplex ? std::sqrt(num / den) : 1.0;
            f[2 * t] = zr / az * scale;
            f[2 * t + 1] = zi / az * scale;
        }
}

}  // namespace fpm
