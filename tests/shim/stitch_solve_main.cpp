// stitch_solve_main.cpp -- test driver of the host factor solve of fpm_stitch
// (fpm-opencv_amd/csrc/stitch_solve.hpp), built without HIP and with
// -fsanitize=address,undefined by tests/test_stitch_cases.py.
//
// stdin:  gy gx mode (0 none, 1 phase, 2 complex), then one line
//         "c_re c_im a b" per neighbour pair in the header's pair order
// stdout: one line "re im" per tile, %.17g
#include <cstdio>
#include <vector>

#include "../../fpm-opencv_amd/csrc/stitch_solve.hpp"

int main() {
    int gy = 0, gx = 0, mode = 0;
    if (scanf("%d %d %d", &gy, &gx, &mode) != 3 || gy < 1 || gx < 1 || gy > 1024 || gx > 1024 || mode < 0 || mode > 2) {
        fprintf(stderr, "stitch_solve_main: want 'gy gx mode'\n");
        return 2;
    }
    std::vector<fpm::StitchPairSums> sums(fpm::stitch_pairs(gy, gx));
    for (auto &s : sums)
        if (scanf("%lf %lf %lf %lf", &s.c_re, &s.c_im, &s.a, &s.b) != 4) {
            fprintf(stderr, "stitch_solve_main: want %zu pair lines\n", sums.size());
            return 2;
        }
    std::vector<double> f(2 * (size_t)gy * gx);
    fpm::stitch_solve(gy, gx, mode, sums.data(), f.data());
    for (int t = 0; t < gy * gx; ++t) printf("%.17g %.17g\n", f[2 * t], f[2 * t + 1]);
    return 0;
}
