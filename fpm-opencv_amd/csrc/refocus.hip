// refocus.hip -- fpm_refocus: the two kernels around objCrop's transform
// (fpm_hip.h has the definition).
//
//   mul    scratch = spec H(zl) over the live band of the centred spectrum, one
//          thread per complex element (8-byte accesses, a wave along a row).
//          Centred element (y, x) is the signed bin (ky, kx) = (y - L/2, x - L/2).
//          s = fl^2 (kx^2 + ky^2) and the phase c = zl sqrt(1 - s) are double;
//          c is reduced to c - rint(c), a fraction of a turn in [-1/2, 1/2], and
//          the fp32 sincospif of twice that fraction is H, so H carries fp32
//          rounding whatever |zl| <= 1e6 is.  s > 1 (evanescent) stores zero.
//          zl is read per (patch, element): a z per patch costs nothing extra.
//          Nothing outside the band is written: the objCrop kernels never read
//          there, and the scratch was cleared when it was allocated.
//   sums   one pass over a plane.  A block takes a strip of kRfRows rows of the
//          interior R = [margin, L - margin)^2 and the one row below it for the
//          vertical pairs; a thread walks a column of the strip, keeps the
//          magnitude above it and takes its right neighbour's from the next lane
//          (the last lane of a wave computes that one itself).  Differences and
//          squares are double, a block folds lanes then waves in a fixed order
//          and writes three partials; a second launch adds a patch's strips in
//          order: no floating-point atomics, two calls give the same bits.
#include "launch.hpp"

namespace fpm {

namespace {

constexpr int kMulX = 64, kMulY = 4;  // block of the multiply: a wave along a row, four rows
constexpr int kRfThreads = 256;
constexpr int kRfRows = 16;           // rows of R per block of the sums pass

__global__ void __launch_bounds__(kMulX *kMulY) k_refocus_mul(DevState st, const double *__restrict__ zl, int zstride,
                                                              double fl2, float2 *__restrict__ scratch) {
    const int x = st.sx0 + blockIdx.x * kMulX + threadIdx.x, y = st.sy0 + blockIdx.y * kMulY + threadIdx.y;
    const int b = blockIdx.z, L = st.L;
    if (x > st.sx1 || y > st.sy1) return;
    const int kx = x - L / 2, ky = y - L / 2;
    const size_t i = (size_t)y * L + x;
    const float2 v = spec_ld(st, b, i);
    const double s = fl2 * (double)(kx * kx + ky * ky);
    float2 o = make_float2(0.f, 0.f);
    if (s <= 1.0) {
        const double c = zl[(size_t)b * zstride] * sqrt(1.0 - s);
        const double frac = c - rint(c);
        float sn, cs;
        sincospif((float)(2.0 * frac), &sn, &cs);
        o = cmul(v, make_float2(cs, sn));
    }
    scratch[(size_t)b * L * L + i] = o;
}

// partials [B][nblk][3]: (sum a, sum a^2, sum of squared differences) of strip blockIdx.x of patch blockIdx.y
__global__ void __launch_bounds__(kRfThreads) k_refocus_sums(const float2 *__restrict__ plane, int L, int margin,
                                                             double *__restrict__ partials) {
    const int strip = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lo = margin, hi = L - margin;
    const int y0 = lo + strip * kRfRows, y1 = min(y0 + kRfRows, hi);
    const float2 *p = plane + (size_t)b * L * L;
    const bool last_lane = tid % warpSize == warpSize - 1;
    double sa = 0, sa2 = 0, sg = 0;
    for (int xb = lo; xb < hi; xb += kRfThreads) {  // uniform: every lane takes part in the shuffles
        const int x = xb + tid;
        const bool in = x < hi, right = x + 1 < hi;
        float prev = 0.f;
        for (int y = y0; y < y1; ++y) {
            const float2 *row = p + (size_t)y * L;
            const float a = in ? cmag(row[x]) : 0.f;
            float ar = __shfl_down(a, 1);
            if (right && last_lane) ar = cmag(row[x + 1]);  // the neighbour is another wave's
            if (in) {
                const double da = a;
                sa += da;
                sa2 += da * da;
                if (right) {
                    const double d = (double)ar - da;
                    sg += d * d;
                }
                if (y > y0) {
                    const double d = da - (double)prev;
                    sg += d * d;
                }
            }
            prev = a;
        }
        if (in && y1 < hi) {  // the pairs between this strip's last row and the next strip's first
            const double d = (double)cmag(p[(size_t)y1 * L + x]) - (double)prev;
            sg += d * d;
        }
    }
    // lanes, then waves, in a fixed order
    for (int o = warpSize / 2; o > 0; o >>= 1) {
        sa += __shfl_down(sa, o);
        sa2 += __shfl_down(sa2, o);
        sg += __shfl_down(sg, o);
    }
    __shared__ double red[kRfThreads / 32][3];  // a row per wave, whichever of the two wave sizes
    const int wave = tid / warpSize, nwave = kRfThreads / warpSize;
    if (tid % warpSize == 0) {
        red[wave][0] = sa;
        red[wave][1] = sa2;
        red[wave][2] = sg;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0;
        for (int w = 0; w < nwave; ++w) s += red[w][tid];
        partials[((size_t)b * gridDim.x + strip) * 3 + tid] = s;
    }
}

// a patch's strips added in order; thread = (patch, sum); a null output is skipped
__global__ void __launch_bounds__(kRfThreads) k_refocus_fold(int B, int nblk, const double *__restrict__ partials,
                                                             double *__restrict__ sum_a, double *__restrict__ sum_a2,
                                                             double *__restrict__ sum_g) {
    const int k = blockIdx.x * kRfThreads + threadIdx.x;
    if (k >= B * 3) return;
    const int b = k / 3, comp = k - 3 * b;
    double *out = comp == 0 ? sum_a : comp == 1 ? sum_a2 : sum_g;
    if (!out) return;
    double s = 0;
    for (int i = 0; i < nblk; ++i) s += partials[((size_t)b * nblk + i) * 3 + comp];
    out[b] = s;
}

}  // namespace

hipError_t launch_refocus_mul(const DevState &st, const double *zl, int zstride, double fl, float2 *scratch,
                              hipStream_t s) {
    const int L = st.L;
    if (st.sy0 < 0 || st.sy1 >= L || st.sy0 > st.sy1 || st.sx0 < 0 || st.sx1 >= L || st.sx0 > st.sx1 || st.B > 65535)
        return hipErrorInvalidValue;
    const int bw = st.sx1 - st.sx0 + 1, bh = st.sy1 - st.sy0 + 1;
    hipLaunchKernelGGL(k_refocus_mul, dim3((bw + kMulX - 1) / kMulX, (bh + kMulY - 1) / kMulY, st.B),
                       dim3(kMulX, kMulY), 0, s, st, zl, zstride, fl * fl, scratch);
    return hipGetLastError();
}

int refocus_sum_blocks(int L, int margin) { return (L - 2 * margin + kRfRows - 1) / kRfRows; }

hipError_t launch_refocus_sums(const float2 *plane, int B, int L, int margin, double *partials, double *sum_a,
                               double *sum_a2, double *sum_g, hipStream_t s) {
    const int nblk = refocus_sum_blocks(L, margin);
    if (margin < 0 || L - 2 * margin < 2 || B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refocus_sums, dim3(nblk, B), dim3(kRfThreads), 0, s, plane, L, margin, partials);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_refocus_fold, dim3((3 * B + kRfThreads - 1) / kRfThreads), dim3(kRfThreads), 0, s, B, nblk,
                       partials, sum_a, sum_a2, sum_g);
    return hipGetLastError();
}

}  // namespace fpm
