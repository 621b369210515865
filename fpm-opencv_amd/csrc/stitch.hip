// stitch.hip -- fpm_stitch / fpm_stitch_tiles: overlapping tiles blended into
// one field (fpm_hip.h has the definition).
//
// Two passes, both plain streaming kernels:
//   pairs   c = sum T[n] conj(T[t]), a = sum |T[n]|^2, b = sum |T[t]|^2 over the
//           region every neighbour pair (n, t) shares, in double.  A pair's
//           region is cut into shares of kPairShare pixels, one workgroup each
//           (grid: shares x pairs), every thread walks its pixels in a fixed
//           order, the workgroup folds lanes then waves in a fixed order, and a
//           second launch adds a pair's shares in order: no floating-point
//           atomics, so two calls give the same bits.  The products of two
//           fp32 values are exact in double.  Pixel pairs by 16-byte loads
//           where L and the region's width and column are even and the tiles
//           are 16-byte aligned, single pixels by 8-byte loads otherwise.
//   blend   gather form: a thread owns V adjacent field pixels of kBlendRows
//           rows, finds the one or two tiles per axis that cover them by
//           arithmetic, and adds w f T over them in ascending tile order in
//           fp32.  V = 2 (16-byte accesses) when L, the column stride and so W
//           are even and both bases are 16-byte aligned: tile borders then fall
//           on even columns, so a pixel pair shares its covering tiles and
//           every access is aligned.  V = 1 (8-byte accesses) otherwise.  A
//           pixel under one tile whose factor is exactly 1 is a copy of bits.
#include "launch.hpp"
#include "stitch_solve.hpp"

namespace fpm {

namespace {

constexpr int kStitchThreads = 256;
constexpr int kPairShare = 4096;  // pixels of a pair's region per workgroup: 16 per thread
constexpr int kBlendRows = 4;     // field rows per thread of the blend

// ---- pair sums --------------------------------------------------------------------------------

// The region pair p shares: h x w pixels, at (ny, nx) in tile n and at (0, 0) in tile t
struct PairRegion {
    int n, t, h, w, ny, nx;
};
__device__ __forceinline__ PairRegion pair_region(const StitchGeom &g, int p) {
    const int n_lr = g.gy * (g.gx - 1);
    PairRegion r;
    if (p < n_lr) {
        const int i = p / (g.gx - 1), j = p - i * (g.gx - 1) + 1;
        r.t = i * g.gx + j;
        r.n = r.t - 1;
        r.h = g.L;
        r.w = g.L - g.sx;
        r.ny = 0;
        r.nx = g.sx;
    } else {
        const int q = p - n_lr;
        r.t = q + g.gx;  // (i, j) = (q / gx + 1, q % gx)
        r.n = q;
        r.h = g.L - g.sy;
        r.w = g.L;
        r.ny = g.sy;
        r.nx = 0;
    }
    return r;
}

// partials [pairs][parts][4]: (c_re, c_im, a, b) of share blockIdx.x of pair blockIdx.y
__global__ void __launch_bounds__(kStitchThreads) k_stitch_pairs(StitchGeom g, const float2 *__restrict__ tiles,
                                                                 int parts, int vec, double *__restrict__ partials) {
    const int p = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const PairRegion r = pair_region(g, p);
    const int npx = r.h * r.w;  // L <= 32768 (fpm_stitch_tiles): L^2 fits
    const int lo = part * kPairShare;
    if (lo >= npx) return;  // the shorter kind of region has fewer shares (k_stitch_fold reads only its own)
    const int hi = min(lo + kPairShare, npx);
    const size_t ll = (size_t)g.L * g.L;
    const float2 *tn = tiles + r.n * ll + (size_t)r.ny * g.L + r.nx;
    const float2 *tt = tiles + r.t * ll;
    double cr = 0, ci = 0, a = 0, b = 0;
    auto add = [&](float2 vn, float2 vt) {
        const double nr = vn.x, ni = vn.y, tr = vt.x, ti = vt.y;
        cr += nr * tr + ni * ti;
        ci += ni * tr - nr * ti;
        a += nr * nr + ni * ni;
        b += tr * tr + ti * ti;
    };
    if (vec && (r.w & 1) == 0 && (r.nx & 1) == 0) {
        // pixel pairs by 16-byte loads: L and the region's width and column are
        // even, so a pair stays in its row and every address is aligned
        for (int e = lo + 2 * tid; e < hi; e += 2 * kStitchThreads) {
            const int y = e / r.w, x = e - y * r.w;
            const float4 qn = *reinterpret_cast<const float4 *>(tn + (size_t)y * g.L + x);
            const float4 qt = *reinterpret_cast<const float4 *>(tt + (size_t)y * g.L + x);
            add(make_float2(qn.x, qn.y), make_float2(qt.x, qt.y));
            add(make_float2(qn.z, qn.w), make_float2(qt.z, qt.w));
        }
    } else {
        for (int e = lo + tid; e < hi; e += kStitchThreads) {
            const int y = e / r.w, x = e - y * r.w;
            add(tn[(size_t)y * g.L + x], tt[(size_t)y * g.L + x]);
        }
    }
    // lanes, then waves, in a fixed order
    for (int o = warpSize / 2; o > 0; o >>= 1) {
        cr += __shfl_down(cr, o);
        ci += __shfl_down(ci, o);
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
    }
    __shared__ double red[kStitchThreads / 32][4];  // a row per wave, whichever of the two wave sizes
    const int wave = tid / warpSize, nwave = kStitchThreads / warpSize;
    if (tid % warpSize == 0) {
        red[wave][0] = cr;
        red[wave][1] = ci;
        red[wave][2] = a;
        red[wave][3] = b;
    }
    __syncthreads();
    if (tid < 4) {
        double s = 0;
        for (int w = 0; w < nwave; ++w) s += red[w][tid];
        partials[((size_t)p * parts + part) * 4 + tid] = s;
    }
}

// sums [pairs][4]: a pair's shares added in order; thread = (pair, component)
__global__ void __launch_bounds__(kStitchThreads) k_stitch_fold(StitchGeom g, int parts, int parts_lr, int parts_ud,
                                                                const double *__restrict__ partials,
                                                                double *__restrict__ sums) {
    const int k = blockIdx.x * kStitchThreads + threadIdx.x;
    const int npairs = g.gy * (g.gx - 1) + (g.gy - 1) * g.gx;
    if (k >= npairs * 4) return;
    const int p = k >> 2, comp = k & 3;
    const int cnt = p < g.gy * (g.gx - 1) ? parts_lr : parts_ud;
    double s = 0;
    for (int i = 0; i < cnt; ++i) s += partials[((size_t)p * parts + i) * 4 + comp];
    sums[k] = s;
}

// ---- blend ------------------------------------------------------------------------------------

// The tiles that cover coordinate x of an axis with count n, stride s: the
// last one that starts at or before x (index hi, local coordinate u, weight
// w_hi) and, when x lies in its overlap with the one before, that one too
// (index hi - 1, local coordinate u + s, weight w_lo).
struct Cover {
    int hi, u;
    bool two;
    float w_hi, w_lo;
};
__device__ __forceinline__ Cover cover(int x, int s, int n, int L) {
    Cover c;
    c.hi = min(x / s, n - 1);
    c.u = x - c.hi * s;
    const int v = L - s;
    c.two = c.hi > 0 && c.u < v;
    c.w_hi = c.two ? (float)(c.u + 1) / (float)(v + 1) : 1.f;
    c.w_lo = c.two ? (float)(v - c.u) / (float)(v + 1) : 0.f;  // (L - (u + s)) / (V + 1)
    return c;
}

template <int V>
struct Px;
template <>
struct Px<1> {
    float2 v[1];
    __device__ __forceinline__ void load(const float2 *p) { v[0] = *p; }
    __device__ __forceinline__ void store(float2 *p) const { *p = v[0]; }
};
template <>
struct Px<2> {
    float2 v[2];
    __device__ __forceinline__ void load(const float2 *p) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = make_float2(q.x, q.y);
        v[1] = make_float2(q.z, q.w);
    }
    __device__ __forceinline__ void store(float2 *p) const {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    }
};

// The column weights of a thread's V pixels: they share their covering tiles
// (cx is pixel 0's), not their place in the overlap
template <int V>
struct ColW {
    float hi[V], lo[V];
    __device__ __forceinline__ ColW(const Cover &cx, int v) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            hi[k] = cx.two ? (float)(cx.u + k + 1) / (float)(v + 1) : 1.f;
            lo[k] = cx.two ? (float)(v - cx.u - k) / (float)(v + 1) : 0.f;
        }
    }
};

// acc += wy wx (f T): one complex multiply, the weight, the addition
template <int V, bool UNIT>
__device__ __forceinline__ void add_tile(Px<V> &acc, const float2 *__restrict__ tiles, const float2 *__restrict__ fac,
                                         int t, int L, int ly, int lx, float wy, const float (&wx)[V]) {
    Px<V> px;
    px.load(tiles + ((size_t)t * L + ly) * L + lx);
    float2 f = make_float2(1.f, 0.f);
    if (!UNIT) f = fac[t];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float2 v = px.v[k];
        if (!UNIT) v = make_float2(f.x * px.v[k].x - f.y * px.v[k].y, f.x * px.v[k].y + f.y * px.v[k].x);
        const float w = wy * wx[k];
        acc.v[k].x += w * v.x;
        acc.v[k].y += w * v.y;
    }
}

// UNIT: every factor is 1 (no alignment), fac is not read
template <int V, bool UNIT>
__global__ void __launch_bounds__(kStitchThreads) k_stitch_blend(StitchGeom g, const float2 *__restrict__ tiles,
                                                                 const float2 *__restrict__ fac,
                                                                 float2 *__restrict__ field) {
    const int x = (blockIdx.x * kStitchThreads + threadIdx.x) * V;
    if (x >= g.W) return;  // V = 2: W is even, so x + 1 < W as well
    const Cover cx = cover(x, g.sx, g.gx, g.L);
    const ColW<V> wx(cx, g.L - g.sx);
    const int y0 = blockIdx.y * kBlendRows;
#pragma unroll
    for (int r = 0; r < kBlendRows; ++r) {
        const int y = y0 + r;
        if (y >= g.H) break;
        const Cover cy = cover(y, g.sy, g.gy, g.L);
        const int t11 = cy.hi * g.gx + cx.hi;
        float2 *dst = field + (size_t)y * g.W + x;
        Px<V> acc;
        if (!cx.two && !cy.two) {
            // one tile: a copy of its bits when its factor is exactly 1
            bool copy = UNIT;
            if (!UNIT) {
                const float2 f = fac[t11];
                copy = f.x == 1.f && f.y == 0.f;
            }
            if (copy) {
                acc.load(tiles + ((size_t)t11 * g.L + cy.u) * g.L + cx.u);
                acc.store(dst);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = make_float2(0.f, 0.f);
        // ascending tile order: (upper, left), (upper, right), (lower, left), (lower, right)
        if (cy.two) {
            if (cx.two) add_tile<V, UNIT>(acc, tiles, fac, t11 - g.gx - 1, g.L, cy.u + g.sy, cx.u + g.sx, cy.w_lo, wx.lo);
            add_tile<V, UNIT>(acc, tiles, fac, t11 - g.gx, g.L, cy.u + g.sy, cx.u, cy.w_lo, wx.hi);
        }
        if (cx.two) add_tile<V, UNIT>(acc, tiles, fac, t11 - 1, g.L, cy.u, cx.u + g.sx, cy.w_hi, wx.lo);
        add_tile<V, UNIT>(acc, tiles, fac, t11, g.L, cy.u, cx.u, cy.w_hi, wx.hi);
        acc.store(dst);
    }
}

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

StitchParts stitch_pair_parts(const StitchGeom &g) {
    StitchParts p;
    p.lr = g.gx > 1 ? ceil_div((long long)g.L * (g.L - g.sx), kPairShare) : 0;
    p.ud = g.gy > 1 ? ceil_div((long long)(g.L - g.sy) * g.L, kPairShare) : 0;
    p.parts = p.lr > p.ud ? p.lr : p.ud;
    if (p.parts < 1) p.parts = 1;
    return p;
}

hipError_t launch_stitch_pairs(const StitchGeom &g, const float2 *tiles, double *partials, double *sums,
                               hipStream_t s) {
    const int npairs = stitch_pairs(g.gy, g.gx);
    if (npairs < 1) return hipSuccess;
    const StitchParts p = stitch_pair_parts(g);
    if (npairs > 65535) return hipErrorInvalidValue;  // grid.y; fpm_stitch_tiles refuses such a grid
    hipLaunchKernelGGL(k_stitch_pairs, dim3(p.parts, npairs), dim3(kStitchThreads), 0, s, g, tiles, p.parts,
                       (int)(g.L % 2 == 0 && (uintptr_t)tiles % 16 == 0), partials);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_stitch_fold, dim3(ceil_div(4ll * npairs, kStitchThreads)), dim3(kStitchThreads), 0, s, g,
                       p.parts, p.lr, p.ud, partials, sums);
    return hipGetLastError();
}

bool stitch_blend_vector(const StitchGeom &g, const float2 *tiles, const float2 *field) {
    return g.L % 2 == 0 && g.sx % 2 == 0 && ((uintptr_t)tiles | (uintptr_t)field) % 16 == 0;
}

hipError_t launch_stitch_blend(const StitchGeom &g, const float2 *tiles, const float2 *factors, float2 *field,
                               hipStream_t s) {
    const bool vec = stitch_blend_vector(g, tiles, field);
    const dim3 grid(ceil_div(g.W, (vec ? 2 : 1) * kStitchThreads), ceil_div(g.H, kBlendRows)), block(kStitchThreads);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (vec) {
        if (factors) hipLaunchKernelGGL((k_stitch_blend<2, false>), grid, block, 0, s, g, tiles, factors, field);
        else hipLaunchKernelGGL((k_stitch_blend<2, true>), grid, block, 0, s, g, tiles, factors, field);
    } else {
        if (factors) hipLaunchKernelGGL((k_stitch_blend<1, false>), grid, block, 0, s, g, tiles, factors, field);
        else hipLaunchKernelGGL((k_stitch_blend<1, true>), grid, block, 0, s, g, tiles, factors, field);
    }
    return hipGetLastError();
}

}  // namespace fpm
