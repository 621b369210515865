"""Case table of the transform-size sweep: plain data and builders, no GPU.

fpm_create takes every even Np = 2^a 3^b 5^c >= 4 and every even 5-smooth
L >= Np, and each size gets its own radix plan from make_plan (create.cpp:
8s, then 4s, 2s, 3s, 5s).  That plan drives the Stockham passes of the
small-patch fused kernel (fft_lds.hpp), fft_inplace_pass in the general path's
LDS ladder and in the residual sweep, and k_fft_batch as fpm_init's fft2 and as
objCrop.  The other tables pin each kernel at a few sizes; this one sweeps the
size.

SIZES    every even 5-smooth Np in [4, 96] at L = 3 Np, radii 1, Np / 4 and
         min(Np / 2 - 1, 31), on the general path and, from Np 8 on, on the
         fused path (k_fused_small; k_fused_s90 at Np 90).  Np 4 and 6 lie below
         the small-patch kernel: PATH_FUSED is refused, PATH_AUTO is the general
         path.
CORNERS  of the accepted domain:
  r0     naRadius 0, a one-pixel pupil: no fused and no register kernel takes
         it, PATH_AUTO is the LDS ladder with one pupil-maximum partial;
  LeqNp  L = Np: every crop is (0, 0), the live band is the init box, objCrop
         runs at L = Np.  Two stack entries at the same crop whose images
         differ by their Poisson noise, order (0, 1) -- the smallest n_order
         fpm_create takes.  PATH_AUTO; the kernel each context must report is
         part of the row (the fused kernels take L = Np);
  Lmod   L no multiple of Np, both paths.

Every case: two distinct patches (make_stack, a seed per case), a 3 x 3
centred LED grid (LeqNp: the two entries above), two iterations, delta1 5 /
delta2 10, and the project's parity bound for two iterations (DESIGN.md
section 2).

tests/test_size_cases.py (CPU) checks that the table is what it claims and
that every case is well posed and well conditioned in fp32;
tests/test_gpu_sizes.py runs it on the device.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fpm_amd
from tools.synth import grid_geometry, make_stack

ITERS, DELTA1, DELTA2, B = 2, 5, 10, 2
TOL = 5e-5                  # relative L2 against the fp64 oracle after two iterations
FUSED_VS_GENERAL = 2e-6     # the bound of test_small_fused_equals_general_path, per output and patch

SIZES = (4, 6, 8, 10, 12, 16, 18, 20, 24, 30, 32, 36, 40, 48, 50, 54, 60, 64, 72, 80, 90, 96)

_G, _F, _A = fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED, fpm_amd.PATH_AUTO


@dataclass(frozen=True)
class Context:
    """One fpm_create of a case."""
    path: int
    kernel: int | None          # fpm_info.fused_kernel it must report; None: fpm_create refuses with FPM_ERR_INVAL
    general_kind: int = -1      # fpm_debug_get_plan
    run: bool = True            # False: only what the context reports is asserted

    @property
    def name(self):
        return {_G: "general", _F: "fused", _A: "auto"}[self.path]


GENERAL = Context(_G, fpm_amd.KERNEL_GENERAL, fpm_amd.GENERAL_LDS)
AUTO_GENERAL = Context(_A, fpm_amd.KERNEL_GENERAL, fpm_amd.GENERAL_LDS)


def fused_kernel(Np):
    """The LED-update kernel of a fused context at Np in [8, 96]."""
    return fpm_amd.KERNEL_FUSED_NP90 if Np == 90 else fpm_amd.KERNEL_FUSED_SMALL


@dataclass(frozen=True)
class Case:
    id: str
    Np: int
    L: int
    r: int
    x0: tuple
    y0: tuple
    order: tuple
    seed: int
    contexts: tuple

    @property
    def nb(self):
        return 2 * self.r + 1

    @property
    def tol(self):
        return TOL

    def problem(self, ctx):
        return fpm_amd.Problem(self.Np, self.L, np.array(self.order), np.array(self.x0), np.array(self.y0), self.r,
                               DELTA1, DELTA2, n_patch=B, path=ctx.path)

    def stack(self):
        """uint16 [n_stack][B][Np][Np], read-only."""
        return _stack(self.Np, self.L, self.r, self.x0, self.y0, self.seed)

    def band(self):
        """(sy0, sy1, sx0, sx1), inclusive: the live band (fpm_state.hpp) of the used LEDs."""
        h, r, c = self.Np // 2, self.r, self.L // 2
        ys = [c] + [self.y0[i] + h for i in self.order]
        xs = [c] + [self.x0[i] + h for i in self.order]
        return (max(min(ys) - r, 0), min(max(ys) + r, self.L - 1), max(min(xs) - r, 0), min(max(xs) + r, self.L - 1))


@functools.lru_cache(maxsize=2)
def _stack(Np, L, r, x0, y0, seed):
    st = make_stack(Np, L, r, x0, y0, n_patch=B, seed=seed)
    st.setflags(write=False)
    return st


@dataclass(frozen=True)
class Row:
    """One GPU test: the cases of one Np, or one corner."""
    id: str
    cases: tuple


def _grid(Np, L, step):
    x0, y0, order = grid_geometry(Np, L, 3, step)
    return tuple(int(v) for v in x0), tuple(int(v) for v in y0), tuple(order)


def radii(Np):
    return tuple(sorted({r for r in (1, Np // 4, min(Np // 2 - 1, 31)) if r >= 1 and 2 * r + 1 <= Np}))


def _size_row(Np):
    if Np >= 8:
        ctxs = (GENERAL, Context(_F, fused_kernel(Np)))
    else:   # below fused_small_supported
        ctxs = (GENERAL, Context(_F, None), Context(_A, fpm_amd.KERNEL_GENERAL, fpm_amd.GENERAL_LDS, run=False))
    return Row(f"np{Np}", tuple(Case(f"np{Np}_r{r}", Np, 3 * Np, r, *_grid(Np, 3 * Np, max(1, r)),
                                     seed=8000 + 100 * Np + r, contexts=ctxs) for r in radii(Np)))


SIZE_ROWS = tuple(_size_row(Np) for Np in SIZES)

# ---- the corners ---------------------------------------------------------------------
R0 = ((4, 12), (32, 96), (96, 288), (256, 512))
# (Np, r, the kernel PATH_AUTO must report, further contexts): every fused kernel takes L = Np
L_EQ_NP = (
    (32, 6, fpm_amd.KERNEL_FUSED_SMALL, (GENERAL,)),
    (90, 30, fpm_amd.KERNEL_FUSED_NP90, ()),
    (200, 26, fpm_amd.KERNEL_FUSED_NP200, ()),
    # two patches on a whole MI355X: the distributed mode of the Np 256 kernel
    (256, 33, fpm_amd.KERNEL_FUSED_NP256_DIST, ()),
)
L_NO_MULTIPLE = ((32, 50, 6), (30, 36, 5), (90, 100, 12), (96, 100, 31))

CORNER_ROWS = tuple(
    [Row(f"r0_np{Np}_L{L}", (Case(f"r0_np{Np}_L{L}", Np, L, 0, *_grid(Np, L, 1), seed=9100 + Np,
                                  contexts=(AUTO_GENERAL,)),)) for Np, L in R0]
    + [Row(f"LeqNp_np{Np}", (Case(f"LeqNp_np{Np}_r{r}", Np, Np, r, (0, 0), (0, 0), (0, 1), seed=9300 + Np,
                                  contexts=(Context(_A, k),) + more),)) for Np, r, k, more in L_EQ_NP]
    + [Row(f"Lmod_np{Np}_L{L}", (Case(f"Lmod_np{Np}_L{L}_r{r}", Np, L, r, *_grid(Np, L, min(r, (L - Np) // 2)),
                                      seed=9500 + Np, contexts=(GENERAL, Context(_F, fused_kernel(Np)))),))
       for Np, L, r in L_NO_MULTIPLE])

ROWS = SIZE_ROWS + CORNER_ROWS
CASES = tuple(c for row in ROWS for c in row.cases)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) and len({r.id for r in ROWS}) == len(ROWS)


def radices(n):
    """make_plan (create.cpp): the radix of every pass, in the plan's order."""
    out = []
    for r in (8, 4, 2, 3, 5):
        while n % r == 0:
            out.append(r)
            n //= r
    assert n == 1
    return tuple(out)
