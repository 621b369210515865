"""Case table of the objCrop tests: plain data and builders, no GPU.

objCrop = IDFT2(fftShift(spec)) / L^2 runs on one of six kernel families
(csrc/objcrop.hip plan_objcrop and launch_objcrop; the kernels in
csrc/crop256m.hip, crop600.hip, crop360.hip, crop4k.hip and fft_batch.hip), and
each skips everything outside the live band [sy0, sy1] x [sx0, sx1] of the
centred spectrum.  A context (CONTEXTS) selects the family -- asserted from
the library's planner (tests/test_objcrop_cases.py) and from each live
context's plan (tests/test_gpu_objcrop.py); a band (BANDS) is a shape
the launchers accept (0 <= lo <= hi < L) whether or not an LED geometry could
plan it.  fpm_debug_objcrop (Solver.debug_objcrop) runs the context's own
launch on a given spectrum and band.

Input of a case: N(0,1) + i N(0,1) complex64 inside the band, seeded by the
case's name, and NaN everywhere outside it -- the kernels must take what is
outside as zero without reading it (every masked load is a select), and the
objCrop buffer is poisoned with NaN before the launch, so a mask one element
too wide, an element no pass writes and an intermediate row read although no
pass wrote it all end as a NaN in the result.  On an fp16-storage context the
values are drawn as float16 and divided by hscale = 2^-ceil(log2 Np^2), so the
store half(v * hscale) is exact and the reference needs no quantisation model.

Reference: np.fft.ifft2(np.fft.ifftshift(masked)) in complex128, masked = the
input with zeros for the NaNs.  BOUND is the bound test_objcrop_live_band
(test_gpu_parity.py) already holds these kernels to; an fp32 CPU transform of
exactly these inputs gives 1.2e-7 .. 2.3e-7 (tests/test_objcrop_cases.py keeps
it below BOUND / 5), and one dropped or misplaced band-edge element in a dense
random band gives 1e-3 or more.

tests/test_objcrop_cases.py (CPU) re-derives what the table claims to reach;
tests/test_gpu_objcrop.py runs it on the device.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

import fpm_amd
from tools.synth import grid_geometry

BOUND = 2e-6

# how the row pass cuts the live rows into blocks
REGS = "regs"        # grid starts at sy0, Gr rows per block (k_crop_rows, c600, c360)
BATCHED = "batched"  # k_fft_batch: blocks of C = Gr sequences, aligned in the objF row index (spec row + L/2) mod L
C4K = "c4k"          # six-step columns first: no row blocks; Gr only sizes the bands


@dataclass(frozen=True)
class Context:
    id: str
    Np: int
    L: int
    r: int
    step: int                   # of the 3 x 3 LED grid
    Gr: int                     # rows per block of the row pass (batched: sequences per block C)
    family: str
    kernel: str                 # what the context's objCrop plan launches
    flags: int = 0
    path: int = fpm_amd.PATH_AUTO
    env: dict = field(default_factory=dict)   # environment at fpm_create
    bands: tuple = ()           # () = all seven
    n_patch_of: dict = field(default_factory=dict)  # band id -> n_patch where it is not the default

    @property
    def fp16(self):
        return bool(self.flags & fpm_amd.FLAG_SPEC_FP16)

    @property
    def hscale(self):
        """fp16 storage scale 2^-ceil(log2 Np^2) (fpm_state.hpp)."""
        e = 0
        while (1 << e) < self.Np * self.Np:
            e += 1
        return 2.0 ** -e

    def n_patch(self, band):
        return self.n_patch_of.get(band, 2 if self.L <= 1024 else 1)

    def problem(self, band):
        x0, y0, order = grid_geometry(self.Np, self.L, 3, self.step)
        return fpm_amd.Problem(self.Np, self.L, order, x0, y0, self.r, 5, 10, n_patch=self.n_patch(band),
                               path=self.path, flags=self.flags)


FP16, GENERAL = fpm_amd.FLAG_SPEC_FP16, fpm_amd.PATH_GENERAL
BIG = ("full", "lo_hi", "upper_only", "straddle")
CONTEXTS = (
    Context("L512", 256, 512, 33, 24, 4, REGS, "k_crop_rows/cols<2>"),
    Context("L768", 256, 768, 33, 24, 4, REGS, "k_crop_rows/cols<3>"),
    Context("L1024", 256, 1024, 33, 24, 4, REGS, "k_crop_rows/cols<4>: the per-half strip load"),
    Context("L600", 200, 600, 26, 20, 12, REGS, "c600"),
    Context("L360", 90, 360, 30, 25, 6, REGS, "c360"),
    Context("L4096", 1024, 4096, 333, 100, 16, C4K, "c4k fp32", bands=BIG, n_patch_of={"full": 2}),
    Context("L4096h", 1024, 4096, 333, 100, 16, C4K, "c4k fp16", flags=FP16, bands=BIG),
    Context("L4096b", 1024, 4096, 333, 100, 2, BATCHED, "k_fft_batch C 2", env={"FPM_NO_CROP4K": "1"},
            bands=("straddle",)),
    Context("L3000", 2700, 3000, 4, 50, 2, BATCHED, "k_fft_batch C 2, radix 5", path=GENERAL, bands=BIG),
    Context("L90", 30, 90, 5, 4, 16, BATCHED, "k_fft_batch C 16, tail block of 10 sequences", path=GENERAL),
    Context("L96", 32, 96, 6, 4, 16, BATCHED, "k_fft_batch C 16", path=GENERAL),
    # the C the capacity rule gives falls with L: 810 = 2 3^4 5 has C 8 and 2430 = 2 3^5 5 has C 4, each with a last
    # block of 2 sequences; 5400 = 2^3 3^3 5^2 is the smallest L whose block holds one sequence
    Context("L810", 30, 810, 5, 4, 8, BATCHED, "k_fft_batch C 8, tail block of 2 sequences", path=GENERAL),
    Context("L2430", 30, 2430, 5, 4, 4, BATCHED, "k_fft_batch C 4, tail block of 2 sequences", path=GENERAL),
    # 233 MB per array in complex64: two bands
    Context("L5400", 30, 5400, 5, 4, 1, BATCHED, "k_fft_batch C 1", path=GENERAL, bands=("lo_hi", "straddle")),
    Context("L192", 64, 192, 10, 6, 16, BATCHED, "k_fft_batch C 16", path=GENERAL),
    Context("L96h", 32, 96, 6, 4, 16, BATCHED, "k_fft_batch C 16, fp16 input", flags=FP16),
    Context("L768h", 256, 768, 33, 24, 16, BATCHED, "k_fft_batch C 16, fp16 input", flags=FP16),
)
BY_ID = {c.id: c for c in CONTEXTS}
assert len(BY_ID) == len(CONTEXTS)

BANDS = ("full", "one_row", "lo_hi", "hi_lo", "upper_only", "lower_only", "straddle")


def band(ctx, name):
    """(sy0, sy1, sx0, sx1), inclusive; H = L / 2 is the half / piece boundary of
    the column passes and the row the spectrum's centre sits on."""
    L, H, Gr = ctx.L, ctx.L // 2, ctx.Gr
    rows, cols = {
        "full": ((0, L - 1), (0, L - 1)),                      # no masking at all
        "one_row": ((H, H), (H - 3, H + 3)),                   # one live group in one block
        "lo_hi": ((0, Gr), (L - 7, L - 1)),                    # both spectrum edges; a full block and one live row
        "hi_lo": ((L - 2 * Gr, L - 1), (0, 6)),                # the opposite edges; exactly two blocks
        "upper_only": ((3, H - 1), (1, L - 2)),                # ends on the boundary; the other half has no live row
        "lower_only": ((H, L - 2), (H - 5, H + 9)),            # starts on the boundary; first half empty
        "straddle": ((H - 1, H), (H - H // 3, H + H // 3 + 1)),  # two rows across it; column edges inside a strip
    }[name]
    cols = (max(cols[0], 0), min(cols[1], L - 1))
    return rows + cols


def cases():
    """(context, band id) of every case, in table order."""
    return [(c, b) for c in CONTEXTS for b in (c.bands or BANDS)]


def case_id(ctx, name):
    return f"{ctx.id}-{name}"


def make_input(ctx, name):
    """complex64 [n_patch][L][L], read-only: the centred spectrum of the case,
    NaN outside the band."""
    sy0, sy1, sx0, sx1 = band(ctx, name)
    B, L = ctx.n_patch(name), ctx.L
    rng = np.random.default_rng(zlib.crc32(case_id(ctx, name).encode()))
    shape = (B, sy1 - sy0 + 1, sx1 - sx0 + 1)
    re, im = rng.standard_normal(shape, np.float32), rng.standard_normal(shape, np.float32)
    if ctx.fp16:
        hs = np.float32(ctx.hscale)
        re, im = (v.astype(np.float16).astype(np.float32) / hs for v in (re, im))
        for v in (re, im):  # the fp16 store is exact
            assert np.array_equal((v * hs).astype(np.float16).astype(np.float32), v * hs)
    spec = np.full((B, L, L), np.nan + 1j * np.nan, np.complex64)
    spec[:, sy0:sy1 + 1, sx0:sx1 + 1] = re + 1j * im
    spec.setflags(write=False)
    return spec


def masked(spec):
    """The input with zeros in place of the NaNs (same dtype)."""
    return np.where(np.isnan(spec.real), 0, spec).astype(spec.dtype)


def reference(spec):
    """complex128 [n_patch][L][L]: objCrop of the case."""
    return np.stack([np.fft.ifft2(np.fft.ifftshift(masked(s).astype(np.complex128))) for s in spec])
