"""Case table of the per-pixel LED-step tests: plain data and builders, no GPU.

Two LED steps (n_order 2) from an installed state, on every LED-update kernel,
compared pixel by pixel with restate_step.iterate in complex128.
tests/test_step_cases.py shows on the CPU that the table holds cases;
tests/test_gpu_step.py runs it on the device.

rows      every row of state_cases.ROWS on its S2 3 x 3 grid and stack, and
          fused_np90_r42 on a 3 x 3 grid of step 45 whose corner LED (8) reaches
          row 177 of L 180: the spectrum's partial tile.
seed      a white spectrum: complex N(0, 1) on the whole live band of the
          case's order, exactly zero outside it, one draw per patch, scaled so
          that |psi| ~ sqrt(mean I) (of the brightest image used); magnitudes
          below a quarter of the scale are raised to it (FLOOR).  On the Np 1024
          shape, which has an fp16-storage row, every value is an exact fp16
          times 1 / hscale, so the fp32 and the fp16 row install the same state
          and share a yardstick.
          The pupil is state_cases.seed_pupil, installed unmasked.
planted   one pixel of 4 x the white rms amplitude, the global maximum:
          "outside"  in the band, outside the disks of both LEDs of the order
                     (as far from their centres as the band allows): max|objF|
                     of the pupil coefficient is not in what the step writes
          "inside"   in the first LED's disk: the step itself changes the maximum
stack     the row's stack with a 3 x 3 block of every image at 0 and another at 65535
orders    (4, 8), (0, 1), (4, 4) for one iteration, (4, 8) for two
params    plain   delta1 5, delta2 10, eps float32(1e-10): the project's values
          deltas  delta1 = float32(median |O_seed|^2 over the band), delta2 0.5
          eps     the deltas values and eps = float32(16 sqrt(mean I))
          deltas and eps under both readings of the cv::add scalar
          (FPM_FLAG_SCALAR_RE_ONLY).  eps of the order of |psi| is left out on
          purpose: psi + eps (1 + i) passes near zero there and complex64 itself
          loses the result.
          The Np 1024 rows take plain on (4, 8) in both variants and eps on
          (4, 8) for two iterations under both readings ("inside").

The bound of a pixel k of one array (objF or pupil) of one patch:
    bound(k) = C[row] 2^-24 s(k),  s(k) = |ref(k)| + rms over the touched pixels of |ref - seed|
where a pixel is touched if the complex128 result differs from the seed.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass

import numpy as np

import fpm_amd
import restate_step
import schedules
import state_cases as sc
from tools.synth import grid_geometry

# The largest error of the complex64 yardstick (restate_step.iterate with
# dtype=complex64 under a numpy whose np.fft keeps float32) over every case and
# patch of the rows of one shape (Np, L, r) (Np 1024: patch 0), in units of
# 2^-24 s(k); tests/test_step_cases.py prints it and holds it to C / 8.
C64_WORST_UNITS = {
    (32, 96, 6): 7.2, (30, 90, 5): 8.6, (90, 180, 10): 9.0, (200, 600, 12): 8.8, (256, 512, 33): 10.9,
    (256, 512, 40): 13.6, (1024, 2048, 100): 4.3, (90, 180, 42): 40.7,
}
# C: 8 x that, rounded up to a power of two.  The 8 is for what separates a kernel
# from the complex64 yardstick: other transform factorisations, v_rcp / v_rsq
# at 1 ulp, maxima carried at 4 ulp.  It comes from the
# reference alone and is never raised to fit a kernel.
# One constant per shape, not one for the table: the r 42 row alone would put a
# single C at 512 (its disk fills two thirds of the window, so one pixel of psi
# near zero under the order (4, 4) with delta2 0.5 moves every pixel of objF by
# 20 - 40 units in complex64 itself), and at 512 the sensitivity caps of
# tests/test_step_cases.py no longer hold on the Np 90 and Np 200 rows.  No
# shape's C exceeds that single one.
C_OF_SHAPE = {k: float(2.0 ** np.ceil(np.log2(8.0 * v))) for k, v in C64_WORST_UNITS.items()}
UNIT = 2.0 ** -24

RE_ONLY = fpm_amd.FLAG_SCALAR_RE_ONLY
ROWS = sc.ROWS + ("fused_np90_r42",)
R42_STEP = 45
ORDERS = (((4, 8), 1), ((0, 1), 1), ((4, 4), 1), ((4, 8), 2))
VARIANTS = ("outside", "inside")
PARAMS = (("plain", 0), ("deltas", 0), ("deltas", RE_ONLY), ("eps", 0), ("eps", RE_ONLY))
# (order, iters, pset, flags, variant) of the Np 1024 rows
BIG = (((4, 8), 1, "plain", 0, "outside"), ((4, 8), 1, "plain", 0, "inside"),
       ((4, 8), 2, "eps", 0, "inside"), ((4, 8), 2, "eps", RE_ONLY, "inside"))
PLANT = 4.0            # of the white rms amplitude
# The magnitudes of N(0,1) + i N(0,1) below FLOOR (3 % of the pixels) are raised to
# it, phase kept.  With a large eps the amplitude replacement all but removes psi,
# the pupil update of a pixel goes with |O|^3, and under the order (4, 4) nothing
# else reaches that pixel: the Rayleigh tail alone leaves 0.2 % of the support
# with an update below 4 bound(k), twice the cap.
FLOOR = 0.25
PLANT_PHASE = 0.7
SEED = 11
BLOCK_ZERO, BLOCK_FULL = (1 / 3, 1 / 4), (2 / 3, 1 / 2)    # block corners as fractions of Np (+1, +3 for the second)


def _r42_base():
    row = schedules.ROWS["fused_np90_r42"]
    x0, y0, _ = grid_geometry(row.Np, row.L, 3, R42_STEP)
    return schedules.Case(row, "S2", sc.TAG, tuple(int(v) for v in x0), tuple(int(v) for v in y0),
                          schedules.S2_ORDER, 2, 5, 10, init_pos=1, unused=(6, 7))


BASE = dict(sc.BY_ROW, fused_np90_r42=_r42_base())
# the constant of bound(k) by row
C = {n: C_OF_SHAPE[(b.row.Np, b.row.L, b.row.r)] for n, b in BASE.items()}


@dataclass(frozen=True)
class StepCase:
    name: str          # the kernel row
    order: tuple
    iters: int
    pset: str          # plain / deltas / eps
    flags: int         # 0 or RE_ONLY
    variant: str       # outside / inside

    @property
    def id(self):
        o = "".join(str(i) for i in self.order)
        return f"{self.name}-o{o}x{self.iters}-{self.pset}{'-reonly' if self.flags else ''}-{self.variant}"

    @property
    def row(self):
        return BASE[self.name].row

    @property
    def all_channels(self):
        return not self.flags

    @property
    def geo(self):
        """The schedules.Case of the row's grid with this case's order: band(), box(), stack() of the
        unedited measurements, and what maxima_check.check_maxima reads."""
        return dataclasses.replace(BASE[self.name], order=self.order, iters=self.iters, flags=self.flags, unused=())

    @property
    def shape(self):
        """What the seed and the yardstick depend on: rows that agree in it share both."""
        b = BASE[self.name]
        r = b.row
        return (r.Np, r.L, r.r, r.B, b.x0, b.y0)

    def scalars(self):
        """(delta1, delta2, eps) as the doubles the problem carries."""
        if self.pset == "plain":
            return 5.0, 10.0, float(np.float32(1e-10))
        d1 = float(np.float32(_median_o2(self.shape, self.order, self.variant)))
        eps = float(np.float32(16.0 * np.sqrt(_mean_i(self.shape)))) if self.pset == "eps" else float(np.float32(1e-10))
        return d1, 0.5, eps

    def problem(self):
        r = self.row
        b = BASE[self.name]
        d1, d2, eps = self.scalars()
        return fpm_amd.Problem(r.Np, r.L, np.array(self.order), np.array(b.x0), np.array(b.y0), r.r, d1, d2,
                               n_patch=r.B, init_pos=1, eps=eps, path=r.path, flags=r.flags | self.flags)

    def stack(self):
        return _stack(self.shape)

    def seed(self, patch):
        """Un-centred complex64 [L][L], read-only."""
        return _seed(self.shape, self.order, self.variant, patch)

    def planted(self):
        """(y, x) of the planted pixel in the centred spectrum."""
        return _planted(self.shape, self.order, self.variant)

    def disks(self):
        """bool [L][L], centred: the union of the disks of the order's LEDs (what the steps may write)."""
        return _disks(self.shape, self.order)

    def circle(self):
        """bool [L][L], centred: the pixels with kx^2 + ky^2 == r^2 about an LED of the order."""
        return _disks(self.shape, self.order, on_circle=True)


def cases(name):
    if BASE[name].row.Np >= 1024:
        return tuple(StepCase(name, o, it, p, f, v) for o, it, p, f, v in BIG)
    return tuple(StepCase(name, o, it, p, f, v) for o, it in ORDERS for p, f in PARAMS for v in VARIANTS)


CASES = tuple(c for n in ROWS for c in cases(n))


# ---- stack ----------------------------------------------------------------------------------
def _base_of(shape):
    return next(b for n, b in BASE.items() if StepCase(n, (4, 8), 1, "plain", 0, "outside").shape == shape)


def blocks(Np):
    """((y, x) of the 3 x 3 block at 0, (y, x) of the one at 65535)."""
    (a, b), (c, d) = BLOCK_ZERO, BLOCK_FULL
    return (int(Np * a), int(Np * b)), (int(Np * c) + 1, int(Np * d) + 3)


@functools.lru_cache(maxsize=2)
def _stack(shape):
    st = _base_of(shape).stack().copy()
    (zy, zx), (fy, fx) = blocks(shape[0])
    st[..., zy:zy + 3, zx:zx + 3] = 0
    st[..., fy:fy + 3, fx:fx + 3] = 65535
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def _mean_i(shape):
    """"mean I" of the seed's amplitude and of eps: the mean of the brightest image
    among those the orders use.  Where the grid step exceeds the radius (the
    r 42 row) all images but the centre's are dark field, and a seed scaled to the
    mean over the whole stack is so far below the bright-field measurement that
    the object update with delta2 0.5 grows past the planted maximum."""
    used = sorted({led for o, _ in ORDERS for led in o})
    return float(_stack(shape)[used].mean(axis=(2, 3), dtype=np.float64).max())


# ---- seed -----------------------------------------------------------------------------------
def _geo(shape, order):
    return dataclasses.replace(_base_of(shape), order=order, unused=())


def _fp16_exact(shape):
    return any(b.row.fp16 for b in BASE.values() if (b.row.Np, b.row.L, b.row.r) == shape[:3])


def hscale(Np):
    """fpm_state.hpp: the power of two the fp16 storage scales the spectrum by."""
    return 2.0 ** -int(np.ceil(np.log2(Np * Np)))


@functools.lru_cache(maxsize=None)
def _disks(shape, order, on_circle=False):
    Np, L, r = shape[:3]
    g = _geo(shape, order)
    yy, xx = np.mgrid[0:L, 0:L]
    m = np.zeros((L, L), bool)
    for led in set(order):
        d2 = (yy - (g.y0[led] + Np // 2)) ** 2 + (xx - (g.x0[led] + Np // 2)) ** 2
        m |= (d2 == r * r) if on_circle else (d2 <= r * r)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _planted(shape, order, variant):
    Np, L, r = shape[:3]
    g = _geo(shape, order)
    cy = [g.y0[led] + Np // 2 for led in order]
    cx = [g.x0[led] + Np // 2 for led in order]
    if variant == "inside":
        return cy[0] + r // 2, cx[0] - r // 3
    sy0, sy1, sx0, sx1 = g.band()
    yy, xx = np.mgrid[sy0:sy1 + 1, sx0:sx1 + 1]
    d2 = np.minimum.reduce([(yy - a) ** 2 + (xx - b) ** 2 for a, b in zip(cy, cx)])
    assert d2.max() > r * r
    y, x = np.unravel_index(int(np.argmax(d2)), d2.shape)
    return sy0 + int(y), sx0 + int(x)


def white_amplitude(shape):
    """a of seed = a (N(0,1) + i N(0,1)): with n pixels in the disk, Parseval gives
    mean |psi|^2 = n 2 a^2 mean|P|^2 / Np^4, which is set to mean I."""
    Np, _, r = shape[:3]
    S = sc.support_centred(Np, r)
    p2 = float((np.abs(sc.seed_pupil(Np, r).astype(np.complex128)) ** 2)[S].sum())
    return Np * Np * np.sqrt(_mean_i(shape) / (2.0 * p2))


@functools.lru_cache(maxsize=64)
def _seed(shape, order, variant, patch):
    Np, L = shape[:2]
    sy0, sy1, sx0, sx1 = _geo(shape, order).band()
    rng = np.random.default_rng(SEED + patch)
    h, w = sy1 - sy0 + 1, sx1 - sx0 + 1
    a = white_amplitude(shape)
    z = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
    z = a * z * np.maximum(1.0, FLOOR / np.abs(z))
    py, px = _planted(shape, order, variant)
    z[py - sy0, px - sx0] = PLANT * a * np.sqrt(2.0) * np.exp(1j * PLANT_PHASE)
    z = z.astype(np.complex64)
    if _fp16_exact(shape):
        hs = np.float32(hscale(Np))
        re, im = ((v * hs).astype(np.float16).astype(np.float32) / hs for v in (z.real, z.imag))
        z = (re + 1j * im).astype(np.complex64)
    spec = np.zeros((L, L), np.complex64)
    spec[sy0:sy1 + 1, sx0:sx1 + 1] = z
    out = np.ascontiguousarray(np.fft.ifftshift(spec))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _median_o2(shape, order, variant):
    sy0, sy1, sx0, sx1 = _geo(shape, order).band()
    o = np.fft.fftshift(_seed(shape, order, variant, 0))[sy0:sy1 + 1, sx0:sx1 + 1].astype(np.complex128)
    return float(np.median(np.abs(o) ** 2))


def seed_state(case):
    """(objF [B][L][L] un-centred, pupil [Np][Np] unmasked): what set_state takes."""
    r = case.row
    return np.stack([case.seed(b) for b in range(r.B)]), sc.seed_pupil(r.Np, r.r)


def masked_pupil(case):
    """The pupil as the library installs it: seed_pupil on the support, 0 outside."""
    r = case.row
    return (sc.seed_pupil(r.Np, r.r) * sc.support_centred(r.Np, r.r)).astype(np.complex64)


# ---- yardstick ------------------------------------------------------------------------------
def iterate(case, objF, pupil, patch, dtype=np.complex128, **kw):
    """restate_step.iterate of the case from a given state of one patch (objCrop left out)."""
    r = case.row
    b = BASE[case.name]
    d1, d2, eps = case.scalars()
    return restate_step.iterate(objF, pupil, case.stack()[:, patch], case.order, b.x0, b.y0, r.Np, r.L, r.r, d1, d2,
                                case.iters, eps=eps, all_channels=case.all_channels, dtype=dtype, objcrop=False, **kw)


def yardstick(case, patch, dtype=np.complex128):
    """From the seed with the masked pupil: dict(objF, pupil, record); objF is the
    band of the CENTRED spectrum only (outside it the result is the seed's zero,
    asserted here), so a cached Np 1024 result is 1 MB and not 64."""
    return _yardstick(case.shape, case.order, case.iters, case.pset, case.flags, case.variant, patch,
                      np.dtype(dtype).name)


@functools.lru_cache(maxsize=400)
def _yardstick(shape, order, iters, pset, flags, variant, patch, dtype):
    name = next(n for n in BASE if StepCase(n, order, iters, pset, flags, variant).shape == shape)
    case = StepCase(name, order, iters, pset, flags, variant)
    rec = []
    out = iterate(case, case.seed(patch), masked_pupil(case), patch, dtype=np.dtype(dtype), record=rec)
    spec = np.fft.fftshift(out["objF"])
    sy0, sy1, sx0, sx1 = case.geo.band()
    band = spec[sy0:sy1 + 1, sx0:sx1 + 1].copy()
    spec[sy0:sy1 + 1, sx0:sx1 + 1] = 0
    assert not spec.any(), "the yardstick wrote outside the band"
    return dict(objF=band, pupil=out["pupil"], record=tuple(rec))


def band_of(case, objF):
    """The band of the centred spectrum of an un-centred [L][L] array."""
    sy0, sy1, sx0, sx1 = case.geo.band()
    return np.fft.fftshift(objF)[sy0:sy1 + 1, sx0:sx1 + 1]


# ---- the bound and check 2's comparison ------------------------------------------------------
def touched(ref, seed):
    return np.asarray(ref, np.complex128) != np.asarray(seed, np.complex128)


def scale(ref, seed):
    """s(k) of one array of one patch, float64; (s, touched)."""
    ref, seed = np.asarray(ref, np.complex128), np.asarray(seed, np.complex128)
    t = ref != seed
    rms = float(np.sqrt(np.mean(np.abs(ref - seed)[t] ** 2))) if t.any() else 0.0
    return np.abs(ref) + rms, t


def units(got, ref, seed):
    """|got - ref| in units of 2^-24 s(k), float64, and the touched mask."""
    s, t = scale(ref, seed)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.abs(np.asarray(got, np.complex128) - np.asarray(ref, np.complex128)) / (UNIT * s)
    return np.where(s > 0, u, 0.0), t


def compare(got, ref, seed, c):
    """Check 2 with the row's constant c = C[row]: (largest |got - ref| / bound
    over the touched pixels, its index).  The arrays pass if the ratio is <= 1."""
    u, t = units(got, ref, seed)
    u = np.where(t, u, 0.0) / c
    k = np.unravel_index(int(np.argmax(u)), u.shape)
    return float(u[k]), tuple(int(v) for v in k)
