"""Inputs of the fpm_set_state tests: plain data and builders, no GPU.

The shapes are the rows of schedules.KERNELS that have the S2-init1-cv case
(11 LED steps over a 3 x 3 grid with repeats, two iterations): every
LED-update kernel at its smallest structured shape.

seed_pupil     a centred pupil that is not a support disk: nonzero outside the
               disk (so the library's mask is observable), its maximum
               off-centre and not 1 (so max|P| must be rebuilt, not assumed).
seed_spectrum  fpm_init's spectrum plus noise on every element of the case's
               live band (so tiles fpm_init leaves at zero carry a maximum),
               exactly zero outside it.

tests/test_state_cases.py shows on the CPU that these are cases: fp32 carries
them with a tenth of the parity bound to spare, and the mask changes the
result far beyond the bound.
"""
from __future__ import annotations

import functools

import numpy as np

import restate_step
import schedules

TAG = "S2-init1-cv"
CASES = tuple(c for c in schedules.CASES if c.tag == TAG)
BY_ROW = {c.row.name: c for c in CASES}
ROWS = tuple(BY_ROW)
GENERAL_ROWS = tuple(n for n in ROWS if n.startswith("general"))
FUSED_ROWS = tuple(n for n in ROWS if n.startswith("fused"))
NOISE = 0.02   # of max|spec|
SEED = 7


def seed_pupil(Np, r, variant=0):
    """Centred complex64 [Np][Np].  With k = index - Np/2, rho^2 = (kx^2 + ky^2) / r^2:
    P = (0.7 + 0.5 (kx/r) exp(-rho^2)) exp(i (0.8 (2 rho^2 - 1) + 0.3 ky/r)).
    variant v > 0 (per-patch pupils) scales the defocus term by 1 + v / 4."""
    k = (np.arange(Np) - Np // 2).astype(np.float64)
    ky, kx = np.meshgrid(k, k, indexing="ij")
    rho2 = (kx * kx + ky * ky) / float(r * r)
    amp = 0.7 + 0.5 * (kx / r) * np.exp(-rho2)
    ph = 0.8 * (1.0 + variant / 4.0) * (2.0 * rho2 - 1.0) + 0.3 * ky / r
    return (amp * np.exp(1j * ph)).astype(np.complex64)


def support_centred(Np, r):
    k = np.arange(Np) - Np // 2
    return (k[:, None] ** 2 + k[None, :] ** 2) <= r * r


def seed_spectrum(case, patch=0):
    """Un-centred complex64 [L][L]: restate_step.initial_state in complex64 plus
    complex N(0, 1) noise of amplitude NOISE max|spec| on the live band."""
    return _seed_spectrum(_geometry(case), patch)


def _geometry(case):
    r = case.row
    return (r.Np, r.L, r.r, r.B, case.x0, case.y0, case.order, case.init_pos)


@functools.lru_cache(maxsize=8)
def _seed_spectrum(geo, patch):
    Np, L, r, B, x0, y0, order, init_pos = geo
    case = next(c for c in CASES if _geometry(c) == geo)
    objF, _ = restate_step.initial_state(case.stack()[:, patch], order, Np, L, r, init_pos, dtype=np.complex64)
    spec = np.fft.fftshift(objF)
    sy0, sy1, sx0, sx1 = case.band()
    rng = np.random.default_rng(SEED + patch)
    h, w = sy1 - sy0 + 1, sx1 - sx0 + 1
    noise = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
    spec = spec.astype(np.complex128)
    spec[sy0:sy1 + 1, sx0:sx1 + 1] += NOISE * np.abs(spec).max() * noise
    out = np.fft.ifftshift(spec.astype(np.complex64))
    out.setflags(write=False)
    return out


def seed_state(case):
    """(objF [B][L][L], pupil [Np][Np] unmasked) of every patch of the case."""
    r = case.row
    return np.stack([seed_spectrum(case, b) for b in range(r.B)]), seed_pupil(r.Np, r.r)


def iterate(case, objF, pupil, iters, patch=0, dtype=np.complex128):
    """restate_step.iterate on the case's stack and tables from the given state of one patch."""
    r = case.row
    return restate_step.iterate(objF, pupil, case.stack()[:, patch], case.order, case.x0, case.y0, r.Np, r.L, r.r,
                                case.delta1, case.delta2, iters, all_channels=case.all_channels, dtype=dtype)


# ---- .npy files for fpmMain --init-pupil / --init-objf -------------------------------------
def npy_bytes(a, version=(1, 0), fortran=False, descr=None, shape=None):
    """A .npy file image of `a` with the header written by hand: version 1.0 or
    2.0, C or Fortran order, `descr` overriding the dtype string and `shape`
    the shape the header claims."""
    a = np.asarray(a)
    d = descr or a.dtype.str
    hdr = f"{{'descr': '{d}', 'fortran_order': {bool(fortran)}, 'shape': {tuple(shape or a.shape)!r}, }}"
    pre = 10 if version == (1, 0) else 12
    pad = (-(pre + len(hdr) + 1)) % 64
    hdr = (hdr + " " * pad + "\n").encode("latin1")
    n = len(hdr).to_bytes(2 if version == (1, 0) else 4, "little")
    data = a.tobytes(order="F" if fortran else "C")
    return b"\x93NUMPY" + bytes(version) + n + hdr + data
