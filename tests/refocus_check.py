"""The yardstick of fpm_refocus, in float64 numpy (no GPU, no library).

Definition (include/fpm_hip.h): with objF un-centred as download() returns it
and signed bin indices ky, kx in [-L/2, L/2),
    s   = fl^2 (kx^2 + ky^2),   fl = lambda / (L ps)
    H   = exp(+i 2 pi zl sqrt(1 - s)) for s <= 1,  0 for s > 1 (evanescent)
    u_z = IDFT2(objF H) / L^2 = np.fft.ifft2(objF H)
and the focus sums over R = [margin, L - margin)^2 of a = |u_z|:
    sum_a, sum_a2, sum_g = sum of squared differences of horizontally and
    vertically adjacent a, over the pairs wholly in R.
Planes are computed from a DOWNLOADED objF, so both sides read the same fp32
state; the sums are evaluated on a given plane (the GPU's own), so they test
the reduction and not the transform again.

The bounds:
  PLANE_BOUND = objcrop_cases.BOUND + 5e-7 relative L2: what the project
    already holds objCrop's transforms to, plus H's fp32 rounding and one
    complex multiply (about 4 * 2^-24 per element).
  SUM_BOUND = 1e-6 relative for sum_a and sum_a2: a is the kernels' fp32
    magnitude (<= 1.5 ulp = 9e-8 relative), everything after it is double.
  GRAD_BOUND = 2e-5 relative for sum_g: an error e = 1e-6 a per magnitude moves
    sum_g by at most 2 sqrt(sum_g) 2 e sqrt(sum_a2) (Cauchy-Schwarz), relative
    to sum_g that is 4e-6 sqrt(sum_a2 / sum_g) / 2 <= 2e-5 where
    sum_g / sum_a2 >= GRAD_CONDITION = 1e-2.
    The bound is conditional: the relative error of sum_g grows as
    1 / sqrt(sum_g / sum_a2), and a flatter interior than the condition allows
    (4e-3 turned up in a 2 x 2 interior) is outside what these tests show;
    fpm_hip.h says so to the caller.
"""
from __future__ import annotations

import numpy as np

import objcrop_cases

PLANE_BOUND = objcrop_cases.BOUND + 5e-7
SUM_BOUND = 1e-6
GRAD_BOUND = 2e-5
GRAD_CONDITION = 1e-2
MEASURES = ("nvar", "tamura", "grad")


def bins(L):
    """Signed bin index of every un-centred position: [0, L/2) then [-L/2, 0)."""
    k = np.arange(L)
    return np.where(k < L // 2, k, k - L).astype(np.int64)


def transfer(L, zl, fl):
    """H [L][L] complex128 in the un-centred layout of download()'s objF."""
    k = bins(L)
    k2 = (k[:, None] ** 2 + k[None, :] ** 2).astype(np.float64)
    s = (float(fl) * float(fl)) * k2
    live = s <= 1.0
    c = float(zl) * np.sqrt(np.where(live, 1.0 - s, 0.0))
    frac = c - np.rint(c)   # exp(2 pi i c) = exp(2 pi i frac): the integer turns carry no phase
    return np.where(live, np.exp(2j * np.pi * frac), 0.0)


def plane(objF, zl, fl):
    """u_z complex128 [L][L] of one patch's downloaded objF [L][L]."""
    o = np.asarray(objF)
    return np.fft.ifft2(o.astype(np.complex128) * transfer(o.shape[-1], zl, fl))


def planes(objF, zl, fl):
    """[nz][B][L][L] complex128 of objF [B][L][L]; zl [nz] or [nz][B].  A plane
    whose zl entries are all exactly 0 is objCrop itself, the transform of the
    stored spectrum with its evanescent bins (fpm_hip.h): nothing is multiplied."""
    z = np.asarray(zl, np.float64)
    B = len(objF)
    z = np.broadcast_to(z[:, None], (len(z), B)) if z.ndim == 1 else z
    out = []
    for zi in z:
        if not zi.any():
            out.append(np.stack([np.fft.ifft2(np.asarray(o).astype(np.complex128)) for o in objF]))
        else:
            out.append(np.stack([plane(objF[b], zi[b], fl) for b in range(B)]))
    return np.stack(out)


def sums(u, margin):
    """(sum_a, sum_a2, sum_g) float64 over the leading axes of u [...][L][L];
    a = |u| is taken in u's own precision (complex64 -> the fp32 magnitude),
    everything after it in float64."""
    u = np.asarray(u)
    L = u.shape[-1]
    a = np.abs(u).astype(np.float64)[..., margin:L - margin, margin:L - margin]
    dx, dy = np.diff(a, axis=-1), np.diff(a, axis=-2)
    return a.sum((-2, -1)), (a * a).sum((-2, -1)), (dx * dx).sum((-2, -1)) + (dy * dy).sum((-2, -1))


def measures(sum_a, sum_a2, sum_g, L, margin):
    """The three focus measures from the sums (what fpm_amd.focus.measures computes)."""
    N = float((L - 2 * margin) ** 2)
    m = np.asarray(sum_a) / N
    v = np.maximum(np.asarray(sum_a2) / N - m * m, 0.0)
    return dict(nvar=v / (m * m), tamura=np.sqrt(np.sqrt(v) / m), grad=np.asarray(sum_g) / np.asarray(sum_a2))


def band_of(prob):
    """(sy0, sy1, sx0, sx1) inclusive, of the centred spectrum, from the
    geometry: the support boxes (crop0 + Np/2) +- r of the used LEDs united with
    the init placement L/2 +- r (csrc/fpm_state.hpp)."""
    order = np.asarray(prob.order)
    r, h = prob.radius, prob.np_ // 2
    cx = np.concatenate([np.asarray(prob.x0)[order] + h, [prob.L // 2]])
    cy = np.concatenate([np.asarray(prob.y0)[order] + h, [prob.L // 2]])
    return int(cy.min() - r), int(cy.max() + r), int(cx.min() - r), int(cx.max() + r)


def half_band(prob):
    """The band's largest |signed bin index| (rows or columns)."""
    sy0, sy1, sx0, sx1 = band_of(prob)
    H = prob.L // 2
    return max(H - sy0, sy1 - H, H - sx0, sx1 - H)


def band_mask(L, band):
    """bool [L][L] in the UN-CENTRED layout: True on the band's bins."""
    sy0, sy1, sx0, sx1 = band
    m = np.zeros((L, L), bool)
    m[sy0:sy1 + 1, sx0:sx1 + 1] = True
    return np.fft.ifftshift(m)


def scene(L, band, zstar, fl, seed, block=8):
    """The autofocus scene: random blocks of block x block pixels, amplitude 0.2
    or 1.0, on the L x L grid, its spectrum masked to the band (the band-limited
    sharp object) and multiplied by H(-zstar), so propagating by +zstar restores
    it.  Returns (objF complex128 [L][L] un-centred, sharp complex128 [L][L])."""
    rng = np.random.default_rng(seed)
    amp = np.where(rng.random((L // block, L // block)) < 0.5, 0.2, 1.0)
    obj = np.kron(amp, np.ones((block, block)))
    assert obj.shape == (L, L)
    F = np.fft.fft2(obj) * band_mask(L, band)
    # every live bin must propagate (|H| = 1), so H(-z) H(+z) = 1 on the band
    assert ((fl * fl) * (bins(L)[:, None] ** 2 + bins(L)[None, :] ** 2))[band_mask(L, band)].max() <= 1.0
    return F * transfer(L, -zstar, fl), np.fft.ifft2(F)


def rel_l2(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the cases both test files run ------------------------------------------------------
# plane parity: objcrop_cases.CONTEXTS id -> (n_patch, zl)
PARITY_ZL = (0.0, 7.25, -1000.5)
PARITY = {"L512": (3, PARITY_ZL), "L600": (3, PARITY_ZL), "L360": (3, PARITY_ZL), "L90": (3, PARITY_ZL),
          "L96": (3, PARITY_ZL), "L96h": (3, PARITY_ZL), "L768h": (3, PARITY_ZL),
          "L4096": (1, (7.25,)), "L4096h": (1, (7.25,))}
# sums: contexts whose row strips have tails (90 = 5 * 16 + 10, 360 = 22 * 16 + 8, 600 = 37 * 16 + 8), B = 3
SUM_CONTEXTS = ("L90", "L360", "L600")
SUM_ZL = (0.0, 7.25)
# Seeds of their random states.  A 2 x 2 interior of a band-limited speckle field
# can be nearly flat (sum_g / sum_a2 of 4e-3 turned up), which the sum_g bound
# does not cover; these are the first seeds whose planes, as THIS module
# computes them, keep sum_g / sum_a2 >= 3e-2 at every margin
# (tests/test_refocus_check.py holds them to GRAD_CONDITION).
SUM_SEED = {"L90": 10, "L360": 1, "L600": 6}


def sum_margins(L):
    """No margin, an odd one, and the largest legal one (R is 2 x 2)."""
    return (0, 7, (L - 2) // 2)


def context_problem(cid, B):
    """The fpm_amd.Problem of an objcrop_cases context at B patches."""
    import dataclasses
    ctx = objcrop_cases.BY_ID[cid]
    return dataclasses.replace(ctx, n_patch_of={"full": B}).problem("full"), ctx


def random_state(prob, ctx, band, seed):
    """objF complex64 [B][L][L] (un-centred): N(0,1) + i N(0,1) inside the band
    of the centred spectrum, zero outside; on an fp16-storage context drawn as
    exact fp16 / hscale, as objcrop_cases.make_input does.  And a pupil of ones."""
    sy0, sy1, sx0, sx1 = band
    B, L = prob.n_patch, prob.L
    rng = np.random.default_rng(seed)
    shape = (B, sy1 - sy0 + 1, sx1 - sx0 + 1)
    re, im = rng.standard_normal(shape, np.float32), rng.standard_normal(shape, np.float32)
    if ctx is not None and ctx.fp16:
        hs = np.float32(ctx.hscale)
        re, im = (v.astype(np.float16).astype(np.float32) / hs for v in (re, im))
    spec = np.zeros((B, L, L), np.complex64)
    spec[:, sy0:sy1 + 1, sx0:sx1 + 1] = re + 1j * im
    objF = np.ascontiguousarray(np.fft.ifftshift(spec, axes=(1, 2)))
    pupil = np.ones((prob.np_, prob.np_), np.complex64)
    return objF, pupil
