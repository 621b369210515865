"""Focus measures and autofocus on top of Solver.refocus (fpm_refocus).

The library returns three sums per plane and patch over the interior
R = [margin, L - margin)^2 of a = |u_z|; the measures are composed here, on
the host, and which one suits a sample is the caller's choice:
    N = |R|,  m = sum_a / N,  v = sum_a2 / N - m^2
    nvar    normalised variance  v / m^2
    tamura  Tamura coefficient   sqrt(sqrt(v) / m)
    grad    gradient energy      sum_g / sum_a2
An amplitude object is sharpest where these peak (pick="max"); a phase object
shows the least amplitude contrast in focus (pick="min").
"""
from __future__ import annotations

import numpy as np

MEASURES = ("nvar", "tamura", "grad")


def bin_frequency(lam: float, L: int, ps: float) -> float:
    """fl = lambda / (L ps): the normalised frequency of one spectrum bin, ps
    the high-resolution pixel size in lambda's unit (fpm_host's ps)."""
    return float(lam) / (int(L) * float(ps))


def measures(sums: dict, L: int, margin: int) -> dict:
    """dict(nvar, tamura, grad), each shaped like the sums ([nz][n_patch]), from
    Solver.refocus's sums over [margin, L - margin)^2."""
    N = float((int(L) - 2 * int(margin)) ** 2)
    sa, sa2, sg = (np.asarray(sums[k], np.float64) for k in ("sum_a", "sum_a2", "sum_g"))
    m = sa / N
    v = np.maximum(sa2 / N - m * m, 0.0)   # rounding can leave a flat plane at -1e-17
    return dict(nvar=v / (m * m), tamura=np.sqrt(np.sqrt(v) / m), grad=sg / sa2)


def pick_planes(values, pick: str = "max") -> np.ndarray:
    """Index [n_patch] of the best plane of values [nz][n_patch]."""
    if pick not in ("max", "min"):
        raise ValueError(f"pick {pick!r}: want 'max' or 'min'")
    v = np.asarray(values)
    return (v.argmax(0) if pick == "max" else v.argmin(0)).astype(np.int64)


def autofocus(solver, z, lam: float, ps: float, measure: str = "nvar", pick: str = "max", margin: int = 8):
    """Sweep the planes z (1-D, in lambda's unit) with sums only, choose every
    patch's plane by `measure`, then fetch every patch at its own z from one
    per-patch call.  Returns dict(index [n_patch], z [n_patch], field complex64
    [n_patch][L][L], values [nz][n_patch] of the chosen measure, sums)."""
    if measure not in MEASURES:
        raise ValueError(f"measure {measure!r}: want one of {MEASURES}")
    z = np.asarray(z, np.float64).ravel()
    L = solver.prob.L
    fl = bin_frequency(lam, L, ps)
    _, sums = solver.refocus(z / lam, fl, margin=margin, planes=False)
    values = measures(sums, L, margin)[measure]
    idx = pick_planes(values, pick)
    field, _ = solver.refocus((z[idx] / lam)[None, :], fl, margin=margin, sums=False)
    return dict(index=idx, z=z[idx], field=field[0], values=values, sums=sums)
