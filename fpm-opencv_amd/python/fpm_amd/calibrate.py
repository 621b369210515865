"""LED calibration on a live Solver: positions (calibrate_positions) and
brightness (calibrate_gains, at the end of this file).

LED position calibration: one window-search step.

A wrong illumination angle puts an LED's sub-aperture window a pixel or a few
away from where the data says it is, and that LED's row of the residual
(Solver.residual) stands out.  The cure is a window search: evaluate the
data-fidelity error E of the CURRENT state with the LED's window moved to the
neighbouring integer positions (Solver.residual_at, one batched sweep on the
GPU for all LEDs and candidates), keep the best, and go on iterating with the
corrected table (Solver.set_crops; the state is kept).

One table serves all patches of a context, so a candidate's score is its E
summed over the patches.
"""
from __future__ import annotations

import numpy as np


def neighbourhood(radius: int) -> np.ndarray:
    """The (2R+1)^2 integer offsets (dx, dy) with |dx|, |dy| <= R as int32
    [n_off][2], (0, 0) first, then by growing dx^2 + dy^2 (dy, then dx, within
    one distance): the first minimum of a row of scores is the tie rule of
    calibrate_positions."""
    R = int(radius)
    if R < 0:
        raise ValueError(f"radius={radius}")
    offs = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    offs.sort(key=lambda o: (o[0] * o[0] + o[1] * o[1], o[1], o[0]))
    return np.array(offs, np.int32)


def probe_list(crops, order, L: int, Np: int, offsets):
    """The entries of a window search as (pos, dx, dy, off) int32 arrays:
    for every position of order[] each offset (off = its index in `offsets`)
    whose window stays inside the L x L spectrum, LED-major -- an LED's
    candidates are adjacent, so its stack image is read while still cached.
    Candidates that would leave the spectrum (0 <= crop + d <= L - Np fails)
    are left out."""
    x0, y0 = (np.asarray(c, np.int64) for c in crops)
    pos, dx, dy, off = [], [], [], []
    for i, led in enumerate(order):
        for j, (ox, oy) in enumerate(np.asarray(offsets, np.int64)):
            x, y = x0[led] + ox, y0[led] + oy
            if 0 <= x <= L - Np and 0 <= y <= L - Np:
                pos.append(i)
                dx.append(ox)
                dy.append(oy)
                off.append(j)
    return tuple(np.array(a, np.int32) for a in (pos, dx, dy, off))


def choose(sums: np.ndarray) -> np.ndarray:
    """Per row of the scores [n][n_off] (offsets in neighbourhood order, +inf
    where a candidate was left out) the offset index to move to: the first
    minimum if it is strictly smaller than the score at (0, 0), else 0."""
    best = np.argmin(sums, axis=1)
    rows = np.arange(len(sums))
    return np.where(sums[rows, best] < sums[:, 0], best, 0)


def calibrate_positions(solver, radius: int = 1) -> dict:
    """One search-and-apply step of radius `radius` on an initialised Solver.

    Every used LED moves to the candidate whose patch-summed E is strictly
    smaller than at (0, 0); ties go to the smaller dx^2 + dy^2, then to list
    order.  The new table is then installed with set_crops; if that refuses
    it, FpmError is raised and the table stays as it was.  A stack index that
    occurs at several positions of order[] has one window: it moves by the
    decision of its first position (the others' scores are the same bits).

    Returns dict(offsets [n_off][2], shift [n_order][2] (dx, dy) per position,
    table float64 [n_order][n_off][n_patch] of E (+inf: candidate outside the
    spectrum), before / after [n_order] the patch sums at (0, 0) and at the
    chosen candidate, moved = LEDs whose window changed, ms = the probe
    sweep's event time)."""
    p = solver.prob
    order = [int(v) for v in p.order]
    x0, y0 = solver.crops()
    offsets = neighbourhood(radius)
    pos, dx, dy, off = probe_list((x0, y0), order, p.L, p.np_, offsets)
    d = solver.residual_at(pos, dx, dy)
    table = np.full((len(order), len(offsets), p.n_patch), np.inf)
    table[pos, off] = d["err"]
    sums = table.sum(axis=-1)
    pick = choose(sums)
    shift = offsets[pick]
    nx, ny = x0.copy(), y0.copy()
    seen = set()
    for i, led in enumerate(order):
        if led not in seen:
            seen.add(led)
            nx[led] += shift[i, 0]
            ny[led] += shift[i, 1]
        else:  # report what its window did
            first = order.index(led)
            pick[i], shift[i] = pick[first], shift[first]
    moved = int(np.count_nonzero((nx != x0) | (ny != y0)))
    if moved:
        solver.set_crops(nx, ny)
    rows = np.arange(len(order))
    return dict(offsets=offsets, shift=shift.astype(np.int32), table=table, before=sums[:, 0].copy(),
                after=sums[rows, pick], moved=moved, ms=d["ms"])


# ---- LED brightness ---------------------------------------------------------------
# A wrong LED brightness (the LEDs of a dome differ, fluctuate between exposures
# and fall off with angle; dark-field frames are divided by a nominal exposure
# multiplier) scales an image by h^2, and that LED's row of E / S stands out
# just as a misplaced one does.  The cure is a per-image amplitude factor g
# (Solver.set_gains): the solver then uses g sqrt(I) wherever it used sqrt(I).
# With Q = sum |psi|^2, C = sum |psi| sqrt(I) and S = sum I of the current
# state (Solver.moments, one sweep on the GPU), E(g) = Q - 2 g C + g^2 S, so
# the best factor for an image is C / S.


def gain_error(g, Q, C, S):
    """E(g) = Q - 2 g C + g^2 S, elementwise."""
    g = np.asarray(g, np.float64)
    return Q - 2.0 * g * C + g * g * S


def estimate_gains(order, old, Q, C, S, clip=(0.25, 4.0)) -> np.ndarray:
    """The rule of calibrate_gains on given moments: `old` float [n_stack][B],
    Q / C / S float64 [n_order][B] (row i = order[i]).  Returns the new table.

    g^ = C / S for every (LED, patch) that is used and has S > 0; the others
    keep their gain.  A stack index that occurs at several positions of
    order[] takes its first position's value.  Gain and object share a scale
    (g -> s g, O -> s O changes nothing), so each patch's estimates are then
    multiplied by one factor that makes the S-weighted mean of g^2 over them
    1, and clipped to [lo, hi]."""
    lo, hi = float(clip[0]), float(clip[1])
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError(f"clip={clip}: want 0 < lo <= hi < inf")
    new = np.array(old, np.float64)
    C, S = np.asarray(C, np.float64), np.asarray(S, np.float64)
    est = np.zeros(new.shape, bool)
    w = np.zeros(new.shape)
    seen = set()
    for i, led in enumerate(int(v) for v in order):
        if led in seen:
            continue
        seen.add(led)
        ok = S[i] > 0
        new[led, ok] = C[i, ok] / S[i, ok]
        est[led] = ok
        w[led, ok] = S[i, ok]
    for b in range(new.shape[1]):
        m = est[:, b]
        den = float(np.sum(w[m, b] * new[m, b] ** 2))
        if den > 0:
            new[m, b] = np.clip(new[m, b] * np.sqrt(np.sum(w[m, b]) / den), lo, hi)
        else:  # nothing to estimate from (the model is dark everywhere): leave the patch alone
            new[m, b] = np.asarray(old, np.float64)[m, b]
    return new.astype(np.float32)


def calibrate_gains(solver, clip=(0.25, 4.0)) -> dict:
    """One estimate-and-apply step on an initialised Solver (estimate_gains on
    Solver.moments(), installed with Solver.set_gains).

    Returns dict(old, new float32 [n_stack][n_patch], model / cross / ref
    float64 [n_order][n_patch], before / after [n_order][n_patch] =
    Q - 2 g C + g^2 S at the old and new gains of each position's LED, ms =
    the moments sweep's event time)."""
    order = np.asarray(solver.prob.order, np.int64)
    old = solver.gains()
    m = solver.moments()
    Q, Cx, S = m["model"], m["cross"], m["ref"]
    new = estimate_gains(order, old, Q, Cx, S, clip)
    solver.set_gains(new)
    return dict(old=old, new=new, model=Q, cross=Cx, ref=S, before=gain_error(old[order], Q, Cx, S),
                after=gain_error(new[order], Q, Cx, S), ms=m["ms"])
