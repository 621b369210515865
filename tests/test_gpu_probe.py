"""LED position calibration on the GPU: fpm_residual_at (the residual of the
current state with windows moved), fpm_set_crops / fpm_get_crops (the crop
table of a live context) and fpm_amd.calibrate.

Yardsticks (tests/test_probe.py shows on the CPU that they are yardsticks):
  parity     float64 numpy evaluation of the DOWNLOADED state with the shifted
             window (window_reference), at fpm_residual's own bound
             |dE| <= 2e-5 sqrt(E Q) + 1e-10 Q and ref == sum I exactly
             (tests/test_gpu_residual.py derives it).  Where the model is
             exactly dark (Q = 0: a window outside the live band) the exact
             value is E = S, asserted to the bit.
  one path   bit equality: (i, 0, 0) against fpm_residual, a list against its
             permutation, its pieces and FPM_RES_BATCH=1.
  set_crops  bit equality with a context created with the new table; mid-run,
             restate_step.iterate from the downloaded state with the new
             table at the project's one-iteration bound 1e-5 (relative L2), and
             the carried-maxima invariants of tests/test_gpu_schedules.py.
  calibrate  the decisions of the same rule evaluated in float64, wherever
             float64's margin exceeds the parity bounds (float64_decisions).
Each context asserts its kernel and, through fpm_debug_get_plan, its plan.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import residual_check
import restate_step
import schedules
from fpm_amd import calibrate
from fpm_oracle import rel_l2
from test_gpu_residual import (BIN, COLS, FUSED, G_LDS, G_REG256, G_REG1024, GENERAL, NP256_KERNELS, R_LDS, R_REG, _case,
                               _context, _env, _plan, _solver)
from maxima_check import check_maxima as _check_maxima
from test_probe import CALIB, float64_decisions, float64_tables, window_reference
from tools.synth import make_stack

pytestmark = pytest.mark.gpu

OFFSETS = ((0, 0), (1, 0), (0, -1), (-2, 3))


def _band(Np, L, r, order, x0, y0):
    """(sy0, sy1, sx0, sx1), inclusive: the live band fpm_create plans (fpm_state.hpp)."""
    b = [L // 2 - r, L // 2 + r, L // 2 - r, L // 2 + r]
    for led in set(int(i) for i in order):
        yc, xc = int(y0[led]) + Np // 2, int(x0[led]) + Np // 2
        b = [min(b[0], yc - r), max(b[1], yc + r), min(b[2], xc - r), max(b[3], xc + r)]
    return max(b[0], 0), min(b[1], L - 1), max(b[2], 0), min(b[3], L - 1)


def _union(a, b):
    return min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3])


# ---- 1. parity ------------------------------------------------------------------------
FP16 = fpm_amd.FLAG_SPEC_FP16
PARITY = {  # case arguments, iterations, kernels, plan, environment, six entries only
    "general_np32_wave": ((32, 96, 6, 5, 4, 3, 7), dict(path=GENERAL), 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                          COLS["wave"], False),
    "general_np32_tiled": ((32, 96, 6, 5, 4, 3, 7), dict(path=GENERAL), 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                           COLS["tiled"], False),
    # L 120: at L 90 no window of Np 30 lies wholly outside this grid's band
    "fused_small_np30_r6": ((30, 120, 6, 5, 9, 2, 71 + 30 + 6), dict(path=FUSED), 2, (fpm_amd.KERNEL_FUSED_SMALL,),
                            _plan(30), {}, False),
    "fused_np90_r30": ((90, 360, 30, 4, 22, 2, 91 + 30), dict(path=FUSED), 2, (fpm_amd.KERNEL_FUSED_NP90,), _plan(9), {},
                       False),
    "fused_np200_r26": ((200, 600, 26, 3, 30, 2, 61 + 26, 10, 3), dict(path=FUSED), 2, (fpm_amd.KERNEL_FUSED_NP200,),
                        _plan(10), {}, False),
    "fused_np256_r33_reg": ((256, 512, 33, 5, 20, 2, 40 + 33, 10, 3), dict(path=FUSED), 2, NP256_KERNELS,
                            _plan(16, -1, R_REG), {}, False),
    "fused_np256_r33_lds": ((256, 512, 33, 5, 20, 2, 40 + 33, 10, 3), dict(path=FUSED), 2, NP256_KERNELS,
                            _plan(16, -1, R_LDS), {"FPM_RES_LDS": "1"}, False),
    "general_np256_r84": ((256, 1024, 84, 3, 100, 2, 40 + 84, 10, 3), dict(path=GENERAL), 2, (fpm_amd.KERNEL_GENERAL,),
                          _plan(16, G_REG256, R_REG), {}, False),
    "general_np1024_fp16": ((1024, 4096, 333, 2, 600, 1, 95), dict(flags=FP16), 1, (fpm_amd.KERNEL_GENERAL,),
                            _plan(1024, G_REG1024), {}, True),
}


def _entries(prob, short=False):
    """(pos, dx, dy) arrays and the index of the entry whose window lies wholly
    outside the live band: the first, the last and a repeated position of
    order[], the offsets of OFFSETS, a window flush against the spectrum edge
    (y = 0) and one outside the band (not flush: x = 1 or L - Np - 1)."""
    Np, L, r, order = prob.np_, prob.L, prob.radius, [int(i) for i in prob.order]
    n = len(order)
    first, last, mid = 0, n - 1, n // 2
    ents = [(first,) + OFFSETS[0], (first,) + OFFSETS[1], (last,) + OFFSETS[2], (last,) + OFFSETS[3]]
    if not short:
        ents += [(mid,) + OFFSETS[0], (mid,) + OFFSETS[1], (mid,) + OFFSETS[0], (mid,) + OFFSETS[3],
                 (first,) + OFFSETS[2], (last,) + OFFSETS[1]]
    ents.append((first, 0, -int(prob.y0[order[first]])))
    _, _, sx0, sx1 = _band(Np, L, r, order, prob.x0, prob.y0)
    far = [x for x in (1, L - Np - 1) if x + Np // 2 + r < sx0 or x + Np // 2 - r > sx1]
    assert far, "no window of this geometry lies outside the band"
    ents.append((last, far[0] - int(prob.x0[order[last]]), 0))
    pos, dx, dy = (np.array(c, np.int32) for c in zip(*ents))
    return pos, dx, dy, len(ents) - 1


def _check_entries(tag, d, ref, outside=None):
    E, Q, S = ref
    np.testing.assert_array_equal(d["ref"], S)
    dark = Q == 0
    if outside is not None:
        assert dark[outside].all(), (tag, "the window outside the band carries signal")
    np.testing.assert_array_equal(d["err"][dark], S[dark], err_msg=f"{tag}: E = S where the model is dark")
    delta, bnd = np.abs(d["err"] - E), residual_check.bound(E, Q)
    ratio = np.divide(delta, bnd, out=np.zeros_like(delta), where=bnd > 0)
    print(f"probe {tag}: max |dE|/bound {ratio.max():.3e} ({int(dark.sum())} of {dark.size} dark; {d['ms']:.3f} ms)")
    assert np.all(np.isfinite(d["err"])) and np.all(delta[~dark] <= bnd[~dark]), (tag, float(ratio.max()))


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_float64(name):
    args, kw, iters, kernels, plan, env, short = PARITY[name]
    prob, stack = _case(*args, **kw)
    pos, dx, dy, outside = _entries(prob, short)
    assert len(pos) == (6 if short else 12)
    with _solver(prob, stack, iters, kernels, plan, **env) as s:
        state = s.download(objCrop=False, support=False)
        d = s.residual_at(pos, dx, dy)
    ref = window_reference(state, stack, prob.np_, prob.order, prob.x0, prob.y0, pos, dx, dy)
    _check_entries(name, d, ref, outside)
    assert (ref[1] > 0).any()
    if not short:   # the repeated entry returns the same bits
        np.testing.assert_array_equal(d["err"][4], d["err"][6])


# ---- 2. one path ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_one_path(which):
    tag, (prob, stack), kernels = _context(which)
    n = len(prob.order)
    idx, zero = np.arange(n), np.zeros(n, np.int32)
    pos = np.arange(3 * n + 1) % n                  # longer than any scratch sized for n_order
    off = np.array([OFFSETS[(k // n + k) % 4] for k in range(3 * n + 1)])
    got = {}
    for batch in (None, "1"):
        env = {"FPM_RES_BATCH": batch} if batch else {}
        with _solver(prob, stack, 1, kernels, **env) as s:
            sweep = s.residual()
            ident = s.residual_at(idx, zero, zero)
            rev = s.residual_at(idx[::-1], zero, zero)
            long = s.residual_at(pos, off[:, 0], off[:, 1])
            pieces = [s.residual_at(pos[k:k + 7], off[k:k + 7, 0], off[k:k + 7, 1]) for k in range(0, 3 * n + 1, 7)]
            for k in ("err", "ref"):
                np.testing.assert_array_equal(ident[k], sweep[k], err_msg=f"{tag}: (i, 0, 0) {k}")
                np.testing.assert_array_equal(rev[k], sweep[k][::-1], err_msg=f"{tag}: reversed {k}")
                np.testing.assert_array_equal(np.concatenate([p[k] for p in pieces]), long[k],
                                              err_msg=f"{tag}: {3 * n + 1} entries against their pieces, {k}")
                np.testing.assert_array_equal(s.residual()[k], sweep[k])     # the sweep after the probes
            assert (long["err"][:n] != long["err"][n:2 * n]).any()           # the offsets matter
            got[batch] = (sweep, long)
    for a, b in zip(got[None], got["1"]):
        for k in ("err", "ref"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: FPM_RES_BATCH=1 {k}")


# ---- 3. read-only ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_probe_is_read_only(which):
    tag, (prob, stack), kernels = _context(which)
    pos, dx, dy, _ = _entries(prob)
    with _solver(prob, stack, 1, kernels) as s:
        before, stack_before = s.download(), s.download_stack()
        mx0, t0, k0 = s.debug_maxima(), s.timing(), s.clock()
        a = s.residual_at(pos, dx, dy)
        b = s.residual_at(pos, dx, dy)
        for k in ("err", "ref"):
            np.testing.assert_array_equal(a[k], b[k])
        after, mx1 = s.download(), s.debug_maxima()
        for k in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=f"{tag} {k}")
        for k in ("tmax", "dirty", "pmax"):
            np.testing.assert_array_equal(mx0[k], mx1[k], err_msg=f"{tag} {k}")
        np.testing.assert_array_equal(s.download_stack(), stack_before)
        np.testing.assert_array_equal(stack_before, stack)
        t1, k1 = s.timing(), s.clock()
        for f, _ in fpm_amd.fpm_timing._fields_:
            assert getattr(t0, f) == getattr(t1, f), f
        for f, _ in fpm_amd.fpm_clock._fields_:
            assert getattr(k0, f) == getattr(k1, f), f
        assert t1.led_launches > 0
        s.run(1)
        with_probe = s.download()
    with _solver(prob, stack, 1, kernels) as s:
        s.run(1)
        without = s.download()
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(with_probe[k], without[k], err_msg=f"{tag} {k}")


# ---- 4. / 5. the crop table of a live context --------------------------------------------
def _row_solver(row, prob):
    """A context of schedules.KERNELS row `row` (its environment, kernel, mode and kind asserted)."""
    with _env(**dict(row.env)):
        s = fpm_amd.Solver(prob)
    try:
        info = s.info()
        assert info.fused_kernel == row.kernel, (info.fused_kernel, row.kernel)
        assert info.wg_per_patch == row.wg, info.wg_per_patch
        assert s.debug_plan()["general_kind"] == row.general_kind
    except BaseException:
        s.close()
        raise
    return s


@functools.lru_cache(maxsize=None)
def _tables(name, midrun):
    """(A, B, order, (dx, dy) per stack index) for a row: A a 3 x 3 grid, B = A
    with three LEDs moved by one or two pixels.
      midrun False   the centre LED and two edge LEDs moved along their edge: no
                     LED leaves A's band, A and B plan the same band
      midrun True    the grid shifted so that the band's low edge lies on a
                     16-pixel tile boundary, and the corner LED 0 moved outwards
                     by (-2, -1): the band grows by a tile row and a tile column
                     on the low side, which renumbers the fused kernels' band
                     tiles"""
    row = schedules.ROWS[name]
    Np, L, r = row.Np, row.L, row.r
    step = max(1, round(r / 1.5))
    c = L // 2 - Np // 2
    o = -((c - step + Np // 2 - r) % 16) if midrun else 0
    x0 = np.array([c + o + ix * step for iy in (-1, 0, 1) for ix in (-1, 0, 1)])
    y0 = np.array([c + o + iy * step for iy in (-1, 0, 1) for ix in (-1, 0, 1)])
    order = sorted(range(9), key=lambda i: ((x0[i] - c - o) ** 2 + (y0[i] - c - o) ** 2, i))
    move = {0: (-2, -1), 4: (1, 0), 5: (0, 2)} if midrun else {4: (1, -2), 1: (2, 0), 3: (0, -1)}
    d = np.zeros((9, 2), np.int64)
    for led, v in move.items():
        d[led] = v
    xb, yb = x0 + d[:, 0], y0 + d[:, 1]
    assert min(xb.min(), yb.min()) >= 0 and max(xb.max(), yb.max()) <= L - Np
    a, b = _band(Np, L, r, order, x0, y0), _band(Np, L, r, order, xb, yb)
    if midrun:
        u = _union(a, b)
        assert (u[0] // 16, u[2] // 16) == (a[0] // 16 - 1, a[2] // 16 - 1), (a, u)
    else:
        assert a == b
    return (x0, y0), (xb, yb), order, d


@functools.lru_cache(maxsize=4)
def _truth_stack(Np, L, r, B, xb, yb):
    st = make_stack(Np, L, r, np.array(xb), np.array(yb), n_patch=B, seed=20261019)
    st.setflags(write=False)
    return st


def _problem(row, order, x0, y0):
    return fpm_amd.Problem(row.Np, row.L, np.array(order), x0, y0, row.r, 5, 10, n_patch=row.B, path=row.path,
                           flags=row.flags)


SAME_PLAN = ["general_lds", "fused_small", "fused_np90", "fused_np256", "fused_np256_split", "fused_np256_dist"]


@pytest.mark.parametrize("name", SAME_PLAN)
def test_set_crops_is_create(name):
    row = schedules.ROWS[name]
    (xa, ya), (xb, yb), order, _ = _tables(name, False)
    stack = _truth_stack(row.Np, row.L, row.r, row.B, tuple(xb), tuple(yb))
    outs = []
    for first in ((xa, ya), (xb, yb)):
        with _row_solver(row, _problem(row, order, *first)) as s:
            if first[0] is xa:
                np.testing.assert_array_equal(s.crops(), (xa, ya))
                s.set_crops(xb, yb)
            np.testing.assert_array_equal(s.crops(), (xb, yb))
            s.upload(stack)
            s.init()
            s.run(2)
            outs.append((s.download(), s.residual()))
    (a, ra), (b, rb) = outs
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
    for k in ("err", "ref"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=f"{name} residual {k}")


class _Band:
    """What maxima_check.check_maxima reads of a case: the row and the live band."""

    def __init__(self, row, band):
        self.row, self._band = row, band

    def band(self):
        return self._band


MID_RUN = ["general_lds", "general_reg256", "fused_small", "fused_np256", "fused_np256_dist"]


@pytest.mark.parametrize("name", MID_RUN)
def test_set_crops_between_runs(name):
    row = schedules.ROWS[name]
    Np, L, r = row.Np, row.L, row.r
    (xa, ya), (xb, yb), order, d = _tables(name, True)
    stack = _truth_stack(Np, L, r, row.B, tuple(xb), tuple(yb))
    band = _union(_band(Np, L, r, order, xa, ya), _band(Np, L, r, order, xb, yb))
    n = len(order)
    with _row_solver(row, _problem(row, order, xa, ya)) as s:
        s.upload(stack)
        s.init()
        s.run(1)
        one = s.download()
        probe = s.residual_at(np.arange(n), d[order, 0], d[order, 1])
        s.set_crops(xb, yb)
        np.testing.assert_array_equal(s.crops(), (xb, yb))
        kept = s.download()
        for k in ("objF", "objCrop", "pupil"):      # the state is kept
            np.testing.assert_array_equal(kept[k], one[k], err_msg=f"{name} {k}")
        dirty = _check_maxima(s, _Band(row, band), "after fpm_set_crops")
        sweep = s.residual()
        for k in ("err", "ref"):
            np.testing.assert_array_equal(sweep[k], probe[k], err_msg=f"{name}: row i against (i, dx_i, dy_i), {k}")
        s.run(1)
        two = s.download()
        _check_maxima(s, _Band(row, band), "after the run with the new table")
    worst = 0.0
    for b in range(row.B):
        ref = restate_step.iterate(one["objF"][b], one["pupil"][b], stack[:, b], order, xb, yb, Np, L, r, 5, 10, 1)
        for k in ("objF", "objCrop", "pupil"):
            e = rel_l2(two[k][b], ref[k])
            worst = max(worst, e)
            assert e < 1e-5, (name, b, k, e)
        # the old table's step from the same state is far from it: a stale graph or table would show
        stale = restate_step.iterate(one["objF"][b], one["pupil"][b], stack[:, b], order, xa, ya, Np, L, r, 5, 10, 1)
        assert rel_l2(stale["objF"], ref["objF"]) > 1e-4
    print(f"{name}: one iteration after fpm_set_crops, max rel L2 {worst:.2e} (bound 1e-5); {dirty} dirty tiles "
          f"carried over the band's growth")


# ---- 6. errors ------------------------------------------------------------------------
def test_errors():
    import ctypes as C
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    L, Np, n = prob.L, prob.np_, len(prob.order)
    lib = fpm_amd.load_library()
    dp = C.POINTER(C.c_double)

    def raw(s, ents, err=True, ref=True, n_=None):
        """fpm_residual_at itself; the output arrays start as -1 (untouched on a refusal)."""
        p = (fpm_amd.fpm_probe * max(len(ents), 1))(*[fpm_amd.fpm_probe(*e) for e in ents])
        e, r = np.full((max(len(ents), 1), prob.n_patch), -1.0), np.full((max(len(ents), 1), prob.n_patch), -1.0)
        rc = lib.fpm_residual_at(s._h, p, len(ents) if n_ is None else n_, e.ctypes.data_as(dp) if err else None,
                                 r.ctypes.data_as(dp) if ref else None, None)
        return rc, e, r, lib.fpm_last_error().decode()

    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.residual_at([0], [0], [0])
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        s.set_crops(*s.crops())                     # legal before fpm_init
        s.init()
        s.run(1)
        want = s.residual()
        x0, y0 = s.crops()
        led = int(prob.order[2])
        bad = [
            ("right of the spectrum", [(0, 0, 0), (2, L - Np - int(x0[led]) + 1, 0)], "entry 1"),
            ("above the spectrum", [(2, 0, -int(y0[led]) - 1)], "entry 0"),
            ("pos = n_order", [(0, 0, 0), (0, 1, 0), (n, 0, 0)], "entry 2"),
            ("pos < 0", [(-1, 0, 0)], "entry 0"),
        ]
        for what, ents, names in bad:
            rc, e, r, msg = raw(s, ents)
            assert rc == fpm_amd.FPM_ERR_INVAL and names in msg, (what, rc, msg)
            assert np.all(e == -1.0) and np.all(r == -1.0), what     # validated before the first launch
            np.testing.assert_array_equal(s.residual()["err"], want["err"], err_msg=what)
        assert raw(s, [], n_=0)[0] == fpm_amd.FPM_ERR_INVAL
        assert raw(s, [(0, 0, 0)], n_=-3)[0] == fpm_amd.FPM_ERR_INVAL
        assert raw(s, [(0, 0, 0)], err=False, ref=False)[0] == fpm_amd.FPM_ERR_INVAL
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.residual_at([], [], [])
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL
        # the window flush against the edge is legal; err or ref alone is enough
        rc, e, r, _ = raw(s, [(2, L - Np - int(x0[led]), 0)], ref=False)
        assert rc == fpm_amd.FPM_OK and np.all(e >= 0) and np.all(r == -1.0)
        rc, e, r, _ = raw(s, [(2, 0, 0)], err=False)
        assert rc == fpm_amd.FPM_OK and np.all(e == -1.0)
        np.testing.assert_array_equal(r[0], want["ref"][2])
        # a table that validation refuses leaves the table as it was
        for k, v in ((3, -1), (5, L - Np + 1)):
            for axis in (0, 1):
                t = [x0.copy(), y0.copy()]
                t[axis][k] = v
                with pytest.raises(fpm_amd.FpmError) as ei:
                    s.set_crops(*t)
                assert ei.value.code == fpm_amd.FPM_ERR_INVAL and f"LED {k}" in str(ei.value)
                np.testing.assert_array_equal(s.crops(), (x0, y0))
        ip = C.POINTER(C.c_int32)
        assert lib.fpm_set_crops(s._h, None, y0.ctypes.data_as(ip)) == fpm_amd.FPM_ERR_INVAL
        with pytest.raises(ValueError):
            s.set_crops(x0[:-1], y0[:-1])
        for k in ("err", "ref"):
            np.testing.assert_array_equal(s.residual()[k], want[k])
        s.run(1)                                     # and the context still runs


def test_set_crops_refuses_a_table_that_plans_another_context():
    """Np 96 on the small-patch fused kernel: its LDS holds the band's tile
    maxima, so two LEDs sent to opposite corners of an L 1152 spectrum (68 x 68
    band tiles) no longer fit and fpm_create would pick the general path."""
    Np, L, r = 96, 1152, 10
    c = L // 2 - Np // 2
    prob = fpm_amd.Problem(Np, L, [0, 1], np.array([c, c + 4]), np.array([c, c + 4]), r, 5, 10, n_patch=1)
    far = np.array([0, L - Np]), np.array([0, L - Np])
    with fpm_amd.Solver(prob) as s:
        assert s.info().fused_kernel == fpm_amd.KERNEL_FUSED_SMALL
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.set_crops(*far)
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "LED-update kernel" in str(ei.value)
        np.testing.assert_array_equal(s.crops(), (prob.x0, prob.y0))
        assert s.info().fused_kernel == fpm_amd.KERNEL_FUSED_SMALL
    with fpm_amd.Solver(fpm_amd.Problem(Np, L, [0, 1], *far, r, 5, 10, n_patch=1)) as s:
        assert s.info().fused_kernel == fpm_amd.KERNEL_GENERAL


def test_capturing_stream_is_refused():
    """As fpm_residual (test_residual_on_a_capturing_stream_is_refused): both
    calls block, so FPM_ERR_INVAL before anything is enqueued or changed."""
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    pos, dx, dy, _ = _entries(prob)
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        want, sweep = s.residual_at(pos, dx, dy), s.residual()
        x0, y0 = s.crops()
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        for call in (lambda: s.residual_at(pos, dx, dy), lambda: s.set_crops(x0 + 1, y0)):
            g = torch.cuda.CUDAGraph()
            with pytest.raises(fpm_amd.FpmError) as ei:
                with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                    call()
            assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        np.testing.assert_array_equal(s.crops(), (x0, y0))
        np.testing.assert_array_equal(s.residual_at(pos, dx, dy)["err"], want["err"])   # no longer capturing
        s.set_stream(None)
        np.testing.assert_array_equal(s.residual_at(pos, dx, dy)["err"], want["err"])
        np.testing.assert_array_equal(s.residual()["err"], sweep["err"])


# ---- 7. the calibration step ------------------------------------------------------------
def test_calibration_step_agrees_with_float64():
    c = CALIB
    _, (wx, wy), order = c.tables()
    stack = c.stack()
    prob = fpm_amd.Problem(c.Np, c.L, np.array(order), wx, wy, c.r, c.d1, c.d2, n_patch=c.B)
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(c.iters)
        state = s.download(objCrop=False, support=False)
        before = s.residual()
        out = calibrate.calibrate_positions(s, radius=1)
        after = s.residual()
        nx, ny = s.crops()
        s.run(1)                                   # and the iterations go on
    E, Q = float64_tables(state, stack, c.Np, c.L, order, wx, wy)
    pick, sure = float64_decisions(E, Q)
    print(f"calibration: float64 decides {int(sure.sum())} of {len(order)} LEDs clearly, {int((pick != 0).sum())} move; "
          f"the device moved {out['moved']}, probe {out['ms']:.3f} ms")
    assert (~sure).sum() <= len(order) // 10
    offs = out["offsets"]
    np.testing.assert_array_equal(offs, calibrate.neighbourhood(1))
    np.testing.assert_array_equal(out["shift"][sure], offs[pick][sure])
    assert out["moved"] == np.count_nonzero(out["shift"].any(axis=1)) > 0
    # the table itself meets the parity bound
    fin = np.isfinite(E)
    assert fin.all() and out["table"].shape == E.shape      # this grid touches no spectrum edge
    assert np.all(np.abs(out["table"] - E) <= residual_check.bound(E, Q))
    # the table in use is the old one plus the shifts
    for i, led in enumerate(order):
        assert (nx[led], ny[led]) == (wx[led] + out["shift"][i, 0], wy[led] + out["shift"][i, 1])
    # no LED's patch-summed residual grew, and each is the chosen candidate's sum to the bit
    b0, b1 = before["err"].sum(axis=-1), after["err"].sum(axis=-1)
    np.testing.assert_array_equal(out["before"], b0)
    np.testing.assert_array_equal(out["after"], b1)
    assert np.all(b1 <= b0) and np.all(b1[out["shift"].any(axis=1)] < b0[out["shift"].any(axis=1)])
    np.testing.assert_array_equal(after["ref"], before["ref"])


# ---- 8. CLI ---------------------------------------------------------------------------
def test_cli_calibrate_leds(tmp_path):
    from dataset_fixture import make_dataset
    from fpm_amd import host
    ds = make_dataset(str(tmp_path / "data"))
    hd = host.Dataset(ds["json"])        # the table the CLI starts from, in processing order
    hd.scan()
    hd.geometry()
    initial = np.stack(hd.crops(), 1)
    hd.close()
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    iters = 3
    outs = {}
    for tag, extra in (("both", ["--calibrate-leds", "1", "--residual"]), ("alone", ["--calibrate-leds", "1"]),
                       ("plain", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], str(iters), "--out", str(out)] + extra, capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = json.loads((out / "result.json").read_text())
    plain = outs["plain"]
    assert "led_calibration" not in plain
    for tag in ("both", "alone"):
        meta = outs[tag]
        cal = meta["led_calibration"]
        assert set(cal) == {"radius", "shift_total", "moved_per_iteration", "crop_x0", "crop_y0", "probe_ms"}
        used = meta["leds_used"]
        assert cal["radius"] == 1 and cal["probe_ms"] > 0
        assert len(cal["moved_per_iteration"]) == iters - 1          # after every iteration but the last
        assert all(0 <= m <= used for m in cal["moved_per_iteration"])
        shift = np.array(cal["shift_total"])
        assert shift.shape == (used, 2) and np.abs(shift).max() <= iters - 1
        final = np.stack([cal["crop_x0"], cal["crop_y0"]], 1)
        assert final.shape == initial.shape == (used, 2)
        np.testing.assert_array_equal(final, initial + shift)
        assert (sum(cal["moved_per_iteration"]) == 0) == (not shift.any())
        assert set(meta) - {"led_calibration", "residual"} == set(plain)
    # the sweep is read-only: with and without --residual the search decides the same
    assert {k: v for k, v in outs["both"]["led_calibration"].items() if k != "probe_ms"} == \
        {k: v for k, v in outs["alone"]["led_calibration"].items() if k != "probe_ms"}
    assert len(outs["both"]["residual"]["per_iteration"]) == iters + 1
