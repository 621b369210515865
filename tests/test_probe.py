"""LED position calibration without a GPU: the boundary (header, library,
Python mirror), the yardsticks of tests/test_gpu_probe.py and the host side of
fpm_amd.calibrate.

  restate_step.iterate   the oracle's loop body from a given state: from the
                         oracle's own initial state it is run_fpm bit for bit,
                         so it can judge a crop table that changes mid-run
  window_reference       float64 E, Q, S of a state for (position, offset)
                         entries: residual_check.reference with the window moved
  float64_decisions      calibrate_positions' rule evaluated on float64 sums,
                         and which decisions a comparison may rely on
  CALIB                  the calibration case of the GPU test; here: float64
                         alone decides at least 90 % of its LEDs clearly
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import fpm_amd
import residual_check
import restate_step
from fpm_amd import calibrate
from fpm_oracle import run_fpm
from tools.synth import grid_geometry, make_stack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the boundary -------------------------------------------------------------------
def test_header_declares_the_calibration_entry_points():
    text = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()
    assert re.search(r"typedef\s+struct\s+fpm_probe\s*\{[^}]*int32_t\s+pos\s*;[^}]*int32_t\s+dx\s*,\s*dy\s*;[^}]*\}\s*"
                     r"fpm_probe\s*;", text)
    assert re.search(r"\bint\s+fpm_residual_at\s*\(\s*fpm_ctx\s*\*\s*\w+\s*,\s*const\s+fpm_probe\s*\*\s*\w+\s*,\s*int\s+"
                     r"\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+fpm_set_crops\s*\(\s*fpm_ctx\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*const\s+"
                     r"int32_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+fpm_get_crops\s*\(\s*const\s+fpm_ctx\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*"
                     r"\*\s*\w+\s*\)\s*;", text)


def test_library_exports_and_mirror_follow():
    so = C.CDLL(fpm_amd.HIP_LIB)
    for name in ("fpm_residual_at", "fpm_set_crops", "fpm_get_crops"):
        assert hasattr(so, name), name
        assert name in fpm_amd.HIP_SYMBOLS
    assert C.sizeof(fpm_amd.fpm_probe) == 12
    for name in ("residual_at", "set_crops", "crops"):
        assert callable(getattr(fpm_amd.Solver, name))


def test_entry_points_refuse_a_null_context():
    lib = fpm_amd.load_library()
    assert lib.fpm_residual_at(None, None, 1, None, None, None) == fpm_amd.FPM_ERR_INVAL
    assert lib.fpm_set_crops(None, None, None) == fpm_amd.FPM_ERR_INVAL
    assert lib.fpm_get_crops(None, None, None) == fpm_amd.FPM_ERR_INVAL


# ---- restate_step -------------------------------------------------------------------
@pytest.mark.parametrize("all_channels", [True, False], ids=["cv", "reonly"])
def test_iterate_from_the_initial_state_is_run_fpm(all_channels):
    Np, L, r, iters = 32, 64, 6, 2
    x0, y0, order = grid_geometry(Np, L, 5, 3)
    stack = make_stack(Np, L, r, x0, y0, n_patch=1, seed=31)[:, 0]
    want = run_fpm(stack, order, x0, y0, Np, L, r, 5, 10, iters, all_channels=all_channels)
    objF, pupil = restate_step.initial_state(stack, order, Np, L, r)
    zero = run_fpm(stack, order, x0, y0, Np, L, r, 5, 10, 0, all_channels=all_channels)
    np.testing.assert_array_equal(objF, zero["objF"])
    np.testing.assert_array_equal(pupil, zero["pupil"])
    got = restate_step.iterate(objF, pupil, stack, order, x0, y0, Np, L, r, 5, 10, iters, all_channels=all_channels)
    for k in ("objF", "objCrop", "pupil", "support"):
        assert got[k].dtype == want[k].dtype
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # one iteration, then one more from the state it returned: the same bits again
    one = restate_step.iterate(objF, pupil, stack, order, x0, y0, Np, L, r, 5, 10, 1, all_channels=all_channels)
    two = restate_step.iterate(one["objF"], one["pupil"], stack, order, x0, y0, Np, L, r, 5, 10, 1,
                               all_channels=all_channels)
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(two[k], want[k], err_msg=k)


# ---- neighbourhood / probe_list -----------------------------------------------------
@pytest.mark.parametrize("R", [0, 1, 2, 3])
def test_neighbourhood(R):
    offs = calibrate.neighbourhood(R)
    assert offs.shape == ((2 * R + 1) ** 2, 2) and offs.dtype == np.int32
    assert tuple(offs[0]) == (0, 0)
    assert len({tuple(o) for o in offs}) == len(offs) and np.abs(offs).max(initial=0) == R
    d2 = (offs.astype(np.int64) ** 2).sum(1)
    assert np.all(np.diff(d2) >= 0)        # the first minimum of a row of scores is the nearest one


def test_probe_list_is_led_major_and_drops_what_leaves_the_spectrum():
    Np, L = 32, 64
    x0, y0, order = grid_geometry(Np, L, 3, 16)       # crops 0, 16, 32: the grid touches 0 and L - Np
    assert x0.min() == 0 and x0.max() == L - Np
    offs = calibrate.neighbourhood(1)
    pos, dx, dy, off = calibrate.probe_list((x0, y0), order, L, Np, offs)
    assert all(a.dtype == np.int32 for a in (pos, dx, dy, off))
    assert np.all(np.diff(pos) >= 0)                  # LED-major: an LED's candidates are adjacent
    for i, led in enumerate(order):
        mine = pos == i
        assert (dx[mine][0], dy[mine][0], off[mine][0]) == (0, 0, 0)     # (0, 0) first
        assert np.all(np.diff(off[mine]) > 0)                            # then in neighbourhood order
        np.testing.assert_array_equal(offs[off[mine]], np.stack([dx[mine], dy[mine]], 1))
        keep = [j for j, (ox, oy) in enumerate(offs)
                if 0 <= x0[led] + ox <= L - Np and 0 <= y0[led] + oy <= L - Np]
        assert off[mine].tolist() == keep
    count = {led: int((pos == i).sum()) for i, led in enumerate(order)}
    corners = [k for k in range(9) if x0[k] in (0, L - Np) and y0[k] in (0, L - Np)]
    edges = [k for k in range(9) if (x0[k] in (0, L - Np)) != (y0[k] in (0, L - Np))]
    assert len(corners) == 4 and len(edges) == 4
    assert all(count[k] == 4 for k in corners) and all(count[k] == 6 for k in edges) and count[4] == 9


def test_choose_moves_only_to_a_strictly_smaller_sum():
    inf = np.inf
    sums = np.array([[5.0, 5.0, 5.0, 7.0],      # nothing smaller: stay
                     [5.0, 4.0, 4.0, 3.0],      # the smallest
                     [5.0, 4.0, 4.0, 4.0],      # a tie: the first in neighbourhood order (the nearest)
                     [5.0, inf, inf, 6.0],      # candidates outside the spectrum never win
                     [5.0, inf, 4.5, inf]])
    assert calibrate.choose(sums).tolist() == [0, 3, 1, 0, 2]


# ---- the float64 yardstick of a probe list --------------------------------------------
def window_reference(state, stack, Np, order, x0, y0, pos, dx, dy):
    """float64 E, Q [n][B] and the integer S of the downloaded state for the
    entries (pos[k], dx[k], dy[k]): residual_check.reference with the window of
    order[pos[k]] at (x0 + dx, y0 + dy)."""
    B = state["objF"].shape[0]
    n = len(pos)
    E, Q, S = np.empty((n, B)), np.empty((n, B)), np.empty((n, B))
    for b in range(B):
        O = np.fft.fftshift(state["objF"][b].astype(np.complex128))
        P = np.fft.ifftshift(state["pupil"][b].astype(np.complex128))
        for k in range(n):
            led = int(order[int(pos[k])])
            xs, ys = int(x0[led]) + int(dx[k]), int(y0[led]) + int(dy[k])
            assert 0 <= xs <= O.shape[1] - Np and 0 <= ys <= O.shape[0] - Np
            a = np.abs(np.fft.ifft2(np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np]) * P))
            I = stack[led, b].astype(np.float64)
            E[k, b] = ((a - np.sqrt(I)) ** 2).sum()
            Q[k, b] = (a * a).sum()
            S[k, b] = float(stack[led, b].astype(np.int64).sum())
    return E, Q, S


def float64_decisions(E, Q):
    """calibrate_positions' rule on float64 tables E, Q [n][n_off][B] (+inf /
    0 where a candidate is left out): the chosen offset index per row, and
    whether a device result must agree with it -- the patch sum of the chosen
    candidate lies below EVERY other candidate's by more than twice the larger
    of the two sums' parity bounds (the sum over patches of
    residual_check.bound), so no error within those bounds can reorder them;
    the runner-up is the closest of the others."""
    sums = E.sum(axis=-1)
    with np.errstate(invalid="ignore"):
        bnd = np.where(np.isfinite(E), residual_check.bound(np.where(np.isfinite(E), E, 0.0), Q), 0.0).sum(axis=-1)
    pick = calibrate.choose(sums)
    rows = np.arange(len(sums))
    margin = sums - sums[rows, pick][:, None] - 2.0 * np.maximum(bnd, bnd[rows, pick][:, None])
    margin[rows, pick] = np.inf
    return pick, margin.min(axis=1) > 0


# ---- the calibration case ---------------------------------------------------------------
class CALIB:
    """5 x 5 LEDs, Np 32 / L 64 / r 6, step 3, two patches: the stack is
    measured at the true table, the context starts from a table with four
    LEDs off by a pixel, and the search runs after four iterations."""
    Np, L, r, B, iters, seed, d1, d2 = 32, 64, 6, 2, 4, 20261019, 5, 10
    WRONG = {7: (1, 0), 11: (0, -1), 13: (-1, 1), 17: (1, 1)}      # stack index -> table error (dx, dy)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def tables(cls):
        x0, y0, order = grid_geometry(cls.Np, cls.L, 5, 3)
        wx, wy = x0.copy(), y0.copy()
        for led, (ex, ey) in cls.WRONG.items():
            wx[led] += ex
            wy[led] += ey
        return (x0, y0), (wx, wy), order

    @classmethod
    @functools.lru_cache(maxsize=None)
    def stack(cls):
        (x0, y0), _, _ = cls.tables()
        st = make_stack(cls.Np, cls.L, cls.r, x0, y0, n_patch=cls.B, seed=cls.seed)
        st.setflags(write=False)
        return st


def float64_tables(state, stack, Np, L, order, x0, y0, radius=1):
    """E, Q [n_order][n_off][B] of the state over neighbourhood(radius); a
    candidate outside the spectrum has E = +inf, Q = 0."""
    offs = calibrate.neighbourhood(radius)
    pos, dx, dy, off = calibrate.probe_list((x0, y0), order, L, Np, offs)
    e, q, _ = window_reference(state, stack, Np, order, x0, y0, pos, dx, dy)
    B = state["objF"].shape[0]
    E, Q = np.full((len(order), len(offs), B), np.inf), np.zeros((len(order), len(offs), B))
    E[pos, off], Q[pos, off] = e, q
    return E, Q


def test_float64_alone_decides_the_calibration_case():
    """The GPU test compares a decision only where float64's margin exceeds the
    parity bounds; here, on the fp64 oracle's state of the same case, at most
    10 % of the LEDs fall short of that."""
    c = CALIB
    _, (wx, wy), order = c.tables()
    stack = c.stack()
    outs = [run_fpm(stack[:, b], order, wx, wy, c.Np, c.L, c.r, c.d1, c.d2, c.iters) for b in range(c.B)]
    state = dict(objF=np.stack([o["objF"] for o in outs]), pupil=np.stack([o["pupil"] for o in outs]))
    E, Q = float64_tables(state, stack, c.Np, c.L, order, wx, wy)
    pick, sure = float64_decisions(E, Q)
    sums = E.sum(-1)
    gap = np.sort(sums, axis=1)
    print(f"calibration case: {int(sure.sum())} of {len(order)} LEDs decided clearly, {int((pick != 0).sum())} move; "
          f"best-to-runner-up gap {100 * ((gap[:, 1] - gap[:, 0]) / gap[:, 0]).min():.2f} % .. "
          f"{100 * ((gap[:, 1] - gap[:, 0]) / gap[:, 0]).max():.2f} % of E")
    assert (~sure).sum() <= len(order) // 10
    assert (pick != 0).any()           # the search has something to do
