"""LED gains without a GPU: the boundary (header, library, Python mirror), the
conditions that make tests/test_gpu_gains.py's cases cases, and the host side
of fpm_amd.calibrate.calibrate_gains.

  headroom   the update cases of tests/gain_cases.py (coarsened stacks, gains
             from {0.5, 1, 2}) restated in complex64 drift less than a tenth of
             the parity bound from the fp64 oracle, as tests/test_schedules.py
             shows for the ungained stacks: a GPU case that misses the bound is
             wrong, not ill-conditioned.  And the oracle on the same stack
             WITHOUT the gains is far away: a kernel that ignores the factor fails.
  moments    the float64 yardstick satisfies E(g) = Q - 2 g C + g^2 S.
  rule       estimate_gains on known moments: estimate, repeats, normalisation,
             clip, S = 0, unused LEDs.
  GAINCAL    float64 alone shows the claim of the calibration test.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fpm_amd
import gain_cases
import oracle_lib
from fpm_amd import calibrate
from fpm_oracle import rel_l2, run_fpm
from gain_cases import GAINCAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the boundary -------------------------------------------------------------------
def test_header_declares_the_gain_entry_points():
    text = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()
    assert re.search(r"^#define\s+FPM_HAS_LED_GAINS\s+1\s*$", text, re.M)
    assert re.search(r"^#define\s+FPM_ABI_VERSION\s+6\s*$", text, re.M)
    assert re.search(r"\bint\s+fpm_set_gains\s*\(\s*fpm_ctx\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+fpm_get_gains\s*\(\s*const\s+fpm_ctx\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+fpm_moments\s*\(\s*fpm_ctx\s*\*\s*\w+\s*,\s*const\s+fpm_probe\s*\*\s*\w+\s*,\s*int\s+\w+\s*"
                     r"(,\s*double\s*\*\s*\w+\s*){4}\)\s*;", text)


def test_library_exports_and_mirror_follow():
    so = C.CDLL(fpm_amd.HIP_LIB)
    for name in ("fpm_set_gains", "fpm_get_gains", "fpm_moments"):
        assert hasattr(so, name), name
        assert name in fpm_amd.HIP_SYMBOLS
    for name in ("set_gains", "gains", "moments"):
        assert callable(getattr(fpm_amd.Solver, name))
    assert callable(calibrate.calibrate_gains)


def test_entry_points_refuse_a_null_context():
    lib = fpm_amd.load_library()
    assert lib.fpm_set_gains(None, None) == fpm_amd.FPM_ERR_INVAL
    assert lib.fpm_get_gains(None, None) == fpm_amd.FPM_ERR_INVAL
    assert lib.fpm_moments(None, None, 0, None, None, None, None) == fpm_amd.FPM_ERR_INVAL


# ---- the update cases -----------------------------------------------------------------
def _inputs(c):
    r = c.row
    return (r.Np, r.L, r.r, c.x0, c.y0, c.order, c.init_pos, c.flags)


def _distinct():
    seen = {}
    for c in gain_cases.UPDATE:
        seen.setdefault(_inputs(c), c)
    return list(seen.values())


def test_update_cases_cover_every_kernel_with_s2():
    rows = [k.name for k in gain_cases.schedules.KERNELS if "S2" in k.schedules]
    assert len(rows) == 12 and [c.row.name for c in gain_cases.UPDATE if c.tag == "S2-init1-cv"] == rows
    assert len(gain_cases.UPDATE) == 12 + 2 * 3
    for c in gain_cases.UPDATE:
        g = gain_cases.step_gains(c)
        assert g.dtype == np.float32 and g.shape == (len(c.x0), c.row.B)
        assert set(np.unique(g)) == set(gain_cases.GAIN_VALUES)       # every value occurs
        st = gain_cases.base_stack(c)
        assert st.max() <= 16380 and st.max() > 8000 and not (st % 4).any()
        assert gain_cases.gained_stack(c).max() <= 65520


@pytest.mark.parametrize("case", _distinct(), ids=lambda c: c.id)
def test_fp32_headroom_with_gains(case):
    """tests/test_schedules.py::test_fp32_headroom on the gained stacks, patch 0."""
    r = case.row
    st = gain_cases.gained_stack(case)[:, 0]
    kw = dict(all_channels=case.all_channels, init_pos=case.init_pos)
    ref = oracle_lib.run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, case.iters, **kw)
    c64 = run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, case.iters,
                  dtype=np.complex64, **kw)
    drift = {k: rel_l2(c64[k], ref[k]) for k in ("objF", "objCrop", "pupil")}
    # the same stack without the gains: what a kernel that drops the factor computes
    plain = oracle_lib.run_fpm(gain_cases.base_stack(case)[:, 0], case.order, case.x0, case.y0, r.Np, r.L, r.r,
                               case.delta1, case.delta2, case.iters, **kw)
    away = min(rel_l2(plain[k], ref[k]) for k in ("objF", "objCrop", "pupil"))
    print(f"{case.id}: complex64 drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()) +
          f"; ungained oracle {away:.2e} away")
    for k, v in drift.items():
        assert c64[k].dtype == np.complex64 and v < case.tol / 10, (k, v)
    assert away > 100 * case.tol


# ---- the moments ------------------------------------------------------------------------
def test_moment_reference_is_the_expansion_of_the_residual():
    c = GAINCAL
    x0, y0, order = c.geometry()
    d = gain_cases.float64_calibration(False)
    g = gain_cases.uniform_gains(len(x0), c.B)
    E, Q, Cx, S = gain_cases.moment_reference(d["state"], c.stack(), c.Np, order, x0, y0, gain=g)
    np.testing.assert_allclose(E, calibrate.gain_error(g[order], Q, Cx, S), rtol=1e-9)
    E1 = gain_cases.moment_reference(d["state"], c.stack(), c.Np, order, x0, y0)[0]
    assert np.all(Q - Cx * Cx / S <= E1 * (1 + 1e-12))        # the minimum over g lies below g = 1


# ---- calibrate_gains' rule -----------------------------------------------------------------
class _FakeSolver:
    def __init__(self, order, gain, Q, Cx, S):
        self.prob = type("P", (), dict(order=np.asarray(order)))()
        self._g, self._m, self.installed = np.asarray(gain, np.float32), (Q, Cx, S), None

    def gains(self):
        return self._g.copy()

    def moments(self):
        Q, Cx, S = self._m
        return dict(model=Q, cross=Cx, ref=S, ms=0.25)

    def set_gains(self, g):
        self.installed = np.array(g)


def test_calibrate_gains_rule():
    # 5 stack entries, 2 patches; LED 3 is never used, LED 1 occurs twice, LED 4 has S = 0 in patch 1
    order = [0, 1, 2, 1, 4]
    old = np.array([[1, 1], [1, 2], [1, 1], [7, 7], [3, 5]], np.float32)
    S = np.array([[100, 400], [100, 100], [200, 100], [50, 50], [100, 0]], np.float64)
    ghat = np.array([[1.0, 0.5], [2.0, 1.0], [0.5, 2.0], [9.0, 9.0], [1.0, 3.0]])    # row 3: LED 1 again, ignored
    Cx = ghat * S
    Q = 2.0 * ghat * ghat * S + 1.0
    s = _FakeSolver(order, old, Q, Cx, S)
    out = calibrate.calibrate_gains(s, clip=(0.25, 4.0))
    new = out["new"]
    assert new.dtype == np.float32 and new.shape == old.shape
    np.testing.assert_array_equal(s.installed, new)
    np.testing.assert_array_equal(out["old"], old)
    np.testing.assert_array_equal(new[3], old[3])                  # unused: as it was
    assert new[4, 1] == old[4, 1]                                  # S = 0: as it was
    for b in (0, 1):
        rows = [0, 1, 2, 4] if b == 0 else [0, 1, 2]               # first positions with S > 0
        leds = [order[i] for i in rows]
        w, g = S[rows, b], ghat[rows, b]
        scale = np.sqrt(w.sum() / (w * g * g).sum())
        np.testing.assert_allclose(new[leds, b], g * scale, rtol=1e-6)
        np.testing.assert_allclose((w * new[leds, b].astype(np.float64) ** 2).sum() / w.sum(), 1.0, rtol=1e-6)
    # before / after are E(g) at the old and new gains of each position's LED
    np.testing.assert_allclose(out["before"], Q - 2 * old[order] * Cx + old[order].astype(np.float64) ** 2 * S)
    np.testing.assert_allclose(out["after"], Q - 2 * new[order].astype(np.float64) * Cx +
                               new[order].astype(np.float64) ** 2 * S)
    assert out["ms"] == 0.25
    # the clip acts after the normalisation
    tight = calibrate.estimate_gains(order, old, Q, Cx, S, clip=(0.9, 1.1))
    used = np.array([[True, True], [True, True], [True, True], [False, False], [True, False]])
    assert tight[used].min() >= np.float32(0.9) and tight[used].max() <= np.float32(1.1)
    assert (tight[used] == np.float32(0.9)).any() and (tight[used] == np.float32(1.1)).any()
    for bad in ((0.0, 1.0), (2.0, 1.0), (0.5, np.inf)):
        with pytest.raises(ValueError):
            calibrate.estimate_gains(order, old, Q, Cx, S, clip=bad)
    # a model that is dark everywhere estimates nothing
    np.testing.assert_array_equal(calibrate.estimate_gains(order, old, Q, 0 * Cx, S), old)


# ---- the calibration case --------------------------------------------------------------------
def test_float64_alone_decides_the_gain_calibration_case():
    """The claim of the GPU test, in float64 (restate_step) alone: after the
    step the scaled LEDs' gains undo their factors better than gains of 1, and
    the run that calibrates ends at a smaller sum E / sum S than the run of
    equal length that does not."""
    c = GAINCAL
    h = c.factors()
    assert (h != 1).sum() == len(h) // 3 and h.min() >= 0.6 and h.max() <= 1.6 and np.abs(h[h != 1] - 1).min() > 0.02
    cal, plain = gain_cases.float64_calibration(True), gain_cases.float64_calibration(False)
    e1, e0 = c.gain_error(cal["gain"]), c.gain_error(plain["gain"])
    after = calibrate.gain_error(cal["gain"][list(c.geometry()[2])], cal["Q"], cal["C"], cal["S"])
    before = calibrate.gain_error(1.0, cal["Q"], cal["C"], cal["S"])
    print(f"gain calibration case: |g h / mean - 1| of the scaled LEDs {e0.min():.3f} .. {e0.max():.3f} with gains 1, "
          f"{e1.min():.3f} .. {e1.max():.3f} after the step (largest ratio {(e1 / e0).max():.3f}); sum E / sum S "
          f"{plain['e_over_s']} without, {cal['e_over_s']} with the step; E(g) of the step's state: "
          f"after / before {((after.sum(1)) / before.sum(1)).min():.3f} .. {(after.sum(1) / before.sum(1)).max():.3f} "
          f"per LED")
    assert np.all(e1 < e0)
    assert np.all(cal["e_over_s"] < plain["e_over_s"])
