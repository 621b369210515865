"""Cases and float64 yardsticks of the LED-gain tests: plain data and numpy, no
GPU.  tests/test_gains.py (CPU) shows that each case is a case and
tests/test_gpu_gains.py runs them on the device.

A gain g on the image I is by construction the solver without gains on the
image g^2 I (fpm_init and the LED step alike), so the oracle needs no gain:

UPDATE    every row of schedules.KERNELS that has S2, with its case
          S2-init1-cv (and init0-cv / init10-reonly on three rows).  The stack
          is I = (case.stack() // 16) * 4, multiples of 4 up to 16 380, the
          gains are drawn from {0.5, 1, 2}: g^2 I is an integer <= 65 520, so
          the oracle runs on uint16(g^2 I) exactly what the device must compute
          from (I, g).
ARBITRARY gains uniform in [0.7, 1.4]: g^2 I is no integer, so the yardstick is
          restate_step.iterate on the float64 stack g^2 I from a downloaded state.
moments   residual_check.reference with the window anywhere, a gain and the
          cross column C = sum |psi| sqrt(I).
GAINCAL   the brightness-calibration case: a third of the LEDs measured h^2
          too bright or too dark.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib
import schedules
from tools.synth import grid_geometry, make_stack

GAIN_VALUES = (0.5, 1.0, 2.0)
_EXTRA_TAGS = ("S2-init0-cv", "S2-init10-reonly")
_EXTRA_ROWS = ("general_lds", "fused_small", "fused_np256_dist")


def _update_cases():
    out = []
    for row in schedules.KERNELS:
        if "S2" not in row.schedules:
            continue
        tags = ("S2-init1-cv",) + (_EXTRA_TAGS if row.name in _EXTRA_ROWS else ())
        out += [schedules.BY_ID[f"{row.name}-{t}"] for t in tags]
    return tuple(out)


UPDATE = _update_cases()
NEUTRAL_ROWS = ("general_lds", "fused_np90", "fused_np200", "general_reg256", "fused_np256", "fused_np256_split",
                "fused_np256_dist")
ARBITRARY_ROWS = ("general_lds", "fused_np256")


def base_stack(case):
    """I: the case's stack coarsened to multiples of 4 <= 16 380."""
    return _base_stack(case.row.Np, case.row.L, case.row.r, case.row.B, case.x0, case.y0)


@functools.lru_cache(maxsize=4)
def _base_stack(Np, L, r, B, x0, y0):
    st = ((schedules._stack_of("S2", Np, L, r, B, x0, y0, None).astype(np.uint32) // 16) * 4).astype(np.uint16)
    assert st.max() <= 16380 and not (st % 4).any()
    st.setflags(write=False)
    return st


def step_gains(case):
    """float32 [n_stack][B] from GAIN_VALUES, seeded; rows of one shape that
    differ in the patch count share the leading patches."""
    g = np.random.default_rng(20261020).choice(np.array(GAIN_VALUES, np.float32), size=(len(case.x0), 4))
    return np.ascontiguousarray(g[:, :case.row.B])


def gained_stack(case):
    """uint16(g^2 I), exact."""
    g2 = step_gains(case).astype(np.float64) ** 2
    v = base_stack(case).astype(np.float64) * g2[:, :, None, None]
    assert v.max() <= 65520 and np.array_equal(v, np.rint(v))
    return v.astype(np.uint16)


def oracle_key(case):
    r = case.row
    return (r.Np, r.L, r.r, r.B, case.tag)


_BY_KEY = {}
for _c in UPDATE:
    _BY_KEY.setdefault(oracle_key(_c), _c)


@functools.lru_cache(maxsize=1)
def oracle(key):
    """The C++ fp64 oracle of every patch on the gained stack (no gains)."""
    case = _BY_KEY[key]
    r = case.row
    return oracle_lib.run_fpm_batch(gained_stack(case), case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1,
                                    case.delta2, case.iters, threads=r.B, all_channels=case.all_channels, objF=True,
                                    init_pos=case.init_pos)


def uniform_gains(n_stack, B, seed=5, lo=0.7, hi=1.4):
    return np.random.default_rng(seed).uniform(lo, hi, (n_stack, B)).astype(np.float32)


# ---- the float64 yardstick of the sweeps ------------------------------------------------
def moment_reference(state, stack, Np, order, x0, y0, pos=None, dx=None, dy=None, gain=None):
    """float64 E, Q, C [n][B] and the integer S of the downloaded state for the
    entries (pos[k], dx[k], dy[k]) (default: the identity list), E under the
    gain table `gain` [n_stack][B] (default: ones):
      E = sum (|psi| - g sqrt(I))^2, Q = sum |psi|^2, C = sum |psi| sqrt(I), S = sum I."""
    B = state["objF"].shape[0]
    if pos is None:
        pos = np.arange(len(order))
    n = len(pos)
    dx = np.zeros(n, np.int64) if dx is None else dx
    dy = np.zeros(n, np.int64) if dy is None else dy
    E, Q, C, S = (np.empty((n, B)) for _ in range(4))
    for b in range(B):
        O = np.fft.fftshift(state["objF"][b].astype(np.complex128))
        P = np.fft.ifftshift(state["pupil"][b].astype(np.complex128))
        for k in range(n):
            led = int(order[int(pos[k])])
            xs, ys = int(x0[led]) + int(dx[k]), int(y0[led]) + int(dy[k])
            assert 0 <= xs <= O.shape[1] - Np and 0 <= ys <= O.shape[0] - Np
            a = np.abs(np.fft.ifft2(np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np]) * P))
            I = stack[led, b].astype(np.float64)
            g = 1.0 if gain is None else float(gain[led, b])
            E[k, b] = ((a - g * np.sqrt(I)) ** 2).sum()
            Q[k, b] = (a * a).sum()
            C[k, b] = (a * np.sqrt(I)).sum()
            S[k, b] = float(stack[led, b].astype(np.int64).sum())
    return E, Q, C, S


# ---- the brightness-calibration case ------------------------------------------------------
class GAINCAL:
    """5 x 5 LEDs, Np 32 / L 96 / r 6, two patches.  Every third LED of the
    stack is measured h^2 too bright or too dark, h drawn from [0.6, 1.6]
    (rounded to uint16 again): two iterations, one calibrate_gains step, two
    more iterations.

    Two choices make the brightness identifiable, and float64 alone shows
    (tests/test_gains.py) what happens without them:
      step 2     every window holds the spectrum's DC peak (|offset| <= 4 < r),
                 so all 25 images are bright field and share the object's
                 dominant component; at step 4 the sixteen outer LEDs are dark
                 field, their model is still a third of the data after two
                 iterations, and C / S measures that, not the brightness.
      delta1     1e13, far above |O|^2: the pupil stays at its support.  A
                 bright-field image is |P(k_led)|^2 |O_DC|^2 to first order, so
                 a free pupil (delta1 5) absorbs an LED's brightness into the
                 one pupil pixel its DC peak lands on: C / S is then 1, not 1 / h.
    """
    Np, L, r, B, seed, d1, d2, step = 32, 96, 6, 2, 20261020, 1e13, 10, 2
    iters_before, iters_after = 2, 2

    @classmethod
    @functools.lru_cache(maxsize=None)
    def geometry(cls):
        return grid_geometry(cls.Np, cls.L, 5, cls.step)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def factors(cls):
        """h [n_stack]: 1 for the LEDs left alone."""
        x0, _, _ = cls.geometry()
        h = np.ones(len(x0))
        idx = np.arange(1, len(x0), 3)
        h[idx] = np.random.default_rng(cls.seed).uniform(0.6, 1.6, len(idx))
        return h

    @classmethod
    @functools.lru_cache(maxsize=None)
    def stack(cls):
        x0, y0, _ = cls.geometry()
        # a quarter of the usual peak, so the brightest LED times 1.6^2 does not saturate
        clean = make_stack(cls.Np, cls.L, cls.r, x0, y0, n_patch=cls.B, seed=cls.seed, peak=10000.0)
        st = np.rint(clean.astype(np.float64) * (cls.factors() ** 2)[:, None, None, None])
        assert st.max() < 65535
        st = st.astype(np.uint16)
        st.setflags(write=False)
        return st

    @classmethod
    def gain_error(cls, g):
        """|g h / mean - 1| per scaled LED and patch: the gain that undoes h is
        1 / h up to the scale gain and object share, so g h is constant; the
        mean is taken over all used LEDs of the patch."""
        h = cls.factors()[:, None]
        gh = np.asarray(g, np.float64) * h
        return np.abs(gh / gh.mean(axis=0, keepdims=True) - 1.0)[cls.factors() != 1.0]


def float64_calibration(calibrate_step: bool, clip=(0.25, 4.0)):
    """GAINCAL in float64 alone (restate_step): iters_before iterations, one
    estimate_gains step on float64 moments (or none), iters_after iterations on
    the float64 stack g^2 I.  Returns dict(gain [n_stack][B], mid = the state
    the step saw, Q / C / S of it, state = the final one, e_over_s [B] = sum E /
    sum S of the final state under the final gains)."""
    import restate_step
    from fpm_amd import calibrate
    c = GAINCAL
    x0, y0, order = c.geometry()
    stack = c.stack()

    def run(states, st64, iters):
        outs = [restate_step.iterate(states["objF"][b], states["pupil"][b], st64[:, b], order, x0, y0, c.Np, c.L, c.r,
                                     c.d1, c.d2, iters) for b in range(c.B)]
        return dict(objF=np.stack([o["objF"] for o in outs]), pupil=np.stack([o["pupil"] for o in outs]))

    init = [restate_step.initial_state(stack[:, b], order, c.Np, c.L, c.r) for b in range(c.B)]
    state = dict(objF=np.stack([i[0] for i in init]), pupil=np.stack([i[1] for i in init]))
    mid = run(state, stack, c.iters_before)
    _, Q, C, S = moment_reference(mid, stack, c.Np, order, x0, y0)
    gain = np.ones((len(x0), c.B), np.float32)
    if calibrate_step:
        gain = calibrate.estimate_gains(order, gain, Q, C, S, clip)
    g2 = gain.astype(np.float64) ** 2
    fin = run(mid, stack.astype(np.float64) * g2[:, :, None, None], c.iters_after)
    E, _, _, S1 = moment_reference(fin, stack, c.Np, order, x0, y0, gain=gain)
    return dict(gain=gain, mid=mid, Q=Q, C=C, S=S, state=fin, e_over_s=E.sum(0) / S1.sum(0))
