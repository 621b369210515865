"""LED gains on the GPU: fpm_set_gains / fpm_get_gains (a per-image amplitude
factor in every LED-update kernel, fpm_init and the residual sweep),
fpm_moments (the sums a gain is estimated from) and
fpm_amd.calibrate.calibrate_gains.  tests/gain_cases.py holds the cases and
the float64 yardsticks, tests/test_gains.py their CPU conditions.

  update     every LED-update kernel with gains from {0.5, 1, 2} on a stack of
             multiples of 4 against the C++ fp64 oracle on uint16(g^2 I), at the
             project's bounds (case.tol), objF / objCrop / pupil of every patch.
  arbitrary  gains in [0.7, 1.4] set BETWEEN two run(1): one iteration against
             restate_step.iterate on the float64 stack g^2 I from the downloaded
             state at 1e-5; a stale captured graph or a gain held by value would
             show.  Then the carried-maxima invariants.
  neutral    set_gains(ones), and set_gains(x) then set_gains(None), end bit for
             bit where a context without the call ends: run(2), residual(),
             residual_at over a radius-1 list.  Such a context launches the
             kernels' ungained instances; a table that is 1 on every used LED
             and 2 on an unused one launches the gained instances, where
             g = 1.0f must be the neutral element of the arithmetic itself:
             the same bits again.
  moments    Q, C, S and the gained E against float64 of the downloaded state:
             with the project's eps = 1e-5 for the relative error of |psi|
             (tests/test_gpu_residual.py),
               |dQ| <= 2e-5 Q,  |dC| <= 2e-5 sqrt(Q S),  ref == sum I,
               |dE| <= residual_check.bound(E, Q) under a gain table.
             Where the model is exactly dark Q = C = 0 exactly, and the gained
             E is sum g^2 I up to its fp32 lane sums: every term fl(fl(g g) I)
             carries two roundings and a lane adds fewer than Np of them, so
             the relative error stays below (Np + 2) 2^-24.
  one path   bit equality of moments and of the gained residual_at: (i, 0, 0)
             against the identity list, a list against its reverse, its pieces
             and FPM_RES_BATCH=1.
  calibrate  GAINCAL on the device: the estimate against float64 of the
             downloaded state, and the claim tests/test_gains.py shows in float64.
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import gain_cases
import residual_check
import restate_step
import schedules
from fpm_amd import calibrate
from fpm_oracle import rel_l2
from gain_cases import GAINCAL
from test_gpu_probe import OFFSETS, PARITY, _entries
from test_gpu_residual import BIN, GENERAL, _case, _context, _env, _solver
from maxima_check import check_maxima as _check_maxima
from test_gpu_schedules import _solver as _case_solver

pytestmark = pytest.mark.gpu

# cases that share an oracle next to each other
UPDATE = sorted(gain_cases.UPDATE, key=lambda c: (list(gain_cases._BY_KEY).index(gain_cases.oracle_key(c)), c.row.name))


# ---- 1. the update step, every kernel -----------------------------------------------------
@pytest.mark.parametrize("case", UPDATE, ids=lambda c: c.id)
def test_update_step_with_gains(case):
    row = case.row
    g = gain_cases.step_gains(case)
    with _case_solver(case) as s:           # asserts kernel, mode and kind; uploads case.stack()
        s.upload(gain_cases.base_stack(case))
        s.set_gains(g)
        np.testing.assert_array_equal(s.gains(), g)
        s.init()
        s.run(case.iters)
        out = s.download()
        name = fpm_amd.KERNEL_NAMES[s.info().fused_kernel]
    ref = gain_cases.oracle(gain_cases.oracle_key(case))
    errs = {k: max(rel_l2(out[k][b], ref[k][b]) for b in range(row.B)) for k in ("objF", "objCrop", "pupil")}
    print(f"{case.id}: kernel {name} x{row.wg}; gains {sorted(set(g.ravel().tolist()))}; max rel L2 " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {case.tol:g})")
    for k, v in errs.items():
        assert v < case.tol, (k, v)


# ---- 2. arbitrary gains, set between two runs ----------------------------------------------
@pytest.mark.parametrize("name", gain_cases.ARBITRARY_ROWS)
def test_arbitrary_gains_between_runs(name):
    case = schedules.BY_ID[f"{name}-S2-init1-cv"]
    row = case.row
    stack = case.stack()
    g = gain_cases.uniform_gains(len(case.x0), row.B)
    with _case_solver(case) as s:
        s.init()
        s.run(1)                            # the general path captures its graphs here
        one = s.download()
        s.set_gains(g)
        kept = s.download()
        for k in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(kept[k], one[k], err_msg=f"{name}: fpm_set_gains changed {k}")
        np.testing.assert_array_equal(s.download_stack(), stack)
        s.run(1)
        two = s.download()
        _check_maxima(s, case, "after the run with gains")
    g2 = g.astype(np.float64) ** 2
    worst = 0.0
    for b in range(row.B):
        args = (case.order, case.x0, case.y0, row.Np, row.L, row.r, case.delta1, case.delta2, 1)
        ref = restate_step.iterate(one["objF"][b], one["pupil"][b], stack[:, b] * g2[:, b, None, None], *args)
        for k in ("objF", "objCrop", "pupil"):
            e = rel_l2(two[k][b], ref[k])
            worst = max(worst, e)
            assert e < 1e-5, (name, b, k, e)
        stale = restate_step.iterate(one["objF"][b], one["pupil"][b], stack[:, b], *args)
        assert rel_l2(stale["objF"], ref["objF"]) > 1e-3     # the ungained step is far away
    print(f"{name}: one iteration after fpm_set_gains, max rel L2 {worst:.2e} (bound 1e-5)")


# ---- 3. the neutral element -------------------------------------------------------------------
@pytest.mark.parametrize("name", gain_cases.NEUTRAL_ROWS)
def test_unit_gains_change_no_bit(name):
    case = schedules.BY_ID[f"{name}-S2-init1-cv"]
    row = case.row
    n_stack = len(case.x0)
    pos, dx, dy, _ = calibrate.probe_list((case.x0, case.y0), case.order, row.L, row.Np, calibrate.neighbourhood(1))
    ones = np.ones((n_stack, row.B), np.float32)
    x = gain_cases.uniform_gains(n_stack, row.B)
    outs = {}
    unused = ones.copy()
    unused[list(case.unused)] = 2.0             # no order[] position reads these rows
    assert case.unused and not set(case.unused) & set(case.order)
    for how in ("fresh", "ones", "reset", "unused"):
        with _case_solver(case) as s:
            np.testing.assert_array_equal(s.gains(), ones)
            if how == "ones":
                s.set_gains(ones)
            elif how == "reset":
                s.set_gains(x)
                np.testing.assert_array_equal(s.gains(), x)
                s.set_gains(None)
            elif how == "unused":
                s.set_gains(unused)
            np.testing.assert_array_equal(s.gains(), unused if how == "unused" else ones)
            s.init()
            s.run(2)
            outs[how] = (s.download(), s.residual(), s.residual_at(pos, dx, dy))
    for how in ("ones", "reset", "unused"):
        for k in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(outs[how][0][k], outs["fresh"][0][k], err_msg=f"{name} {how} {k}")
        for i in (1, 2):
            for k in ("err", "ref"):
                np.testing.assert_array_equal(outs[how][i][k], outs["fresh"][i][k], err_msg=f"{name} {how} {i} {k}")


# ---- 4. moments and the gained residual --------------------------------------------------------
def _ratio(delta, bnd):
    return float(np.divide(delta, bnd, out=np.zeros_like(delta), where=bnd > 0).max())


@pytest.mark.parametrize("name", list(PARITY))
def test_moments_and_gained_residual_against_float64(name):
    args, kw, iters, kernels, plan, env, short = PARITY[name]
    prob, stack = _case(*args, **kw)
    pos, dx, dy, outside = _entries(prob, short)
    g = gain_cases.uniform_gains(len(prob.x0), prob.n_patch, seed=11)
    with _solver(prob, stack, iters, kernels, plan, **env) as s:
        state = s.download(objCrop=False, support=False)
        m_id, m_at = s.moments(), s.moments(pos, dx, dy)
        plain = s.residual_at(pos, dx, dy)
        s.set_gains(g)
        m_g = s.moments(pos, dx, dy)            # raw: the gain table does not enter
        e_id, e_at = s.residual(), s.residual_at(pos, dx, dy)
    for k in ("model", "cross", "ref"):
        np.testing.assert_array_equal(m_g[k], m_at[k], err_msg=f"{name}: moments under a gain table, {k}")
    np.testing.assert_array_equal(plain["ref"], m_at["ref"])
    np.testing.assert_array_equal(e_at["ref"], m_at["ref"])
    worst = {}
    for tag, m, e, ent in (("identity", m_id, e_id, {}), ("entries", m_at, e_at, dict(pos=pos, dx=dx, dy=dy))):
        E, Q, Cx, S = gain_cases.moment_reference(state, stack, prob.np_, prob.order, prob.x0, prob.y0, gain=g, **ent)
        np.testing.assert_array_equal(m["ref"], S)
        dark = Q == 0
        assert not np.any(m["model"][dark]) and not np.any(m["cross"][dark]), (name, tag, "Q = C = 0 where dark")
        dq, dc, de = np.abs(m["model"] - Q), np.abs(m["cross"] - Cx), np.abs(e["err"] - E)
        bq, bc, be = 2e-5 * Q, 2e-5 * np.sqrt(Q * S), residual_check.bound(E, Q)
        worst[tag] = (_ratio(dq, bq), _ratio(dc, bc), _ratio(de, be))
        assert np.all(np.isfinite(m["model"])) and np.all(dq <= bq), (name, tag, "Q", worst[tag])
        assert np.all(np.isfinite(m["cross"])) and np.all(dc <= bc), (name, tag, "C", worst[tag])
        assert np.all(np.isfinite(e["err"])) and np.all(de[~dark] <= be[~dark]), (name, tag, "E", worst[tag])
        assert np.all(de[dark] <= (prob.np_ + 2) * 2.0 ** -24 * E[dark]), (name, tag, "gained E of a dark window")
        if tag == "entries":
            assert dark[outside].all() and (~dark).any()
    print(f"moments {name}: max |d|/bound identity Q {worst['identity'][0]:.3e} C {worst['identity'][1]:.3e} "
          f"gained E {worst['identity'][2]:.3e}; entries Q {worst['entries'][0]:.3e} C {worst['entries'][1]:.3e} "
          f"gained E {worst['entries'][2]:.3e}; sweep {m_id['ms']:.3f} ms")


@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_one_path(which):
    tag, (prob, stack), kernels = _context(which)
    n = len(prob.order)
    idx, zero = np.arange(n), np.zeros(n, np.int32)
    pos = np.arange(3 * n + 1) % n                  # longer than any scratch sized for n_order
    off = np.array([OFFSETS[(k // n + k) % 4] for k in range(3 * n + 1)])
    g = gain_cases.uniform_gains(len(prob.x0), prob.n_patch, seed=12)
    keys = {"moments": ("model", "cross", "ref"), "residual_at": ("err", "ref")}
    got = {}
    for batch in (None, "1"):
        env = {"FPM_RES_BATCH": batch} if batch else {}
        with _solver(prob, stack, 1, kernels, **env) as s:
            s.set_gains(g)
            sweeps = {"moments": s.moments(), "residual_at": s.residual()}
            for fn, ks in keys.items():
                call = getattr(s, fn)
                ident, rev = call(idx, zero, zero), call(idx[::-1], zero, zero)
                long = call(pos, off[:, 0], off[:, 1])
                pieces = [call(pos[k:k + 7], off[k:k + 7, 0], off[k:k + 7, 1]) for k in range(0, 3 * n + 1, 7)]
                for k in ks:
                    np.testing.assert_array_equal(ident[k], sweeps[fn][k], err_msg=f"{tag}: {fn} (i, 0, 0) {k}")
                    np.testing.assert_array_equal(rev[k], sweeps[fn][k][::-1], err_msg=f"{tag}: {fn} reversed {k}")
                    np.testing.assert_array_equal(np.concatenate([p[k] for p in pieces]), long[k],
                                                  err_msg=f"{tag}: {fn} {3 * n + 1} entries against their pieces, {k}")
                assert (long[ks[0]][:n] != long[ks[0]][n:2 * n]).any()           # the offsets matter
                got[batch, fn] = (sweeps[fn], long)
            # the two sweeps share their scratch: one after the other returns the same bits again
            for k in keys["moments"]:
                np.testing.assert_array_equal(s.moments()[k], sweeps["moments"][k])
            np.testing.assert_array_equal(s.residual()["err"], sweeps["residual_at"]["err"])
    for fn, ks in keys.items():
        for a, b in zip(got[None, fn], got["1", fn]):
            for k in ks:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {fn} FPM_RES_BATCH=1 {k}")


def test_moments_are_read_only():
    tag, (prob, stack), kernels = _context("general_np32")
    with _solver(prob, stack, 1, kernels) as s:
        before, mx0, g0 = s.download(), s.debug_maxima(), s.gains()
        b0 = s.info().device_bytes
        a, b = s.moments(), s.moments()
        for k in ("model", "cross", "ref"):
            np.testing.assert_array_equal(a[k], b[k])
        assert s.info().device_bytes > b0           # its scratch is counted
        after, mx1 = s.download(), s.debug_maxima()
        for k in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
        for k in ("tmax", "dirty", "pmax"):
            np.testing.assert_array_equal(mx0[k], mx1[k], err_msg=k)
        np.testing.assert_array_equal(s.download_stack(), stack)
        np.testing.assert_array_equal(s.gains(), g0)


# ---- 5. calibration ---------------------------------------------------------------------------
def test_gain_calibration_step():
    c = GAINCAL
    x0, y0, order = c.geometry()
    stack = c.stack()
    prob = fpm_amd.Problem(c.Np, c.L, np.array(order), x0, y0, c.r, c.d1, c.d2, n_patch=c.B)

    def e_over_s(s):
        d = s.residual()
        return d["err"].sum(0) / d["ref"].sum(0)

    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(c.iters_before)
        state = s.download(objCrop=False, support=False)
        out = calibrate.calibrate_gains(s)
        np.testing.assert_array_equal(s.gains(), out["new"])
        s.run(c.iters_after)
        with_step = e_over_s(s)
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(c.iters_before + c.iters_after)
        without = e_over_s(s)
    # the estimate against float64 of the state it was made from: the moment bounds divided by S
    _, Q, Cx, S = gain_cases.moment_reference(state, stack, c.Np, order, x0, y0)
    ghat = out["cross"] / out["ref"]
    dg, bg = np.abs(ghat - Cx / S), 2e-5 * np.sqrt(Q / S)
    np.testing.assert_array_equal(out["ref"], S)
    assert np.all(dg <= bg), _ratio(dg, bg)
    np.testing.assert_array_equal(out["new"], calibrate.estimate_gains(order, out["old"], out["model"], out["cross"],
                                                                       out["ref"]))
    np.testing.assert_array_equal(out["old"], np.ones_like(out["new"]))
    # the claim (tests/test_gains.py shows it in float64)
    e1, e0 = c.gain_error(out["new"]), c.gain_error(out["old"])
    print(f"gain calibration: max |dg|/bound {_ratio(dg, bg):.3e}; |g h / mean - 1| of the scaled LEDs "
          f"{e0.min():.3f} .. {e0.max():.3f} before, {e1.min():.4f} .. {e1.max():.4f} after; sum E / sum S {without} "
          f"without, {with_step} with the step; after / before per LED at most "
          f"{(out['after'].sum(1) / out['before'].sum(1)).max():.3f}; moments {out['ms']:.3f} ms")
    assert np.all(e1 < e0)
    assert np.all(with_step < without)
    assert np.all(out["after"].sum(axis=1) <= out["before"].sum(axis=1))


# ---- 6. the boundary ----------------------------------------------------------------------------
def test_errors():
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    lib = fpm_amd.load_library()
    n_stack, B = len(prob.x0), prob.n_patch
    dp = C.POINTER(C.c_double)
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.moments()
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        g = gain_cases.uniform_gains(n_stack, B)
        s.set_gains(g)                               # legal before fpm_init
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            t = g.copy()
            t[4, 1] = bad
            with pytest.raises(fpm_amd.FpmError) as ei:
                s.set_gains(t)
            assert ei.value.code == fpm_amd.FPM_ERR_INVAL and f"gain[{4 * B + 1}]" in str(ei.value), str(ei.value)
            np.testing.assert_array_equal(s.gains(), g)
        t = g.copy()
        t[2, 0], t[7, 2] = -3.0, 0.0                 # the first bad index is named
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.set_gains(t)
        assert f"gain[{2 * B}]" in str(ei.value)
        with pytest.raises(ValueError):
            s.set_gains(g[:-1])
        s.set_gains(np.full((n_stack, B), 256.0, np.float32))     # fp32 storage takes it
        s.set_gains(g)
        s.init()
        s.run(1)
        assert lib.fpm_moments(s._h, None, 0, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
        want = s.moments()
        q = np.full((len(prob.order), B), -1.0)
        assert lib.fpm_moments(s._h, None, 0, None, q.ctypes.data_as(dp), None, None) == fpm_amd.FPM_OK   # one is enough
        np.testing.assert_array_equal(q, want["cross"])
        # fpm_residual_at's validation, before the first launch
        p = (fpm_amd.fpm_probe * 2)(fpm_amd.fpm_probe(0, 0, 0), fpm_amd.fpm_probe(len(prob.order), 0, 0))
        q[:] = -1.0
        assert lib.fpm_moments(s._h, p, 2, q.ctypes.data_as(dp), None, None, None) == fpm_amd.FPM_ERR_INVAL
        assert "entry 1" in lib.fpm_last_error().decode() and np.all(q == -1.0)
        assert lib.fpm_moments(s._h, p, 0, q.ctypes.data_as(dp), None, None, None) == fpm_amd.FPM_ERR_INVAL
        with pytest.raises(ValueError):
            s.moments(None, [0], [0])
        s.run(1)                                     # and the context still runs
    # fp16 spectrum storage: 256 g must stay below 65504
    prob16, _ = _case(1024, 4096, 333, 2, 600, 1, 95, flags=fpm_amd.FLAG_SPEC_FP16)
    with fpm_amd.Solver(prob16) as s:
        one = np.ones((len(prob16.x0), 1), np.float32)
        t = one.copy()
        t[3, 0] = 256.0
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.set_gains(t)
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "gain[3]" in str(ei.value)
        np.testing.assert_array_equal(s.gains(), one)
        t[3, 0] = 255.0
        s.set_gains(t)
        np.testing.assert_array_equal(s.gains(), t)


def test_capturing_stream_is_refused():
    """As fpm_run (test_run_on_a_capturing_stream_is_refused): both calls block,
    so FPM_ERR_INVAL before anything is enqueued or changed, the capture stays valid."""
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    g = gain_cases.uniform_gains(len(prob.x0), prob.n_patch)
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        want, g0 = s.moments(), s.gains()
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        for call in (lambda: s.moments(), lambda: s.set_gains(g)):
            graph = torch.cuda.CUDAGraph()
            with pytest.raises(fpm_amd.FpmError) as ei:
                with torch.cuda.graph(graph, stream=cs, capture_error_mode="relaxed"):
                    call()
            assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        np.testing.assert_array_equal(s.gains(), g0)
        np.testing.assert_array_equal(s.moments()["model"], want["model"])      # no longer capturing
        s.set_stream(None)
        np.testing.assert_array_equal(s.moments()["cross"], want["cross"])
        s.set_gains(g)
        s.run(1)


# ---- 7. CLI -------------------------------------------------------------------------------------
def test_cli_calibrate_gains(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    iters = 3
    outs, dirs = {}, {}
    for tag, extra in (("gains", ["--calibrate-gains"]), ("all", ["--calibrate-leds", "1", "--calibrate-gains",
                                                                  "--residual"]), ("plain", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], str(iters), "--out", str(out)] + extra, capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag], dirs[tag] = json.loads((out / "result.json").read_text()), out
    plain = outs["plain"]
    assert "led_gains" not in plain
    for tag in ("gains", "all"):
        meta = outs[tag]
        lg = meta["led_gains"]
        assert set(lg) == {"clip", "gain", "before_per_step", "after_per_step", "moments_ms"}
        used = meta["leds_used"]
        gain = np.array(lg["gain"])
        assert gain.shape == (used, 1) and np.all(np.isfinite(gain)) and np.all(gain > 0)      # per used LED and patch
        assert lg["clip"][0] <= gain.min() and gain.max() <= lg["clip"][1] and lg["moments_ms"] > 0
        before, after = np.array(lg["before_per_step"]), np.array(lg["after_per_step"])
        assert before.shape == after.shape == (iters - 1, 1)         # after every iteration but the last, per patch
        assert np.all(np.isfinite(before)) and np.all(after >= 0)
        assert set(meta) - {"led_gains", "led_calibration", "residual"} == set(plain)
    assert "led_calibration" in outs["all"] and "residual" in outs["all"]
    assert np.any(np.array(outs["gains"]["led_gains"]["gain"]) != 1.0)
    # without the flag the outputs are today's: a second plain run writes the same bytes
    again = tmp_path / "again"
    again.mkdir()
    r = subprocess.run([BIN, ds["json"], str(iters), "--out", str(again)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for f in ("objCrop.npy", "objF.npy", "pupil.npy"):
        assert (again / f).read_bytes() == (dirs["plain"] / f).read_bytes(), f
        assert (dirs["gains"] / f).read_bytes() != (dirs["plain"] / f).read_bytes(), f
