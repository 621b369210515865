"""Every rung of the general path's kernel ladder on the device
(tests/ladder_cases.py; the CPU half is tests/test_ladder.py).

Per row and switch setting:
  * fpm_debug_get_ladder of the live context, for the update step and for the
    residual sweep, equals what fpm_debug_plan_ladder returns for the row's
    (Np, nb, B) and names the rung the row claims (the read-back also compares
    each launched kernel's static LDS constant with its compiled code);
  * objF, objCrop and the pupil of three sampled patches (first, last, one
    between) match the C++ fp64 oracle within the project's bounds (DESIGN.md
    section 2): relative L2 < 1e-5 after one iteration, < 5e-5 after two;
  * patches with identical inputs end with identical bits, whichever tile and
    block they land in;
  * objCrop equals numpy's complex128 ifft2 of the GPU's own objF, < 2e-6 as in
    test_objcrop_live_band (L 500 / 720 / 750 / 972 / 1000 are sizes of
    k_fft_batch no other test runs, each with a partial last block; at L 3000
    it runs after K1 and K3 launches above 64 KiB);
  * fpm_residual matches the float64 evaluation of the downloaded state with
    the bound of test_gpu_residual.py (tests/residual_check.py), and is
    bit-equal for patches with identical inputs;
  * wave-private and tiled columns agree to < 2e-6 where a row runs both, as
    test_wave_and_tiled_column_passes_agree asserts at Np 64 / 90 / 200.
One line of measured errors per row and switch is printed (pytest -s) and
copied into DESIGN.md section 4.7.

Np 486 / 600 / 2916 launch K2 (Np 2916: K1 and K3 too) with more than 64 KiB
of dynamic LDS, which the update step never did before.
"""
import contextlib
import functools
import os
import types

import numpy as np
import pytest

import fpm_amd
import ladder_cases
import oracle_lib
import residual_check
from fpm_oracle import rel_l2
from ladder_cases import ENV, NO_WAVE, WAVE

pytestmark = pytest.mark.gpu

KEYS = ("objF", "objCrop", "pupil")


@contextlib.contextmanager
def _env(kw):
    """Environment switches for the context created inside (read at fpm_create)."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=1)
def _oracle(name):
    """fp64 objF / objCrop / pupil of the row's sampled patches, computed once per row."""
    row = ladder_cases.BY_NAME[name]
    x0, y0, order = row.geometry()
    stack, _ = row.stack()
    return oracle_lib.run_fpm_batch(stack[:, row.sample], order, x0, y0, row.Np, row.L, row.r, 5, 10, row.iters,
                                    threads=len(row.sample), pupil=True, objF=True)


def _run(row, switch):
    """The row under one switch setting: every check that needs that context alone;
    returns the sampled patches' outputs for the comparison between settings."""
    prob = row.problem()
    stack, idx = row.stack()
    nd = row.n_distinct
    with _env(ENV[switch]):
        s = fpm_amd.Solver(prob)
    try:
        assert s.info().fused_kernel == fpm_amd.KERNEL_GENERAL
        assert s.debug_plan() == dict(meas_g=0, general_kind=fpm_amd.GENERAL_LDS, residual_kind=fpm_amd.RESIDUAL_LDS)
        # the live context runs what the planner says, and that is the rung the row is here for
        step, sweep = s.debug_ladder(False), s.debug_ladder(True)
        assert step == ladder_cases.plan(row, switch, True) and sweep == ladder_cases.plan(row, switch, False)
        names = (ladder_cases.rung_name(step["rows"], "lr"), ladder_cases.rung_name(step["cols"], "lc"),
                 ladder_cases.rung_name(sweep["rows"], "lr"), ladder_cases.rung_name(sweep["cols"], "lc"))
        assert names == row.rungs[switch]
        s.upload(stack)
        s.init()
        s.run(row.iters)
        out = s.download(support=False)
        res = s.residual()
    finally:
        s.close()
    # parity with the fp64 oracle on the sampled patches
    ref = _oracle(row.name)
    err = {k: max(rel_l2(out[k][b], ref[k][i]) for i, b in enumerate(row.sample)) for k in KEYS}
    # objCrop is the IDFT of the GPU's own spectrum
    crop = max(rel_l2(out["objCrop"][b], np.fft.ifft2(out["objF"][b].astype(np.complex128))) for b in row.sample)
    print(f"ladder {row.name} {switch}: step {names[0]} / {names[1]} ({step['rows']['lds_dynamic']} / "
          f"{step['cols']['lds_dynamic']} B), sweep {names[2]} / {names[3]}; rel L2 "
          + " ".join(f"{k} {v:.2e}" for k, v in err.items()) + f", objCrop vs ifft2(objF) {crop:.2e}")
    for k, v in err.items():
        assert np.isfinite(v) and v < row.tol, (k, v)
    assert crop < 2e-6
    # identical inputs, identical bits: patch b reads base patch b % nd
    for b in range(nd, row.B):
        for k in KEYS:
            assert np.array_equal(out[k][b], out[k][idx[b]]), (k, b)
        assert np.array_equal(res["err"][:, b], res["err"][:, idx[b]]) and \
            np.array_equal(res["ref"][:, b], res["ref"][:, idx[b]]), b
    # the sweep against the float64 evaluation of the downloaded state: the nd distinct patches
    sub = types.SimpleNamespace(np_=row.Np, n_patch=nd, order=prob.order, x0=prob.x0, y0=prob.y0)
    state = {k: out[k][:nd] for k in ("objF", "pupil")}
    E, Q, S = residual_check.reference(state, stack[:, :nd], sub)
    assert np.all(Q > 0)        # every window carries signal
    residual_check.check(f"ladder {row.name} {switch}", dict(err=res["err"][:, :nd], ref=res["ref"][:, :nd],
                                                             ms=res["ms"]), (E, Q, S))
    return {k: [out[k][b] for b in row.sample] for k in KEYS}


@pytest.mark.parametrize("row", ladder_cases.ROWS, ids=lambda r: r.name)
def test_ladder_row(row):
    got = {switch: _run(row, switch) for switch in row.rungs}
    if WAVE in got and NO_WAVE in got:
        gap = max(rel_l2(a, b) for k in KEYS for a, b in zip(got[WAVE][k], got[NO_WAVE][k]))
        print(f"ladder {row.name}: wave vs tiled columns rel L2 {gap:.2e}")
        assert gap < 2e-6


def test_create_refuses_np10240():
    """Np 10240: the one-sequence K3 needs 163 840 B of dynamic LDS and 16 B of
    its own, 16 more than a workgroup can have (the sweep's K2: 64 more).
    plan_context refuses before anything is allocated or launched."""
    Np = L = 10240
    prob = fpm_amd.Problem(Np, L, [0, 1], np.array([0, 0]), np.array([0, 0]), 4, 5, 10, path=fpm_amd.PATH_GENERAL)
    with pytest.raises(fpm_amd.FpmError, match="LDS") as e:
        fpm_amd.Solver(prob)
    assert e.value.code == fpm_amd.FPM_ERR_INVAL and "Np=10240" in str(e.value)


def test_create_refuses_nlarge10240():
    """Nlarge 10240: objCrop's batched transform holds one sequence per block
    and asks for (10241 + 10240) * 8 = 163 848 B of LDS, 8 more than a workgroup
    can have.  plan_context refuses before anything is allocated; the step and
    the sweep of Np 32 fit."""
    from tools.synth import grid_geometry
    Np, L, r = 32, 10240, 6
    x0, y0, order = grid_geometry(Np, L, 3, 4)
    prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=1)
    with pytest.raises(fpm_amd.FpmError, match="LDS") as e:
        fpm_amd.Solver(prob)
    assert e.value.code == fpm_amd.FPM_ERR_INVAL and "10240" in str(e.value) and "objCrop" in str(e.value)


def test_get_ladder_refuses_fused_and_register_contexts():
    from tools.synth import grid_geometry
    for Np, L, r, path in ((256, 512, 33, fpm_amd.PATH_FUSED), (256, 512, 40, fpm_amd.PATH_GENERAL)):
        x0, y0, order = grid_geometry(Np, L, 3, 24)
        with fpm_amd.Solver(fpm_amd.Problem(Np, L, order, x0, y0, r, 10, 3, path=path)) as s:
            for residual in (False, True):
                with pytest.raises(fpm_amd.FpmError) as e:
                    s.debug_ladder(residual)
                assert e.value.code == fpm_amd.FPM_ERR_INVAL
