"""Every LED-update kernel on LED schedules the grid-geometry tests never
produce (tests/schedules.py: S1 chain to a spectrum corner, S2 repeats /
unused LEDs / init_pos, S3 moving maximum), GPU only.  tests/test_schedules.py
shows on the CPU that each case is non-trivial and well conditioned in fp32.

Per case, every patch:
  parity    objF, objCrop, pupil against the C++ fp64 oracle at the project's
            bounds (relative L2 < 5e-5 after two or three iterations, 1e-2 with
            fp16 spectrum storage: DESIGN.md section 2), support exactly equal.
  maxima    the carried max|objF| / max|P| bookkeeping (fpm_debug_get_maxima)
            against the downloaded fp32 state, magnitudes in float64, after
            fpm_init, after each run(1) and at the end:
              clean tile   |tmax - max|spec| over the tile| <= 4 ulp (two
                           roundings in x^2 + y^2, one in the square root)
              dirty tile   tmax >= that maximum - 4 ulp
              max of tmax over the clean tiles = max|objF| (4 ulp): every LED
                           step ends with an exact maximum
              general path no dirty tile; rmax[ty] == max(tmax[ty]) bit for bit
              max(pmax) = max|pupil| (4 ulp)
            fp16 spectrum storage: against the dequantised spectrum with the
            relative bound 2^-10 (half-precision rounding of each component).
            The read-back changes nothing: two calls return the same bits and
            the state after them is bit-identical.
  S1        the spectrum is exactly zero outside the band of the used LEDs;
            objCrop equals numpy's complex128 ifft2 of the GPU's objF (< 2e-6).
  S2        fpm_residual is [11][B], rows of repeated LEDs are bit-equal, and it
            meets test_gpu_residual.py's bound.
  ledtab    FPM_NO_LEDTAB=1 (the global-table branch of LedTab::at, otherwise
            reached only past ~20 000 order entries) is bit-identical.
Each case prints the kernel it asserted (pytest -s).
"""
import functools

import numpy as np
import pytest

import fpm_amd
import oracle_lib
import schedules
from fpm_oracle import disk_support, rel_l2
from maxima_check import check_maxima as _check_maxima
from test_gpu_residual import _bound, _env, _reference

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _oracle(key):
    """The C++ fp64 oracle of every patch; `key` = what it depends on, so rows
    that differ in the kernel or the storage only (adjacent in CASES) share it."""
    case = _BY_KEY[key]
    r = case.row
    return oracle_lib.run_fpm_batch(case.stack(), case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1,
                                    case.delta2, case.iters, threads=r.B, all_channels=case.all_channels, objF=True,
                                    init_pos=case.init_pos)


def _key(c):
    r = c.row
    return (r.Np, r.L, r.r, r.B, c.sched, c.tag, r.s3, r.s1_delta2)


_BY_KEY = {}
for _c in schedules.CASES:
    _BY_KEY.setdefault(_key(_c), _c)
# cases that share a reference next to each other
CASES = sorted(schedules.CASES, key=lambda c: (list(_BY_KEY).index(_key(c)), c.row.name))


def _solver(case, **env):
    row = case.row
    with _env(**dict(row.env), **env):
        s = fpm_amd.Solver(case.problem())
    try:
        info = s.info()
        assert info.fused_kernel == row.kernel, (info.fused_kernel, row.kernel)
        assert info.wg_per_patch == row.wg, info.wg_per_patch
        assert s.debug_plan()["general_kind"] == row.general_kind
        s.upload(case.stack())
    except BaseException:
        s.close()
        raise
    return s


def _run(case, **env):
    """fpm_init, then iters x run(1) with the maxima invariant at every stop; the final download."""
    with _solver(case, **env) as s:
        s.init()
        nd = [_check_maxima(s, case, "after fpm_init")]
        for it in range(case.iters):
            s.run(1)
            nd.append(_check_maxima(s, case, f"after iteration {it + 1}"))
        out = s.download()
        res = s.residual() if case.sched == "S2" else None
        name = fpm_amd.KERNEL_NAMES[s.info().fused_kernel]
    return out, res, name, nd


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_schedule(case):
    row = case.row
    out, res, name, nd = _run(case)
    ref = _oracle(_key(case))
    sup = disk_support(row.Np, row.r).astype(np.float32)   # un-centred, as the oracle's
    errs = []
    for b in range(row.B):
        np.testing.assert_array_equal(out["support"][b], sup)
        e = {k: rel_l2(out[k][b], ref[k][b]) for k in ("objF", "objCrop", "pupil")}
        errs.append(max(e.values()))
        for k, v in e.items():
            assert v < case.tol, (b, k, v)
    print(f"{case.id}: kernel {name} x{row.wg}, general_kind {row.general_kind}; max rel L2 {max(errs):.2e} "
          f"(bound {case.tol:g}); dirty tiles at the stops {nd}")

    if case.sched == "S1":
        sy0, sy1, sx0, sx1 = case.band()
        live = np.zeros((row.L, row.L), bool)
        live[sy0:sy1 + 1, sx0:sx1 + 1] = True
        assert not live.all()
        for b in range(row.B):
            spec = np.fft.fftshift(out["objF"][b])
            assert np.count_nonzero(spec[~live]) == 0 and np.count_nonzero(spec[live]) > 0
            assert rel_l2(out["objCrop"][b], np.fft.ifft2(out["objF"][b].astype(np.complex128))) < 2e-6

    if case.sched == "S2":
        prob = case.problem()
        assert res["err"].shape == res["ref"].shape == (11, row.B)
        for grp in schedules.S2_REPEATS:
            for i in grp[1:]:
                np.testing.assert_array_equal(res["err"][i], res["err"][grp[0]])
                np.testing.assert_array_equal(res["ref"][i], res["ref"][grp[0]])
        E, Q, S = _reference(out, case.stack(), prob)
        delta, bound = np.abs(res["err"] - E), _bound(E, Q)
        assert np.all(np.isfinite(res["err"])) and np.all(delta <= bound), \
            float((delta / np.maximum(bound, 1e-300)).max())
        np.testing.assert_array_equal(res["ref"], S)


LEDTAB = [c for c in schedules.CASES if c.row.ledtab and c.tag == "S2-init1-cv"]


@pytest.mark.parametrize("case", LEDTAB, ids=lambda c: c.id)
def test_led_table_fallback_is_bit_identical(case):
    """The four kernels with an LDS LED table (Np 256 in its three modes) read
    order / x0 / y0 from the global tables under FPM_NO_LEDTAB=1."""
    a, _, name, _ = _run(case)
    b, _, _, _ = _run(case, FPM_NO_LEDTAB="1")
    print(f"{case.id}: kernel {name} x{case.row.wg}, LDS table vs global tables")
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(a[k], b[k])
