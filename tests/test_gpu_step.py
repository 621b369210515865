"""Two LED steps from an installed state on every LED-update kernel, checked
pixel by pixel (GPU only).  Cases, seeds and the bound: tests/step_cases.py;
tests/test_step_cases.py shows on the CPU that they are cases and that the
comparison used here rejects a skipped rim pixel, a stale maximum and a mixed-up
measurement block.

Per case: a context of the row's kernel (kernel, wg_per_patch and general_kind
asserted), the edited stack uploaded, set_state(seed), download ("before"),
run(iters), download.  Per patch:

  1 untouched   objF outside the union of the order's disks is bit-equal to
                "before"; the pupil outside the support is exactly 0; support
                is the oracle's disk.
  2 touched     |got - ref| <= bound(k) = C[row] 2^-24 s(k) for objF and the
                pupil at every touched pixel, ref = restate_step.iterate in
                complex128 from "before".  (On fp32 storage "before" is the
                seed bit for bit, asserted, so rows of one shape share ref.)
  3 objCrop     against numpy's complex128 ifft2 of the GPU's own objF at 2e-6.
  4 maxima      maxima_check.check_maxima after the run.

fp16 spectrum storage runs 1 (against its own "before"), 3 and 4 and then the
row's relative L2 of 1e-2 instead of 2: the 2^-11 rounding of the stored
spectrum after step 1 enters the pupil update of step 2 pixel by pixel, far
above a bound built on 2^-24, so per-pixel values under fp16 storage are not
what this file checks.
"""
import time

import numpy as np
import pytest

import fpm_amd
import state_cases as sc
import step_cases as st
from fpm_oracle import disk_support, rel_l2
from maxima_check import check_maxima
from test_gpu_residual import _env

pytestmark = pytest.mark.gpu

OBJCROP_BOUND = 2e-6


def _groups(name):
    """The row's cases by context: cases that differ only in the seed's variant and
    agree in every scalar of the problem (plain) run in one context."""
    out = {}
    for c in st.cases(name):
        out.setdefault((c.order, c.iters, c.pset, c.flags) + c.scalars(), []).append(c)
    return list(out.values())


GROUPS = [g for n in st.ROWS for g in _groups(n)]


def _gid(g):
    c = g[0]
    return c.id.rsplit("-", 1)[0] + "-" + "+".join(x.variant for x in g)


def _solver(case):
    """A context of the row's kernel, asserted as test_gpu_state._solver does, the edited stack uploaded."""
    row = case.row
    with _env(**dict(row.env)):
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


def _reference(case, before, b):
    """The complex128 yardstick from the downloaded state of patch b: the cached one where that is the seed."""
    if np.array_equal(before["objF"][b], case.seed(b)) and np.array_equal(before["pupil"][b], st.masked_pupil(case)):
        return st.yardstick(case, b)
    assert case.row.fp16, (case.id, b, "set_state did not install the seed bit for bit")
    out = st.iterate(case, before["objF"][b], before["pupil"][b], b)
    return dict(objF=st.band_of(case, out["objF"]), pupil=out["pupil"])


def _check(case, s):
    row = case.row
    objF, P = st.seed_state(case)
    s.set_state(objF, P)
    before = s.download(objCrop=False, support=False)
    s.run(case.iters)
    out = s.download()
    check_maxima(s, case.geo, f"{case.id}: after the run")                                  # 4
    name = fpm_amd.KERNEL_NAMES[s.info().fused_kernel]

    outside = np.fft.ifftshift(~case.disks())
    S = sc.support_centred(row.Np, row.r)
    sup = disk_support(row.Np, row.r).astype(np.float32)
    worst = (0.0, None)
    for b in range(row.B):
        np.testing.assert_array_equal(out["objF"][b][outside], before["objF"][b][outside],  # 1
                                      err_msg=f"{case.id}: patch {b}, objF outside the disks")
        assert not out["pupil"][b][~S].any(), (case.id, b, "pupil outside the support")
        np.testing.assert_array_equal(out["support"][b], sup, err_msg=f"{case.id}: patch {b}, support")
        e = rel_l2(out["objCrop"][b], np.fft.ifft2(out["objF"][b].astype(np.complex128)))   # 3
        assert e < OBJCROP_BOUND, (case.id, b, "objCrop", e)
        ref = _reference(case, before, b)
        got = dict(objF=st.band_of(case, out["objF"][b]), pupil=out["pupil"][b])
        seed = dict(objF=st.band_of(case, before["objF"][b]), pupil=before["pupil"][b])
        if row.fp16:
            for k in ("objF", "pupil"):
                e = rel_l2(got[k], ref[k])
                worst = max(worst, (e, (k, b)))
                assert e < 1e-2, (case.id, b, k, e)
            continue
        for k in ("objF", "pupil"):                                                         # 2
            ratio, where = st.compare(got[k], ref[k], seed[k], st.C[case.name])
            worst = max(worst, (ratio, (k, b) + where))
    if row.fp16:
        print(f"{case.id}: kernel {name} x{row.wg}, general_kind {row.general_kind}; fp16 storage, max rel L2 "
              f"{worst[0]:.2e} at {worst[1]} (bound 1e-2)")
        return
    print(f"{case.id}: kernel {name} x{row.wg}, general_kind {row.general_kind}; worst |got - ref| / bound "
          f"{worst[0]:.3f} at (array, patch, y, x) {worst[1]} (C {st.C[case.name]:g})")
    assert worst[0] <= 1.0, (case.id, worst)


@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_step(group):
    t0 = time.perf_counter()
    with _solver(group[0]) as s:
        for case in group:
            _check(case, s)
    print(f"{_gid(group)}: {time.perf_counter() - t0:.2f} s")
