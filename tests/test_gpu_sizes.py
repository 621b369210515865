"""Every accepted transform size up to Np 96 and the corners of the accepted
domain on the device (tests/size_cases.py; the CPU half is
tests/test_size_cases.py).

One test per Np and one per corner; per case (a radius of the Np) and context
(general path, fused path):
  * the context reports the kernel the table names (fpm_info.fused_kernel,
    fpm_debug_get_plan); below the small-patch kernel (Np 4, 6) PATH_FUSED is
    refused with FPM_ERR_INVAL and PATH_AUTO is the general path;
  * objF, objCrop and the pupil of both patches are finite and match the C++
    fp64 oracle within the project's bound: relative
    L2 < 5e-5 after two iterations;
  * fpm_residual of the final state meets test_gpu_residual.py's bound against
    its float64 evaluation (tests/residual_check.py): the sweep's transforms
    run at every size too;
  * the carried maxima (fpm_debug_get_maxima) agree with the downloaded
    spectrum (tests/maxima_check.py);
  * where the general and the fused path both run, they agree to < 2e-6 per
    output and patch, the bound of test_small_fused_equals_general_path.
One line per row (pytest -s): the worst relative L2 against the oracle and the
worst fused-against-general difference.
"""
import functools
import types

import numpy as np
import pytest

import fpm_amd
import oracle_lib
import residual_check
import size_cases as sc
from fpm_oracle import rel_l2
from maxima_check import check_maxima

pytestmark = pytest.mark.gpu

KEYS = ("objF", "objCrop", "pupil")


@functools.lru_cache(maxsize=1)
def _oracle(cid):
    """fp64 objF / objCrop / pupil of both patches, computed once per case."""
    c = sc.BY_ID[cid]
    return oracle_lib.run_fpm_batch(c.stack(), c.order, c.x0, c.y0, c.Np, c.L, c.r, sc.DELTA1, sc.DELTA2, sc.ITERS,
                                    threads=sc.B, objF=True)


def _create(case, ctx):
    """The context, or None where the table says fpm_create refuses."""
    if ctx.kernel is None:
        with pytest.raises(fpm_amd.FpmError) as e:
            fpm_amd.Solver(case.problem(ctx))
        assert e.value.code == fpm_amd.FPM_ERR_INVAL, (case.id, ctx.name)
        return None
    s = fpm_amd.Solver(case.problem(ctx))
    try:
        info = s.info()
        assert info.fused_kernel == ctx.kernel, (case.id, ctx.name, fpm_amd.KERNEL_NAMES[info.fused_kernel])
        fused = ctx.kernel != fpm_amd.KERNEL_GENERAL
        assert info.path == (fpm_amd.PATH_FUSED if fused else fpm_amd.PATH_GENERAL), (case.id, ctx.name)
        assert s.debug_plan()["general_kind"] == ctx.general_kind, (case.id, ctx.name)
    except BaseException:
        s.close()
        raise
    return s


def _run(case, ctx):
    """One context of a case; its outputs, or None where nothing runs."""
    s = _create(case, ctx)
    if s is None:
        return None
    with s:
        if not ctx.run:
            return None
        stack = case.stack()
        s.upload(stack)
        s.init()
        s.run(sc.ITERS)
        out = s.download(support=False)
        res = s.residual()
        tag = f"{case.id} {ctx.name}"
        check_maxima(s, types.SimpleNamespace(row=types.SimpleNamespace(B=sc.B, fp16=False, kernel=ctx.kernel),
                                              band=case.band), tag)
    for k in KEYS:
        assert np.isfinite(out[k]).all(), (tag, k)
    prob = types.SimpleNamespace(np_=case.Np, n_patch=sc.B, order=case.order, x0=case.x0, y0=case.y0)
    residual_check.check(tag, res, residual_check.reference(out, stack, prob))
    return out


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_size_row(row):
    worst, gap, ran = 0.0, 0.0, []
    for case in row.cases:
        ref = _oracle(case.id)
        got = {}
        for ctx in case.contexts:
            out = _run(case, ctx)
            if out is None:
                continue
            got[ctx.path] = out
            err = {k: max(rel_l2(out[k][b], ref[k][b]) for b in range(sc.B)) for k in KEYS}
            print(f"sizes {case.id} {ctx.name} ({fpm_amd.KERNEL_NAMES[ctx.kernel]}): rel L2 "
                  + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
            for k, v in err.items():
                assert np.isfinite(v) and v < case.tol, (case.id, ctx.name, k, v)
            worst = max(worst, *err.values())
        ran.append(len(got))
        if fpm_amd.PATH_GENERAL in got:
            for path, out in got.items():
                if path == fpm_amd.PATH_GENERAL:
                    continue
                d = max(rel_l2(out[k][b], got[fpm_amd.PATH_GENERAL][k][b]) for k in KEYS for b in range(sc.B))
                print(f"sizes {case.id}: fused against general rel L2 {d:.2e}")
                assert d < sc.FUSED_VS_GENERAL, (case.id, d)
                gap = max(gap, d)
    assert all(n == sum(c.run and c.kernel is not None for c in case.contexts)
               for n, case in zip(ran, row.cases))
    print(f"sizes {row.id}: worst rel L2 against the oracle {worst:.2e}"
          + (f", worst fused against general {gap:.2e}" if gap else ""))
