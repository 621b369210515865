"""objCrop on dense spectra and every live-band shape (GPU only).

Every case of tests/objcrop_cases.py -- a context that reaches one of the six
objCrop kernel families, a band the launchers accept -- through
fpm_debug_objcrop: the product's launch_objcrop with the context's own plan
on a spectrum that is dense N(0,1) noise inside the band and NaN outside it,
into an objCrop buffer filled with NaN.  The plan read back from the context
(fpm_debug_get_objcrop_plan) must name the family and the rows per block of
the table row, so a context that stopped reaching its family fails.  The result must be finite everywhere (nothing outside the band was
used, every element was written, no intermediate row was read that no pass
wrote) and within BOUND = 2e-6 relative L2 of numpy's complex128 ifft2, per
patch.  An fp32 CPU transform of the same inputs gives 1.2e-7 .. 2.3e-7
(tests/test_objcrop_cases.py).

Largest relative L2 measured on an MI355X, per context (all bands, all patches):
  L512 1.50e-7   L768 1.61e-7   L1024 1.57e-7   L600 1.69e-7   L360 1.54e-7
  L4096 1.80e-7  L4096h 1.73e-7  L4096b 1.38e-7  L3000 1.82e-7
  L90 1.37e-7    L96 1.31e-7    L192 1.40e-7    L96h 1.22e-7   L768h 1.48e-7
  L810 1.68e-7   L2430 1.82e-7  L5400 1.51e-7
The smallest, 6.2e-8, is L512 one_row; no case left an element not finite.
The longest cases are the two of L 5400 (233 MB per array, one sequence per
block of k_fft_batch): 0.7 s each, most of it the complex128 reference.
"""
import ctypes

import numpy as np
import pytest

import fpm_amd
import objcrop_cases as oc
from fpm_oracle import rel_l2
from objcrop_cases import BOUND
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

CASES = oc.cases()
# fpm_objcrop_plan.kind of each family of the table
KINDS = {oc.REGS: (fpm_amd.OBJCROP_REGS_256M, fpm_amd.OBJCROP_REGS_600, fpm_amd.OBJCROP_REGS_360),
         oc.C4K: (fpm_amd.OBJCROP_SIX_STEP_4K,), oc.BATCHED: (fpm_amd.OBJCROP_BATCHED,)}


@pytest.mark.parametrize("ctx,name", CASES, ids=[oc.case_id(c, b) for c, b in CASES])
def test_objcrop_case(ctx, name, monkeypatch):
    spec = oc.make_input(ctx, name)
    ref = oc.reference(spec)
    for k, v in ctx.env.items():
        monkeypatch.setenv(k, v)
    with fpm_amd.Solver(ctx.problem(name)) as s:
        plan = s.debug_objcrop_plan()
        out = s.debug_objcrop(spec, oc.band(ctx, name))
    # what the context launches is what the table row names (the switch was read at create)
    assert plan["kind"] in KINDS[ctx.family] and plan["per_block"] == ctx.Gr, (ctx.id, plan)
    assert plan == fpm_amd.debug_plan_objcrop(ctx.L, ctx.fp16, "FPM_NO_CROP4K" in ctx.env)
    assert out.shape == spec.shape and out.dtype == np.complex64
    bad = ~np.isfinite(out)
    assert not bad.any(), f"{np.count_nonzero(bad)} elements not finite, first at {tuple(np.argwhere(bad)[0])}"
    errs = [rel_l2(out[b], ref[b]) for b in range(len(spec))]
    print(f"objcrop {oc.case_id(ctx, name)}: rel L2 " + " ".join(f"{e:.3e}" for e in errs))
    for b, e in enumerate(errs):
        assert e < BOUND, (b, e)


def test_arguments_are_checked():
    ctx = oc.BY_ID["L96"]
    L = ctx.L
    spec = oc.make_input(ctx, "one_row")
    with fpm_amd.Solver(ctx.problem("one_row")) as s:
        for bad in ((-1, 5, 0, 5), (6, 5, 0, 5), (0, L, 0, 5), (0, 5, -1, 5), (0, 5, 6, 5), (0, 5, 0, L)):
            with pytest.raises(fpm_amd.FpmError) as e:
                s.debug_objcrop(spec, bad)
            assert e.value.code == fpm_amd.FPM_ERR_INVAL, bad
        lib = fpm_amd.load_library()
        band = (ctypes.c_int * 4)(0, 5, 0, 5)
        out = np.empty_like(spec)
        f = fpm_amd._f32p
        for args in ((None, f(spec), band, f(out)), (s._h, None, band, f(out)), (s._h, f(spec), None, f(out)),
                     (s._h, f(spec), band, None)):
            assert lib.fpm_debug_objcrop(*args) == fpm_amd.FPM_ERR_INVAL


def test_context_recovers_after_debug_objcrop():
    """fpm_debug_objcrop clobbers the spectrum: fpm_run and fpm_download refuse
    until fpm_init, and after upload and fpm_init a run gives the bits of a
    fresh context -- the planned band and everything else the context planned
    are as they were."""
    Np, L, r = 32, 96, 6
    x0, y0, order = grid_geometry(Np, L, 3, 4)
    stack = make_stack(Np, L, r, x0, y0, n_patch=2, seed=17)
    prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=2)
    fresh = fpm_amd.run_fpm(prob, stack, 2)
    ctx = oc.BY_ID["L96"]
    assert (ctx.Np, ctx.L) == (Np, L)
    spec = oc.make_input(ctx, "lo_hi")
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(1)
        s.debug_objcrop(spec, oc.band(ctx, "lo_hi"))
        for call in (lambda: s.run(1), s.download):
            with pytest.raises(fpm_amd.FpmError) as e:
                call()
            assert e.value.code == fpm_amd.FPM_ERR_STATE
        s.upload(stack)
        s.init()
        s.run(2)
        again = s.download()
    for k in ("objF", "objCrop", "pupil", "support"):
        np.testing.assert_array_equal(again[k], fresh[k], err_msg=k)


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")  # the refused capture records nothing
def test_capturing_stream_is_refused():
    """As fpm_run (test_run_on_a_capturing_stream_is_refused): the call blocks, so
    FPM_ERR_INVAL before anything is enqueued or changed -- the state is kept."""
    import torch
    Np, L, r = 32, 96, 6
    x0, y0, order = grid_geometry(Np, L, 3, 4)
    stack = make_stack(Np, L, r, x0, y0, n_patch=2, seed=17)
    ctx = oc.BY_ID["L96"]
    spec = oc.make_input(ctx, "one_row")
    with fpm_amd.Solver(fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=2)) as s:
        s.upload(stack)
        s.init()
        s.run(1)
        want = s.download()
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(fpm_amd.FpmError) as ei:
            with torch.cuda.graph(graph, stream=cs, capture_error_mode="relaxed"):
                s.debug_objcrop(spec, oc.band(ctx, "one_row"))
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        s.set_stream(None)
        got = s.download()      # still initialised, nothing overwritten
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
