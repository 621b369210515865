"""fpm_set_state / fpm_download_state_device on every LED-update kernel (GPU
only).  Shapes and inputs: tests/state_cases.py (the S2-init1-cv case of every
row of schedules.KERNELS; tests/test_state_cases.py shows on the CPU that the
seeds are cases).

  1 round trip   set_state(seed) then download: bit-identical objF and pupil * S
                 (fp16 storage: from a state that came from a download); the
                 carried maxima pass maxima_check, no tile dirty, tiles outside
                 the band 0.
  2 resume       a fresh context continued from a download equals the run it
                 came from: bit for bit on the general path (maxima included),
                 within 2e-6 on the fused kernels (printed whether bit-identical).
  3 seeded       set_state(seed) + run(2) against restate_step.iterate in
                 complex128 from the installed state, at the case's bound.
  4 pupil only   init, set_state(None, P), run(1) against iterate.
  5 device       the same through device pointers equals the host path bit for
                 bit; a 1-patch source seeds a 2-patch context's pupil.
  6 refusals     every violation of the contract: code, message, and the
                 context bit for bit as it was.
  7 no stack     a state without a stack: downloads work, runs are refused.
  8 CLI          fpmMain --init-pupil / --init-objf.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import state_cases as sc
from fpm_oracle import rel_l2
from maxima_check import check_maxima
from test_gpu_residual import BIN, _env

pytestmark = pytest.mark.gpu

INVAL, STATE = fpm_amd.FPM_ERR_INVAL, fpm_amd.FPM_ERR_STATE
K3 = ("objF", "objCrop", "pupil")
FUSED_BOUND = 2e-6      # the project's bound for paths that differ only in fp32 rounding


def _solver(case, upload=True, problem=None, **env):
    """A context of the row's kernel (asserted as test_gpu_schedules._solver does), the stack uploaded."""
    row = case.row
    with _env(**dict(row.env), **env):
        s = fpm_amd.Solver(problem or case.problem())
    try:
        info = s.info()
        assert info.fused_kernel == row.kernel, (info.fused_kernel, row.kernel)
        if problem is None:
            assert info.wg_per_patch == row.wg, info.wg_per_patch
        assert s.debug_plan()["general_kind"] == row.general_kind
        if upload:
            s.upload(case.stack())
    except BaseException:
        s.close()
        raise
    return s


def _masked(P, row):
    return (np.asarray(P) * sc.support_centred(row.Np, row.r)).astype(np.complex64)


def _snapshot(s):
    return s.download(objCrop=False, support=False), s.debug_maxima()


def _assert_same(a, b, where):
    (da, ma), (db, mb) = a, b
    for k in ("objF", "pupil"):
        np.testing.assert_array_equal(da[k], db[k], err_msg=f"{where}: {k}")
    for k in ("tmax", "dirty", "pmax", "rmax"):
        if ma[k] is not None:
            np.testing.assert_array_equal(ma[k], mb[k], err_msg=f"{where}: {k}")


def _clean_outside_band(s, case, where):
    assert s.debug_band() == tuple(case.band()), (where, s.debug_band(), case.band())
    mx = s.debug_maxima()
    assert not mx["dirty"].any(), (where, "dirty tiles", int(mx["dirty"].sum()))
    sy0, sy1, sx0, sx1 = case.band()
    out = np.ones(mx["tmax"].shape[1:], bool)
    out[sy0 // 16:sy1 // 16 + 1, sx0 // 16:sx1 // 16 + 1] = False
    assert out.any() and not mx["tmax"][:, out].any(), (where, "tiles outside the band")
    assert np.array_equal(mx["pmax"][:, 1:], np.zeros_like(mx["pmax"][:, 1:])), (where, "pmax partials")
    return mx


# ---- 1. round trip ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ROWS)
def test_round_trip(name):
    case = sc.BY_ROW[name]
    row = case.row
    objF, P = sc.seed_state(case)
    with _solver(case) as s:
        s.set_state(objF, P)
        out = s.download()
        if row.fp16:   # the stored values: a second round trip from them is exact
            with _solver(case) as t:
                t.set_state(out["objF"], out["pupil"])
                again = t.download()
                check_maxima(t, case, "after set_state of a downloaded state")
            np.testing.assert_array_equal(again["objF"], out["objF"])
            np.testing.assert_array_equal(again["pupil"], out["pupil"])
            assert rel_l2(out["objF"], objF) < 2.0 ** -10
        else:
            np.testing.assert_array_equal(out["objF"], objF)
        for b in range(row.B):
            np.testing.assert_array_equal(out["pupil"][b], _masked(P, row))
            assert rel_l2(out["objCrop"][b], np.fft.ifft2(out["objF"][b].astype(np.complex128))) < 2e-6
        assert check_maxima(s, case, "after set_state") == 0
        mx = _clean_outside_band(s, case, name)
        if mx["rmax"] is not None:
            np.testing.assert_array_equal(mx["rmax"], mx["tmax"].max(axis=2))


# ---- 2. resume ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ROWS)
def test_resume(name):
    case = sc.BY_ROW[name]
    row = case.row
    with _solver(case) as a:
        a.init()
        a.run(1)
        mid, mx_a = _snapshot(a)
        a.run(1)
        end_a = a.download()
    with _solver(case) as b:
        b.set_state(mid["objF"], mid["pupil"])
        mx_b = b.debug_maxima()
        assert not mx_b["dirty"].any()
        b.run(1)
        end_b = b.download()
    if row.kernel == fpm_amd.KERNEL_GENERAL:
        np.testing.assert_array_equal(mx_b["tmax"], mx_a["tmax"])
        np.testing.assert_array_equal(mx_b["rmax"], mx_a["rmax"])
        np.testing.assert_array_equal(mx_b["pmax"].max(axis=1), mx_a["pmax"].max(axis=1))
        for k in K3:
            np.testing.assert_array_equal(end_b[k], end_a[k], err_msg=k)
        print(f"{name}: resumed bit-identically (maxima and final state)")
        return
    same = all(np.array_equal(end_b[k], end_a[k]) for k in K3)
    worst = max(rel_l2(end_b[k][p], end_a[k][p]) for k in K3 for p in range(row.B))
    print(f"{name}: resumed {'bit-identically' if same else 'NOT bit-identically'}; max rel L2 {worst:.2e} "
          f"(bound {FUSED_BOUND:g})")
    assert worst < FUSED_BOUND, worst


# ---- 3. seeded parity ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _yardstick_1024(shape):
    """Patch 0 of the Np 1024 rows from the seed itself (the fp32 row installs it
    bit for bit, test_round_trip; the fp16 row's quantisation of it, 2^-11 per
    component, is far inside that row's 1e-2): one yardstick for both rows."""
    case = next(c for c in sc.CASES if (c.row.Np, c.row.L, c.row.r) == shape)
    return sc.iterate(case, sc.seed_spectrum(case, 0), _masked(sc.seed_pupil(case.row.Np, case.row.r), case.row), 2)


@pytest.mark.parametrize("name", sc.ROWS)
def test_seeded_parity(name):
    case = sc.BY_ROW[name]
    row = case.row
    objF, P = sc.seed_state(case)
    with _solver(case) as s:
        s.set_state(objF, P)
        st0 = s.download(objCrop=False, support=False)
        s.run(2)
        out = s.download()
        check_maxima(s, case, "after set_state and two iterations")
    worst = 0.0
    for b in range(row.B if row.Np < 1024 else 1):
        ref = (_yardstick_1024((row.Np, row.L, row.r)) if row.Np >= 1024
               else sc.iterate(case, st0["objF"][b], st0["pupil"][b], 2, patch=b))
        for k in K3:
            e = rel_l2(out[k][b], ref[k])
            worst = max(worst, e)
            assert e < case.tol, (b, k, e)
    print(f"{name}: max rel L2 {worst:.2e} (bound {case.tol:g})")


# ---- 4. pupil only ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_patch", [("fused_small", False), ("fused_np256", False), ("general_reg256", False),
                                            ("general_lds", True)])
def test_pupil_only(name, per_patch):
    case = sc.BY_ROW[name]
    row = case.row
    Ps = [sc.seed_pupil(row.Np, row.r, variant=b if per_patch else 0) for b in range(row.B)]
    with _solver(case) as s:
        s.init()
        o0 = s.download(objCrop=False, pupil=False, support=False)["objF"]
        s.set_state(None, np.stack(Ps) if per_patch else Ps[0])
        got = s.download(objCrop=False, support=False)
        np.testing.assert_array_equal(got["objF"], o0)           # the spectrum is kept
        check_maxima(s, case, "after a pupil-only set_state")
        s.run(1)
        out = s.download()
    if per_patch:
        assert not np.array_equal(Ps[0], Ps[1])
    for b in range(row.B):
        np.testing.assert_array_equal(got["pupil"][b], _masked(Ps[b], row))
        ref = sc.iterate(case, o0[b], _masked(Ps[b], row), 1, patch=b)
        for k in K3:
            assert rel_l2(out[k][b], ref[k]) < 1e-5, (b, k)      # the project's bound for one iteration


# ---- 5. device pointers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused_np200", "general_reg1024_fp16"])
def test_device_pointers_equal_the_host_path(name):
    import torch
    case = sc.BY_ROW[name]
    row = case.row
    tF = torch.empty((row.B, row.L, row.L, 2), dtype=torch.float32, device="cuda")
    tP = torch.empty((row.B, row.Np, row.Np, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with _solver(case) as a:
        a.init()
        a.run(1)
        a.download_state_device(tF.data_ptr(), tP.data_ptr())
        mid = a.download(objCrop=False, support=False)
    np.testing.assert_array_equal(tF.cpu().numpy().view(np.complex64)[..., 0], mid["objF"])
    np.testing.assert_array_equal(tP.cpu().numpy().view(np.complex64)[..., 0], mid["pupil"])
    outs = []
    for device in (True, False):
        with _solver(case) as b:
            if device:
                b.set_state_device(tF.data_ptr(), tP.data_ptr())
            else:
                b.set_state(mid["objF"], mid["pupil"])
            mx = b.debug_maxima()
            b.run(1)
            outs.append((b.download(), mx))
    for k in K3:
        np.testing.assert_array_equal(outs[0][0][k], outs[1][0][k], err_msg=k)
    for k in ("tmax", "pmax"):
        np.testing.assert_array_equal(outs[0][1][k], outs[1][1][k], err_msg=k)


def test_one_patch_seeds_a_field_through_a_shared_device_pupil():
    import torch
    case = sc.BY_ROW["fused_np200"]
    row = case.row
    one = case.problem()
    one.n_patch = 1
    tP = torch.empty((row.Np, row.Np, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with _solver(case, upload=False, problem=one) as a:
        a.upload(case.stack()[:, :1])
        a.init()
        a.run(1)
        a.download_state_device(None, tP.data_ptr())
        src = a.download(objF=False, objCrop=False, support=False)["pupil"][0]
    with _solver(case) as b:
        b.init()
        o0 = b.download(objCrop=False, pupil=False, support=False)["objF"]
        b.set_state_device(None, tP.data_ptr(), pupil_shared=True)
        got = b.download(objCrop=False, support=False)
        b.run(1)
        end_dev = b.download()
    with _solver(case) as h:       # the same seeding through host memory
        h.init()
        h.set_state(None, src)
        h.run(1)
        end_host = h.download()
    assert np.abs(src).max() != 1.0
    np.testing.assert_array_equal(got["objF"], o0)
    for p in range(row.B):
        np.testing.assert_array_equal(got["pupil"][p], src)
    for k in K3:
        np.testing.assert_array_equal(end_dev[k], end_host[k], err_msg=k)


# ---- 6. refusals --------------------------------------------------------------------------------
def _refused(s, call, code, *words):
    with pytest.raises(fpm_amd.FpmError) as ei:
        call()
    assert ei.value.code == code, ei.value
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_refusals_leave_the_context_as_it_was():
    case = sc.BY_ROW["general_lds_L90"]
    row = case.row
    assert case.band() == (35, 55, 35, 55) and row.B == 3
    objF, P = sc.seed_state(case)
    P3 = np.stack([P] * row.B)
    c = row.Np // 2

    def spectrum(edit):
        o = objF.copy()
        edit(o)
        return o

    def pupils(edit):
        q = P3.copy()
        edit(q)
        return q

    def outside(o):
        o[1, 20, 20] = 1e-30      # un-centred (20, 20) is centred (65, 65): outside rows / columns 35..55
        o[2, 20, 20] = 1.0

    def nans(o):
        o[0, 50, 7] = complex(np.nan, 0)
        o[2, 1, 1] = complex(0, np.nan)

    def inf_inside(q):
        q[1, c + 1, c - 2] = complex(0, np.inf)

    def zero_patch_1(q):
        q[1] = 0

    with _solver(case) as s, _solver(case) as control:
        for t in (s, control):
            t.init()
            t.run(1)
        before = _snapshot(s)
        bad = [
            ("outside the band", lambda: s.set_state(spectrum(outside), P3), INVAL,
             ("objF", "(patch 1, y 20, x 20)", "band", "rows [35, 55]")),
            ("NaN in objF", lambda: s.set_state(spectrum(nans), P3), INVAL, ("objF", "finite", "(patch 0, y 50, x 7)")),
            ("NaN in objF, spectrum only", lambda: s.set_state(spectrum(nans), None), INVAL, ("objF", "finite")),
            ("Inf in the pupil", lambda: s.set_state(objF, pupils(inf_inside)), INVAL,
             ("pupil", "finite", f"(patch 1, y {c + 1}, x {c - 2})")),
            ("zero pupil of patch 1", lambda: s.set_state(None, pupils(zero_patch_1)), INVAL, ("pupil", "patch 1", "zero")),
            ("both NULL", lambda: s.set_state(None, None), INVAL, ("both NULL",)),
        ]
        for what, call, code, words in bad:
            _refused(s, call, code, *words)
            _assert_same(before, _snapshot(s), what)

        import torch
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        tF = torch.zeros((row.B, row.L, row.L, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for call in (lambda: s.set_state(objF, P3), lambda: s.download_state_device(tF.data_ptr(), None)):
            g = torch.cuda.CUDAGraph()
            with pytest.raises(fpm_amd.FpmError) as ei:
                with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                    call()
            assert ei.value.code == INVAL and "capturing" in str(ei.value)
        s.set_stream(None)
        _assert_same(before, _snapshot(s), "a capturing stream")

        s.run(1)
        control.run(1)
        got, want = s.download(), control.download()
        for k in K3:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_nan_outside_the_disk_is_accepted():
    case = sc.BY_ROW["general_lds_L90"]
    row = case.row
    P = sc.seed_pupil(row.Np, row.r).copy()
    S = sc.support_centred(row.Np, row.r)
    P[~S] = complex(np.nan, np.inf)
    with _solver(case) as s:
        s.init()
        s.set_state(None, P)
        got = s.download(objF=False, objCrop=False, support=False)["pupil"]
        for b in range(row.B):
            np.testing.assert_array_equal(got[b], np.where(S, P, 0).astype(np.complex64))
        check_maxima(s, case, "NaN outside the disk")


def test_one_array_before_a_state_exists_is_refused():
    case = sc.BY_ROW["general_lds_L90"]
    objF, P = sc.seed_state(case)
    with _solver(case) as s:
        _refused(s, lambda: s.set_state(None, P), STATE, "objF NULL")
        _refused(s, lambda: s.set_state(objF, None), STATE, "pupil NULL")
        _refused(s, lambda: s.download_state_device(1, None), STATE)
        _refused(s, lambda: s.download(), STATE)
        s.set_state(objF, P)
        s.run(1)


def test_fp16_overflow_is_refused():
    case = sc.BY_ROW["general_reg1024_fp16"]
    row = case.row
    with _solver(case) as s, _solver(case) as control:
        for t in (s, control):
            t.init()
        before = _snapshot(s)
        objF = before[0]["objF"].copy()
        objF[1, 0, 3] = 65504.0 * row.Np ** 2     # un-centred (0, 3) is centred (L/2, L/2 + 3): inside the band
        _refused(s, lambda: s.set_state(objF, before[0]["pupil"]), INVAL, "objF", "fp16", "(patch 1, y 0, x 3)")
        _assert_same(before, _snapshot(s), "fp16 overflow")
        objF[1, 0, 3] = 65503.0 * row.Np ** 2     # the largest accepted magnitude class
        s.set_state(objF, None)
        s.set_state(before[0]["objF"], None)
        _assert_same(before, _snapshot(s), "the state put back")
        s.run(1)
        control.run(1)
        got, want = s.download(), control.download()
        for k in K3:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---- 7. no stack --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general_lds", "fused_small"])
def test_state_without_a_stack(name):
    case = sc.BY_ROW[name]
    row = case.row
    objF, P = sc.seed_state(case)
    with _solver(case, upload=False) as s:
        _refused(s, lambda: s.download(), STATE)
        s.set_state(objF, P)
        out = s.download()
        np.testing.assert_array_equal(out["objF"], objF)
        for b in range(row.B):
            assert rel_l2(out["objCrop"][b], np.fft.ifft2(objF[b].astype(np.complex128))) < 2e-6
        check_maxima(s, case, "a state without a stack")
        _refused(s, lambda: s.run(1), STATE, "stack")
        _refused(s, lambda: s.residual(), STATE, "stack")
        np.testing.assert_array_equal(s.download(objCrop=False, support=False)["objF"], objF)   # still there
        # after the debug objCrop entry, which leaves the context without a state
        spec = np.fft.fftshift(objF, axes=(-2, -1))
        s.debug_objcrop(spec, case.band())
        _refused(s, lambda: s.download(), STATE)
        s.set_state(objF, P)
        # a stack upload clears the state, as it always did; with a stack the state runs
        s.upload(case.stack())
        _refused(s, lambda: s.download(), STATE)
        s.set_state(objF, P)
        s.run(2)
        got = s.download()
    with _solver(case) as t:
        t.set_state(objF, P)
        t.run(2)
        want = t.download()
    for k in K3:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---- 8. CLI -------------------------------------------------------------------------------------
def test_cli_initial_state(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")

    def run(tag, iters, *extra):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], str(iters), "--out", str(out), *extra], capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return out, json.loads((out / "result.json").read_text())

    two, meta2 = run("two", 2)
    one, _ = run("one", 1)
    assert "initial_state" not in meta2
    res, meta = run("resumed", 1, "--init-objf", str(one / "objF.npy"), "--init-pupil", str(one / "pupil.npy"))
    assert meta["initial_state"] == dict(pupil=str(one / "pupil.npy"), pupil_shared=True, objf=str(one / "objF.npy"),
                                         replaces_init=True)
    same = True                           # the fused bound of test_resume (a general-path context meets it with zeros)
    for k in ("objF", "objCrop", "pupil"):
        a, b = np.load(res / f"{k}.npy"), np.load(two / f"{k}.npy")
        same = same and np.array_equal(a, b)
        assert rel_l2(a, b) < FUSED_BOUND, k
    print(f"fpmMain resumed from objF.npy + pupil.npy {'bit-identically' if same else 'within the bound'}")

    # a path with the two characters a JSON string must escape
    odd = tmp_path / 'pu"pil\\seed.npy'
    odd.write_bytes((one / "pupil.npy").read_bytes())
    seeded, meta = run("seeded", 1, "--init-pupil", str(odd))
    assert meta["initial_state"] == dict(pupil=str(odd), pupil_shared=True, objf=None, replaces_init=False)
    assert not np.array_equal(np.load(seeded / "pupil.npy"), np.load(one / "pupil.npy"))
