"""fpm_gradient: the gradient of the data-fidelity cost f = sum (|psi| - g sqrt(I))^2
with respect to the spectrum and the pupil, G = df/dRe + i df/dIm, through the
GradArgs tail of the residual sweep's column kernels (csrc/residual_dev.hpp),
the rows-out and the gather-form accumulate kernels (csrc/gradient.hip).

The yardstick, the bound and its derivation are tests/gradient_check.py's: a
float64 numpy evaluation of the DOWNLOADED state, so both sides read the same
fp32 state.  At least one iteration runs before a comparison, so the pupil is
not flat, and every parity case has a gain table that is nowhere 1.  The
measured ratios to the bounds are printed (pytest -s).
"""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fpm_amd
import gradient_check as gc
import ladder_cases
import residual_check
from fpm_amd import descent
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

GENERAL, FUSED = fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED
NP256_KERNELS = (fpm_amd.KERNEL_FUSED_NP256, fpm_amd.KERNEL_FUSED_NP256_DIST)
G_LDS = fpm_amd.GENERAL_LDS
R_LDS, R_REG = fpm_amd.RESIDUAL_LDS, fpm_amd.RESIDUAL_REG256


@contextlib.contextmanager
def _env(**kw):
    """Environment switches for the contexts created inside (read at fpm_create)."""
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in kw:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _stack(Np, L, r, x0, y0, B, seed, peak):
    st = make_stack(Np, L, r, np.array(x0), np.array(y0), n_patch=B, seed=seed, peak=peak)
    st.setflags(write=False)
    return st


def _case(Np, L, r, nside, step, B, seed, d1=5, d2=10, path=fpm_amd.PATH_AUTO, peak=40000.0):
    x0, y0, order = grid_geometry(Np, L, nside, step)
    stack = _stack(Np, L, r, tuple(int(v) for v in x0), tuple(int(v) for v in y0), B, seed, peak)
    return fpm_amd.Problem(Np, L, order, x0, y0, r, d1, d2, n_patch=B, path=path), stack


@contextlib.contextmanager
def _solver(prob, stack, iters, kernels=None, plan=None, **env):
    with _env(**env):
        s = fpm_amd.Solver(prob)
    try:
        if kernels is not None:
            assert s.info().fused_kernel in kernels, s.info().fused_kernel
        if plan is not None:
            assert s.debug_plan() == plan
        if stack is not None:
            s.upload(stack)
            s.init()
            s.run(iters)
        yield s
    finally:
        s.close()


def _state(s):
    return s.download(objCrop=False, support=False)


def _gains(prob, seed, lo=0.6, hi=1.7):
    """A gain table that is nowhere 1: float32 [n_stack][B] in [lo, hi]."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(lo, hi, (len(prob.x0), prob.n_patch)).astype(np.float32)
    assert not np.any(g == 1)
    return g


# The bound's cap (bound <= 1e-2 ||G_ref||) depends on the case's state, not on the code under test.  The
# Np 256 r 31 windows overlap little (step 40), and with gains around 1 some images nearly fit, so ||G|| is
# small beside the worst pixel's conditioning: over six seeds and one or two iterations the cap came out
# at 0.98e-2 .. 3e-2 there.  Its table keeps every image clearly off its model instead.
GAIN_RANGE = {"fused_np256_r31_reg": (1.3, 1.9)}


def _plan(meas_g, general_kind=-1, residual_kind=R_LDS):
    return dict(meas_g=meas_g, general_kind=general_kind, residual_kind=residual_kind)


# the geometries of tests/test_gpu_predict.py's TAILS: each the smallest shape that reaches its
# column rung and stack layout
TAILS = {  # name: (Np, L, r, nside, step, B, seed, d1, d2, path, iters, kernels, plan, env, sweep column rung)
    "general_np32_wave": (32, 96, 6, 5, 4, 3, 7, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS), {},
                          "wave<4,4>"),
    "general_np32_tiled": (32, 96, 6, 5, 4, 3, 7, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                           {"FPM_NO_WAVE_COLS": "1"}, "tiled<256,16> lc 4"),
    "general_np30_one_seq": (30, 90, 5, 5, 4, 2, 11, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                             {"FPM_RES_ONE_SEQ": "1"}, "one_seq"),
    "ladder_np40_partial_tile": (40, 120, 19, 3, 19, 2, 7040, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,),
                                 _plan(0, G_LDS), {"FPM_NO_WAVE_COLS": "1"}, "tiled<256,16> lc 4"),
    # (two iterations: after one, a pixel with |psi| tiny under a bright measurement puts the bound above its cap)
    "ladder_np360_512_threads": (360, 720, 40, 3, 40, 2, 7360, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,),
                                 _plan(0, G_LDS), {"FPM_NO_WAVE_COLS": "1"}, "tiled<512,16> lc 4"),
    "fused_small_np8_gNp": (8, 24, 1, 2, 3, 2, 71 + 8 + 1, 5, 10, FUSED, 1, (fpm_amd.KERNEL_FUSED_SMALL,), _plan(8),
                            {}, None),
    "fused_np90_g9": (90, 180, 3, 2, 10, 2, 91 + 3, 5, 10, FUSED, 2, (fpm_amd.KERNEL_FUSED_NP90,), _plan(9), {}, None),
    "fused_np200_g10": (200, 600, 1, 2, 3, 2, 61 + 1, 10, 3, FUSED, 1, (fpm_amd.KERNEL_FUSED_NP200,), _plan(10), {},
                        None),
    "fused_np256_r31_reg": (256, 512, 31, 3, 40, 2, 140 + 31, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_REG), {},
                            None),
    "fused_np256_r33_reg": (256, 512, 33, 3, 20, 3, 40 + 33, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_REG), {},
                            None),
    "fused_np256_r33_lds": (256, 512, 33, 3, 20, 2, 40 + 33, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_LDS),
                            {"FPM_RES_LDS": "1"}, None),
}
EXACT = ("general_np32_wave", "fused_np256_r33_reg")


def _open(name, **more_env):
    Np, L, r, nside, step, B, seed, d1, d2, path, iters, kernels, plan, env, rung = TAILS[name]
    prob, stack = _case(Np, L, r, nside, step, B, seed, d1, d2, path)
    return prob, stack, seed, rung, _solver(prob, stack, iters, kernels, plan, **dict(env, **more_env))


@functools.lru_cache(maxsize=None)
def _tail_run(name):
    """One context per case: the downloaded state, the gains, the gradient with
    its sums, fpm_residual_at's sums of the same list and the float64
    reference.  Shared by the tests that compare against it; read-only."""
    prob, stack, seed, rung, ctx = _open(name)
    n = len(prob.order)
    with ctx as s:
        if rung is not None:
            assert ladder_cases.rung_name(s.debug_ladder(True)["cols"], "lc") == rung
        state = _state(s)
        g = _gains(prob, seed, *GAIN_RANGE.get(name, ()))
        s.set_gains(g)
        got = s.gradient(sums=True)
        ms = s.gradient_ms
        res = s.residual_at(np.arange(n), np.zeros(n, int), np.zeros(n, int))
    ref = gc.gradient(state, prob, stack, g)
    for v in list(got.values()) + [a for a in ref.values()]:
        v.setflags(write=False)
    return dict(prob=prob, stack=stack, state=state, g=g, got=got, res=res, ref=ref, ms=ms)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)  # complex64 and float64 alike: one word per element


def _same(a, b, what=""):
    for k in ("objF", "pupil"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what} {k}")


# ---- 1. parity on every column rung and stack layout; 3. the sums -----------------------
@pytest.mark.parametrize("name", list(TAILS))
def test_parity_and_sums_on_every_rung_and_layout(name):
    d = _tail_run(name)
    got, ref, res = d["got"], d["ref"], d["res"]
    gc.check(name, got, ref)
    # E / S of the same pass against fpm_residual_at's for the same list
    bnd = residual_check.bound(ref["err"], ref["Q"])
    gap = np.abs(got["err"] - res["err"])
    print(f"gradient {name} sums: max |E_grad - E_residual_at|/bound "
          f"{np.divide(gap, bnd, out=np.zeros_like(gap), where=bnd > 0).max():.3e}; equal to the bit: "
          f"{np.array_equal(_bits(got['err']), _bits(res['err']))}; sweep {d['ms']:.3f} ms")
    assert np.all(gap <= bnd)
    np.testing.assert_array_equal(got["ref"], res["ref"])
    np.testing.assert_array_equal(got["ref"], ref["ref"])


# ---- 2. exactness, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT)
def test_exactness(name):
    import torch
    d = _tail_run(name)
    prob, stack, seed, _, ctx = _open(name)
    n, B, Np, L = len(prob.order), prob.n_patch, prob.np_, prob.L
    want = d["got"]
    with ctx as s:
        s.set_gains(d["g"])
        before, stack_before, crops_before = s.download(), s.download_stack(), s.crops()
        t0, k0 = s.timing(), s.clock()
        first = s.gradient(sums=True)
        _same(first, want, "another context")
        _same(s.gradient(), first, "second call")
        np.testing.assert_array_equal(first["err"], want["err"])
        # only one output asked for: the bits of both
        _same(dict(s.gradient(pupil=False), pupil=first["pupil"]), first, "objF alone")
        _same(dict(s.gradient(objF=False), objF=first["objF"]), first, "pupil alone")
        # read-only
        after = s.download()
        for f in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(after[f], before[f], err_msg=f)
        np.testing.assert_array_equal(s.download_stack(), stack_before)
        np.testing.assert_array_equal(s.gains(), d["g"])
        for u, v in zip(s.crops(), crops_before):
            np.testing.assert_array_equal(u, v)
        t1, k1 = s.timing(), s.clock()
        for f, _ in fpm_amd.fpm_timing._fields_:
            assert getattr(t0, f) == getattr(t1, f), f
        for f, _ in fpm_amd.fpm_clock._fields_:
            assert getattr(k0, f) == getattr(k1, f), f
        # exactly zero outside the union of the disks and outside the support
        assert not np.any(_bits(first["objF"])[:, ~gc.union_of_disks(prob)])
        assert not np.any(_bits(first["pupil"])[:, gc.support(Np, prob.radius) == 0])
        assert np.any(first["objF"][:, gc.union_of_disks(prob)]) and np.any(first["pupil"])
        # a device-pointer result (the memory dirty before the call) equals the host result
        dO = torch.full((B, L, L, 2), 7.0, dtype=torch.float32, device="cuda")
        dP = torch.full((B, Np, Np, 2), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out = s.gradient(device_ptrs=(dO.data_ptr(), dP.data_ptr()), sums=True)
        assert set(out) == {"err", "ref"}
        torch.cuda.synchronize()
        assert dO.cpu().numpy().tobytes() == first["objF"].tobytes()
        assert dP.cpu().numpy().tobytes() == first["pupil"].tobytes()
        np.testing.assert_array_equal(out["err"], first["err"])
        # a dark entry appended: LED order[0] with its window moved to the corner, clear of the band
        led = int(prob.order[0])
        pos, zero = list(range(n)), [0] * n
        lit = s.gradient(pos=pos, dx=zero, dy=zero, sums=True)
        _same(lit, first, "the identity list as probes")
        dark = s.gradient(pos=pos + [0], dx=zero + [-int(prob.x0[led])], dy=zero + [-int(prob.y0[led])], sums=True)
        assert np.all(dark["err"][n] > 0) and s.moments([0], [-int(prob.x0[led])], [-int(prob.y0[led])])["model"].max() == 0
        _same(dark, first, "dark entry appended")
        np.testing.assert_array_equal(dark["err"][:n], first["err"])
        # gains of 1.0f: the bits of no table
        s.set_gains(np.ones_like(d["g"]))
        ones = s.gradient(sums=True)
        s.set_gains(None)
        none = s.gradient(sums=True)
        _same(ones, none, "unit gains")
        np.testing.assert_array_equal(ones["err"], none["err"])
        assert not np.array_equal(none["objF"], first["objF"])
    # FPM_RES_BATCH=1: every entry a launch of its own
    prob, stack, seed, _, ctx = _open(name, FPM_RES_BATCH="1")
    with ctx as s:
        s.set_gains(d["g"])
        one = s.gradient(sums=True)
    _same(one, want, "FPM_RES_BATCH=1")
    np.testing.assert_array_equal(one["err"], want["err"])


# ---- 4. moved windows, repeats, additivity ---------------------------------------------------
def test_moved_windows_repeats_and_split_lists():
    d = _tail_run("general_np32_wave")
    prob, stack, seed, _, ctx = _open("general_np32_wave")
    pos, dx, dy = [0, 3, 24, 7, 3, 12], [1, -2, 0, 3, -2, 0], [0, 2, -3, -1, 2, 1]  # entries 1 and 4 repeat
    with ctx as s:
        s.set_gains(d["g"])
        got = s.gradient(pos=pos, dx=dx, dy=dy, sums=True)
        res = s.residual_at(pos, dx, dy)
        a = s.gradient(pos=pos[:2], dx=dx[:2], dy=dy[:2])
        b = s.gradient(pos=pos[2:], dx=dx[2:], dy=dy[2:])
    ref = gc.gradient(d["state"], prob, stack, d["g"], pos, dx, dy)
    gc.check("moved windows and a repeat", got, ref)
    assert np.all(np.abs(got["err"] - res["err"]) <= residual_check.bound(ref["err"], ref["Q"]))
    assert not np.array_equal(got["objF"], d["got"]["objF"])
    assert not np.any(_bits(got["objF"])[:, ~gc.union_of_disks(prob, pos, dx, dy)])
    for name in ("objF", "pupil"):
        for p in range(prob.n_patch):
            gap = np.linalg.norm(got[name][p].astype(np.complex128) - a[name][p].astype(np.complex128) -
                                 b[name][p].astype(np.complex128))
            lim = ref["acc_" + name][p]
            print(f"gradient split list {name} patch {p}: ||G(AB) - G(A) - G(B)|| / accumulation term {gap / lim:.3e}")
            assert gap <= lim


# ---- 5. the majorised step, end to end -------------------------------------------------------
@pytest.mark.parametrize("name", EXACT)
def test_majorised_steps_never_increase_the_cost(name):
    Np, L, r, nside, step, B, seed, d1, d2, path, _, kernels, plan, env, _ = TAILS[name]
    prob, stack = _case(Np, L, r, nside, step, B, seed, d1, d2, path)
    with _solver(prob, stack, 1, kernels, plan, **env) as s:
        s.set_gains(_gains(prob, seed))

        def cost():
            E, Q = s.residual()["err"], s.moments()["model"]
            return E.sum(), residual_check.bound(E, Q).sum()

        f = [cost()]
        for do in (descent.object_step, descent.object_step, descent.pupil_step):
            do(s)
            f.append(cost())
    print(f"majorised steps {name}: " + " -> ".join(f"{v:.6g}" for v, _ in f) + f"; slack {f[0][1]:.3g}")
    for (a, slack), (b, _) in zip(f, f[1:]):
        assert b <= a + slack, f
    assert f[1][0] < f[0][0] - f[0][1], f


# ---- 6. autograd -----------------------------------------------------------------------------
def test_autograd_cost_function():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    d = _tail_run("general_np32_wave")
    prob, stack, seed, _, ctx = _open("general_np32_wave")
    with ctx as s:
        s.set_gains(d["g"])
        zO = torch.tensor(d["state"]["objF"], device="cuda", requires_grad=True)
        zP = torch.tensor(d["state"]["pupil"], device="cuda", requires_grad=True)
        f = descent.CostFunction.apply(zO, zP, s)
        assert f.dtype == torch.float64 and f.is_cuda
        assert float(f.detach()) == s.residual()["err"].sum()
        f.backward()
        want = s.gradient()
        assert zO.grad.cpu().numpy().tobytes() == want["objF"].tobytes()
        assert zP.grad.cpu().numpy().tobytes() == want["pupil"].tobytes()
    _same(want, d["got"], "the installed state is the downloaded one")


# ---- 7. errors -------------------------------------------------------------------------------
def test_errors_leave_the_context_unchanged():
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    lib = fpm_amd.load_library()
    n, B, Np, L = len(prob.order), prob.n_patch, prob.np_, prob.L
    gO = np.empty((B, L, L), np.complex64)
    pO = gO.ctypes.data_as(C.c_void_p)

    def msg():
        return lib.fpm_last_error().decode()

    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:  # before a state exists
            s.gradient()
        assert ei.value.code == fpm_amd.FPM_ERR_STATE and "fpm_gradient" in str(ei.value)
        s.init()
        s.run(1)
        state, bytes0 = s.download(), None
        want = s.gradient(sums=True)
        bytes0 = s.info().device_bytes
        assert lib.fpm_gradient(s._h, None, 0, 0, None, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
        assert "both NULL" in msg()
        assert lib.fpm_gradient(s._h, None, 0, 2, pO, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
        assert "unknown flag bits 0x2" in msg()
        for pos, dx, what in (([0, n], [0, 0], "entry 1: pos="), ([0, 1, 2], [0, 0, 4096], "entry 2: window"),
                              ([-1], [0], "entry 0: pos=")):
            with pytest.raises(fpm_amd.FpmError) as ei:
                s.gradient(pos=pos, dx=dx)
            assert ei.value.code == fpm_amd.FPM_ERR_INVAL and what in str(ei.value) and "fpm_gradient" in str(ei.value)
        probes = (fpm_amd.fpm_probe * 1)()
        assert lib.fpm_gradient(s._h, probes, 0, 0, pO, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
        assert "n < 1" in msg()
        # a capturing stream: refused before anything is enqueued
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(fpm_amd.FpmError) as ei:
            with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                s.gradient()
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        s.set_stream(None)
        # nothing moved
        after = s.download()
        for f in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(after[f], state[f], err_msg=f)
        assert s.info().device_bytes == bytes0
        ms = C.c_double(-1.0)
        assert lib.fpm_gradient(s._h, None, -5, 0, pO, None, None, None, C.byref(ms)) == fpm_amd.FPM_OK  # n is ignored
        assert ms.value >= 0 and gO.tobytes() == want["objF"].tobytes()
        again = s.gradient(sums=True)
        _same(again, want, "after the refusals")
        np.testing.assert_array_equal(again["err"], want["err"])
    with fpm_amd.Solver(prob) as s:  # a state, no stack
        s.set_state(state["objF"], state["pupil"])
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.gradient()
        assert ei.value.code == fpm_amd.FPM_ERR_STATE and "no stack uploaded" in str(ei.value)


def test_device_bytes_count_the_scratch():
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    n, B, Np, L, nb = len(prob.order), prob.n_patch, prob.np_, prob.L, 2 * prob.radius + 1
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        s.residual()  # the sweep's own scratch
        b0 = s.info().device_bytes
        dO = torch.zeros((B, L, L, 2), dtype=torch.float32, device="cuda")
        s.gradient(device_ptrs=(dO.data_ptr(), None))
        b1 = s.info().device_bytes
        assert b1 == b0 + n * B * nb * nb * 8  # R of one launch (nl = n_order here); a device output needs no copy
        s.gradient(pupil=False)
        assert s.info().device_bytes == b1 + B * L * L * 8
        s.gradient()
        assert s.info().device_bytes == b1 + B * L * L * 8 + B * Np * Np * 8
        s.gradient()
        assert s.info().device_bytes == b1 + B * L * L * 8 + B * Np * Np * 8
