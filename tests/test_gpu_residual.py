"""fpm_residual (ABI 6): the per-LED data-fidelity residual of the current
state, E[i][b] = sum (|psi| - sqrt(I))^2 and S[i][b] = sum I, computed on the
GPU by a read-only sweep (csrc/residual.hip).

The yardstick is a float64 numpy evaluation of the DOWNLOADED state with the
conventions of tools/synth.forward_intensities: O = fftshift(objF[b]),
P = ifftshift(pupil[b]), psi = ifft2(ifftshift(O[y0:y0+Np, x0:x0+Np]) P),
E_ref = sum (|psi| - sqrt(I))^2, Q = sum |psi|^2.  Both sides read the same
fp32 (or dequantised fp16) state and differ by the GPU's fp32 transform
rounding only.  With ||psi_gpu - psi_ref|| <= eps ||psi_ref|| the reverse
triangle inequality and Cauchy-Schwarz give
    |E_gpu - E_ref| <= 2 eps sqrt(E_ref Q) + eps^2 Q,
and eps = 1e-5 is the project's one-iteration relative-L2 bound of an fp32
transform chain, so every parity test asserts
    |E_gpu - E_ref| <= 2e-5 sqrt(E_ref Q) + 1e-10 Q   per (LED, patch)
and ref == I.sum() exactly.  At least one iteration runs before every
comparison: straight after fpm_init some LEDs' windows miss the support and
E = S whatever the indexing.

Each parity test asserts the kernel (info().fused_kernel) and, through the
test-only fpm_debug_get_plan, the stack's device layout meas_g, the general
path's kind and the residual's kernel pair it means to exercise.  The
measured |dE| / bound maxima are printed (pytest -s) and copied into
DESIGN.md section 4.6.
"""
import contextlib
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import residual_check
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")
GENERAL, FUSED = fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED
NP256_KERNELS = (fpm_amd.KERNEL_FUSED_NP256, fpm_amd.KERNEL_FUSED_NP256_DIST)
G_LDS, G_REG1024, G_REG256 = fpm_amd.GENERAL_LDS, fpm_amd.GENERAL_REG1024, fpm_amd.GENERAL_REG256
R_LDS, R_REG = fpm_amd.RESIDUAL_LDS, fpm_amd.RESIDUAL_REG256


def _plan(meas_g, general_kind=-1, residual_kind=R_LDS):
    """What fpm_debug_get_plan must report (general_kind -1: a fused context)."""
    return dict(meas_g=meas_g, general_kind=general_kind, residual_kind=residual_kind)


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
def _stack(Np, L, r, x0, y0, B, seed):
    st = make_stack(Np, L, r, np.array(x0), np.array(y0), n_patch=B, seed=seed)
    st.setflags(write=False)
    return st


def _case(Np, L, r, nside, step, B, seed, d1=5, d2=10, path=fpm_amd.PATH_AUTO, flags=0, geom=None):
    """(Problem, stack) of a synthetic LED grid (or of geom = (x0, y0, order))."""
    x0, y0, order = geom if geom else grid_geometry(Np, L, nside, step)
    stack = _stack(Np, L, r, tuple(int(v) for v in x0), tuple(int(v) for v in y0), B, seed)
    return fpm_amd.Problem(Np, L, order, x0, y0, r, d1, d2, n_patch=B, path=path, flags=flags), stack


@contextlib.contextmanager
def _solver(prob, stack, iters, kernels, plan=None, **env):
    with _env(**env):
        s = fpm_amd.Solver(prob)
    try:
        assert s.info().fused_kernel in kernels, s.info().fused_kernel
        if plan is not None:
            assert s.debug_plan() == plan
        s.upload(stack)
        s.init()
        s.run(iters)
        yield s
    finally:
        s.close()


# the float64 yardstick, its bound and the comparison: shared with tests/test_gpu_ladder.py
_reference, _bound, _check = residual_check.reference, residual_check.bound, residual_check.check


def _parity(tag, prob, stack, iters, kernels, plan, **env):
    with _solver(prob, stack, iters, kernels, plan, **env) as s:
        state = s.download(objCrop=False, support=False)
        d = s.residual()
    ref = _reference(state, stack, prob)
    _check(tag, d, ref)
    return d, ref


# ---- layout g = 0, the LDS pair ---------------------------------------------------
LDS_CASES = [  # Np, L, r, nside, step, B, seed, delta1, delta2
    (32, 96, 6, 5, 4, 3, 7, 5, 10),        # 25 LEDs, B not a multiple of 8
    (30, 90, 5, 5, 4, 2, 11, 5, 10),       # radix 2 x 3 x 5
    (40, 120, 7, 3, 6, 2, 13, 1000, 70),   # radix 8 x 5, large regularisers
]


# the LDS pair's column kernel: wave-private columns (Np <= 512) or, with FPM_NO_WAVE_COLS=1, the tiled one
COLS = {"wave": {}, "tiled": {"FPM_NO_WAVE_COLS": "1"}}


@pytest.mark.parametrize("cols", list(COLS))
@pytest.mark.parametrize("Np,L,r,nside,step,B,seed,d1,d2", LDS_CASES, ids=[f"np{c[0]}" for c in LDS_CASES])
def test_general_path_c_abi_layout(Np, L, r, nside, step, B, seed, d1, d2, cols):
    prob, stack = _case(Np, L, r, nside, step, B, seed, d1, d2, path=GENERAL)
    _parity(f"general Np {Np} g=0 {cols}", prob, stack, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS), **COLS[cols])


@pytest.mark.parametrize("which", ["general_np30", "fused_small_np8", "fused_np90"])
def test_one_sequence_per_block_kernels_small(which):
    """FPM_RES_ONE_SEQ=1 runs the fallback pair of sizes whose tiles do not
    fit (one row / one column per block) at sizes a test can afford, in the
    C-ABI, the transposed and the g = 9 layout."""
    if which == "general_np30":
        prob, stack = _case(30, 90, 5, 5, 4, 2, 11, path=GENERAL)
        kern, plan = fpm_amd.KERNEL_GENERAL, _plan(0, G_LDS)
    elif which == "fused_small_np8":
        prob, stack = _case(8, 24, 1, 2, 3, 2, 71 + 8 + 1, path=FUSED)
        kern, plan = fpm_amd.KERNEL_FUSED_SMALL, _plan(8)
    else:
        prob, stack = _case(90, 180, 3, 2, 10, 2, 91 + 3, path=FUSED)
        kern, plan = fpm_amd.KERNEL_FUSED_NP90, _plan(9)
    _parity(f"one-sequence {which}", prob, stack, 1, (kern,), plan, FPM_RES_ONE_SEQ="1")


def test_one_sequence_rows_np2700():
    """Np 2700: two box rows do not fit a 256-thread tile, so the row IDFTs run
    one row per block (k_gather_rowifft<ResArgs>) and the columns two per 512-thread block
    (k_colpass_tiled<512, 16, ResArgs>; no wave holds a column of this length);
    the two LEDs of test_one_sequence_row_kernels_match_oracle."""
    geom = (np.array([150, 50]), np.array([150, 150]), [0, 1])
    prob, stack = _case(2700, 3000, 4, 0, 0, 1, 20261015, path=GENERAL, geom=geom)
    _parity("general Np 2700", prob, stack, 1, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS))


# ---- transposed layout (g = Np) ---------------------------------------------------
@pytest.mark.parametrize("cols", list(COLS))
def test_small_fused_kernel_transposed_layout(cols):
    prob, stack = _case(8, 24, 1, 2, 3, 2, 71 + 8 + 1, path=FUSED)  # the smallest of test_gpu_fused_small.py
    _parity(f"fused small Np 8 g=Np {cols}", prob, stack, 1, (fpm_amd.KERNEL_FUSED_SMALL,), _plan(8), **COLS[cols])


# The smallest geometries above (the ones the fused kernels' own tests start
# from) leave 6 of 8 windows off the support for good (Q = 0, E = S whatever
# the indexing).  The same three layouts again with LEDs closer than 2 r, so
# that every window carries signal and the layout and LED order are checked
# on every (LED, patch).
OVERLAP_CASES = [  # Np, L, r, nside, step, seed, d1, d2, kernel, g
    (30, 90, 6, 5, 9, 71 + 30 + 6, 5, 10, fpm_amd.KERNEL_FUSED_SMALL, 30),
    (90, 360, 30, 4, 22, 91 + 30, 5, 10, fpm_amd.KERNEL_FUSED_NP90, 9),
    (200, 600, 26, 3, 30, 61 + 26, 10, 3, fpm_amd.KERNEL_FUSED_NP200, 10),
]


@pytest.mark.parametrize("cols", list(COLS))
@pytest.mark.parametrize("Np,L,r,nside,step,seed,d1,d2,kernel,g", OVERLAP_CASES,
                         ids=[f"np{c[0]}_g{c[-1]}" for c in OVERLAP_CASES])
def test_fused_layouts_with_overlapping_leds(Np, L, r, nside, step, seed, d1, d2, kernel, g, cols):
    prob, stack = _case(Np, L, r, nside, step, 2, seed, d1, d2, path=FUSED)
    _, (E, Q, _) = _parity(f"fused Np {Np} g={g} overlapping {cols}", prob, stack, 2, (kernel,), _plan(g), **COLS[cols])
    assert np.all(Q > 0)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("reg", [True, False], ids=["reg1024", "no_reg1024"])
def test_np1024_l4096(reg, fp16):
    """Np 1024 / L 4096 / r 333, the LED grid of test_gpu_np1024.py's L 4096
    cases (2 x 2 at step 600: that file's grid has 4 LEDs), fp32 and fp16
    spectrum storage (spec_ld); the columns run tiled, 8 per block: the
    register general path reads the stack transposed (g = Np); with
    FPM_NO_REG1024=1 the stack stays in the C-ABI layout (g = 0) at a size
    where a wave cannot hold two columns."""
    flags = fpm_amd.FLAG_SPEC_FP16 if fp16 else 0
    prob, stack = _case(1024, 4096, 333, 2, 600, 1, 95, flags=flags)
    env = {} if reg else {"FPM_NO_REG1024": "1"}
    plan = _plan(1024, G_REG1024) if reg else _plan(0, G_LDS)
    _parity(f"general Np 1024 {'g=Np' if reg else 'g=0'} {'fp16' if fp16 else 'fp32'}", prob, stack, 1,
            (fpm_amd.KERNEL_GENERAL,), plan, **env)


# ---- g = 9 / g = 10 ---------------------------------------------------------------
@pytest.mark.parametrize("cols", list(COLS))
def test_np90_fused_layout_g9(cols):
    prob, stack = _case(90, 180, 3, 2, 10, 2, 91 + 3, path=FUSED)  # the smallest of test_gpu_fused_s90.py
    _parity(f"fused Np 90 g=9 {cols}", prob, stack, 3, (fpm_amd.KERNEL_FUSED_NP90,), _plan(9), **COLS[cols])


@pytest.mark.parametrize("cols", list(COLS))
def test_np200_fused_layout_g10(cols):
    prob, stack = _case(200, 600, 1, 2, 3, 2, 61 + 1, 10, 3, path=FUSED)  # the smallest of test_gpu_fused_mr.py
    _parity(f"fused Np 200 g=10 {cols}", prob, stack, 1, (fpm_amd.KERNEL_FUSED_NP200,), _plan(10), **COLS[cols])


# ---- g = 16, the register pair and its LDS cross-check ----------------------------
REG_CASES = [  # L, r, nside, step, path, kernels
    (512, 31, 3, 40, FUSED, NP256_KERNELS),     # NB 63
    (512, 33, 5, 20, FUSED, NP256_KERNELS),     # NB 67, 25 LEDs
    (512, 34, 3, 30, FUSED, NP256_KERNELS),     # NB 69
    (1024, 84, 3, 100, GENERAL, (fpm_amd.KERNEL_GENERAL,)),  # Reg256 general path
]


@pytest.mark.parametrize("L,r,nside,step,path,kernels", REG_CASES, ids=[f"L{c[0]}_r{c[1]}" for c in REG_CASES])
def test_np256_register_pair_and_lds_pair(L, r, nside, step, path, kernels):
    prob, stack = _case(256, L, r, nside, step, 2, 40 + r, 10, 3, path=path)
    kind = G_REG256 if path == GENERAL else -1
    reg, ref = _parity(f"Np 256 r {r} register pair", prob, stack, 2, kernels, _plan(16, kind, R_REG))
    E, Q, _ = ref
    bound = _bound(E, Q)
    assert np.all(bound > 0)
    for cols, env in COLS.items():
        lds, _ = _parity(f"Np 256 r {r} LDS pair {cols}", prob, stack, 2, kernels, _plan(16, kind, R_LDS),
                         FPM_RES_LDS="1", **env)
        gap = np.abs(reg["err"] - lds["err"])
        print(f"residual Np 256 r {r}: register vs LDS pair {cols} max |dE|/bound {(gap / bound).max():.3e}")
        assert np.all(gap <= 2.0 * bound)
        np.testing.assert_array_equal(reg["ref"], lds["ref"])


# ---- batching and determinism -----------------------------------------------------
def test_batching_is_bit_identical():
    """25 LEDs: FPM_RES_BATCH=4 (seven launches, the last with one LED) and
    FPM_RES_BATCH=1 return the default's bits; so do two consecutive calls."""
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    got = {}
    for batch in (None, "4", "1"):
        env = {"FPM_RES_BATCH": batch} if batch else {}
        with _solver(prob, stack, 2, (fpm_amd.KERNEL_GENERAL,), **env) as s:
            got[batch] = s.residual()
            again = s.residual()
        for k in ("err", "ref"):
            np.testing.assert_array_equal(again[k], got[batch][k])
            np.testing.assert_array_equal(got[batch][k], got[None][k])


# ---- read-only --------------------------------------------------------------------
def _context(which):
    if which == "general_np32":
        return "general Np 32", _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL), (fpm_amd.KERNEL_GENERAL,)
    return "fused Np 256 r 33", _case(256, 512, 33, 5, 20, 2, 40 + 33, 10, 3, path=FUSED), NP256_KERNELS


@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_residual_is_read_only(which):
    tag, (prob, stack), kernels = _context(which)
    with _solver(prob, stack, 1, kernels) as s:
        before, stack_before = s.download(), s.download_stack()
        t0, k0 = s.timing(), s.clock()
        s.residual()
        after = s.download()
        for k in ("objF", "objCrop", "pupil"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=f"{tag} {k}")
        np.testing.assert_array_equal(s.download_stack(), stack_before)
        np.testing.assert_array_equal(stack_before, stack)
        t1, k1 = s.timing(), s.clock()
        for f, _ in fpm_amd.fpm_timing._fields_:
            assert getattr(t0, f) == getattr(t1, f), f
        for f, _ in fpm_amd.fpm_clock._fields_:
            assert getattr(k0, f) == getattr(k1, f), f
        assert t1.led_launches > 0
        s.run(1)
        with_sweep = s.download()
    with _solver(prob, stack, 1, kernels) as s:
        s.run(1)
        without = s.download()
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(with_sweep[k], without[k], err_msg=f"{tag} {k}")


@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_split_iterations_equal_one_run(which):
    """fpmMain --residual runs fpm_run(ctx, 1) per iteration: three single
    iterations end bit for bit where fpm_run(ctx, 3) does."""
    tag, (prob, stack), kernels = _context(which)
    with _solver(prob, stack, 3, kernels) as s:
        whole = s.download()
    with _solver(prob, stack, 1, kernels) as s:
        s.run(1)
        s.run(1)
        split = s.download()
    for k in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(split[k], whole[k], err_msg=f"{tag} {k}")


def test_device_bytes_count_the_scratch():
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        b0 = s.info().device_bytes
        s.residual()
        b1 = s.info().device_bytes
        s.residual()
        assert b1 > b0 and s.info().device_bytes == b1


# ---- errors -----------------------------------------------------------------------
def test_errors():
    import ctypes as C
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.residual()
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        s.init()
        lib = fpm_amd.load_library()
        assert lib.fpm_residual(s._h, None, None, None) == fpm_amd.FPM_ERR_INVAL
        ms = C.c_double(-1.0)
        err = np.empty((len(prob.order), prob.n_patch))
        dp = C.POINTER(C.c_double)
        assert lib.fpm_residual(s._h, err.ctypes.data_as(dp), None, C.byref(ms)) == fpm_amd.FPM_OK  # ref may be NULL
        assert ms.value >= 0 and np.all(err >= 0)


def test_residual_on_a_capturing_stream_is_refused():
    """As fpm_run (test_run_on_a_capturing_stream_is_refused): blocking, so
    FPM_ERR_INVAL before anything is enqueued; the capture stays valid and the
    context works afterwards."""
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        want = s.residual()
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(fpm_amd.FpmError) as ei:
            with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                s.residual()
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        got = s.residual()  # on the caller's stream, no longer capturing
        np.testing.assert_array_equal(got["err"], want["err"])
        s.set_stream(None)
        np.testing.assert_array_equal(s.residual()["err"], want["err"])


# ---- CLI --------------------------------------------------------------------------
def test_cli_residual_flag(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    outs = {}
    for tag, extra in (("with", ["--residual"]), ("without", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], "2", "--out", str(out)] + extra, capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = out
    meta = json.loads((outs["with"] / "result.json").read_text())
    res = meta["residual"]
    assert set(res) == {"per_iteration", "per_patch_last", "per_led_last", "sweep_ms"}
    assert len(res["per_iteration"]) == 3 and all(np.isfinite(v) and v > 0 for v in res["per_iteration"])
    assert len(res["per_led_last"]) == meta["leds_used"] and len(res["per_patch_last"]) == 1
    assert all(np.isfinite(v) and v >= 0 for v in res["per_led_last"]) and res["sweep_ms"] > 0
    assert res["per_patch_last"][0] == pytest.approx(res["per_iteration"][-1], rel=1e-12)
    plain = json.loads((outs["without"] / "result.json").read_text())
    assert "residual" not in plain
    assert set(meta) - {"residual"} == set(plain)
    for f in ("objCrop.npy", "objF.npy", "pupil.npy"):
        assert (outs["with"] / f).read_bytes() == (outs["without"] / f).read_bytes(), f
