"""fpm_predict: the forward model's per-LED images of the current state,
psi = ifft2(window * P), stored per pixel by a fourth tail of the residual
sweep's column kernels (csrc/residual_dev.hpp: PredArgs) as float32 |psi|
(AMPLITUDE), uint16 rint((|psi| / g)^2) saturated at 65535 (COUNTS) or float32
|psi| - g sqrt(I) (DIFF).

The yardstick, the bounds and their derivation are tests/predict_check.py's: a
float64 numpy evaluation of the DOWNLOADED state, so both sides read the same
fp32 state and differ by the GPU's fp32 transform only.  At least one
iteration runs before a parity comparison, so the pupil is not flat.  The
measured ratios to the bounds are printed (pytest -s).
"""
import contextlib
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import ladder_cases
import predict_check as pc
import residual_check
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")
GENERAL, FUSED = fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED
NP256_KERNELS = (fpm_amd.KERNEL_FUSED_NP256, fpm_amd.KERNEL_FUSED_NP256_DIST)
G_LDS = fpm_amd.GENERAL_LDS
R_LDS, R_REG = fpm_amd.RESIDUAL_LDS, fpm_amd.RESIDUAL_REG256
KINDS = ("amplitude", "counts", "diff")


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


def _gains(prob, seed):
    """A gain table that is nowhere 1: float32 [n_stack][B] in [0.6, 1.7]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.6, 1.7, (len(prob.x0), prob.n_patch)).astype(np.float32)


def _rows(prob, a, pos=None):
    """Rows of a [n_stack][B]... table or stack by entry: row k = order[pos[k]]."""
    order = np.asarray(prob.order)
    return a[order if pos is None else order[np.asarray(pos)]]


# ---- 1. every tail, every stack layout, all three kinds -------------------------------
def _plan(meas_g, general_kind=-1, residual_kind=R_LDS):
    return dict(meas_g=meas_g, general_kind=general_kind, residual_kind=residual_kind)


TAILS = {  # name: (Np, L, r, nside, step, B, seed, d1, d2, path, iters, kernels, plan, env, sweep column rung)
    "general_np32_wave": (32, 96, 6, 5, 4, 3, 7, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS), {},
                          "wave<4,4>"),
    "general_np32_tiled": (32, 96, 6, 5, 4, 3, 7, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                           {"FPM_NO_WAVE_COLS": "1"}, "tiled<256,16> lc 4"),
    "general_np30_one_seq": (30, 90, 5, 5, 4, 2, 11, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,), _plan(0, G_LDS),
                             {"FPM_RES_ONE_SEQ": "1"}, "one_seq"),
    "fused_small_np8_gNp": (8, 24, 1, 2, 3, 2, 71 + 8 + 1, 5, 10, FUSED, 1, (fpm_amd.KERNEL_FUSED_SMALL,), _plan(8),
                            {}, None),
    "fused_np90_g9": (90, 180, 3, 2, 10, 2, 91 + 3, 5, 10, FUSED, 2, (fpm_amd.KERNEL_FUSED_NP90,), _plan(9), {}, None),
    "fused_np200_g10": (200, 600, 1, 2, 3, 2, 61 + 1, 10, 3, FUSED, 1, (fpm_amd.KERNEL_FUSED_NP200,), _plan(10), {},
                        None),
    "fused_np256_r31_reg": (256, 512, 31, 3, 40, 2, 40 + 31, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_REG), {},
                            None),
    "fused_np256_r33_reg": (256, 512, 33, 3, 20, 3, 40 + 33, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_REG), {},
                            None),
    "fused_np256_r33_lds": (256, 512, 33, 3, 20, 2, 40 + 33, 10, 3, FUSED, 2, NP256_KERNELS, _plan(16, -1, R_LDS),
                            {"FPM_RES_LDS": "1"}, None),
    # the ladder's Np 40 geometry (40 = 16 * 2 + 8: the last column tile holds 8 of 16 columns) at B = 2
    "ladder_np40_partial_tile": (40, 120, 19, 3, 19, 2, 7040, 5, 10, GENERAL, 2, (fpm_amd.KERNEL_GENERAL,),
                                 _plan(0, G_LDS), {"FPM_NO_WAVE_COLS": "1"}, "tiled<256,16> lc 4"),
    # the ladder's Np 360 geometry: tiled columns on 512 threads (360 = 16 * 22 + 8)
    "ladder_np360_512_threads": (360, 720, 40, 3, 40, 2, 7360, 5, 10, GENERAL, 1, (fpm_amd.KERNEL_GENERAL,),
                                 _plan(0, G_LDS), {"FPM_NO_WAVE_COLS": "1"}, "tiled<512,16> lc 4"),
}


@functools.lru_cache(maxsize=None)
def _tail_run(name):
    """One context per case: the downloaded state, the gains, the three kinds
    (B = 2 or 3 patches), fpm_residual's E of the same state and gains, and the
    float64 reference.  Shared by the tests that compare against it; read-only."""
    Np, L, r, nside, step, B, seed, d1, d2, path, iters, kernels, plan, env, rung = TAILS[name]
    prob, stack = _case(Np, L, r, nside, step, B, seed, d1, d2, path)
    with _solver(prob, stack, iters, kernels, plan, **env) as s:
        if rung is not None:
            assert ladder_cases.rung_name(s.debug_ladder(True)["cols"], "lc") == rung
        state = _state(s)
        unit = {k: s.predict(k) for k in ("amplitude", "counts")}
        g = _gains(prob, seed)
        s.set_gains(g)
        got = {k: s.predict(k) for k in KINDS}
        err = s.residual()["err"]
    a_ref = pc.amplitudes(state, prob)
    for v in list(got.values()) + list(unit.values()) + [a_ref]:
        v.setflags(write=False)
    return dict(prob=prob, stack=stack, state=state, g=g, got=got, unit=unit, err=err, a_ref=a_ref)


@pytest.mark.parametrize("name", list(TAILS))
def test_every_tail_layout_and_kind(name):
    d = _tail_run(name)
    prob, a_ref = d["prob"], d["a_ref"]
    g, I = _rows(prob, d["g"]), _rows(prob, d["stack"])
    pc.check_amplitude(name, d["got"]["amplitude"], a_ref)
    np.testing.assert_array_equal(d["got"]["amplitude"], d["unit"]["amplitude"])  # raw: the gains do not enter
    pc.check_counts(name, d["got"]["counts"], a_ref, g)
    pc.check_counts(name + " g=1", d["unit"]["counts"], a_ref, np.ones_like(g))
    E, Q = pc.residual_sums(a_ref, I, g)
    pc.check_diff(name, d["got"]["diff"], a_ref, I, g, err=d["err"], E=E, Q=Q)


# ---- 2. exact cases -------------------------------------------------------------------
def _delta_state(prob, led, k, second=None):
    """Pupil 1 at the centre pixel, spectrum k Np^2 at the centre of `led`'s
    window (second: (dy, dx, value) one more spectrum pixel relative to it)."""
    Np, L, B = prob.np_, prob.L, prob.n_patch
    pupil = np.zeros((B, Np, Np), np.complex64)
    pupil[:, Np // 2, Np // 2] = 1
    objF = np.zeros((B, L, L), np.complex64)
    yc, xc = int(prob.y0[led]) + Np // 2, int(prob.x0[led]) + Np // 2
    objF[:, (yc - L // 2) % L, (xc - L // 2) % L] = k * Np * Np
    if second:
        dy, dx, v = second
        objF[:, (yc + dy - L // 2) % L, (xc + dx - L // 2) % L] = v * Np * Np
        pupil[:, Np // 2 + dy, Np // 2 + dx] = 1
    return objF, pupil


@pytest.mark.parametrize("Np,L,r", [(32, 96, 6), (256, 512, 33)], ids=["np32", "np256"])
def test_exact_scaling_saturation_and_gain(Np, L, r):
    """A one-pixel pupil and a one-pixel spectrum: psi is the constant k on one
    LED, exactly, and 0 on every other."""
    x0, y0, order = grid_geometry(Np, L, 3, 4)
    prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=2)
    pos = 4
    led = int(order[pos])
    others = [i for i in range(len(order)) if i != pos]
    with _solver(prob, None, 0) as s:
        for k, want in ((1, 1), (255, 65025), (256, 65535), (300, 65535)):
            s.set_gains(None)
            s.set_state(*_delta_state(prob, led, k))
            a, c = s.predict("amplitude"), s.predict("counts")
            assert np.all(a[pos] == np.float32(k)) and not np.any(a[others])
            assert np.all(c[pos] == want) and not np.any(c[others])
            g = np.ones((len(x0), 2), np.float32)
            g[led] = 2
            s.set_gains(g)
            a2, c2 = s.predict("amplitude"), s.predict("counts")
            np.testing.assert_array_equal(a2, a)
            assert np.all(c2[pos] == int(np.rint(k * k / 4))) and not np.any(c2[others])
        # a second pixel: |psi| = |3 + 2 exp(2 pi i (y + 2 x) / Np)|, which a transposed output would not match
        s.set_gains(None)
        s.set_state(*_delta_state(prob, led, 3, second=(1, 2, 2)))
        a = s.predict("amplitude")
        a_ref = pc.amplitudes(_state(s), prob)
        y, x = np.mgrid[0:Np, 0:Np]
        np.testing.assert_allclose(a_ref[pos, 0], np.abs(3 + 2 * np.exp(2j * np.pi * (y + 2 * x) / Np)), atol=1e-9)
        assert pc._norm(a_ref[pos, 0] - a_ref[pos, 0].T) > 1.0  # transposition-sensitive
        pc.check_amplitude(f"two pixels Np {Np}", a, a_ref)


# ---- 3. closed loop, no oracle --------------------------------------------------------
@pytest.mark.parametrize("which", ["general_np32", "fused_np256"])
def test_closed_loop(which):
    """Predict a stack from a state, upload it, install the state: the residual
    is of quantisation size and S is the sum of the counts."""
    if which == "general_np32":
        prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL, peak=20000.0)
    else:
        prob, stack = _case(256, 512, 33, 3, 20, 2, 40 + 33, 10, 3, path=FUSED, peak=20000.0)
    Np = prob.np_
    with _solver(prob, stack, 2) as s:
        X = _state(s)
        counts = s.predict("counts")
    a_ref = pc.amplitudes(X, prob)
    assert (a_ref ** 2).max() < 65535  # on the float64 reference: nothing saturates
    pred = fpm_amd.scatter_to_stack(prob, counts)
    with _solver(prob, None, 0) as s:
        s.upload(pred)
        s.set_state(X["objF"], X["pupil"])
        d = s.residual()
    I = _rows(prob, pred)
    E, Q = pc.residual_sums(a_ref, I, np.ones(I.shape[:2]))
    lim = Np * Np / 2 + residual_check.bound(E, Q)
    print(f"closed loop {which}: max E / (Np^2/2 + bound) {(d['err'] / lim).max():.3e}, max E {d['err'].max():.4g}")
    assert np.all(d["err"] <= lim)
    np.testing.assert_array_equal(d["ref"], I.astype(np.int64).sum(axis=(-2, -1)))
    sim = fpm_amd.simulate(prob, X["objF"], X["pupil"])
    assert sim.dtype == np.uint16 and sim.tobytes() == pred.tobytes()


# ---- 4. no stack ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general_np32_wave", "fused_np256_r33_reg"])
def test_without_a_stack(name):
    d = _tail_run(name)
    prob = d["prob"]
    with _solver(prob, None, 0) as s:
        s.set_state(d["state"]["objF"], d["state"]["pupil"])
        for k in ("amplitude", "counts"):
            np.testing.assert_array_equal(s.predict(k), d["unit"][k])
        s.set_gains(d["g"])
        np.testing.assert_array_equal(s.predict("counts"), d["got"]["counts"])
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.predict("diff")
        assert ei.value.code == fpm_amd.FPM_ERR_STATE and "no stack uploaded" in str(ei.value)


# ---- 5. determinism and independence --------------------------------------------------
def test_batching_lists_and_outputs_are_bit_identical():
    """25 LEDs: FPM_RES_BATCH=4 (seven launches, the last with one entry), =1
    and the default; two calls; host and device output; probe lists."""
    import torch
    d = _tail_run("general_np32_wave")
    prob, stack, want = d["prob"], d["stack"], d["got"]
    n, B, Np = len(prob.order), prob.n_patch, prob.np_
    rng = np.random.default_rng(5)
    for batch in (None, "4", "1"):
        env = {"FPM_RES_BATCH": batch} if batch else {}
        with _solver(prob, stack, 2, **env) as s:
            s.set_gains(d["g"])
            for k in KINDS:
                got = s.predict(k)
                np.testing.assert_array_equal(got, want[k], err_msg=f"batch {batch} {k}")
                np.testing.assert_array_equal(s.predict(k), got)
                dev = torch.zeros(got.shape, dtype=torch.int16 if k == "counts" else torch.float32, device="cuda")
                assert s.predict(k, device_ptr=dev.data_ptr()) is None
                torch.cuda.synchronize()
                assert dev.cpu().numpy().tobytes() == got.tobytes(), f"batch {batch} {k} device"
                # (pos, 0, 0) in shuffled order; a list longer than n_order
                perm = rng.permutation(n)
                np.testing.assert_array_equal(s.predict(k, pos=perm), got[perm])
                long = np.concatenate([perm, np.arange(n), perm[:1]])
                assert len(long) == 2 * n + 1
                np.testing.assert_array_equal(s.predict(k, pos=long), got[long])
                dev = torch.zeros((len(long), B, Np, Np), dtype=dev.dtype, device="cuda")
                s.predict(k, pos=long, device_ptr=dev.data_ptr())
                torch.cuda.synchronize()
                assert dev.cpu().numpy().tobytes() == got[long].tobytes()
            if batch is None:  # moved windows against the reference with those windows
                pos, dx, dy = [0, 3, 24, 7], [1, -2, 0, 3], [0, 2, -3, -1]
                a = s.predict("amplitude", pos=pos, dx=dx, dy=dy)
                a_ref = pc.amplitudes(d["state"], prob, pos, dx, dy)
                pc.check_amplitude("moved windows", a, a_ref)
                assert not np.array_equal(a, want["amplitude"][pos])
                mixed = s.predict("amplitude", pos=pos + [3], dx=dx + [0], dy=dy + [0])
                np.testing.assert_array_equal(mixed[:4], a)  # an entry does not depend on its neighbours
                np.testing.assert_array_equal(mixed[4], want["amplitude"][3])


# ---- 6. read-only ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["general_np32", "fused_np256_r33"])
def test_predict_is_read_only(which):
    if which == "general_np32":
        (prob, stack), kernels = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL), (fpm_amd.KERNEL_GENERAL,)
    else:
        (prob, stack), kernels = _case(256, 512, 33, 5, 20, 2, 40 + 33, 10, 3, path=FUSED), NP256_KERNELS
    g = _gains(prob, 3)
    with _solver(prob, stack, 1, kernels) as s:
        s.set_gains(g)
        before, stack_before, crops_before = s.download(), s.download_stack(), s.crops()
        t0, k0 = s.timing(), s.clock()
        for k in KINDS:
            s.predict(k)
            after = s.download()
            for f in ("objF", "objCrop", "pupil"):
                np.testing.assert_array_equal(after[f], before[f], err_msg=f"{which} {k} {f}")
            np.testing.assert_array_equal(s.download_stack(), stack_before)
            np.testing.assert_array_equal(s.gains(), g)
            for u, v in zip(s.crops(), crops_before):
                np.testing.assert_array_equal(u, v)
            t1, k1 = s.timing(), s.clock()
            for f, _ in fpm_amd.fpm_timing._fields_:
                assert getattr(t0, f) == getattr(t1, f), f
            for f, _ in fpm_amd.fpm_clock._fields_:
                assert getattr(k0, f) == getattr(k1, f), f
        np.testing.assert_array_equal(stack_before, stack)
        s.run(1)
        with_calls = s.download()
    with _solver(prob, stack, 1, kernels) as s:
        s.set_gains(g)
        s.run(1)
        without = s.download()
    for f in ("objF", "objCrop", "pupil"):
        np.testing.assert_array_equal(with_calls[f], without[f], err_msg=f"{which} {f}")


# ---- 7. errors and bookkeeping --------------------------------------------------------
def test_errors():
    import ctypes as C
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    lib = fpm_amd.load_library()
    n, B, Np = len(prob.order), prob.n_patch, prob.np_
    out = np.empty((n, B, Np, Np), np.float32)
    dst = out.ctypes.data_as(C.c_void_p)

    def msg():
        return lib.fpm_last_error().decode()

    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:  # before a state exists
            s.predict("amplitude")
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        s.init()
        assert lib.fpm_predict(s._h, None, 0, fpm_amd.PREDICT_AMPLITUDE, None, None) == fpm_amd.FPM_ERR_INVAL
        assert "out is NULL" in msg()
        assert lib.fpm_predict(s._h, None, 0, fpm_amd.PREDICT_COUNTS | fpm_amd.PREDICT_DIFF, dst, None) == \
            fpm_amd.FPM_ERR_INVAL
        assert "more than one kind" in msg() and "0x3" in msg()
        assert lib.fpm_predict(s._h, None, 0, 8 | fpm_amd.PREDICT_DEVICE, dst, None) == fpm_amd.FPM_ERR_INVAL
        assert "unknown flag bits 0x8" in msg()
        assert lib.fpm_predict(None, None, 0, 0, dst, None) == fpm_amd.FPM_ERR_INVAL
        for pos, dx, what in (([0, n], [0, 0], "entry 1: pos="), ([0, 1, 2], [0, 0, 4096], "entry 2: window"),
                              ([-1], [0], "entry 0: pos=")):
            with pytest.raises(fpm_amd.FpmError) as ei:
                s.predict("amplitude", pos=pos, dx=dx)
            assert ei.value.code == fpm_amd.FPM_ERR_INVAL and what in str(ei.value) and "fpm_predict" in str(ei.value)
        probes = (fpm_amd.fpm_probe * 1)()
        assert lib.fpm_predict(s._h, probes, 0, 0, dst, None) == fpm_amd.FPM_ERR_INVAL and "n < 1" in msg()
        ms = C.c_double(-1.0)
        assert lib.fpm_predict(s._h, None, -5, 0, dst, C.byref(ms)) == fpm_amd.FPM_OK  # identity list: n is ignored
        assert ms.value >= 0 and np.all(np.isfinite(out))
        with pytest.raises(ValueError):
            s.predict("phase")


def test_predict_on_a_capturing_stream_is_refused():
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        want = s.predict("counts")
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(fpm_amd.FpmError) as ei:
            with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                s.predict("counts")
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        np.testing.assert_array_equal(s.predict("counts"), want)  # on the caller's stream, no longer capturing
        s.set_stream(None)
        np.testing.assert_array_equal(s.predict("counts"), want)


def test_device_bytes_count_the_staging_buffer():
    import torch
    prob, stack = _case(32, 96, 6, 5, 4, 3, 7, path=GENERAL)
    n, B, Np = len(prob.order), prob.n_patch, prob.np_
    with _solver(prob, stack, 1, (fpm_amd.KERNEL_GENERAL,)) as s:
        s.residual()  # the sweep's own scratch
        b0 = s.info().device_bytes
        dev = torch.zeros((n, B, Np, Np), dtype=torch.float32, device="cuda")
        s.predict("amplitude", device_ptr=dev.data_ptr())
        assert s.info().device_bytes == b0  # a device output needs no staging
        s.predict("counts")
        b1 = s.info().device_bytes
        assert b1 == b0 + n * B * Np * Np * 4  # nl = n_order here: one launch's batch of 4-byte elements
        s.predict("amplitude")
        s.predict("diff")
        assert s.info().device_bytes == b1


# ---- CLI ------------------------------------------------------------------------------
def test_cli_write_predicted(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    outs = {}
    for tag, extra in (("counts", ["--write-predicted", "counts"]), ("amplitude", ["--write-predicted", "amplitude"]),
                       ("without", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], "2", "--out", str(out)] + extra, capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = out
    plain = json.loads((outs["without"] / "result.json").read_text())
    assert "predicted" not in plain and not (outs["without"] / "predicted.npy").exists()
    arrays = {}
    for tag, dtype in (("counts", np.uint16), ("amplitude", np.float32)):
        meta = json.loads((outs[tag] / "result.json").read_text())
        assert set(meta) - {"predicted"} == set(plain)
        p = meta["predicted"]
        assert set(p) == {"kind", "shape", "ms"} and p["kind"] == tag and p["ms"] > 0
        a = np.load(outs[tag] / "predicted.npy")
        assert a.dtype == dtype and list(a.shape) == p["shape"] == [meta["leds_used"], 1, meta["np"], meta["np"]]
        arrays[tag] = a
        for f in ("objCrop.npy", "objF.npy", "pupil.npy"):
            assert (outs[tag] / f).read_bytes() == (outs["without"] / f).read_bytes(), f
    # the two kinds describe one state: counts = rint(amplitude^2) in fp32, unit gains
    amp = arrays["amplitude"]
    np.testing.assert_array_equal(arrays["counts"], np.minimum(np.rint(amp * amp), 65535).astype(np.uint16))
    r = subprocess.run([BIN, ds["json"], "1", "--write-predicted", "phase"], capture_output=True, text=True, env=env,
                       timeout=60)
    assert r.returncode == 2 and "amplitude, counts or diff" in r.stderr
