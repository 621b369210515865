"""fpm_predict without a GPU: the header declares the entry point, its flags
and its feature macro, the ctypes mirror covers them, fpmMain names the flag,
and tests/predict_check.py's own arithmetic holds on a numpy-only example."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import fpm_amd
import predict_check as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")


def test_header_declares_predict():
    assert re.search(r"^#define\s+FPM_HAS_PREDICT\s+1\b", HEADER, re.M)
    assert re.search(r"^#define\s+FPM_ABI_VERSION\s+6\b", HEADER, re.M)  # the revision stands
    decl = re.search(r"int\s+fpm_predict\s*\(([^)]*)\)\s*;", HEADER)
    assert decl, "fpm_predict is not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("fpm_ctx *ctx, const fpm_probe *probes, int n, uint32_t flags, void *out, "
                    "double *elapsed_ms")


def test_mirror_covers_predict():
    for name, py in (("AMPLITUDE", fpm_amd.PREDICT_AMPLITUDE), ("COUNTS", fpm_amd.PREDICT_COUNTS),
                     ("DIFF", fpm_amd.PREDICT_DIFF), ("DEVICE", fpm_amd.PREDICT_DEVICE)):
        m = re.search(rf"^#define\s+FPM_PREDICT_{name}\s+(\d+)u\b", HEADER, re.M)
        assert m and int(m.group(1)) == py, name
    assert set(fpm_amd.PREDICT_KINDS.values()) == {0, 1, 2}
    assert "fpm_predict" in fpm_amd.HIP_SYMBOLS
    lib = fpm_amd.load_library()
    assert lib.fpm_predict.restype is not None and len(lib.fpm_predict.argtypes) == 6
    # refused on the host, before any device is touched
    assert lib.fpm_predict(None, None, 0, 0, None, None) == fpm_amd.FPM_ERR_INVAL
    assert callable(fpm_amd.Solver.predict) and callable(fpm_amd.simulate)


def test_scatter_to_stack():
    prob = types.SimpleNamespace(x0=np.zeros(5), order=[3, 0, 4])
    rows = np.arange(3 * 2 * 2 * 2, dtype=np.uint16).reshape(3, 2, 2, 2) + 1
    st = fpm_amd.scatter_to_stack(prob, rows)
    assert st.shape == (5, 2, 2, 2) and st.dtype == np.uint16
    for i, led in enumerate(prob.order):
        np.testing.assert_array_equal(st[led], rows[i])
    assert not st[1].any() and not st[2].any()  # stack indices order[] does not name


def test_fpmmain_help_names_the_flag():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--write-predicted amplitude|counts|diff" in r.stdout


def _example():
    """A 2-LED, 1-patch state in download()'s layouts: a smooth spectrum and a disk pupil."""
    Np, L = 8, 16
    rng = np.random.default_rng(1)
    objF = (rng.normal(size=(1, L, L)) + 1j * rng.normal(size=(1, L, L))).astype(np.complex64) * 400
    ky, kx = np.mgrid[-Np // 2:Np // 2, -Np // 2:Np // 2]
    pupil = ((ky ** 2 + kx ** 2 <= 4) * np.exp(0.3j * (ky + kx)))[None].astype(np.complex64)
    prob = types.SimpleNamespace(np_=Np, L=L, n_patch=1, order=[1, 0], x0=[3, 5], y0=[4, 2])
    return prob, dict(objF=objF, pupil=pupil)


def test_reference_and_bounds_on_a_numpy_example():
    prob, state = _example()
    a = pc.amplitudes(state, prob)
    assert a.shape == (2, 1, 8, 8) and a.dtype == np.float64
    # row i is order[i]'s LED, and a probe list reproduces it; a moved window is another image
    O = np.fft.fftshift(state["objF"][0].astype(np.complex128))
    P = np.fft.ifftshift(state["pupil"][0].astype(np.complex128))
    want = np.abs(np.fft.ifft2(np.fft.ifftshift(O[4:12, 3:11]) * P))  # row 1 is LED 0: x0 3, y0 4
    np.testing.assert_array_equal(a[1, 0], want)
    np.testing.assert_array_equal(pc.amplitudes(state, prob, [1, 0, 1], [0, 0, 0], [0, 0, 0]), a[[1, 0, 1]])
    moved = pc.amplitudes(state, prob, [0], [1], [-1])
    np.testing.assert_array_equal(moved[0, 0], np.abs(np.fft.ifft2(np.fft.ifftshift(O[1:9, 6:14]) * P)))  # LED 1 moved
    # the amplitude bound: 1e-5 of the image's norm, 0 for a dark image
    np.testing.assert_allclose(pc.amplitude_bound(a), 1e-5 * np.sqrt((a ** 2).sum(axis=(2, 3))))
    assert pc.amplitude_bound(np.zeros((1, 1, 8, 8)))[0, 0] == 0
    g = np.array([[2.0], [0.5]])
    # counts: the reference saturates, rounding alone meets the bound, a wrong scale does not
    q = pc.counts_reference(a, g)
    np.testing.assert_allclose(q, np.minimum(a ** 2 / g[..., None, None] ** 2, 65535))
    assert pc.counts_reference(np.full((1, 1, 2, 2), 300.0), np.ones((1, 1))).max() == 65535
    c = np.rint(q).astype(np.uint16)
    pc.check_counts("example", c, a, g)
    with pytest.raises(AssertionError):
        pc.check_counts("example, gain ignored", np.rint(np.minimum(a ** 2, 65535)).astype(np.uint16), a, g)
    with pytest.raises(AssertionError):
        pc.check_counts("example, transposed", np.ascontiguousarray(c.transpose(0, 1, 3, 2)), a, g)
    # amplitude: fp32 rounding passes, a relative error of 1e-4 or a transposed image fails
    pc.check_amplitude("example", a.astype(np.float32), a)
    with pytest.raises(AssertionError):
        pc.check_amplitude("example, scaled", (a * (1 + 1e-4)).astype(np.float32), a)
    with pytest.raises(AssertionError):
        pc.check_amplitude("example, transposed", np.ascontiguousarray(a.transpose(0, 1, 3, 2)).astype(np.float32), a)
    # diff: the reference, its bound, and the agreement of sum d^2 with E
    I = (np.rint(q) + 3).astype(np.uint16)
    d = pc.diff_reference(a, I, g)
    np.testing.assert_allclose(d, a - g[..., None, None] * np.sqrt(I.astype(np.float64)))
    E, Q = pc.residual_sums(a, I, g)
    np.testing.assert_allclose(E, (d * d).sum(axis=(2, 3)))
    np.testing.assert_allclose(Q, (a * a).sum(axis=(2, 3)))
    bnd = pc.diff_bound(a, I, g)
    gs = g[..., None, None] * np.sqrt(I.astype(np.float64))
    np.testing.assert_allclose(bnd, pc.amplitude_bound(a) + 2.0 ** -23 * np.sqrt((gs ** 2).sum(axis=(2, 3))))
    pc.check_diff("example", d.astype(np.float32), a, I, g, err=E, E=E, Q=Q)
    with pytest.raises(AssertionError):
        pc.check_diff("example, gain ignored", (a - np.sqrt(I.astype(np.float64))).astype(np.float32), a, I, g)
    with pytest.raises(AssertionError):
        pc.check_diff("example, wrong E", d.astype(np.float32), a, I, g, err=E * 1.01, E=E, Q=Q)
    # a dark image (Q = 0) must be exactly the float32 -g sqrt(I)
    a0 = np.zeros_like(a)
    E0, Q0 = pc.residual_sums(a0, I, g)
    dark = -(g.astype(np.float32)[..., None, None] * np.sqrt(I.astype(np.float32)))
    pc.check_diff("example, dark", dark, a0, I, g, err=E0, E=E0, Q=Q0)
    with pytest.raises(AssertionError):
        pc.check_diff("example, dark, one ulp", np.nextafter(dark, np.float32(0)), a0, I, g, err=E0, E=E0, Q=Q0)
