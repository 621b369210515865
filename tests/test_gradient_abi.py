"""fpm_gradient without a GPU: the header declares the entry point, its flag
and its feature macro, the revision stands, and the ctypes mirror covers them."""
import os
import re

import numpy as np

import fpm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()


def test_header_declares_gradient():
    assert re.search(r"^#define\s+FPM_HAS_GRADIENT\s+1\b", HEADER, re.M)
    assert re.search(r"^#define\s+FPM_ABI_VERSION\s+6\b", HEADER, re.M)  # the revision stands
    m = re.search(r"^#define\s+FPM_GRAD_DEVICE\s+(\d+)u\b", HEADER, re.M)
    assert m and int(m.group(1)) == fpm_amd.GRAD_DEVICE == 1
    decl = re.search(r"int\s+fpm_gradient\s*\(([^)]*)\)\s*;", HEADER)
    assert decl, "fpm_gradient is not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("fpm_ctx *ctx, const fpm_probe *probes, int n, uint32_t flags, float *grad_objF, "
                    "float *grad_pupil, double *err, double *ref, double *elapsed_ms")


def test_mirror_covers_gradient():
    assert fpm_amd.ABI_VERSION == 6
    assert "fpm_gradient" in fpm_amd.HIP_SYMBOLS
    lib = fpm_amd.load_library()
    assert lib.fpm_abi_version() == 6
    assert lib.fpm_gradient.restype is not None and len(lib.fpm_gradient.argtypes) == 9
    # refused on the host, before any device is touched
    assert lib.fpm_gradient(None, None, 0, 0, None, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
    assert "null ctx" in lib.fpm_last_error().decode()
    assert callable(fpm_amd.Solver.gradient)


def test_descent_coverage_matches_the_yardstick():
    import types

    import gradient_check as gc
    from fpm_amd import descent
    rng = np.random.default_rng(2)
    prob = types.SimpleNamespace(np_=8, L=24, n_patch=2, order=[1, 0, 2], x0=[3, 5, 9], y0=[4, 2, 11], radius=2)
    pupil = (rng.normal(size=(2, 8, 8)) + 1j * rng.normal(size=(2, 8, 8))).astype(np.complex64)
    objF = (rng.normal(size=(2, 24, 24)) + 1j * rng.normal(size=(2, 24, 24))).astype(np.complex64)
    np.testing.assert_allclose(descent.coverage(prob, pupil), gc.coverage(prob, pupil), rtol=1e-12)
    np.testing.assert_allclose(descent.object_coverage(prob, objF), gc.object_coverage(prob, objF), rtol=1e-12)
    np.testing.assert_allclose(descent.coverage(prob, pupil, [0, 0], [1, 0], [0, -1]),
                               gc.coverage(prob, pupil, [0, 0], [1, 0], [0, -1]), rtol=1e-12)
    M = gc.coverage(prob, pupil)
    G = (rng.normal(size=objF.shape) + 1j * rng.normal(size=objF.shape)).astype(np.complex64) * (M > 0)
    step = descent.majorised(objF, G, M, 8)
    assert step.dtype == np.complex64
    np.testing.assert_allclose(step, gc.majorised(objF, G, M, 8), rtol=1e-6)
    try:
        import torch
    except ImportError:
        return
    np.testing.assert_allclose(descent.coverage(prob, torch.tensor(pupil)).numpy(), gc.coverage(prob, pupil), rtol=1e-5)
    np.testing.assert_allclose(descent.object_coverage(prob, torch.tensor(objF)).numpy(),
                               gc.object_coverage(prob, objF), rtol=1e-5)
