"""fpm_refocus without a GPU: the header declares the entry point, its flags and
its feature macro, the ctypes mirror covers them, fpmMain names the options,
and fpm_amd.focus composes the measures the way tests/refocus_check.py does."""
import os
import re
import subprocess

import numpy as np
import pytest

import fpm_amd
import refocus_check as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")


def test_header_declares_refocus():
    assert re.search(r"^#define\s+FPM_HAS_REFOCUS\s+1\b", HEADER, re.M)
    assert re.search(r"^#define\s+FPM_ABI_VERSION\s+6\b", HEADER, re.M)  # the revision stands
    decl = re.search(r"int\s+fpm_refocus\s*\(([^)]*)\)\s*;", HEADER)
    assert decl, "fpm_refocus is not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("fpm_ctx *ctx, const double *zl, int nz, double fl, int margin, uint32_t flags, "
                    "float *planes, double *sum_a, double *sum_a2, double *sum_g, double *elapsed_ms")


def test_mirror_covers_refocus():
    for name, py in (("DEVICE", fpm_amd.REFOCUS_DEVICE), ("Z_PER_PATCH", fpm_amd.REFOCUS_Z_PER_PATCH)):
        m = re.search(rf"^#define\s+FPM_REFOCUS_{name}\s+(\d+)u\b", HEADER, re.M)
        assert m and int(m.group(1)) == py, name
    assert "fpm_refocus" in fpm_amd.HIP_SYMBOLS
    lib = fpm_amd.load_library()
    assert lib.fpm_refocus.restype is not None and len(lib.fpm_refocus.argtypes) == 11
    # refused on the host, before any device is touched
    assert lib.fpm_refocus(None, None, 0, 0.0, 0, 0, None, None, None, None, None) == fpm_amd.FPM_ERR_INVAL
    assert callable(fpm_amd.Solver.refocus)


def test_focus_module():
    from fpm_amd import focus
    assert focus.bin_frequency(0.6292, 96, 0.25) == 0.6292 / (96 * 0.25)
    rng = np.random.default_rng(3)
    u = rng.normal(size=(4, 2, 24, 24)) + 1j * rng.normal(size=(4, 2, 24, 24))
    for margin in (0, 3):
        sa, sa2, sg = rc.sums(u, margin)
        got = focus.measures(dict(sum_a=sa, sum_a2=sa2, sum_g=sg), 24, margin)
        want = rc.measures(sa, sa2, sg, 24, margin)
        assert set(got) == set(focus.MEASURES) == set(rc.MEASURES)
        for k in rc.MEASURES:
            assert got[k].shape == (4, 2)
            np.testing.assert_allclose(got[k], want[k], rtol=1e-14)
        a = np.abs(u)[..., margin:24 - margin, margin:24 - margin]
        np.testing.assert_allclose(got["nvar"], a.var((-2, -1)) / a.mean((-2, -1)) ** 2, rtol=1e-12)
    v = np.array([[1.0, 5.0], [3.0, 2.0], [2.0, 9.0]])
    np.testing.assert_array_equal(focus.pick_planes(v, "max"), [1, 2])
    np.testing.assert_array_equal(focus.pick_planes(v, "min"), [0, 1])
    with pytest.raises(ValueError):
        focus.pick_planes(v, "median")


def test_fpmmain_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--refocus Z0:DZ:N", "--focus-measure nvar|tamura|grad", "--focus-pick max|min", "--focus-margin PX",
                "--write-refocus"):
        assert opt in r.stdout, opt
