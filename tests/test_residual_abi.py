"""fpm_residual at the boundary (ABI 6), without a GPU: the header declares
it, the library exports it and reports the revision, the Python mirror follows,
and the normalised residual is the column quotient."""
import ctypes as C
import os
import re

import numpy as np

import fpm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_fpm_residual_and_abi_6():
    text = open(os.path.join(ROOT, "include", "fpm_hip.h")).read()
    assert re.search(r"#define\s+FPM_ABI_VERSION\s+6\b", text)
    assert re.search(r"\bint\s+fpm_residual\s*\(\s*fpm_ctx\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,"
                     r"\s*double\s*\*\s*\w+\s*\)\s*;", text)


def test_library_exports_fpm_residual_and_reports_abi_6():
    so = C.CDLL(fpm_amd.HIP_LIB)
    assert hasattr(so, "fpm_residual")
    so.fpm_abi_version.restype = C.c_int
    assert so.fpm_abi_version() == 6


def test_python_mirror_follows_abi_6():
    assert fpm_amd.ABI_VERSION == 6
    assert "fpm_residual" in fpm_amd.HIP_SYMBOLS
    assert callable(fpm_amd.Solver.residual)
    assert callable(fpm_amd.normalised_residual)


def test_normalised_residual_is_the_column_quotient():
    err = np.array([[1.0, 2.0, 0.5], [3.0, 6.0, 0.25]])
    ref = np.array([[10.0, 4.0, 1.0], [30.0, 12.0, 2.0]])
    got = fpm_amd.normalised_residual(dict(err=err, ref=ref, ms=0.0))
    assert got.shape == (3,)
    np.testing.assert_array_equal(got, np.array([4.0 / 40.0, 8.0 / 16.0, 0.75 / 3.0]))
