"""Row pairs of the Np 256 fused kernel (fpm_fused.hip, two column halves cut
on the low column digit; fused256.hpp "row pairs", tests/test_rowpair_model.py
for the index maps): in passes A and C one four-step transform serves both FFT
rows of a 16-lane group, lanes 0-7 the first row and lanes 8-15 the second.

The radii are the smallest set that reaches every row configuration of the 32
groups (group g owns FFT rows g and g + 32 of the 2r + 1 box rows):

   r   rows
  10   21            no group has a second row; some groups have none
  15   31            no second row; one group without a row
  16   33            exactly one group with a second row
  20   41            second rows in part of a wave
  31   63            one second row missing
  32   64 + 1 tail row
  33   64 + 3 tail rows (the metric's)
  34   64 + 5 tail rows (the kernel's limit)

Per radius: one workgroup per patch against the fp64 oracle after two
iterations (5e-5, the project's bound) and after one (1e-5), both patches,
objF / objCrop / pupil; and two workgroups per patch (one half each) bit for
bit equal to one.  A wrong column map, twiddle index or row / lane pairing
gives O(1) errors.  r 33 also runs through the GAIN instance the way
tests/test_gpu_gains.py does: gains from {0.5, 1, 2} on a stack of multiples
of 4 against the oracle on uint16(g^2 I).
"""
import functools
import os

import numpy as np
import pytest

import fpm_amd
import oracle_lib
from fpm_oracle import rel_l2
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

NP, L, B, D1, D2 = 256, 512, 2, 10, 3
RADII = (10, 15, 16, 20, 31, 32, 33, 34)
KEYS = ("objF", "objCrop", "pupil")


@functools.lru_cache(maxsize=None)
def _geometry():
    return grid_geometry(NP, L, 3, 24)


@functools.lru_cache(maxsize=None)
def _stack(r):
    x0, y0, _ = _geometry()
    st = make_stack(NP, L, r, x0, y0, n_patch=B, seed=100 + r)
    st.setflags(write=False)
    return st


def _solve(r, stack, iters, ks, gains=None):
    x0, y0, order = _geometry()
    prob = fpm_amd.Problem(NP, L, order, x0, y0, r, D1, D2, n_patch=B, path=fpm_amd.PATH_FUSED)
    env = {"FPM_NO_SPLIT": "1", "FPM_NO_DIST": "1"} if ks == 1 else {"FPM_SPLIT": str(ks), "FPM_NO_DIST": "1"}
    os.environ.update(env)
    try:
        with fpm_amd.Solver(prob) as s:
            info = s.info()
            assert info.fused_kernel == fpm_amd.KERNEL_FUSED_NP256 and info.wg_per_patch == ks
            s.upload(stack)
            if gains is not None:
                s.set_gains(gains)
            s.init()
            s.run(iters)
            return s.download()
    finally:
        for k in env:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _one_workgroup(r, iters):
    return _solve(r, _stack(r), iters, 1)


def _oracle(stack, iters, r):
    x0, y0, order = _geometry()
    return [oracle_lib.run_fpm(stack[:, b], order, x0, y0, NP, L, r, D1, D2, iters) for b in range(B)]


def _check(out, ref, tol, what):
    errs = {k: max(rel_l2(out[k][b], ref[b][k]) for b in range(B)) for k in KEYS}
    print(f"{what}: max rel L2 " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {tol:g})")
    for k, v in errs.items():
        assert v < tol, (what, k, v)


@pytest.mark.parametrize("r", RADII)
def test_two_iterations_vs_oracle(r):
    _check(_one_workgroup(r, 2), _oracle(_stack(r), 2, r), 5e-5, f"r {r}, 2 iterations")


@pytest.mark.parametrize("r", RADII)
def test_one_iteration_vs_oracle(r):
    _check(_one_workgroup(r, 1), _oracle(_stack(r), 1, r), 1e-5, f"r {r}, 1 iteration")


@pytest.mark.parametrize("r", RADII)
def test_two_workgroups_equal_one(r):
    one = _one_workgroup(r, 2)
    two = _solve(r, _stack(r), 2, 2)
    for k in KEYS:
        np.testing.assert_array_equal(two[k], one[k], err_msg=f"r {r} {k}")


def test_gain_instance_vs_oracle():
    r = 33
    x0, _, _ = _geometry()
    base = ((_stack(r).astype(np.uint32) // 16) * 4).astype(np.uint16)
    g = np.random.default_rng(20261020).choice(np.array((0.5, 1.0, 2.0), np.float32), size=(len(x0), B))
    assert (g != 1.0).any()
    gained = base.astype(np.float64) * g.astype(np.float64)[:, :, None, None] ** 2
    assert gained.max() <= 65520 and np.array_equal(gained, np.rint(gained))
    ref = _oracle(gained.astype(np.uint16), 2, r)
    for ks in (1, 2):
        _check(_solve(r, base, 2, ks, gains=g), ref, 5e-5, f"r 33 with gains, {ks} workgroup(s) per patch")
