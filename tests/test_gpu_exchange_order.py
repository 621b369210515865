"""Four-step exchange of the Np 256 fused kernel with its LDS traffic spread out
(fused256.hpp "the exchange, spread out"; dft16.hpp exch_put / exch_get): a
row store goes out behind the twiddle block that finishes it, and the reads
come back in the order their consumer needs them.  These are re-orderings of
independent instructions, so every result is what it was:

  * one workgroup per patch (KS 1) against the fp64 oracle after two
    iterations at 5e-5, the bound of tests/test_gpu_rowpair.py, every patch;
  * two workgroups per patch (KS 2, the same row-pair code) bit for bit equal
    to KS 1; four (KS 4, one transform per row, pass B shared) against the
    oracle at the same bound;
  * the same problem solved twice in one process, bit for bit: the exchange
    tile is reused by the next transform, and a store that overtook a read of
    the tile would show as a wrong, typically run-dependent, value.

Np 256, L 512, the 3 x 3 LED grid of the row-pair test.  r 10 leaves groups
without a row, r 33 is the metric's (64 FFT rows + 3 tail rows), r 34 the
kernel's limit; with B = 1 and B = 3 patches the loops' first and last rounds
run on a machine that is almost empty, where no other workgroup's traffic hides
an ordering slip.
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

NP, L, D1, D2, ITERS, BMAX = 256, 512, 10, 3, 2, 3
KEYS = ("objF", "objCrop", "pupil")
CASES = [(r, B) for r in (10, 33, 34) for B in (1, 3)]
IDS = [f"r{r}_B{B}" for r, B in CASES]


@functools.lru_cache(maxsize=None)
def _geometry():
    return grid_geometry(NP, L, 3, 24)


@functools.lru_cache(maxsize=None)
def _stack(r):
    x0, y0, _ = _geometry()
    st = make_stack(NP, L, r, x0, y0, n_patch=BMAX, seed=300 + r)
    st.setflags(write=False)
    return st


def _solve(r, B, ks):
    x0, y0, order = _geometry()
    stack = np.ascontiguousarray(_stack(r)[:, :B])
    prob = fpm_amd.Problem(NP, L, order, x0, y0, r, D1, D2, n_patch=B, path=fpm_amd.PATH_FUSED)
    env = {"FPM_NO_SPLIT": "1", "FPM_NO_DIST": "1"} if ks == 1 else {"FPM_SPLIT": str(ks), "FPM_NO_DIST": "1"}
    os.environ.update(env)
    try:
        with fpm_amd.Solver(prob) as s:
            info = s.info()
            assert info.fused_kernel == fpm_amd.KERNEL_FUSED_NP256 and info.wg_per_patch == ks
            s.upload(stack)
            s.init()
            s.run(ITERS)
            return s.download()
    finally:
        for k in env:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _one_workgroup(r, B):
    return _solve(r, B, 1)


@functools.lru_cache(maxsize=None)
def _oracle(r, b):
    """patch b of the radius' stack in fp64 (patch b is the same data for every B)"""
    x0, y0, order = _geometry()
    return oracle_lib.run_fpm(_stack(r)[:, b], order, x0, y0, NP, L, r, D1, D2, ITERS)


def _check_oracle(out, r, B, what):
    errs = {k: max(rel_l2(out[k][b], _oracle(r, b)[k]) for b in range(B)) for k in KEYS}
    print(f"{what}: max rel L2 " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + " (bound 5e-05)")
    for k, v in errs.items():
        assert v < 5e-5, (what, k, v)


@pytest.mark.parametrize("r,B", CASES, ids=IDS)
def test_one_workgroup_vs_oracle(r, B):
    _check_oracle(_one_workgroup(r, B), r, B, f"r {r}, B {B}, KS 1")


@pytest.mark.parametrize("r,B", CASES, ids=IDS)
def test_two_workgroups_equal_one(r, B):
    one, two = _one_workgroup(r, B), _solve(r, B, 2)
    for k in KEYS:
        np.testing.assert_array_equal(two[k], one[k], err_msg=f"r {r} B {B} {k}")


@pytest.mark.parametrize("r,B", CASES, ids=IDS)
def test_four_workgroups_vs_oracle(r, B):
    _check_oracle(_solve(r, B, 4), r, B, f"r {r}, B {B}, KS 4")


@pytest.mark.parametrize("r,B", CASES, ids=IDS)
def test_solved_twice_bit_equal(r, B):
    first, again = _one_workgroup(r, B), _solve(r, B, 1)
    for k in KEYS:
        np.testing.assert_array_equal(again[k], first[k], err_msg=f"r {r} B {B} {k}")
