"""tests/refocus_check.py alone satisfies what the GPU tests demand of it: the
transfer function is a group in z and unitary where it propagates, the planes
conserve energy, the autofocus scene peaks at the planted z under all three
measures with a clear margin, and the scenes the sums are compared on meet the
condition behind the sum_g bound.  No GPU."""
import functools

import numpy as np
import pytest

import fpm_amd
import refocus_check as rc
from tools.synth import grid_geometry

# (Np, L, r, step) of a 3 x 3 LED grid: half-bands of 16 and 57 bins
GEOMETRIES = {"L192": (64, 192, 10, 6), "L512": (256, 512, 33, 24)}
Z_PLANES = np.arange(-24.0, 24.0 + 1, 4.0)   # wavelengths
Z_STAR, MARGIN = 12.0, 8


def _problem(name, B=1):
    Np, L, r, step = GEOMETRIES[name]
    x0, y0, order = grid_geometry(Np, L, 3, step)
    return fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=B, path=fpm_amd.PATH_GENERAL)


def test_band_and_bins():
    p = _problem("L192")
    assert rc.band_of(p) == (96 - 16, 96 + 16, 96 - 16, 96 + 16) and rc.half_band(p) == 16
    assert rc.half_band(_problem("L512")) == 57
    np.testing.assert_array_equal(rc.bins(8), [0, 1, 2, 3, -4, -3, -2, -1])
    m = rc.band_mask(8, (3, 5, 4, 6))   # centred rows 3..5 = bins -1..1, columns 4..6 = bins 0..2
    assert m.sum() == 9 and m[0, 0] and m[-1, 2] and m[1, 0] and not m[0, -1] and not m[2, 0]


@pytest.mark.parametrize("fl", [0.5 / 32, 1 / (0.8 * 32)])
def test_transfer_is_a_group_and_unitary(fl):
    L = 64
    k = rc.bins(L)
    s = fl * fl * (k[:, None] ** 2 + k[None, :] ** 2)
    live = s <= 1.0
    assert live[0, 0] and (fl < 0.02) == bool(live.all())   # the second fl has evanescent bins
    for z1, z2 in ((7.25, -3.5), (-1000.5, 1000.5), (123456.75, 0.25)):
        H1, H2, H12 = rc.transfer(L, z1, fl), rc.transfer(L, z2, fl), rc.transfer(L, z1 + z2, fl)
        np.testing.assert_allclose(np.abs(H1[live]), 1.0, rtol=0, atol=1e-15)
        assert not H1[~live].any()
        # |z| <= 1.3e5 wavelengths: the reduced phase carries <= 2^-53 * 1.3e5 turns = 1e-10 rad
        np.testing.assert_allclose((H1 * H2)[live], H12[live], rtol=0, atol=1e-9)
    assert np.array_equal(rc.transfer(L, 0.0, fl)[live], np.ones(live.sum()))
    # the definition itself, without the reduction
    want = np.exp(2j * np.pi * 7.25 * np.sqrt(1 - s[live]))
    np.testing.assert_allclose(rc.transfer(L, 7.25, fl)[live], want, rtol=0, atol=1e-13)


def test_energy_is_conserved_without_evanescent_bins():
    p = _problem("L192", B=2)
    objF, _ = rc.random_state(p, None, rc.band_of(p), 5)
    u = rc.planes(objF, (0.0, 7.25, -1000.5), 0.5 / rc.half_band(p))
    e = (np.abs(u) ** 2).sum((-2, -1))
    np.testing.assert_allclose(e, e[:1].repeat(3, 0), rtol=1e-12)
    np.testing.assert_allclose(rc.sums(u, 0)[1], e, rtol=1e-12)
    # and lost where bins are evanescent
    lossy = rc.planes(objF, (7.25,), 1 / (0.8 * rc.half_band(p)))
    assert ((np.abs(lossy) ** 2).sum((-2, -1)) < 0.9 * e[0]).all()


def test_sums_on_a_small_plane():
    a = np.array([[1.0, 2.0, 4.0], [3.0, 3.0, 0.0], [5.0, 1.0, 2.0]])
    sa, sa2, sg = rc.sums(a * np.exp(0.7j), 0)
    assert np.isclose(sa, a.sum()) and np.isclose(sa2, (a * a).sum())
    horiz = 1 + 4 + 0 + 9 + 16 + 1
    vert = 4 + 4 + 1 + 4 + 16 + 4
    assert np.isclose(sg, horiz + vert)
    # a margin keeps only the pairs wholly inside R
    b = np.pad(a, 2, constant_values=100.0)
    np.testing.assert_allclose(rc.sums(b, 2), (sa, sa2, sg))
    m = rc.measures(sa, sa2, sg, 3, 0)
    assert np.isclose(m["nvar"], a.var() / a.mean() ** 2) and np.isclose(m["grad"], sg / sa2)
    assert np.isclose(m["tamura"], np.sqrt(a.std() / a.mean()))


@functools.lru_cache(maxsize=None)
def _sweep(name):
    p = _problem(name)
    L, fl = p.L, 0.5 / rc.half_band(p)
    objF, sharp = rc.scene(L, rc.band_of(p), Z_STAR, fl, seed=11)
    u = rc.planes(objF[None], Z_PLANES, fl)[:, 0]
    return u, sharp, rc.measures(*rc.sums(u, MARGIN), L, MARGIN)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_autofocus_scene_peaks_at_the_planted_plane(name):
    u, sharp, m = _sweep(name)
    best = int(np.flatnonzero(Z_PLANES == Z_STAR)[0])
    assert rc.rel_l2(u[best], sharp) < 1e-12   # H(-z*) H(+z*) = 1 on the band
    for k in rc.MEASURES:
        v = m[k]
        assert int(v.argmax()) == best, (k, v)
        ratio = np.delete(v, best).max() / v[best]
        print(f"{name} {k}: second-best / best = {ratio:.3f}")
        assert ratio <= 0.9, (k, ratio)


@pytest.mark.parametrize("cid", rc.SUM_CONTEXTS)
def test_sum_scenes_meet_the_gradient_condition(cid):
    prob, ctx = rc.context_problem(cid, 3)
    objF, _ = rc.random_state(prob, ctx, rc.band_of(prob), rc.SUM_SEED[cid])
    u = rc.planes(objF, rc.SUM_ZL, 0.5 / rc.half_band(prob))
    for margin in rc.sum_margins(prob.L):
        _, sa2, sg = rc.sums(u, margin)
        print(f"{cid} margin {margin}: min sum_g / sum_a2 = {(sg / sa2).min():.3g}")
        assert (sg / sa2 >= rc.GRAD_CONDITION).all(), (margin, sg / sa2)
