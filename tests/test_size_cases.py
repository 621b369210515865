"""The transform-size table without a GPU (tests/size_cases.py).

Enumeration  SIZES is every even 5-smooth Np in [4, 96], counted here.
Radix plans  the plans of the table's Np and L values, derived from make_plan's
             rule, hold the pass shapes the sweep is there for: two radix-5
             passes, three radix-3 passes, (8, 2), every radix as the last pass
             and every radix an even size can start with as the first.  An
             accepted size is even, so its plan starts with 8, 4 or 2: a
             radix 3 or 5 runs at Ns = 1 only where a transform walks its plan
             backwards (tile_transform_ex, wave_transform: fft_inplace.hpp),
             and every radix ends a plan of the table.
Geometry     what the module docstring of size_cases.py says of each case.
Conditioning for every case the C++ fp64 oracle is finite on both patches and
             the Python oracle restated in complex64 (run_fpm(dtype=)) stays
             below a tenth of the parity bound on objF, objCrop and the pupil:
             a GPU case that misses the bound is wrong, not ill-conditioned.
             The drifts are printed (pytest -s).
Pupil moves  except at r = 0 the pupil leaves its support mask by more than
             1e-6, so a wrong pupil update shows.
"""
import numpy as np
import pytest

import fpm_amd
import oracle_lib
import size_cases as sc
from fpm_oracle import disk_support, fftshift2, rel_l2, run_fpm

KEYS = ("objF", "objCrop", "pupil")


def _smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def test_sizes_are_every_even_5_smooth_np_up_to_96():
    want = tuple(n for n in range(4, 97) if n % 2 == 0 and _smooth(n))
    assert sc.SIZES == want and len(want) == 22
    assert [r.id for r in sc.SIZE_ROWS] == [f"np{n}" for n in want]


def test_radix_plans():
    sizes = sorted({c.Np for c in sc.CASES} | {c.L for c in sc.CASES})
    plans = {n: sc.radices(n) for n in sizes}
    for n, p in plans.items():
        assert int(np.prod(p)) == n and list(p) == sorted(p, key=(8, 4, 2, 3, 5).index), (n, p)
        assert n % 2 == 0 and p[0] in (8, 4, 2), (n, p)    # an even size never starts with 3 or 5
    have = set(plans.values())
    assert any(p.count(5) == 2 for p in have)
    assert any(p.count(3) == 3 for p in have)
    assert (8, 2) in have and (2, 5, 5) in have and (2, 3, 3, 3) in have and (8, 2, 5) in have and (4, 3, 5) in have
    assert {p[0] for p in have} == {2, 4, 8}
    assert {p[-1] for p in have} == {2, 3, 4, 5, 8}
    # the same of the patch sizes alone: the LDS ladder and the fused kernels transform Np only
    np_plans = {sc.radices(n) for n in sc.SIZES}
    assert {p[0] for p in np_plans} == {2, 4, 8} and {p[-1] for p in np_plans} == {2, 3, 4, 5, 8}
    # a later pass (Ns > 1) of every radix whose index path is the non-power-of-two udiv: Ns has a factor 3 or 5
    later = {(R, bool(int(np.prod(p[:i])) & (int(np.prod(p[:i])) - 1))) for p in np_plans for i, R in enumerate(p) if i}
    assert {(3, True), (5, True)} <= later and {(2, False), (3, False), (5, False)} <= later


def test_table_is_what_it_claims():
    assert len(sc.ROWS) == 22 + 4 + 4 + 4
    for row in sc.SIZE_ROWS:
        Np = int(row.id[2:])
        want = sorted({1, Np // 4, min(Np // 2 - 1, 31)})
        assert [c.r for c in row.cases] == want, row.id
        for c in row.cases:
            assert c.L == 3 * Np and len(c.x0) == 9 and sorted(c.order) == list(range(9))
            assert c.x0[1] - c.x0[0] == max(1, c.r)
            paths = [x.path for x in c.contexts]
            if Np >= 8:
                want_k = fpm_amd.KERNEL_FUSED_NP90 if Np == 90 else fpm_amd.KERNEL_FUSED_SMALL
                assert paths == [fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED] and c.contexts[1].kernel == want_k
            else:
                assert paths == [fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED, fpm_amd.PATH_AUTO]
                assert c.contexts[1].kernel is None and c.contexts[2].kernel == fpm_amd.KERNEL_GENERAL
    assert [c.r for c in sc.BY_ID.values() if c.Np == 4 and c.L == 12 and c.r] == [1]
    assert [c.r for c in sc.ROWS[1].cases] == [1, 2]
    corners = {r.id: r.cases[0] for r in sc.CORNER_ROWS}
    assert [(c.Np, c.L) for k, c in corners.items() if k.startswith("r0_")] == [(4, 12), (32, 96), (96, 288), (256, 512)]
    assert [(c.Np, c.r) for k, c in corners.items() if k.startswith("LeqNp_")] == [(32, 6), (90, 30), (200, 26), (256, 33)]
    assert [(c.Np, c.L, c.r) for k, c in corners.items() if k.startswith("Lmod_")] == \
        [(32, 50, 6), (30, 36, 5), (90, 100, 12), (96, 100, 31)]
    for k, c in corners.items():
        if k.startswith("r0_"):
            assert c.r == 0 and c.x0[1] - c.x0[0] == 1 and [x.path for x in c.contexts] == [fpm_amd.PATH_AUTO]
            assert c.contexts[0].kernel == fpm_amd.KERNEL_GENERAL and c.contexts[0].general_kind == fpm_amd.GENERAL_LDS
        elif k.startswith("LeqNp_"):
            assert c.L == c.Np and c.x0 == c.y0 == (0, 0) and c.order == (0, 1)
            assert c.contexts[0].path == fpm_amd.PATH_AUTO
            assert [x.path for x in c.contexts[1:]] == ([fpm_amd.PATH_GENERAL] if c.Np == 32 else [])
        else:
            assert c.L % c.Np and c.x0[1] - c.x0[0] == min(c.r, (c.L - c.Np) // 2) >= 1
            assert [x.path for x in c.contexts] == [fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED]
    for c in sc.CASES:      # fpm_create's rules
        assert c.Np % 2 == 0 and c.L % 2 == 0 and c.L >= c.Np and 0 <= c.r and 2 * c.r + 1 <= c.Np and len(c.order) >= 2
        assert all(0 <= v <= c.L - c.Np for v in c.x0 + c.y0), c.id
        sy0, sy1, sx0, sx1 = c.band()
        assert 0 <= sy0 <= sy1 < c.L and 0 <= sx0 <= sx1 < c.L
    assert len({c.seed for c in sc.CASES}) == len(sc.CASES)


def test_l_eq_np_images_differ_by_their_noise():
    for row in sc.CORNER_ROWS:
        c = row.cases[0]
        if c.L != c.Np:
            continue
        st = c.stack().astype(np.float64)
        for b in range(sc.B):
            d = rel_l2(st[0, b], st[1, b])
            assert 0 < d < 0.1, (c.id, b, d)        # the same expectation, another draw
        assert rel_l2(st[:, 0], st[:, 1]) > 0.1     # and two distinct patches


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_well_posed_and_fp32_headroom(case):
    st = case.stack()
    assert st.shape == (len(case.x0), sc.B, case.Np, case.Np)
    # two distinct patches; at r = 0 an image is one spectrum pixel's power, flat but for its noise
    assert rel_l2(st[:, 0], st[:, 1]) > (0.01 if case.r else 1e-3)
    args = (case.order, case.x0, case.y0, case.Np, case.L, case.r, sc.DELTA1, sc.DELTA2, sc.ITERS)
    ref = oracle_lib.run_fpm_batch(st, *args, threads=sc.B, objF=True)
    for k in KEYS:
        assert ref[k].shape[0] == sc.B and np.isfinite(ref[k]).all(), k
        assert min(np.abs(ref[k][b]).max() for b in range(sc.B)) > 0, k
    py = run_fpm(st[:, 0], *args)
    c64 = run_fpm(st[:, 0], *args, dtype=np.complex64)
    drift = {k: rel_l2(c64[k], ref[k][0]) for k in KEYS}
    moved = float(np.abs(fftshift2(py["pupil"]) - disk_support(case.Np, case.r)).max())
    print(f"{case.id}: complex64 drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items())
          + f"; max |P - support| {moved:.2e}")
    for k, v in drift.items():
        assert rel_l2(py[k], ref[k][0]) < 1e-10, k      # the two fp64 restatements agree
        assert c64[k].dtype == np.complex64 and v < case.tol / 10, (k, v)
    if case.r > 0:
        assert moved > 1e-6
