"""Conditions on the references alone, over the case table of
tests/schedules.py, so that no GPU case of tests/test_gpu_schedules.py can
pass by being trivial.  CPU only.

S1   the oracle's signal reaches the corner LED, the unused LED's box stays
     exactly zero, and the corner LED's box touches the spectrum's partial
     tile where a valid problem can bring it there (schedules.py docstring).
S3   the oracle's per-step trace of max|objF| (patch 0) moves between tiles,
     decreases while staying in its tile, and decreases while the new maximum
     lies outside the tile window of the LED just processed: the step the
     fused kernels' outside_max / dirty-tile bookkeeping exists for.
fp32 the Python oracle restated in complex64 (run_fpm(dtype=)) stays below
     one tenth of the parity bound for every case: a GPU case that misses the
     bound is wrong, not ill-conditioned.  The drifts are printed (pytest -s)
     and copied into DESIGN.md section 2.
"""
import numpy as np
import pytest

import oracle_lib
import schedules
from fpm_oracle import fftshift2, rel_l2, run_fpm



def _inputs(c):
    """What the references of patch 0 depend on: rows that differ only in the
    kernel, its mode, the patch count or the spectrum's storage share them."""
    r = c.row
    return (r.Np, r.L, r.r, c.x0, c.y0, c.order, c.iters, c.delta1, c.delta2, c.init_pos, c.flags,
            r.s3 if c.sched == "S3" else None)


def _distinct(sched=None):
    seen = {}
    for c in schedules.CASES:
        if sched in (None, c.sched):
            seen.setdefault(_inputs(c), c)
    return list(seen.values())


S1, S3, ALL = _distinct("S1"), _distinct("S3"), _distinct()
_ids = dict(ids=lambda c: c.id)


def _oracle(case, patch=0, **kw):
    r = case.row
    return oracle_lib.run_fpm(case.stack()[:, patch], case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1,
                              case.delta2, case.iters, all_channels=case.all_channels, init_pos=case.init_pos, **kw)


def test_table_covers_every_kernel_and_schedule():
    names = [k.name for k in schedules.KERNELS]
    assert len(set(names)) == len(names) and len({c.id for c in schedules.CASES}) == len(schedules.CASES)
    for k in schedules.KERNELS:
        have = {c.sched for c in schedules.CASES if c.row is k}
        assert have == set(k.schedules), k.name
    for c in schedules.CASES:
        n_stack = len(c.x0)
        assert set(c.used()) | set(c.unused) == set(range(n_stack)) and not set(c.used()) & set(c.unused), c.id
        for led in range(n_stack):  # fpm_create's rule: every crop window inside the spectrum
            assert 0 <= c.x0[led] <= c.row.L - c.row.Np and 0 <= c.y0[led] <= c.row.L - c.row.Np, (c.id, led)
    s2 = next(c for c in schedules.CASES if c.sched == "S2")
    assert len(s2.order) == 11 > len(s2.x0) == 9
    for grp in schedules.S2_REPEATS:
        assert len({s2.order[i] for i in grp}) == 1


@pytest.mark.parametrize("init_pos", [0, 10])
def test_oracles_agree_on_init_pos(init_pos):
    """numpy and C++ restatements with the spectrum seeded from order[0] and
    from the last position of S2's order (the reference hard-codes 1)."""
    case = schedules.BY_ID[f"general_lds-S2-init{init_pos}-cv"]
    r = case.row
    st = case.stack()[:, 0]
    py = run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, case.iters,
                 init_pos=init_pos)
    cc = _oracle(case)
    one = run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, case.iters)
    for k in ("objF", "objCrop", "pupil"):
        assert rel_l2(cc[k], py[k]) < 1e-10, k
        assert rel_l2(py[k], one[k]) > 1e-3, k   # and init_pos is not ignored


def _box(a, box):
    y0, y1, x0, x1 = box
    return a[y0:y1 + 1, x0:x1 + 1]


@pytest.mark.parametrize("case", S1, **_ids)
def test_s1_signal_reaches_the_corner(case):
    r = case.row
    spec = fftshift2(_oracle(case)["objF"])
    for led in case.used():
        assert np.count_nonzero(_box(spec, case.box(led))) > 0, led
    corner = next(led for led in case.used() if (case.x0[led], case.y0[led]) == (0, r.L - r.Np))
    # the unused LED's box, less what the used LEDs' boxes and the init placement cover, is exactly zero
    (unused,) = case.unused
    touched = np.zeros((r.L, r.L), bool)
    _box(touched, (r.L // 2 - r.r, r.L // 2 + r.r, r.L // 2 - r.r, r.L // 2 + r.r))[:] = True
    for led in case.used():
        _box(touched, case.box(led))[:] = True
    free = ~_box(touched, case.box(unused))
    if (r.Np, r.r) != (90, 42):   # r 42 of Np 90: the boxes are 85 wide and overlap the centre LED's
        assert free.all()
    assert free.sum() > free.size // 4
    assert np.count_nonzero(_box(spec, case.box(unused))[free]) == 0
    # one used LED at odd offsets from the centre, x != y
    c = r.L // 2 - r.Np // 2
    assert any((case.x0[i] - c) % 2 and (case.y0[i] - c) % 2 and case.x0[i] != case.y0[i] for i in case.used())
    y1 = case.box(corner)[1]
    if any(k.name in schedules.PARTIAL_TILE for k in schedules.KERNELS if (k.Np, k.L, k.r) == (r.Np, r.L, r.r)):
        assert r.L % 16 and y1 >= 16 * (r.L // 16)
    print(f"{case.id}: {len(case.used())} LEDs, corner box rows {case.box(corner)[0]}..{y1}, "
          f"partial tile from {16 * (r.L // 16)} of {r.L}")


def test_partial_tile_rows_are_the_reachable_ones():
    """Every row with L % 16 != 0 either touches the partial tile in S1 or is
    listed with the reason it cannot (schedules.py docstring)."""
    partial = {k.name for k in schedules.KERNELS if k.L % 16 and "S1" in k.schedules}
    unreachable = dict(schedules.PARTIAL_TILE_UNREACHABLE)
    assert partial == set(schedules.PARTIAL_TILE) | set(unreachable) | {"fused_np90"}
    for name, rmax in unreachable.items():
        k = schedules.ROWS[name]
        assert k.L - k.Np // 2 + rmax < 16 * (k.L // 16)
    k = schedules.ROWS["fused_np90"]
    assert k.L - k.Np // 2 + k.r < 16 * (k.L // 16) <= k.L - k.Np // 2 + schedules.ROWS["fused_np90_r42"].r


@pytest.mark.parametrize("case", S3, **_ids)
def test_s3_maximum_moves(case):
    trace = schedules.argmax_trace(case)
    moved, left, stayed = schedules.trace_counts(case, trace)
    print(f"{case.id}: {len(trace) - 1} steps, argmax tile changed in {moved}, maximum decreased and left the "
          f"LED's tile window in {left}, decreased in its tile in {stayed}")
    assert len(trace) - 1 == case.iters * len(case.order)
    assert moved >= 2 and left >= 1 and stayed >= 1


@pytest.mark.parametrize("case", ALL, **_ids)
def test_fp32_headroom(case):
    r = case.row
    ref = _oracle(case)
    c64 = run_fpm(case.stack()[:, 0], case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2,
                  case.iters, all_channels=case.all_channels, init_pos=case.init_pos, dtype=np.complex64)
    drift = {k: rel_l2(c64[k], ref[k]) for k in ("objF", "objCrop", "pupil")}
    print(f"{case.id}: complex64 drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
    for k, v in drift.items():
        assert c64[k].dtype == np.complex64 and v < case.tol / 10, (k, v)
