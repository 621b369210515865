"""tests/step_cases.py holds cases (CPU only).  Per kernel row, over every case
and patch of the table:

  * the complex64 yardstick errs by at most C / 8 units of 2^-24 s(k) at every
    touched pixel (the row's C comes from this figure, step_cases.C64_WORST_UNITS;
    Np 1024: patch 0);
  * at most 0.1 % of the touched pixels have an update below 4 bound(k), and no
    pixel ON a support circle (kx^2 + ky^2 == r^2) has: a kernel that skips
    one, or writes one too many, is far outside the bound;
  * what the complex128 yardstick leaves untouched lies outside the disks, and
    the complex64 yardstick leaves exactly that bit-equal to the seed;
  * the planted maximum is the maximum; "outside" it stays the argmax at every
    step, outside both disks, and max|objF| taken over the disk instead moves
    the pupil by more than 16 bound at more than half of the support;
    "inside" the step changes the maximum;
  * deltas differs from plain, eps from deltas and each re-only run from its cv
    twin by more than 16 bound at more than half of the touched pixels;
  * under eps, |psi + eps (1 + i)| >= eps at every step (the conditioning guard);
  * on the shape with an fp16-storage row the seed is exact fp16 / hscale.

And once, with no GPU: check 2's comparison (step_cases.compare) rejects a
result with one on-circle pixel left at its seed value, one whose pupil update
is scaled by max over the disk / max over the band, and one whose patch 0 read
a 3 x 3 block of its measurements from patch 1.
"""
import dataclasses

import numpy as np
import pytest

import restate_step
import state_cases as sc
import step_cases as st

WEAK = 4.0        # x bound: an update below it is "weak"
WEAK_SHARE = 1e-3
DIFFERS = 16.0    # x bound


def _patches(case):
    return range(case.row.B if case.row.Np < 1024 else 1)


def _seed_arrays(case, patch):
    """(band of the centred seed spectrum, masked seed pupil)."""
    return st.band_of(case, case.seed(patch)), st.masked_pupil(case)


def _band_mask(case, m):
    sy0, sy1, sx0, sx1 = case.geo.band()
    return m[sy0:sy1 + 1, sx0:sx1 + 1]


def _circle_np(case):
    r = case.row
    k = np.arange(r.Np) - r.Np // 2
    return (k[:, None] ** 2 + k[None, :] ** 2) == r.r * r.r


def test_table():
    assert st.ROWS == sc.ROWS + ("fused_np90_r42",)
    assert len(st.CASES) == 11 * 40 + 2 * 4 and len({c.id for c in st.CASES}) == len(st.CASES)
    assert all(len(c.order) >= 2 for c in st.CASES)
    # the corner LED of the r 42 row reaches the partial tile of L 180
    c = next(c for c in st.cases("fused_np90_r42") if c.order == (4, 8))
    assert c.geo.band()[1] >= 176 and c.geo.band()[3] >= 176 and c.row.L == 180, c.geo.band()
    assert tuple(st.C) == st.ROWS
    for name in st.ROWS:
        # C is 8 x the measured complex64 error, rounded up to a power of two; the one constant the
        # whole table would share is the largest of them
        r = st.BASE[name].row
        assert st.C[name] == 2.0 ** np.ceil(np.log2(8 * st.C64_WORST_UNITS[(r.Np, r.L, r.r)])) <= 512
        want = {(p, f) for p, f in st.PARAMS} if st.BASE[name].row.Np < 1024 else {("plain", 0), ("eps", 0),
                                                                                    ("eps", st.RE_ONLY)}
        assert {(c.pset, c.flags) for c in st.cases(name)} == want
        assert {c.variant for c in st.cases(name)} == set(st.VARIANTS)


@pytest.mark.parametrize("name", st.ROWS)
def test_stack_and_seed(name):
    case = st.cases(name)[0]
    row = case.row
    stack, base = case.stack(), st.BASE[name].stack()
    (zy, zx), (fy, fx) = st.blocks(row.Np)
    assert stack.shape == base.shape and stack.dtype == np.uint16 and not stack.flags.writeable
    assert not stack[..., zy:zy + 3, zx:zx + 3].any() and (stack[..., fy:fy + 3, fx:fx + 3] == 65535).all()
    diff = stack != base
    assert diff.reshape(-1, row.Np, row.Np).any(axis=0).sum() <= 18
    for case in st.cases(name):
        sy0, sy1, sx0, sx1 = case.geo.band()
        live = np.zeros((row.L, row.L), bool)
        live[sy0:sy1 + 1, sx0:sx1 + 1] = True
        py, px = case.planted()
        assert live[py, px]
        first = st._disks(case.shape, case.order[:1])
        assert (not case.disks()[py, px]) if case.variant == "outside" else first[py, px]
        for b in range(row.B):
            spec = np.fft.fftshift(case.seed(b))
            assert spec.dtype == np.complex64 and not live.all()
            assert np.count_nonzero(spec[~live]) == 0 and np.count_nonzero(spec[live]) == live.sum()
            mag = np.abs(spec.astype(np.complex128))
            assert np.unravel_index(int(np.argmax(mag)), mag.shape) == (py, px)
            assert mag[py, px] > 1.05 * np.partition(mag.ravel(), -2)[-2]       # alone at the top
            if st._fp16_exact(case.shape):
                v = spec.view(np.float32) * np.float32(st.hscale(row.Np))
                np.testing.assert_array_equal(v.astype(np.float16).astype(np.float32), v)
                assert np.abs(v).max() < 65504
        assert not np.array_equal(case.seed(0), case.seed(1))         # one draw per patch
    assert any(st._fp16_exact(c.shape) for c in st.cases(name)) == (row.Np >= 1024)


def _weak_and_circle(C, upd, s, t, circle):
    """(number of weak touched pixels, touched pixels, smallest on-circle update / bound)."""
    bound = C * st.UNIT * s
    weak = t & (upd < WEAK * bound)
    on = circle & t
    assert on.sum() == circle.sum(), "an on-circle pixel is untouched"
    return int(weak.sum()), int(t.sum()), float((upd[on] / bound[on]).min())


@pytest.mark.parametrize("name", st.ROWS)
def test_row_holds_cases(name):
    worst64, weak_n, touched_n, circ, C = 0.0, 0, 0, np.inf, st.C[name]
    for case in st.cases(name):
        row = case.row
        disks, circle = _band_mask(case, case.disks()), _band_mask(case, case.circle())
        S, circle_p = sc.support_centred(row.Np, row.r), _circle_np(case)
        for b in _patches(case):
            seedF, seedP = _seed_arrays(case, b)
            r128, r64 = st.yardstick(case, b), st.yardstick(case, b, np.complex64)
            for k, seed, inside, circ_k in (("objF", seedF, disks, circle), ("pupil", seedP, S, circle_p)):
                u, t = st.units(r64[k], r128[k], seed)
                assert not (t & ~inside).any(), (case.id, b, k, "touched outside the disks")
                assert t.sum() > 0.98 * inside.sum(), (case.id, b, k)
                # the complex64 yardstick: its error where touched, the seed's bits elsewhere
                e = float(u[t].max())
                worst64 = max(worst64, e)
                assert e <= C / 8, (case.id, b, k, e)
                assert r64[k].dtype == np.complex64
                np.testing.assert_array_equal(r64[k][~inside], seed[~inside], err_msg=f"{case.id} {b} {k}")
                s, _ = st.scale(r128[k], seed)
                w, n, c = _weak_and_circle(C, np.abs(r128[k] - seed.astype(np.complex128)), s, t, circ_k)
                assert w <= WEAK_SHARE * n, (case.id, b, k, w, n)
                assert c >= WEAK, (case.id, b, k, c)
                weak_n, touched_n, circ = weak_n + w, touched_n + n, min(circ, c)
            if case.pset == "eps":
                _, _, eps = case.scalars()
                for rec in r128["record"] + r64["record"]:
                    # |psi + eps (1 + i)| >= sqrt(2) eps - max|psi| >= eps; the re-only divisor
                    # |psi + eps| >= eps - max|psi| stays above eps / 2
                    assert rec["psi_max"] <= (np.sqrt(2.0) - 1) * eps, (case.id, b, rec)
                    assert rec["psi_min"] >= (eps if case.all_channels else eps / 2), (case.id, b, rec)
    print(f"{name}: complex64 yardstick errs by at most {worst64:.1f} units (C {C:g}, C / 8 = {C / 8:g}); "
          f"{weak_n} of {touched_n} touched pixels weak ({100.0 * weak_n / touched_n:.4f} %); "
          f"smallest on-circle update {circ:.1f} x bound")


@pytest.mark.parametrize("name", st.ROWS)
def test_planted_maximum(name):
    shown = []
    for case in st.cases(name):
        if case.pset != "plain" and case.row.Np >= 1024:
            continue
        row = case.row
        py, px = case.planted()
        rec = st.yardstick(case, 0)["record"]
        seed_max = float(np.abs(case.seed(0).astype(np.complex128)).max())
        if case.variant == "inside":
            assert rec[0]["objf_max"] != seed_max, case.id
            continue
        for r in rec:
            assert r["objf_argmax"] == (py, px) and r["objf_max"] == seed_max, (case.id, r)
        if case.pset != "plain":
            continue          # the other parameter sets: the record above; the rerun below once per order

        def over_the_disk(objF_c, led, case=case):
            return np.abs(objF_c[st._disks(case.shape, (led,))]).max()

        ref = st.yardstick(case, 0)
        alt = st.iterate(case, case.seed(0), st.masked_pupil(case), 0, objf_max=over_the_disk)
        S = sc.support_centred(row.Np, row.r)
        s, t = st.scale(ref["pupil"], st.masked_pupil(case))
        moved = np.abs(alt["pupil"] - ref["pupil"]) > DIFFERS * st.C[name] * st.UNIT * s
        assert (moved & S).sum() > 0.5 * S.sum(), (case.id, int((moved & S).sum()), int(S.sum()))
        shown.append(f"{(moved & S).sum()}/{S.sum()}")
    print(f"{name}: max over the disk instead of the band moves the pupil beyond {DIFFERS:g} x bound at {shown}")


def _differs(C, a, b, seeds, where):
    """The yardstick results a and b differ by more than DIFFERS bound(k) (b's) at more than half of b's touched pixels."""
    for k in ("objF", "pupil"):
        s, t = st.scale(b[k], seeds[k])
        far = t & (np.abs(a[k] - b[k]) > DIFFERS * C * st.UNIT * s)
        assert far.sum() > 0.5 * t.sum(), (where, k, int(far.sum()), int(t.sum()))


@pytest.mark.parametrize("name", st.ROWS)
def test_parameter_sets_differ(name):
    n = 0
    for case in st.cases(name):
        if case.pset == "plain" and case.row.Np < 1024:
            continue
        seedF, seedP = _seed_arrays(case, 0)
        seeds = dict(objF=seedF, pupil=seedP)
        me = st.yardstick(case, 0)
        twins = []
        if case.flags:
            twins.append(dataclasses.replace(case, flags=0))                       # re-only against its cv twin
        elif case.pset == "deltas":
            twins.append(dataclasses.replace(case, pset="plain"))
        elif case.pset == "eps":
            twins.append(dataclasses.replace(case, pset="deltas"))
        elif case.variant == "inside":                                             # Np 1024, plain: against deltas
            twins.append(dataclasses.replace(case, pset="deltas"))
        for twin in twins:
            _differs(st.C[name], st.yardstick(twin, 0), me, seeds, (case.id, twin.id))
            n += 1
    assert n > 0
    print(f"{name}: {n} pairs of parameter sets differ beyond {DIFFERS:g} x bound at more than half of the touched pixels")


# ---- check 2 rejects what the relative L2 bounds let through ---------------------------------
@pytest.mark.parametrize("name", ["general_lds_L90", "fused_np256", "general_reg256"])
def test_comparison_rejects_the_defects(name):
    case = next(c for c in st.cases(name) if c.order == (4, 8) and c.iters == 1 and c.pset == "plain"
                and c.variant == "outside")
    row, C = case.row, st.C[name]
    seedF, seedP = _seed_arrays(case, 0)
    ref = st.yardstick(case, 0)
    for k, seed in (("objF", seedF), ("pupil", seedP)):
        assert st.compare(ref[k], ref[k], seed, C)[0] == 0.0
        assert st.compare(st.yardstick(case, 0, np.complex64)[k], ref[k], seed, C)[0] <= 1.0 / 8
    out = []

    # 1. one on-circle pixel left at its seed value
    for k, seed, circle in (("objF", seedF, _band_mask(case, case.circle())), ("pupil", seedP, _circle_np(case))):
        y, x = np.argwhere(circle)[len(np.argwhere(circle)) // 3]
        got = ref[k].astype(np.complex64)
        got[y, x] = seed[y, x]
        ratio, where = st.compare(got, ref[k], seed, C)
        assert ratio > 1 and where == (y, x), (k, ratio, where)
        out.append(f"{k} rim pixel {ratio:.0f}")

    # 2. the pupil update scaled by max over the window / max over the band (a stale or local maximum)
    spec0 = np.fft.fftshift(case.seed(0).astype(np.complex128))
    f = np.abs(spec0[case.disks()]).max() / np.abs(spec0).max()
    assert f < 0.9
    got = (seedP + (ref["pupil"] - seedP) * f).astype(np.complex64)
    ratio, _ = st.compare(got, ref["pupil"], seedP, C)
    assert ratio > 1, ratio
    out.append(f"scaled pupil update {ratio:.0f}")

    # 3. patch 0 reads a 3 x 3 block of every image from patch 1
    stack = case.stack()[:, 0].copy()
    y, x = row.Np // 2 + 1, row.Np // 5
    assert (stack[:, y:y + 3, x:x + 3] != case.stack()[:, 1, y:y + 3, x:x + 3]).any()
    stack[:, y:y + 3, x:x + 3] = case.stack()[:, 1, y:y + 3, x:x + 3]
    d1, d2, eps = case.scalars()
    b = st.BASE[name]
    mixed = restate_step.iterate(case.seed(0), st.masked_pupil(case), stack, case.order, b.x0, b.y0, row.Np, row.L,
                                 row.r, d1, d2, case.iters, eps=eps, objcrop=False)
    for k, seed, got in (("objF", seedF, st.band_of(case, mixed["objF"])), ("pupil", seedP, mixed["pupil"])):
        ratio, _ = st.compare(got.astype(np.complex64), ref[k], seed, C)
        assert ratio > 1, (k, ratio)
        out.append(f"{k} mixed block {ratio:.0f}")
    print(f"{name}: worst |got - ref| / bound: " + ", ".join(out))
