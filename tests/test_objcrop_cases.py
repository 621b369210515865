"""The objCrop case table without a GPU (tests/objcrop_cases.py).

Band validity: every band of every context is one the launchers accept.
Coverage: what the table says a band reaches is re-derived by arithmetic from
   the kernels' launch geometry, restated here (crop256m.hip, crop600.hip,
   crop360.hip, crop4k.hip, fft_batch.hip), and the restatement is held against
   the library's own planner (fpm_debug_plan_objcrop: plan_objcrop, no HIP call)
   for every context of the table and over every L fpm_create accepts.
Non-triviality: an fp32 CPU transform (torch complex64 ifft2) of every case's
   input stays below BOUND / 5 against the complex128 reference, so a GPU case
   that misses BOUND is wrong, not ill-conditioned.  The L 4096 contexts are
   checked on one band each (a 4096^2 complex128 transform per band is not paid
   for): their inputs differ only in where the band lies.
"""
import numpy as np
import pytest
import torch

import fpm_amd
import objcrop_cases as oc
from fpm_oracle import rel_l2
from objcrop_cases import BATCHED, BOUND, C4K, REGS

CASES = oc.cases()
IDS = [oc.case_id(c, b) for c, b in CASES]


def test_table_shape():
    assert BOUND == 2e-6
    assert len(CASES) == 12 * 7 + 3 * 4 + 1 + 2
    assert oc.BY_ID["L5400"].bands == ("lo_hi", "straddle")
    assert [oc.BY_ID[k].n_patch("straddle") for k in ("L810", "L2430", "L5400")] == [2, 1, 1]
    for k in ("L810", "L2430", "L5400"):
        c = oc.BY_ID[k]
        assert (c.Np, c.r, c.step, c.family, c.path) == (30, 5, 4, BATCHED, oc.GENERAL)
    assert {c.id for c in oc.CONTEXTS if c.bands == oc.BIG} == {"L4096", "L4096h", "L3000"}
    assert oc.BY_ID["L4096b"].bands == ("straddle",)
    for ctx, name in CASES:
        want = 2 if ctx.L <= 1024 or (ctx.id, name) == ("L4096", "full") else 1
        assert ctx.n_patch(name) == want, (ctx.id, name)
        ctx.problem(name)       # the LED grid stays inside the spectrum
        assert 2 * ctx.r + 1 <= ctx.Np


@pytest.mark.parametrize("ctx,name", CASES, ids=IDS)
def test_band_is_valid(ctx, name):
    sy0, sy1, sx0, sx1 = oc.band(ctx, name)
    assert 0 <= sy0 <= sy1 < ctx.L and 0 <= sx0 <= sx1 < ctx.L


# ---- launch geometry, restated ------------------------------------------------------
def radices(n):
    """make_plan (create.cpp)."""
    out = []
    for r in (8, 4, 2, 3, 5):
        while n % r == 0:
            out.append(r)
            n //= r
    assert n == 1
    return out


def batched_C(L):
    """fft_log2_seq_per_block (fft_batch.hip) with fft_pass_capacity(R) = 24 // R * R * 512
    (fft_inplace.hpp: kFftRegElems 24, kFftThreads 512)."""
    cap = min([24 * 512] + [24 // R * R * 512 for R in radices(L)])
    lc = 0
    while lc < 4 and (L << (lc + 1)) <= cap:
        lc += 1
    assert (L << lc) <= cap
    return 1 << lc


def rows_per_block(ctx):
    if ctx.family == BATCHED:
        return batched_C(ctx.L)
    # crop256m.hip kCropGR 4; crop600.hip WR 2 / crop360.hip WR 1: 6 groups per wave, WR waves; crop4k.hip CW 16
    return {512: 4, 768: 4, 1024: 4, 600: 6 * 2, 360: 6 * 1, 4096: 16}[ctx.L]


def live_rows_per_block(ctx, sy0, sy1):
    """Live rows in each block of the row pass that holds any."""
    G, L, H = rows_per_block(ctx), ctx.L, ctx.L // 2
    if ctx.family == REGS:      # block k: spec rows sy0 + k G ... (grid ceil(nrows / G))
        n = sy1 - sy0 + 1
        return [min(G, n - k * G) for k in range(-(-n // G))]
    # batched: sequence s of the row pass is objF row s = spec row (s + H) mod L; block k: sequences [k G, (k + 1) G)
    live = [(y + H) % L for y in range(sy0, sy1 + 1)]
    per = {}
    for s in live:
        per[s // G] = per.get(s // G, 0) + 1
    return [per[k] for k in sorted(per)]


def test_rows_per_block_are_the_tables():
    for ctx in oc.CONTEXTS:
        assert rows_per_block(ctx) == ctx.Gr, ctx.id
    assert [batched_C(L) for L in (4096, 3000, 90, 96, 192, 768, 810, 2430, 5400)] == [2, 2, 16, 16, 16, 16, 8, 4, 1]
    assert 5 in radices(3000) and 5 in radices(90)
    assert radices(810) == [2, 3, 3, 3, 3, 5] and radices(2430) == [2, 3, 3, 3, 3, 3, 5]
    assert radices(5400) == [8, 3, 3, 3, 5, 5]
    # the first even 5-smooth L of each (C, L mod C): C 8 starts at 720 and C 4 at 1350; 810 is the first C 8 whose
    # last block holds 2 sequences, and no L below 5400 has a block of one sequence
    first = {}
    for L in range(2, 5401, 2):
        try:
            first.setdefault((batched_C(L), L % batched_C(L)), L)
        except AssertionError:      # not 5-smooth
            pass
    assert (first[8, 0], first[8, 2], first[4, 2], first[1, 0]) == (720, 810, 1350, 5400)
    assert min(k[0] for k in first) == 1


# ---- the restatement against the library's own planner ---------------------------------
KINDS = {REGS: (fpm_amd.OBJCROP_REGS_256M, fpm_amd.OBJCROP_REGS_600, fpm_amd.OBJCROP_REGS_360),
         C4K: (fpm_amd.OBJCROP_SIX_STEP_4K,), BATCHED: (fpm_amd.OBJCROP_BATCHED,)}
LDS_LIMIT = 160 * 1024     # bytes of LDS a gfx950 workgroup can have


def batched_lds(L):
    """Tile of C padded sequences plus the twiddle table, complex64."""
    return (batched_C(L) * (L + 1) + L) * 8


@pytest.mark.parametrize("ctx", oc.CONTEXTS, ids=lambda c: c.id)
def test_planner_names_the_tables_family(ctx):
    """fpm_debug_plan_objcrop (plan_objcrop itself, no HIP call) for the
    context's L, storage and switch: the row's family and rows per block."""
    assert set(ctx.env) <= {"FPM_NO_CROP4K"}
    plan = fpm_amd.debug_plan_objcrop(ctx.L, ctx.fp16, "FPM_NO_CROP4K" in ctx.env)
    assert plan["kind"] in KINDS[ctx.family], (ctx.id, plan)
    assert plan["per_block"] == ctx.Gr, (ctx.id, plan)
    if ctx.family == REGS:
        want = {600: fpm_amd.OBJCROP_REGS_600, 360: fpm_amd.OBJCROP_REGS_360}.get(ctx.L, fpm_amd.OBJCROP_REGS_256M)
        assert plan["kind"] == want
    if ctx.family == BATCHED:
        assert plan["per_block"] == batched_C(ctx.L)


def expected_kind(L, fp16, no_crop4k):
    """The dispatch rule: register kinds only without fp16 storage, L 4096
    six-step unless FPM_NO_CROP4K, everything else batched."""
    if not fp16 and L in (512, 768, 1024):
        return fpm_amd.OBJCROP_REGS_256M
    if not fp16 and L == 600:
        return fpm_amd.OBJCROP_REGS_600
    if not fp16 and L == 360:
        return fpm_amd.OBJCROP_REGS_360
    if L == 4096 and not no_crop4k:
        return fpm_amd.OBJCROP_SIX_STEP_4K
    return fpm_amd.OBJCROP_BATCHED


def test_planner_over_the_whole_domain():
    """Every even 5-smooth L from 4 to 10240 (fft_max_len), fp32 and fp16
    storage, with and without FPM_NO_CROP4K."""
    sizes = []
    for L in range(4, 10241, 2):
        try:
            radices(L)
        except AssertionError:
            continue
        sizes.append(L)
    assert {4, 360, 600, 768, 4096, 10000, 10240} <= set(sizes)
    over = {}
    for L in sizes:
        for fp16 in (False, True):
            for no_crop4k in (False, True):
                plan = fpm_amd.debug_plan_objcrop(L, fp16, no_crop4k)
                assert plan["kind"] == expected_kind(L, fp16, no_crop4k), (L, fp16, no_crop4k, plan)
                if plan["kind"] == fpm_amd.OBJCROP_BATCHED:
                    assert plan["per_block"] == batched_C(L)
                    assert plan["rows_lds_dynamic"] == plan["cols_lds_dynamic"] == batched_lds(L), (L, plan)
                    assert plan["rows_lds_static"] == plan["cols_lds_static"] == 0
                for p in ("rows", "cols"):
                    total = plan[p + "_lds_dynamic"] + plan[p + "_lds_static"]
                    if total > LDS_LIMIT:
                        over.setdefault(L, set()).add(total)
    assert over == {10240: {163848}}, over
    assert batched_lds(10000) == 160008 and batched_lds(10240) == 163848
    for bad in (2, 7, 14, 10242, 10368):    # below 4, odd, not 5-smooth (10242 too), 5-smooth beyond the limit
        with pytest.raises(fpm_amd.FpmError) as e:
            fpm_amd.debug_plan_objcrop(bad)
        assert e.value.code == fpm_amd.FPM_ERR_INVAL, bad


# H mod C sequences of lo_hi / hi_lo lie before the first block boundary: 45 mod 16 = 13, 405 mod 8 = 5, 1215 mod 4 = 3
UNALIGNED = {"L90": {"lo_hi": [3, 14], "hi_lo": [3, 16, 13], "one_row": [1]},
             "L810": {"lo_hi": [3, 6], "hi_lo": [3, 8, 5], "one_row": [1]},
             "L2430": {"lo_hi": [1, 4], "hi_lo": [1, 4, 3], "one_row": [1]}}


@pytest.mark.parametrize("ctx", [c for c in oc.CONTEXTS if c.family != C4K], ids=lambda c: c.id)
def test_block_edges(ctx):
    """lo_hi: a full block and a tail block with exactly one live row; hi_lo:
    exactly two full blocks; one_row: one live row.  L 90, 810 and 2430 are the
    exceptions: their blocks of C sequences are not aligned with H = L / 2, so
    lo_hi's C + 1 rows (L 90: 17 = 3 + 14) and hi_lo's 2 C fall into partly
    live blocks -- the tail block these sizes are here for is the launch's own
    (test_l90_tail_block)."""
    G = ctx.Gr
    for name, want in (("lo_hi", [G, 1]), ("hi_lo", [G, G]), ("one_row", [1])):
        if name not in (ctx.bands or oc.BANDS):
            continue
        sy0, sy1, _, _ = oc.band(ctx, name)
        got = live_rows_per_block(ctx, sy0, sy1)
        if ctx.id in UNALIGNED:
            want = UNALIGNED[ctx.id][name]
        assert got == want, (ctx.id, name, got)


def test_l90_tail_block():
    C = batched_C(90)
    assert C == 16 and -(-90 // C) == 6 and 90 - 5 * C == 10     # cs = min(C, nseq - s0) = 10 in the last block
    C = batched_C(810)
    assert C == 8 and -(-810 // C) == 102 and 810 - 101 * C == 2       # C 8: cs = 2
    C = batched_C(2430)
    assert C == 4 and -(-2430 // C) == 608 and 2430 - 607 * C == 2     # C 4: cs = 2
    assert batched_C(5400) == 1                                          # C 1: every block is full
    # full bands reach the tail block: its sequences are objF rows L - 2 and L - 1
    for cid in ("L810", "L2430"):
        assert "full" in (oc.BY_ID[cid].bands or oc.BANDS)


@pytest.mark.parametrize("cid,pieces", [("L512", 2), ("L768", 2), ("L1024", 2), ("L600", 2)])
def test_half_boundary(cid, pieces):
    """k_crop_cols / k_crop_cols600 stage the strip in pieces of HH = L / pieces
    rows; piece h holds objF rows [h HH, (h + 1) HH) = spec rows from s0, and its
    live rows relative to the piece are [ya, yb] = [max(sy0 - s0, 0),
    min(sy1 - s0, HH - 1)].  upper_only and lower_only leave one piece with
    ya > yb (no live row) and end / start the other exactly on the boundary;
    straddle has one live row on each side of it."""
    ctx = oc.BY_ID[cid]
    L, H, HH = ctx.L, ctx.L // 2, ctx.L // pieces

    def live(h, sy0, sy1):
        s0 = h * HH - H if h * HH >= H else h * HH + H
        return max(sy0 - s0, 0), min(sy1 - s0, HH - 1)

    sy0, sy1, _, _ = oc.band(ctx, "upper_only")     # spec rows [3, H - 1] = objF rows [H + 3, L - 1]: piece 1
    assert live(0, sy0, sy1) == (0, -1) and live(1, sy0, sy1) == (3, HH - 1)
    sy0, sy1, _, _ = oc.band(ctx, "lower_only")     # spec rows [H, L - 2] = objF rows [0, H - 2]: piece 0
    assert live(0, sy0, sy1) == (0, HH - 2) and live(1, sy0, sy1) == (HH, HH - 1)
    sy0, sy1, _, _ = oc.band(ctx, "straddle")
    assert live(0, sy0, sy1) == (0, 0) and live(1, sy0, sy1) == (HH - 1, HH - 1)
    sy0, sy1, sx0, sx1 = oc.band(ctx, "full")
    assert live(0, sy0, sy1) == live(1, sy0, sy1) == (0, HH - 1)
    # straddle's column edges lie inside a 16-column strip, not on its edge
    _, _, sx0, sx1 = oc.band(ctx, "straddle")
    assert sx0 % 16 not in (0, 15) or sx1 % 16 not in (0, 15)


def test_edges_of_the_spectrum_are_reached():
    for ctx in oc.CONTEXTS:
        names = ctx.bands or oc.BANDS
        if "lo_hi" in names:
            sy0, _, _, sx1 = oc.band(ctx, "lo_hi")
            assert (sy0, sx1) == (0, ctx.L - 1)
        if "hi_lo" in names:
            _, sy1, sx0, _ = oc.band(ctx, "hi_lo")
            assert (sy1, sx0) == (ctx.L - 1, 0)


# ---- non-triviality ------------------------------------------------------------------
C128_BANDS_4096 = {"L4096": "lo_hi", "L4096h": "upper_only", "L4096b": "straddle"}


@pytest.mark.parametrize("ctx,name", [(c, b) for c, b in CASES if C128_BANDS_4096.get(c.id, b) == b],
                         ids=lambda v: v.id if isinstance(v, oc.Context) else v)
def test_fp32_headroom_and_distinct_patches(ctx, name):
    spec = oc.make_input(ctx, name)
    sy0, sy1, sx0, sx1 = oc.band(ctx, name)
    live = np.zeros(spec.shape[1:], bool)
    live[sy0:sy1 + 1, sx0:sx1 + 1] = True
    assert spec.dtype == np.complex64 and np.isnan(spec[:, ~live]).all() and np.isfinite(spec[:, live]).all()
    ref = oc.reference(spec)
    c64 = torch.fft.ifft2(torch.fft.ifftshift(torch.from_numpy(oc.masked(spec)), dim=(-2, -1))).numpy()
    assert c64.dtype == np.complex64
    for b in range(len(spec)):
        e = rel_l2(c64[b], ref[b])
        print(f"{oc.case_id(ctx, name)} patch {b}: complex64 ifft2 rel L2 {e:.2e}")
        assert e < BOUND / 5, (b, e)
    if len(spec) == 2:
        assert rel_l2(spec[0][live], spec[1][live]) > 0.3 and rel_l2(ref[0], ref[1]) > 0.3
    if ctx.fp16:    # the stored halves are the input, exactly
        hs = np.float32(ctx.hscale)
        v = np.ascontiguousarray(spec[:, live]).view(np.float32) * hs
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
