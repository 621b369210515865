"""The kernel ladder of the general path, without a GPU (tests/ladder_cases.py).

Planner audit: fpm_debug_plan_ladder (the library's own plan_lds_ladder and
   pick_lds_kernels, no HIP call) over every valid even Np up to the batched
   transform limit, four box sizes, five batch sizes, both modes and every
   switch combination.  Every plan must fit the register budget of its
   in-place passes (fft_inplace.hpp, restated here), choose wave-private
   columns only where a wave holds them, cover the box rows and the columns
   with its grids, and stay within the 160 KB of LDS a workgroup can have --
   or be one of the geometries fpm_create refuses.
Coverage: the rungs the same sweep reaches are all run by the case table.
Non-triviality: a complex64 numpy restatement stays below a tenth of the
   parity bound for every row up to Np 800, so a GPU case that misses the bound
   is wrong, not ill-conditioned; the sampled patches differ.  For Np 2916 the
   3.6e-7 measured at Np 2700 (test_gpu_parity.py
   test_one_sequence_row_kernels_match_oracle) stands in: a 3000^2 complex64
   run is not paid for.
"""
import itertools

import numpy as np
import pytest

import fpm_amd
import ladder_cases
import oracle_lib
from fpm_oracle import rel_l2, run_fpm
from ladder_cases import WAVE

FFT_MAX_LEN = 10240        # fft_max_len(): Nlarge's limit, hence Np's
LDS_LIMIT = 160 * 1024     # bytes of LDS a gfx950 workgroup can have
ONE, TILED, WAVEGEN = fpm_amd.LADDER_ONE_SEQ, fpm_amd.LADDER_TILED, fpm_amd.LADDER_WAVE


# ---- fft_inplace.hpp and make_plan (create.cpp), restated ----------------------------
def radices(n):
    out = []
    for r in (8, 4, 2, 3, 5):
        while n % r == 0:
            out.append(r)
            n //= r
    return out if n == 1 else None


def pass_capacity(R, nt, e):
    return e // R * R * nt


def colw_cw(np_, rad):
    for cw in (4, 2, 1):
        lpc = 64 // cw
        if all(-(-(np_ // R) // lpc) <= 16 // R for R in rad):
            return cw
    return 0


VALID_NP = [n for n in range(4, FFT_MAX_LEN + 1, 2) if radices(n)]
BATCHES = (1, 16, 64, 256, 1024)
SWITCHES = tuple(itertools.product((False, True), (False, True)))   # (no_wave_cols, one_seq)


def _sweep():
    """(Np, nb, B, step, no_wave_cols, one_seq, record) of the whole audit."""
    for np_ in VALID_NP:
        for nb in sorted({nb for nb in (3, 31, 121, min(np_ - 1, 667)) if nb <= np_ - 1 and nb % 2}):
            for B in BATCHES:
                for step in (True, False):
                    for nw, one in SWITCHES:
                        yield np_, nb, B, step, nw, one, fpm_amd.debug_plan_ladder(np_, nb, B, step, nw, one)


@pytest.fixture(scope="module")
def sweep():
    return list(_sweep())


def test_valid_sizes():
    assert len(VALID_NP) == 144 and VALID_NP[-1] == FFT_MAX_LEN and {30, 250, 486, 2916} <= set(VALID_NP)
    with pytest.raises(fpm_amd.FpmError) as e:
        fpm_amd.debug_plan_ladder(14, 3, 1)
    assert e.value.code == fpm_amd.FPM_ERR_INVAL


def test_planner_audit(sweep):
    over = set()
    for np_, nb, B, step, nw, one, rec in sweep:
        tag = (np_, nb, B, step, nw, one)
        rad = radices(np_)
        rows, cols = rec["rows"], rec["cols"]
        # the tiles fit the register budget of every radix pass at the planned threads and E
        for k in (rows, cols):
            if k["generation"] == TILED:
                assert k["e"] in (16, 24) and k["threads"] in (256, 512) and 1 <= k["tile"] <= 4, tag
                for R in rad:
                    assert (np_ << k["tile"]) <= pass_capacity(R, k["threads"], k["e"]), (tag, R)
            elif k["generation"] == ONE:
                assert (k["tile"], k["e"], k["threads"]) == (0, 0, 256), tag
        assert rows["generation"] != WAVEGEN and rows["threads"] == 256, tag
        # wave-private columns only where a wave holds at least two columns of this length
        if cols["generation"] == WAVEGEN:
            cw = cols["tile"]
            assert cw == colw_cw(np_, rad) and cw >= 2 and np_ <= 64 * 16 // cw and not nw and not one, tag
            assert cols["threads"] == 256 and cols["e"] == 16, tag
        elif not nw and not one:
            assert colw_cw(np_, rad) < 2, tag
        if one:
            assert rows["generation"] == ONE and cols["generation"] == ONE, tag
        # the grids cover the box rows and the columns, with no block past them
        rpb, cpb = 1 << rows["tile"], ladder_cases.columns_per_block(cols)
        assert rows["grid_x"] == -(-nb // rpb) and cols["grid_x"] == -(-np_ // cpb), tag
        assert rows["grid_y"] == B and cols["grid_y"] == B, tag
        # the step keeps shrinking its tiles only while the grid is short of 512 blocks
        if step and rows["generation"] == TILED and rows["tile"] > 1:
            assert rows["grid_x"] * B >= 512, tag
        if step and cols["generation"] == TILED and cols["tile"] > 2:
            assert cols["grid_x"] * B >= 512, tag
        # LDS: the twiddles and the tile, or two sequences
        for k in (rows, cols):
            assert k["lds_dynamic"] >= 8 * (np_ + (np_ << k["tile"] if k["generation"] == TILED else np_)), tag
            assert k["lds_static"] in (0, 16, 64, 128), tag
            if k["lds_dynamic"] + k["lds_static"] > LDS_LIMIT:
                over.add(np_)
    # what fpm_create must refuse (test_gpu_ladder.py test_create_refuses_np10240): DESIGN.md section 4.7 lists them
    assert over == {10240}, sorted(over)


def test_np10240_needs_more_than_the_lds():
    """163 840 B of ping-pong buffers plus the 16 B of K3's reduction (step) or
    the 64 B of the sweep's partial sums: 16 and 64 bytes too many."""
    s, w = fpm_amd.debug_plan_ladder(10240, 9, 1, True), fpm_amd.debug_plan_ladder(10240, 9, 1, False)
    assert (s["rows"]["lds_dynamic"], s["rows"]["lds_static"]) == (163840, 16)
    assert (w["cols"]["lds_dynamic"], w["cols"]["lds_static"]) == (163840, 64)
    assert s["cols"]["lds_dynamic"] + s["cols"]["lds_static"] == LDS_LIMIT


# ---- the table names what the planner picks --------------------------------------------
@pytest.mark.parametrize("row", ladder_cases.ROWS, ids=lambda r: r.name)
def test_rows_select_the_rungs_they_name(row):
    for switch, want in row.rungs.items():
        assert ladder_cases.planned_rungs(row, switch) == want, switch
        s = ladder_cases.plan(row, switch, True)
        if row.partial_rows:
            assert row.nb % (1 << s["rows"]["tile"]), switch
    x0, y0, order = row.geometry()
    assert len(order) == (2 if row.leds else 9)
    step = max(abs(int(x0[order[1]]) - int(x0[order[0]])), abs(int(y0[order[1]]) - int(y0[order[0]])))
    assert 0 < step < 2 * row.r       # neighbouring windows overlap
    idx = np.arange(row.B) % row.n_distinct     # row.stack()'s
    assert len({int(idx[b]) for b in row.sample}) == len(row.sample) == min(row.B, 3)


def test_lds_above_64k_rows():
    """The launches this table exists for, by their dynamic LDS bytes."""
    got = {r.name: (ladder_cases.plan(r, WAVE, True)["rows"]["lds_dynamic"],
                    ladder_cases.plan(r, WAVE, True)["cols"]["lds_dynamic"])
           for r in ladder_cases.ROWS if r.Np in (486, 600, 2916)}
    assert got == {"np486_B18": (36912, 66096), "np600_B16": (14784, 81600), "np2916_B1": (70176, 116640)}


# ---- coverage ----------------------------------------------------------------------
# Rungs the planner can select and no row runs, with the reason; at most two.
EXCLUDED = {
    # A 512-thread tile holds two columns from Np 3073 on (from 2561 with a radix-5 pass), and an fp64 oracle of
    # such a size costs more than the Np 2916 row, the yardstick.  lc 1 is the same instances <512,16> / <512,24>
    # with one more pass of the tile index: the step runs it at Np 2700 (test_gpu_parity.py
    # test_one_sequence_row_kernels_match_oracle), the sweep in test_gpu_residual.py test_one_sequence_rows_np2700.
    "two columns per block": lambda rung: rung[1:] == ("lc", 1),
}


def test_case_table_covers_the_reachable_rungs(sweep):
    reachable = set()
    for np_, nb, B, step, nw, one, rec in sweep:
        reachable |= ladder_cases.coverage(np_, nb, B, step, rec)
    covered = set()
    for row in ladder_cases.ROWS:
        for switch in row.rungs:
            for step in (True, False):
                covered |= ladder_cases.coverage(row.Np, row.nb, row.B, step, ladder_cases.plan(row, switch, step))
    assert len(EXCLUDED) <= 2
    excluded = {rung for rung in reachable if any(f(rung) for f in EXCLUDED.values())}
    for name, f in EXCLUDED.items():
        assert any(f(rung) for rung in reachable - covered), f"exclusion '{name}' excludes nothing"
    missing = reachable - covered - excluded
    assert not missing, sorted(missing, key=str)
    assert covered <= reachable
    # what the issue set out to reach
    for rung in (("step", "cols", "wave<4,2>"), ("sweep", "cols", "wave<4,2>"), ("step", "cols", "one_seq"),
                 ("step", "rows", "tiled<256,24>"), ("sweep", "rows", "tiled<256,24>"),
                 ("step", "cols", "tiled<512,24>"), ("sweep", "cols", "tiled<512,24>"),
                 ("step", "cols", "tiled<256,24>"), ("step", "lr", 4), ("step", "lc", 4),
                 ("step", "above 64 KiB", "rows"), ("step", "above 64 KiB", "cols"),
                 ("step", "partial column tile", "tiled<512,24>"), ("step", "partial column tile", "wave<4,2>")):
        assert rung in covered, rung


# ---- non-triviality ------------------------------------------------------------------
@pytest.mark.parametrize("row", ladder_cases.SMALL, ids=lambda r: r.name)
def test_fp32_headroom_and_distinct_patches(row):
    x0, y0, order = row.geometry()
    base = row.base_stack()
    nd = row.n_distinct
    ref = oracle_lib.run_fpm_batch(base, order, x0, y0, row.Np, row.L, row.r, 5, 10, row.iters, threads=min(nd, 4),
                                   pupil=True, objF=True)
    c64 = run_fpm(base[:, 0], order, x0, y0, row.Np, row.L, row.r, 5, 10, row.iters, dtype=np.complex64)
    drift = {k: rel_l2(c64[k], ref[k][0]) for k in ("objF", "objCrop", "pupil")}
    print(f"{row.name}: complex64 drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
    for k, v in drift.items():
        assert c64[k].dtype == np.complex64 and v < row.tol / 10, (k, v)
    for i, j in itertools.combinations(range(nd), 2):
        assert rel_l2(ref["objCrop"][i], ref["objCrop"][j]) > 1e-3, (i, j)
