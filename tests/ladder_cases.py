"""Case table of the kernel-ladder tests: plain data and builders, no GPU.

The general path (csrc/general.hip) runs any Np = 2^a 3^b 5^c through a ladder
of kernel generations -- one sequence per block, row tiles of 2^lr box rows,
column tiles of 2^lc columns on 256 or 512 threads with 16 or 24 register
elements per thread, wave-private columns -- and plan_lds_ladder picks the
rung from (Np, nb, B) alone.  The update step shrinks its tiles until the grid
has 512 blocks, so a suite of 1-5 patches only ever meets the smallest tiles.
One row here per geometry that selects another rung, each the smallest found
for it; tests/test_ladder.py (CPU) checks through fpm_debug_plan_ladder that
every row selects the rung it names and that the rows together cover what the
planner can select, and tests/test_gpu_ladder.py runs the table on the device.

A rung is named as the kernels are: "tiled<256,24> lr 4", "wave<4,2>",
"tiled<512,24> lc 4", "one_seq".

Every row: a 3 x 3 centred LED grid whose step is the radius (neighbouring
windows overlap, every window carries signal), two iterations, delta1 5 /
delta2 10, and a stack of n_distinct forward-model patches tiled to B
(patch b = base[b % n_distinct]), n_distinct a prime that keeps the sampled
patches -- first, last, one between -- distinct.  Np 2916 is the exception: the
two LEDs and the single iteration of test_one_sequence_row_kernels_match_oracle
(Np 2700), at the smallest size above it whose row tile (70 176 B) and column
tile (116 640 B) both pass 64 KiB.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fpm_amd
from tools.synth import grid_geometry, make_stack

WAVE, NO_WAVE, ONE_SEQ = "default", "FPM_NO_WAVE_COLS", "FPM_ONE_SEQ"
# environment at fpm_create of each switch setting; ONE_SEQ sets the sweep's twin
# too, so the row runs the one-sequence kernels for both argument types
ENV = {WAVE: {}, NO_WAVE: {"FPM_NO_WAVE_COLS": "1"}, ONE_SEQ: {"FPM_ONE_SEQ": "1", "FPM_RES_ONE_SEQ": "1"}}


@dataclass(frozen=True)
class LadderRow:
    Np: int
    L: int
    r: int
    B: int
    # per switch setting: (step rows, step columns, sweep rows, sweep columns) as fpm_debug_plan_ladder names them
    rungs: dict
    partial_rows: bool          # nb is no multiple of the step's row tile
    iters: int = 2
    leds: tuple = ()            # ((x0...), (y0...), order) when not the 3 x 3 grid
    seed: int = 0

    @property
    def name(self):
        return f"np{self.Np}_B{self.B}"

    @property
    def nb(self):
        return 2 * self.r + 1

    @property
    def tol(self):
        """The project's parity bound."""
        return 1e-5 if self.iters <= 1 else 5e-5

    def geometry(self):
        if self.leds:
            x0, y0, order = self.leds
            return np.array(x0), np.array(y0), list(order)
        return grid_geometry(self.Np, self.L, 3, self.r)

    @property
    def n_distinct(self):
        """The smallest prime number of distinct patches for which the sampled
        patches read three different base patches."""
        return self._sampling()[0]

    @property
    def sample(self):
        """First, last and one between (the middle one, or the next that reads a third base patch)."""
        return self._sampling()[1]

    def _sampling(self):
        if self.B <= 3:
            return self.B, tuple(range(self.B))
        for p in (3, 5, 7):
            for mid in range(self.B // 2, self.B - 1):
                if len({0, mid % p, (self.B - 1) % p}) == 3:
                    return p, (0, mid, self.B - 1)
        raise AssertionError(self.B)

    def problem(self):
        x0, y0, order = self.geometry()
        return fpm_amd.Problem(self.Np, self.L, order, x0, y0, self.r, 5, 10, n_patch=self.B,
                               path=fpm_amd.PATH_GENERAL)

    def base_stack(self):
        """uint16 [n_led][n_distinct][Np][Np], read-only: the distinct patches."""
        return _base_stack(self.name)

    def stack(self):
        """The B-patch stack and idx: patch b holds base patch idx[b]."""
        idx = np.arange(self.B) % self.n_distinct
        return self.base_stack()[:, idx], idx


@functools.lru_cache(maxsize=2)
def _base_stack(name):
    row = BY_NAME[name]
    x0, y0, _ = row.geometry()
    st = make_stack(row.Np, row.L, row.r, x0, y0, n_patch=row.n_distinct, seed=7000 + row.Np + row.seed)
    st.setflags(write=False)
    return st


def _np32(B, lr):
    t = f"tiled<256,16> lr {lr}"
    return LadderRow(32, 96, 15, B, {
        WAVE: (t, "wave<4,4>", "tiled<256,16> lr 4", "wave<4,4>"),
        NO_WAVE: (t, f"tiled<256,16> lc {lr}", "tiled<256,16> lr 4", "tiled<256,16> lc 4")}, partial_rows=True)


ROWS = (
    # nb 31: the last row tile is partial at every lr; the step's tiles grow with B
    _np32(64, 2), _np32(128, 3), _np32(256, 4),
    # Np 40 = 16 * 2 + 8: the wave kernel's last block and the tiled kernel's last tile hold 8 of 16 columns
    LadderRow(40, 120, 19, 256, {
        WAVE: ("tiled<256,16> lr 4", "wave<4,4>", "tiled<256,16> lr 4", "wave<4,4>"),
        NO_WAVE: ("tiled<256,16> lr 4", "tiled<256,16> lc 4", "tiled<256,16> lr 4", "tiled<256,16> lc 4")},
        partial_rows=True),
    # radix 5 with E = 24: 4 butterflies of 5 per thread; 250 = 8 * 31 + 2 = 16 * 15 + 10
    LadderRow(250, 500, 60, 64, {
        WAVE: ("tiled<256,24> lr 4", "wave<4,2>", "tiled<256,24> lr 4", "wave<4,2>"),
        NO_WAVE: ("tiled<256,24> lr 4", "tiled<256,24> lc 4", "tiled<256,24> lr 4", "tiled<256,24> lc 4")},
        partial_rows=True),
    # 360 = 8 * 45: full wave blocks; 16 * 22 + 8 on 512 threads
    LadderRow(360, 720, 40, 24, {
        WAVE: ("tiled<256,16> lr 1", "wave<4,2>", "tiled<256,16> lr 3", "wave<4,2>"),
        NO_WAVE: ("tiled<256,16> lr 1", "tiled<512,16> lc 4", "tiled<256,16> lr 3", "tiled<512,16> lc 4")},
        partial_rows=True),
    # the narrowest launch above 64 KiB of dynamic LDS: 66 096 B (486 = 16 * 30 + 6)
    LadderRow(486, 972, 120, 18, {
        WAVE: ("tiled<256,24> lr 3", "tiled<512,24> lc 4", "tiled<256,24> lr 3", "tiled<512,24> lc 4")},
        partial_rows=True),
    # what a realistic size picks on its own: 81 600 B (600 = 16 * 37 + 8)
    LadderRow(600, 750, 50, 16, {
        WAVE: ("tiled<256,16> lr 1", "tiled<512,24> lc 4", "tiled<256,24> lr 3", "tiled<512,24> lc 4")},
        partial_rows=True),
    # the sweep's middle tiles, which no batch size moves: 4 rows, 8 columns per block (Np 769 .. 1536)
    LadderRow(800, 1000, 20, 1, {
        WAVE: ("tiled<256,16> lr 1", "tiled<256,16> lc 2", "tiled<256,16> lr 2", "tiled<512,16> lc 3")},
        partial_rows=True),
    # rows 70 176 B, columns 116 640 B
    LadderRow(2916, 3000, 4, 1, {
        WAVE: ("tiled<256,24> lr 1", "tiled<512,24> lc 2", "tiled<256,24> lr 1", "tiled<512,24> lc 2")},
        partial_rows=True, iters=1, leds=((42, 36), (42, 42), (0, 1))),
    # k_gather_rowifft / k_colpass / k_rowfft_update, which sizes take on their own only past Np 2560
    LadderRow(30, 90, 5, 2, {ONE_SEQ: ("one_seq", "one_seq", "one_seq", "one_seq")}, partial_rows=False),
)
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# rows whose complex64 drift test_ladder.py measures (a 3000^2 complex64 run is not paid for)
SMALL = tuple(r for r in ROWS if r.Np <= 800)


# ---- naming what fpm_debug_plan_ladder returns ---------------------------------------
def rung_name(k, axis):
    """axis 'lr' (rows) or 'lc' (columns); k one kernel of fpm_amd.debug_plan_ladder()."""
    if k["generation"] == fpm_amd.LADDER_ONE_SEQ:
        return "one_seq"
    if k["generation"] == fpm_amd.LADDER_WAVE:
        return f"wave<{k['threads'] // 64},{k['tile']}>"
    return f"tiled<{k['threads']},{k['e']}> {axis} {k['tile']}"


def plan(row, switch, step):
    """The planner's record for the row under a switch setting."""
    one = switch == ONE_SEQ
    return fpm_amd.debug_plan_ladder(row.Np, row.nb, row.B, step=step, no_wave_cols=switch == NO_WAVE, one_seq=one)


def planned_rungs(row, switch):
    s, w = plan(row, switch, True), plan(row, switch, False)
    return (rung_name(s["rows"], "lr"), rung_name(s["cols"], "lc"), rung_name(w["rows"], "lr"),
            rung_name(w["cols"], "lc"))


def columns_per_block(k):
    """Columns a block of the column kernel holds."""
    if k["generation"] == fpm_amd.LADDER_ONE_SEQ:
        return 1
    if k["generation"] == fpm_amd.LADDER_WAVE:
        return k["threads"] // 64 * k["tile"]
    return 1 << k["tile"]


def coverage(np_, nb, B, step, rec):
    """The rungs one planner record exercises, as hashable names: the kernel
    instance and the tile size per argument type, a partial last column tile
    per column-kernel instance, and the step's tiled launches above 64 KiB."""
    a = "step" if step else "sweep"
    rows, cols = rec["rows"], rec["cols"]
    rn, cn = rung_name(rows, "lr"), rung_name(cols, "lc")
    out = {(a, "rows", rn.split(" lr")[0]), (a, "cols", cn.split(" lc")[0]), (a, "lr", rows["tile"] if rows["e"] else 0)}
    if cols["generation"] != fpm_amd.LADDER_WAVE:
        out.add((a, "lc", cols["tile"]))
    if cols["generation"] != fpm_amd.LADDER_ONE_SEQ and np_ % columns_per_block(cols):
        out.add((a, "partial column tile", cn.split(" lc")[0]))
    if step:
        for axis, k in (("rows", rows), ("cols", cols)):
            if k["generation"] == fpm_amd.LADDER_TILED and k["lds_dynamic"] > 64 * 1024:
                out.add((a, "above 64 KiB", axis))
    return out
