"""The loader-preprocessing case tables without a GPU (tests/preprocess_cases.py).

Table check: every edge case reaches the branches it names and gives the
   bg_val and the pixels it names, computed twice -- by reach(), exact integer
   and rational arithmetic, and by fpm_oracle.preprocess_frame -- and the two
   agree bit for bit; together the cases reach every branch of BRANCHES.  A
   condition on the inputs, so the device tests need no measured number.
Host loader: the cases the dataset JSON can express (integer multiplier,
   integer threshold, one patch, darkfield from the LED's NA) through
   libfpm_host's Dataset.load_images(), stack and bg_val bit-exact.
Layout rows: the shapes, the frame sets and the loop counts the rows claim.
"""
import numpy as np
import pytest

import preprocess_cases as pc
from dataset_fixture import central_leds, make_case_dataset
from fpm_amd import host

# (case, Np) of every size a case runs at on the device
SIZES = sorted({(c.name, l.Np) for c, l in pc.edge_runs()})


@pytest.mark.parametrize("name,Np", SIZES, ids=[f"{n}-np{p}" for n, p in SIZES])
def test_case_reaches_what_it_names(name, Np):
    case = pc.CASE[name]
    row = next(l for c, l in pc.edge_runs() if c is case and l.Np == Np)
    inp = case.inputs(Np, row.n)
    counts, want, bgs = pc.reach(inp, Np)
    print(name, Np, {k: int(v) for k, v in counts.items() if v})
    for branch in case.reaches:
        assert branch in pc.BRANCHES
        assert counts[branch] > 0, branch
    o_want, o_bgs = pc.expected(inp, Np)
    np.testing.assert_array_equal(o_bgs, bgs)
    np.testing.assert_array_equal(o_want, want)
    if inp.bg_want is not None:
        assert tuple(int(b) for b in o_bgs) == inp.bg_want
    assert max(abs(int(b)) for b in o_bgs) <= 32767
    for (i, b, y, x, v) in inp.pins:
        assert int(o_want[i, b, y, x]) == v, (i, b, y, x)
    H, W = inp.frames.shape[1:]
    for (x, y) in inp.patches + (inp.bk1, inp.bk2):
        assert 0 <= x <= W - Np and 0 <= y <= H - Np
    assert inp.frames.dtype == np.uint16 and not inp.frames.flags.writeable


def test_named_values():
    """The values the cases are named after, as literals."""
    def bg(name, Np=32, n=9):
        return set(pc.expected(pc.CASE[name].inputs(Np, n), Np)[1].tolist())

    assert bg("bg_fraction_threshold") == {1000}
    assert bg("bg_negative_threshold") == {-7}
    assert bg("bg_negative_half_threshold") == {-8}     # std::round, half away from zero
    assert bg("bg_max_int16") == {32767}
    assert bg("bg_zero") == {0}
    assert bg("bg_at_threshold") == bg("bg_over_threshold") == {1500}
    for name, Np in (("bg_tie", 32), ("bg_tie", 64), ("bg_tie_nonpow2", 90)):
        inp = pc.CASE[name].inputs(Np, 9)
        for i, b in enumerate(pc.expected(inp, Np)[1]):
            s = sum(int(inp.frames[i, y:y + Np, x:x + Np].astype(np.int64).sum()) for x, y in (inp.bk1, inp.bk2))
            assert 2 * s == (2 * int(b) - 1) * 2 * Np * Np, (name, i)      # bg = bg_val - 0.5 exactly
    for name, mult, table in (("dark_tie_even", 2, {5: 2, 7: 4}), ("dark_tie_odd", 4, {6: 2, 10: 2, 14: 4})):
        inp = pc.CASE[name].inputs(32, 9)
        assert inp.dark_mult == mult
        i = int(np.flatnonzero(inp.darkfield)[0])
        x0, y0 = inp.patches[2]
        got = {int(inp.frames[i, y0 + y, x0 + x]): v for (f, b, y, x, v) in inp.pins if f == i}
        assert table.items() <= got.items()


def test_table_reaches_every_branch():
    total = set()
    for name, Np in SIZES:
        case = pc.CASE[name]
        assert set(case.reaches) <= set(pc.BRANCHES)
        total |= set(case.reaches)
    assert total == set(pc.BRANCHES)
    assert [c.name for c in pc.CASES if c.layouts == ("np1024",)] == ["sum_over_32_bits"]
    assert [c.name for c in pc.CASES if c.layouts == ("np90",)] == ["bg_tie_nonpow2"]
    assert all(c.layouts == pc.EDGE_LAYOUTS for c in pc.CASES if len(c.layouts) > 1)
    assert [pc.LAYOUT[l].Np for l in pc.EDGE_LAYOUTS] == [32, 90, 64]


# ---- host loader ---------------------------------------------------------------------
HOST_CASES = [(c.name, 90 if c.layouts == ("np90",) else 32) for c in pc.CASES if c.host]


def test_host_cases_are_the_expressible_ones():
    names = [n for n, _ in HOST_CASES]
    for must in ("dark_tie_even", "dark_tie_odd", "bg_tie", "bg_tie_nonpow2", "bg_negative_threshold",
                 "bg_max_int16", "windows_overlap", "frame_is_patch"):
        assert must in names
    for c in pc.CASES:
        inp = c.inputs(pc.LAYOUT[c.layouts[0]].Np, 4)
        # integer JSON keys, flags the NA can give; the Np 1024 frames (the host sums in double) are not written
        expressible = (float(inp.dark_mult).is_integer() and float(inp.bg_threshold).is_integer()
                       and set(inp.darkfield.tolist()) <= {0, 1} and inp.frames[0].size < 1 << 20)
        assert c.host == expressible, c.name
    leds, dark = central_leds()
    assert len(leds) == 8 and sum(dark.values()) == 4


@pytest.mark.parametrize("name,Np", HOST_CASES, ids=[n for n, _ in HOST_CASES])
def test_host_loader_matches_oracle(name, Np, tmp_path):
    ds = make_case_dataset(str(tmp_path), pc.CASE[name], Np)
    inp, nums = ds["inputs"], ds["leds"]
    d = host.Dataset(ds["json"])
    assert d.scan() == len(nums)
    n = d.geometry()
    assert n == len(nums)                   # every LED written is inside maxIlluminationNA
    assert d.load_images() == n
    cfg = d.config()
    assert cfg.np == Np and cfg.darkfield_exp_multiplier == inp.dark_mult and cfg.bg_threshold == inp.bg_threshold
    stack = d.stack()
    by_led = {l.led: l for l in d.leds()}
    order = d.order()
    assert sorted(order.tolist()) == nums
    want, bgs = pc.expected(inp, Np)
    for s, led in enumerate(order):
        j = nums.index(int(led))
        assert (by_led[led].illumination_na > cfg.objective_na) == ds["dark"][int(led)]
        if inp.dark_mult != 1:              # with multiplier 1 the flags decide nothing
            assert bool(inp.darkfield[j]) == ds["dark"][int(led)]
        np.testing.assert_array_equal(stack[s], want[j, 0], err_msg=f"LED {led}")
        assert by_led[led].bg_val == bgs[j], led


# ---- layout rows ---------------------------------------------------------------------
def test_layout_rows():
    rows = pc.LAYOUTS
    assert [r.id for r in rows] == ["small32", "small96", "small90", "np90", "np200", "np256", "reg256", "general64",
                                    "general320", "np1024"]
    assert [r.meas_g for r in rows] == [32, 96, 90, 9, 10, 16, 16, 0, 0, 1024]
    assert [r.crop_passes for r in rows] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 4]
    assert 320 % 256 != 0                   # general320: the second pass is partial
    for r in rows:
        r.problem()                         # the LED grid stays inside the spectrum
        assert (r.n, r.n_patch) == ((4, 2) if r.Np == 1024 else (9, 3))
        assert 2 * r.r + 1 <= r.Np
        H, W = pc.layout_shape(r.Np)
        assert (H, W) == (r.Np + 40, r.Np + 33) and (W % 2 == 1 or r.Np % 2 == 1)
    assert pc.LAYOUT["reg256"].r > 34 and not pc.LAYOUT["np1024"].solve


@pytest.mark.parametrize("row", [r for r in pc.LAYOUTS if r.Np <= 320], ids=lambda r: r.id)
def test_layout_frames_mix_every_branch(row):
    """Checked below Np 1024, whose frame set is built the same way."""
    inp = pc.layout_inputs(row.id)
    counts, want, bgs = pc.reach(inp, row.Np)
    o_want, o_bgs = pc.layout_expected(row.id)
    np.testing.assert_array_equal(o_bgs, bgs)
    np.testing.assert_array_equal(o_want, want)
    for branch in ("bg_clamped", "bg_unclamped", "dark_divides", "dark_passes", "dark_tie_even", "dark_tie_odd",
                   "sub_clamp_low", "patch_at_origin", "patch_at_far_corner"):
        assert counts[branch] > 0, branch
    assert inp.dark_mult == 2 and len(inp.patches) == row.n_patch
    # every image differs from every other: a permutation that mixes images up cannot pass
    flat = o_want.reshape(-1, row.Np * row.Np)
    assert len({f.tobytes() for f in flat}) == len(flat)
    assert (flat != 0).mean(axis=1).min() > 0.1      # the subtraction leaves every image something to permute
    # and no image is symmetric: a transpose left out or done twice cannot pass
    assert all(not np.array_equal(im, im.T) for im in o_want.reshape(-1, row.Np, row.Np))
