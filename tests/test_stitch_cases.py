"""tests/stitch_cases.py is what it claims (CPU only): the restated weights sum
to one, consistent tiles come back as truth / f_true[0], stride L without
alignment is parallel.stitch, the library's host factor solve
(csrc/stitch_solve.hpp, built stand-alone under ASan + UBSan) agrees with the
restatement, and fpmMain refuses misuse of --overlap / --stitch-align before
any device use.
"""
import os
import subprocess

import numpy as np
import pytest

import stitch_cases as sc
from dataset_fixture import make_dataset
from fpm_amd import parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")
MODE = {"none": 0, "phase": 1, "complex": 2}


@pytest.mark.parametrize("name", sc.CASES)
def test_case_geometry_is_in_contract(name):
    gy, gx, L, sy, sx = sc.CASES[name]
    assert gy >= 1 and gx >= 1 and L >= 2
    assert (L + 1) // 2 <= sy <= L and (L + 1) // 2 <= sx <= L
    n = sc.cover_count(gy, gx, L, sy, sx)
    assert n.min() >= 1 and n.max() <= (2 if gy > 1 and sy < L else 1) * (2 if gx > 1 and sx < L else 1)


@pytest.mark.parametrize("name", sc.CASES)
def test_weights_sum_to_one(name):
    g = sc.CASES[name]
    ones = np.ones((g[0] * g[1], g[2], g[2]), np.complex64)
    total, bound = sc.blend(ones, np.ones(g[0] * g[1]), *g)
    assert np.abs(total - 1).max() <= 1e-14
    assert np.abs(bound - 1).max() <= 1e-14
    for i in range(g[0]):
        for j in range(g[1]):
            w = sc.tile_weights(i, j, *g)
            assert w.min() > 0 and w.max() <= 1


@pytest.mark.parametrize("align", ["phase", "complex"])
@pytest.mark.parametrize("name", sc.CASES)
def test_consistent_tiles_return_the_truth(name, align):
    """Tiles cut from one field and divided by f_true: complex alignment undoes
    phase and scale, phase alignment the phase (so it is tested on tiles whose
    scales are all 1).  With u = 2^-24: a tile value is the fp32 rounding of
    truth / f_true, off by at most sqrt(2) u of its magnitude, so a pair's c, a
    and b are off by at most 2 sqrt(2) u relatively, a factor's ratio to its
    neighbours' by twice that (phase and scale), 6 u, and a factor by 6 u per
    link of its chain to tile 0, at most gy + gx - 2 links.  The field adds the
    tile's own rounding and the rounding of the factor to complex64, 1.5 u each."""
    gy, gx, L, sy, sx = sc.CASES[name]
    inp = sc.consistent(name)
    ft, T = inp.f_true, inp.tiles
    if align == "phase":
        ft = ft / np.abs(ft)
        T = np.stack([(inp.truth[i * sy:i * sy + L, j * sx:j * sx + L] / ft[i * gx + j]).astype(np.complex64)
                      for i in range(gy) for j in range(gx)])
    u, links = 2.0 ** -24, gy + gx - 2
    f = sc.factors(T, gy, gx, L, sy, sx, align)
    want = ft / ft[0]
    assert (np.abs(f - want) <= 6 * links * u * np.abs(want)).all()
    field, _ = sc.blend(T, f, gy, gx, L, sy, sx)
    truth = inp.truth.astype(np.complex128) / ft[0]
    assert (np.abs(field - truth) <= (3 + 6 * links) * u * np.abs(truth)).all()


def test_phases_cover_the_circle():
    ang = np.concatenate([np.angle(sc.consistent(n).f_true) for n in sc.CASES])
    mag = np.concatenate([np.abs(sc.consistent(n).f_true) for n in sc.CASES])
    assert ang.min() < -2.5 and ang.max() > 2.5 and 0.5 <= mag.min() < 0.7 and 1.6 < mag.max() <= 2.0


@pytest.mark.parametrize("name", [n for n, g in sc.CASES.items() if g[3] == g[2] and g[4] == g[2]])
def test_stride_of_a_tile_is_placement(name):
    gy, gx, L, sy, sx = sc.CASES[name]
    T = sc.independent(name).tiles
    field, _ = sc.blend(T, sc.factors(T, gy, gx, L, sy, sx, "none"), gy, gx, L, sy, sx)
    np.testing.assert_array_equal(field.astype(np.complex64), parallel.stitch(T, (gy, gx)))


def test_zero_overlap_gives_factor_one():
    name = "unequal_odd"
    gy, gx, L, sy, sx = sc.CASES[name]
    T = sc.independent(name).tiles.copy()
    T[4, :L - sy, :] = 0
    T[4, :, :L - sx] = 0
    f = sc.factors(T, gy, gx, L, sy, sx, "complex")
    assert f[4] == 1 and np.isfinite(f).all()


# ---- the library's host solve, stand-alone under the sanitizers -----------------------------------
@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    # the sanitizer runtimes are linked statically: the program then runs whatever the environment
    # preloads (a shared ASan runtime insists on being the first library loaded)
    out = str(tmp_path_factory.mktemp("stitch") / "stitch_solve_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "shim", "stitch_solve_main.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


def _pair_lines(sums, gy, gx):
    """pair_sums' dict in the library's pair order: left/right pairs row-major by
    their right tile, then up/down pairs row-major by their lower tile."""
    keys = [(i * gx + j - 1, i * gx + j) for i in range(gy) for j in range(1, gx)]
    keys += [((i - 1) * gx + j, i * gx + j) for i in range(1, gy) for j in range(gx)]
    assert sorted(keys) == sorted(sums)
    return "".join(f"{sums[k][0].real!r} {sums[k][0].imag!r} {sums[k][1]!r} {sums[k][2]!r}\n" for k in keys)


def _solve(solver, gy, gx, align, sums):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([solver], input=f"{gy} {gx} {MODE[align]}\n" + _pair_lines(sums, gy, gx), capture_output=True,
                       text=True, env=env, timeout=60)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    v = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert v.shape == (gy * gx, 2)
    return v[:, 0] + 1j * v[:, 1]


@pytest.mark.parametrize("kind", sorted(sc.INPUTS))
@pytest.mark.parametrize("name", sc.CASES)
def test_host_solve_matches_restatement(solver, name, kind):
    gy, gx, L, sy, sx = sc.CASES[name]
    sums = {k: (complex(c), float(a), float(b))
            for k, (c, a, b) in sc.pair_sums(sc.INPUTS[kind](name).tiles, gy, gx, L, sy, sx).items()}
    for align in sc.ALIGNS:
        got = _solve(solver, gy, gx, align, sums)
        want, _ = sc.solve(sums, gy, gx, align)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (align, got, want)


def test_host_solve_zero_sums_give_one(solver):
    sums = {(0, 1): (0j, 0.0, 0.0), (0, 2): (1 + 1j, 2.0, 0.0), (1, 3): (0j, 1.0, 1.0), (2, 3): (0j, 1.0, 1.0)}
    for align in ("phase", "complex"):
        got = _solve(solver, 2, 2, align, sums)
        want, _ = sc.solve(sums, 2, 2, align)
        np.testing.assert_array_equal(got[[0, 1, 3]], np.ones(3))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- the CLI refuses misuse before any device use -------------------------------------------------
def _cli(args):
    e = dict(os.environ)
    e.pop("OPENCV_OPENCL_DEVICE", None)
    # no device is visible to the process: a refusal that came after device use would not be exit 2
    e.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN] + args, capture_output=True, text=True, env=e, timeout=300)


def test_cli_overlap_needs_grid(tmp_path):
    r = _cli([str(tmp_path / "missing.json"), "1", "--overlap", "8"])
    assert r.returncode == 2 and "--grid" in r.stderr, (r.stdout, r.stderr)


def test_cli_stitch_align_needs_overlap(tmp_path):
    r = _cli([str(tmp_path / "missing.json"), "1", "--grid", "2x2", "--stitch-align", "phase"])
    assert r.returncode == 2 and "--overlap" in r.stderr, (r.stdout, r.stderr)


def test_cli_overlap_above_half_a_patch_is_refused(tmp_path):
    ds = make_dataset(str(tmp_path / "data"), leds=range(1, 4))
    half = ds["keys"]["cropSizeX"] // 2
    r = _cli([ds["json"], "1", "--grid", "2x2", "--overlap", str(half + 1)])
    assert r.returncode == 2 and "Np/2" in r.stderr, (r.stdout, r.stderr)
    assert "Loading Images" not in r.stdout
