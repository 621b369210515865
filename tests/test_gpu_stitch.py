"""fpm_stitch_tiles / fpm_stitch (GPU only): overlapping tiles aligned and blended
into one field (include/fpm_hip.h; csrc/stitch.hip).  Cases, inputs and the
float64 restatement: tests/stitch_cases.py (tests/test_stitch_cases.py shows on
the CPU that the restatement is one).

Bounds, with u = 2^-24:
  factors  |f - f_ref| <= 1e-10 (|z| + sum |terms|) / |z| |f_ref|.  The products of
           fp32 values are exact in double; only the order of at most 2^20
           additions differs from the restatement's, each at 2^-53.  The sums'
           error is 1e-10 (|z| + sum |terms|) in the units of z; a factor is
           z / |z| (times a scale), so the same error divided by |z| and taken
           relative to |f_ref| is what can be asked of it.  |z| >> 1 in every
           case here, so this is tighter than applying 1e-10 (|z| + sum |terms|)
           to the factors as it stands.
  field    every pixel within 16 u sum_t w_t |f_t T_t| of the restatement: one
           fp32 complex multiply, one weight product and three additions per
           pixel; emulating the blend in fp32 on the CPU gives 3.1 u at worst
           over five of the eight grids, so 16 leaves a factor of five.
  truth    consistent tiles, complex alignment: truth / f_true[0] within the
           field's 16 u plus the rounding of the tiles and what it does to the
           factors, (3 + 6 (gy + gx - 2)) u (test_stitch_cases.py has the count).
"""
import functools
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import stitch_cases as sc
from fpm_amd import parallel
from test_gpu_residual import BIN

pytestmark = pytest.mark.gpu

INVAL, STATE = fpm_amd.FPM_ERR_INVAL, fpm_amd.FPM_ERR_STATE
U = 2.0 ** -24
FIELD_UNITS = 16


def _bits(a):
    """The 32-bit words of every element, [..., words]."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (-1,))


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _device(tiles, g, align):
    """The device path: a torch tensor on the GPU in, a torch tensor out."""
    import torch
    t = torch.tensor(np.asarray(tiles), device="cuda")
    field, fac = parallel.stitch_blend(t, (g[0], g[1]), (g[3], g[4]), align)
    assert field.is_cuda and field.dtype == torch.complex64
    return field.cpu().numpy(), fac


def _host(tiles, g, align):
    """The host path: a numpy array in, a numpy array out."""
    field, fac = parallel.stitch_blend(np.asarray(tiles), (g[0], g[1]), (g[3], g[4]), align)
    assert isinstance(field, np.ndarray)
    return field, fac


def _check_field(field, want, bound, units, what):
    err = np.abs(field.astype(np.complex128) - want)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max() / U)
    print(f"{what}: worst pixel {worst:.2f} u of {units}")
    assert np.isfinite(field.view(np.float32)).all(), what
    assert (err <= units * U * bound).all(), (what, worst)


# ---- factors and field ----------------------------------------------------------------------------
@pytest.mark.parametrize("align", sc.ALIGNS)
@pytest.mark.parametrize("kind", sorted(sc.INPUTS))
@pytest.mark.parametrize("name", sc.CASES)
def test_factors_and_field(name, kind, align):
    g = sc.CASES[name]
    inp = sc.INPUTS[kind](name)
    f_ref, cond, want, bound = sc.expected(name, kind, align)
    field, fac = _host(inp.tiles, g, align)
    field_d, fac_d = _device(inp.tiles, g, align)
    assert field.shape == sc.shape(*g) and field.dtype == np.complex64
    _same_bits(field, field_d, "host path against device path: field")
    _same_bits(fac.view(np.float64), fac_d.view(np.float64), "host path against device path: factors")
    err = np.abs(fac - f_ref)
    print(f"{name}/{kind}/{align}: factors off by at most {err.max():.3g}")
    assert (err <= 1e-10 * cond * np.abs(f_ref)).all(), (fac, f_ref)
    if align == "none":
        np.testing.assert_array_equal(fac, np.ones(g[0] * g[1]))
    assert fac[0] == 1
    _check_field(field, want, bound, FIELD_UNITS, f"{name}/{kind}/{align}")
    if kind == "consistent" and align == "complex":
        truth = inp.truth.astype(np.complex128) / inp.f_true[0]
        _check_field(field, truth, bound, FIELD_UNITS + 3 + 6 * (g[0] + g[1] - 2), f"{name}: truth")


# ---- placement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, g in sc.CASES.items() if g[3] == g[2] and g[4] == g[2]])
def test_stride_of_a_tile_is_placement(name):
    import torch
    g = sc.CASES[name]
    T = sc.independent(name).tiles.copy()
    T[0, 0, 0] = complex(-0.0, 5.0)        # a copy keeps the sign of a zero
    T[-1, 3, 5] = complex(np.inf, np.nan)  # and anything else a tile holds
    want = parallel.stitch(T, (g[0], g[1]))
    field, fac = _host(T, g, "none")
    _same_bits(field, want, "host path")
    np.testing.assert_array_equal(fac, np.ones(len(T)))
    t = torch.from_numpy(T).cuda()
    field_d, _ = parallel.stitch_blend(t, (g[0], g[1]), g[2])
    _same_bits(field_d.cpu().numpy(), parallel.stitch(t, (g[0], g[1])).cpu().numpy(), "device path")
    pairs = torch.view_as_real(t).contiguous()       # float32 [P, L, L, 2]: the gathered tiles' layout
    field_p, _ = parallel.stitch_blend(pairs, (g[0], g[1]), g[2])
    assert field_p.dtype == torch.float32 and tuple(field_p.shape) == want.shape + (2,)
    _same_bits(field_p.cpu().numpy(), parallel.stitch(pairs, (g[0], g[1])).cpu().numpy(), "device path, pairs")


@pytest.mark.parametrize("name", sc.CASES)
def test_pixels_under_one_tile_are_copies(name):
    gy, gx, L, sy, sx = g = sc.CASES[name]
    T = sc.independent(name).tiles.copy()
    T[0, 0, 0] = complex(-0.0, 5.0)
    placed = np.zeros(sc.shape(*g), np.complex64)
    for i in range(gy):
        for j in range(gx):
            placed[i * sy:i * sy + L, j * sx:j * sx + L] = T[i * gx + j]
    one = sc.cover_count(*g) == 1
    assert one[0, 0] and one.sum() > 0
    for path in (_host, _device):
        field, _ = path(T, g, "none")
        np.testing.assert_array_equal(_bits(field)[one], _bits(placed)[one], err_msg=path.__name__)


# ---- zero overlaps, determinism -------------------------------------------------------------------
@pytest.mark.parametrize("align", ["phase", "complex"])
def test_zero_overlaps_give_factor_one(align):
    name = "unequal_odd"
    gy, gx, L, sy, sx = g = sc.CASES[name]
    T = sc.independent(name).tiles.copy()
    T[4, :L - sy, :] = 0     # all that tile 4 shares with its upper
    T[4, :, :L - sx] = 0     # and with its left neighbour
    field, fac = _host(T, g, align)
    assert fac[4] == 1 and np.isfinite(fac.view(np.float64)).all()
    assert np.isfinite(field.view(np.float32)).all()
    f_ref = sc.factors(T, *g, align)
    assert f_ref[4] == 1
    want, bound = sc.blend(T, f_ref, *g)
    _check_field(field, want, bound, FIELD_UNITS, f"zeroed overlaps/{align}")
    Z = np.zeros_like(T)     # nothing to align on anywhere
    field, fac = _host(Z, g, align)
    np.testing.assert_array_equal(fac, np.ones(len(T)))
    assert not _bits(field).any()


@pytest.mark.parametrize("name", ["big_pairs", "unequal_odd"])
def test_two_calls_return_the_same_bits(name):
    g = sc.CASES[name]
    T = sc.independent(name).tiles
    for path in (_host, _device):
        a, fa = path(T, g, "complex")
        b, fb = path(T, g, "complex")
        _same_bits(a, b, path.__name__)
        _same_bits(fa.view(np.float64), fb.view(np.float64), path.__name__)


@pytest.mark.parametrize("name", ["big_pairs", "unequal_strides"])
def test_device_tiles_off_the_16_byte_grid(name):
    """Even geometry, but tiles (and a field) that start 8 bytes past a 16-byte address: the 8-byte paths of
    both kernels.  The blend is the same arithmetic per pixel, so without alignment the bits are the aligned
    call's; with it the sums add in another order and the result meets the same bounds."""
    import torch
    g = sc.CASES[name]
    T = sc.independent(name).tiles
    flat = torch.zeros(T.size + 1, dtype=torch.complex64, device="cuda")
    t = flat[1:].view(T.shape)
    t.copy_(torch.tensor(T))
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    field, _ = parallel.stitch_blend(t, (g[0], g[1]), (g[3], g[4]), "none")
    _same_bits(field.cpu().numpy(), _host(T, g, "none")[0], "8-byte path against 16-byte path")
    for align in ("phase", "complex"):
        f_ref, cond, want, bound = sc.expected(name, "independent", align)
        field, fac = parallel.stitch_blend(t, (g[0], g[1]), (g[3], g[4]), align)
        assert (np.abs(fac - f_ref) <= 1e-10 * cond * np.abs(f_ref)).all()
        _check_field(field.cpu().numpy(), want, bound, FIELD_UNITS, f"{name}/unaligned/{align}")
    H, W = sc.shape(*g)
    out = torch.zeros(H * W + 1, dtype=torch.complex64, device="cuda")
    dst = out[1:].view(H, W)
    aligned = torch.tensor(T, device="cuda")
    fpm_amd.stitch_tiles_device(aligned.data_ptr(), dst.data_ptr(), (g[0], g[1]), g[2], (g[3], g[4]), "none")
    _same_bits(dst.cpu().numpy(), _host(T, g, "none")[0], "a field off the 16-byte grid")
    assert out[0].item() == 0


# ---- the context form -----------------------------------------------------------------------------
CTX = dict(Np=32, L=96, r=6, B=4)
CTX_GRID, CTX_STRIDE = (2, 2), (72, 80)


@functools.lru_cache(maxsize=None)
def _ctx_inputs():
    from tools.synth import grid_geometry, make_stack
    x0, y0, order = grid_geometry(CTX["Np"], CTX["L"], 5, 4)
    stack = make_stack(CTX["Np"], CTX["L"], CTX["r"], x0, y0, n_patch=CTX["B"], seed=11)
    stack.setflags(write=False)
    return x0, y0, order, stack


def _ctx(path, kernel, run=True):
    x0, y0, order, stack = _ctx_inputs()
    s = fpm_amd.Solver(fpm_amd.Problem(CTX["Np"], CTX["L"], order, x0, y0, CTX["r"], 5, 10, n_patch=CTX["B"], path=path))
    try:
        assert s.info().fused_kernel == kernel, s.info().fused_kernel
        s.upload(stack)
        if run:
            s.init()
            s.run(2)
    except BaseException:
        s.close()
        raise
    return s


KERNELS = [(fpm_amd.PATH_AUTO, fpm_amd.KERNEL_FUSED_SMALL), (fpm_amd.PATH_GENERAL, fpm_amd.KERNEL_GENERAL)]


def _snapshot(s):
    return s.download(), s.debug_maxima()


def _assert_unchanged(a, b, what):
    (da, ma), (db, mb) = a, b
    for k in ("objF", "objCrop", "pupil", "support"):
        _same_bits(da[k], db[k], f"{what}: {k}")
    for k in ("tmax", "dirty", "pmax", "rmax"):
        if ma[k] is not None:
            np.testing.assert_array_equal(ma[k], mb[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("path,kernel", KERNELS)
def test_context_form(path, kernel):
    import torch
    H, W = fpm_amd.stitch_shape(CTX_GRID, CTX["L"], CTX_STRIDE)
    with _ctx(path, kernel) as s:
        before = _snapshot(s)
        timing, clock = s.timing(), s.clock()
        nbytes = s.info().device_bytes
        tiles = before[0]["objCrop"]
        for align in sc.ALIGNS:
            field, fac = s.stitch(CTX_GRID, CTX_STRIDE, align)
            want, fac_want = fpm_amd.stitch_tiles(tiles, CTX_GRID, CTX_STRIDE, align)
            assert field.shape == (H, W)
            _same_bits(field, want, f"Solver.stitch against stitch_tiles of the download, {align}")
            _same_bits(fac.view(np.float64), fac_want.view(np.float64), f"factors, {align}")
            out = torch.zeros((H, W), dtype=torch.complex64, device="cuda")
            none, fac_d = s.stitch(CTX_GRID, CTX_STRIDE, align, device_ptr=out.data_ptr())
            assert none is None
            _same_bits(out.cpu().numpy(), want, f"field in device memory, {align}")
            _same_bits(fac_d.view(np.float64), fac_want.view(np.float64), f"factors, device field, {align}")
        _assert_unchanged(before, _snapshot(s), "after stitch")
        assert s.info().device_bytes == nbytes
        for a, b in ((timing, s.timing()), (clock, s.clock())):
            assert [getattr(a, n) for n, _ in a._fields_] == [getattr(b, n) for n, _ in b._fields_]

        with pytest.raises(fpm_amd.FpmError) as ei:
            s.stitch((2, 3), CTX_STRIDE)
        assert ei.value.code == INVAL and "gy*gx" in str(ei.value)
        g = fpm_amd.fpm_stitch_grid(2, 2, CTX["L"] - 2, 72, 80)
        buf = np.empty((H, W), np.complex64)
        rc = fpm_amd.load_library().fpm_stitch(s._h, g, 0, buf.ctypes.data, None, None)
        assert rc == INVAL and "tile" in fpm_amd.load_library().fpm_last_error().decode()

        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        # A torch CUDAGraph's destructor calls HIP, which a capturing stream forbids (the process
        # aborts), and the pytest.raises below leaves the graph in a reference cycle that only the
        # collector frees: nothing may be collected while this stream captures, and this test's
        # own graph goes before the next capture anywhere.
        gc.collect()
        graph = torch.cuda.CUDAGraph()
        gc.disable()
        try:
            with pytest.raises(fpm_amd.FpmError) as ei:
                with torch.cuda.graph(graph, stream=cs, capture_error_mode="relaxed"):
                    s.stitch(CTX_GRID, CTX_STRIDE, "phase")
            code, msg = ei.value.code, str(ei.value)
        finally:
            gc.enable()
        del ei, graph
        gc.collect()
        assert code == INVAL and "capturing" in msg
        s.set_stream(None)
        _assert_unchanged(before, _snapshot(s), "after a capturing stream")


@pytest.mark.parametrize("path,kernel", KERNELS)
def test_context_form_is_refused_before_init(path, kernel):
    with _ctx(path, kernel, run=False) as s:
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.stitch(CTX_GRID, CTX_STRIDE)
        assert ei.value.code == STATE
        s.init()
        field, fac = s.stitch(CTX_GRID, CTX_STRIDE, "phase")   # after init a state exists
        assert np.isfinite(field.view(np.float32)).all() and fac[0] == 1


# ---- refusals -------------------------------------------------------------------------------------
def _raw(grid, flags=0, tiles=True, field=True):
    """fpm_stitch_tiles through ctypes with host buffers large enough for any accepted grid here."""
    lib = fpm_amd.load_library()
    t = np.zeros((9, 40, 40), np.complex64)
    f = np.zeros((120, 120), np.complex64)
    g = None if grid is None else fpm_amd.fpm_stitch_grid(*grid)
    rc = lib.fpm_stitch_tiles(0, t.ctypes.data if tiles else None, g, flags, f.ctypes.data if field else None, None,
                              None, None)
    return rc, lib.fpm_last_error().decode()


@pytest.mark.parametrize("what,kw,word", [
    ("a NULL grid", dict(grid=None), "grid"),
    ("NULL tiles", dict(grid=(2, 2, 32, 20, 20), tiles=False), "tiles"),
    ("a NULL field", dict(grid=(2, 2, 32, 20, 20), field=False), "field"),
    ("gy < 1", dict(grid=(0, 2, 32, 20, 20)), "gy"),
    ("gx < 1", dict(grid=(2, -1, 32, 20, 20)), "gx"),
    ("tile < 2", dict(grid=(2, 2, 1, 1, 1)), "tile"),
    ("stride_y below ceil(L/2)", dict(grid=(2, 2, 33, 16, 20)), "stride_y"),
    ("stride_y above L", dict(grid=(2, 2, 32, 33, 20)), "stride_y"),
    ("stride_x below ceil(L/2)", dict(grid=(2, 2, 32, 20, 15)), "stride_x"),
    ("stride_x above L", dict(grid=(2, 2, 32, 20, 33)), "stride_x"),
    ("both align flags", dict(grid=(2, 2, 32, 20, 20), flags=3), "FPM_STITCH_ALIGN_PHASE"),
    ("an unknown flag", dict(grid=(2, 2, 32, 20, 20), flags=8), "flags"),
    ("more tiles than the launches index", dict(grid=(1, 20000, 32, 20, 20)), "gy*gx"),
])
def test_refusals(what, kw, word):
    rc, msg = _raw(**kw)
    assert rc == INVAL, (what, rc, msg)
    assert word in msg and "fpm_stitch_tiles" in msg, (what, msg)


def test_limits_of_the_stride_are_accepted():
    for grid in ((2, 2, 33, 17, 33), (2, 2, 32, 16, 32)):
        rc, msg = _raw(grid=grid)
        assert rc == 0, (grid, msg)
    with pytest.raises(ValueError):
        fpm_amd.stitch_tiles(np.zeros((4, 8, 8), np.complex64), (2, 2), 6, align="tilt")


# ---- the CLI --------------------------------------------------------------------------------------
OVERLAP = 8


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """fpmMain --grid 2x2 --overlap 8 --write-tiles on the dataset_fixture dataset, without alignment and
    with the default one, and the oracle's tile of every patch."""
    from dataset_fixture import make_dataset
    from fpm_amd import host
    from fpm_oracle import run_fpm
    tmp = tmp_path_factory.mktemp("stitch_cli")
    ds = make_dataset(str(tmp / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    runs = {}
    for tag, extra in (("none", ["--stitch-align", "none"]), ("default", [])):
        out = tmp / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], "2", "--out", str(out), "--grid", "2x2", "--overlap", str(OVERLAP),
                            "--write-tiles", *extra], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = dict(meta=json.loads((out / "result.json").read_text()), field=np.load(out / "objCrop_field.npy"),
                         tiles=np.load(out / "objCrop_tiles.npy"), pupils=np.load(out / "pupils.npy"))
    k = ds["keys"]
    Np = k["cropSizeX"]
    oracle = []
    for b in range(4):
        i, j = divmod(b, 2)
        d = host.Dataset(ds["json"])
        d.override("cropX", k["cropX"] + j * (Np - OVERLAP))
        d.override("cropY", k["cropY"] + i * (Np - OVERLAP))
        d.scan()
        n = d.geometry()
        d.load_images()
        cfg = d.config()
        x0, y0 = d.crops()
        oracle.append(run_fpm(d.stack(), np.arange(n), x0, y0, cfg.np, cfg.nlarge, cfg.na_radius, cfg.delta1,
                              cfg.delta2, 2)["objCrop"])
    return dict(runs=runs, oracle=np.stack(oracle), Np=Np)


def _cli_grid(meta, Np):
    L = meta["nlarge"]
    stride = (Np - OVERLAP) * (L // Np)
    return (2, 2, L, stride, stride)


def test_cli_without_alignment(cli):
    from fpm_oracle import rel_l2
    run, Np = cli["runs"]["none"], cli["Np"]
    meta, field, tiles = run["meta"], run["field"], run["tiles"]
    g = _cli_grid(meta, Np)
    L, stride = g[2], g[3]
    st = meta["stitch"]
    assert st["overlap"] == OVERLAP and st["stride"] == stride and st["align"] == "none"
    assert st["field"] == [stride + L, stride + L] and st["stitch_ms"] > 0
    assert st["factors"] == [[1, 0]] * 4
    assert meta["grid"]["patch_step"] == Np - OVERLAP
    assert field.shape == (stride + L, stride + L) and field.dtype == np.complex64
    assert tiles.shape == (4, L, L) and tiles.dtype == np.complex64
    want, bound = sc.blend(tiles, np.ones(4), *g)
    _check_field(field, want, bound, FIELD_UNITS, "CLI field against the blend of the written tiles")
    for b in range(4):
        assert rel_l2(tiles[b], cli["oracle"][b]) < 5e-5, b
    ref, _ = sc.blend(cli["oracle"], np.ones(4), *g)
    assert rel_l2(field, ref) < 1e-4


def test_cli_default_alignment(cli):
    run, Np = cli["runs"]["default"], cli["Np"]
    meta, field, tiles = run["meta"], run["field"], run["tiles"]
    g = _cli_grid(meta, Np)
    st = meta["stitch"]
    assert st["align"] == "phase" and len(st["factors"]) == 4 and st["factors"][0] == [1, 0]
    fac = np.array([complex(re, im) for re, im in st["factors"]])
    np.testing.assert_allclose(np.abs(fac), 1, rtol=0, atol=1e-12)
    f_ref, cond = sc.solve(sc.pair_sums(tiles, *g), g[0], g[1], "phase")
    assert (np.abs(fac - f_ref) <= 1e-10 * cond * np.abs(f_ref)).all()
    want, bound = sc.blend(tiles, fac, *g)
    _check_field(field, want, bound, FIELD_UNITS, "CLI field against the blend of the written tiles and factors")
    _same_bits(tiles, cli["runs"]["none"]["tiles"], "the tiles do not depend on the alignment")
