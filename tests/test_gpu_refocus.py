"""fpm_refocus: the field of the current state propagated to other z planes by
the angular-spectrum method (k_refocus_mul in front of the context's own
objCrop transform) and the three focus sums of every plane (k_refocus_sums and
its fold), csrc/refocus.hip.

The yardstick, the bounds and their derivation are tests/refocus_check.py's: a
float64 numpy evaluation of the DOWNLOADED objF, so both sides read the same
fp32 state, and the sums evaluated in float64 on the GPU's own plane.  States
are installed with set_state: N(0,1) spectra inside the live band (exact fp16 /
hscale on fp16 contexts), pupil all ones.  The measured ratios to the bounds
are printed (pytest -s).
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import fpm_amd
import objcrop_cases
import refocus_check as rc
from fpm_amd import focus
from tools.synth import grid_geometry, make_stack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")


def _solver(cid, B, seed):
    """A context of objcrop_cases.CONTEXTS[cid] at B patches with a random state
    installed; returns (solver, prob, downloaded objF)."""
    prob, ctx = rc.context_problem(cid, B)
    s = fpm_amd.Solver(prob)
    try:
        assert s.debug_band() == rc.band_of(prob)   # the yardstick's band is the context's
        objF, pupil = rc.random_state(prob, ctx, s.debug_band(), seed)
        s.set_state(objF, pupil)
        got = s.download(objCrop=False, pupil=False, support=False)["objF"]
        if not ctx.fp16:
            np.testing.assert_array_equal(got, objF)
        return s, prob, got
    except BaseException:
        s.close()
        raise


def _raw(s, zl, fl, margin, want=(True, True, True), planes=False, flags=0):
    """fpm_refocus through ctypes with any subset of the sum pointers."""
    p = s.prob
    z = np.ascontiguousarray(zl, np.float64)
    nz = z.shape[0]
    dp = C.POINTER(C.c_double)
    out = [np.full((nz, p.n_patch), np.nan) if w else None for w in want]
    pl = np.empty((nz, p.n_patch, p.L, p.L), np.complex64) if planes else None
    rcode = fpm_amd._lib.fpm_refocus(s._h, z.ctypes.data_as(dp), nz, float(fl), int(margin), flags,
                                     None if pl is None else pl.ctypes.data_as(C.c_void_p),
                                     *(None if a is None else a.ctypes.data_as(dp) for a in out), None)
    assert rcode == 0, fpm_amd._lib.fpm_last_error().decode()
    return pl, out


# ---- 1. plane parity on every objCrop family ------------------------------------------
@pytest.mark.parametrize("cid", sorted(rc.PARITY))
def test_plane_parity(cid):
    B, zl = rc.PARITY[cid]
    ctx = objcrop_cases.BY_ID[cid]
    s, prob, objF = _solver(cid, B, 4000 + ctx.L + ctx.fp16)
    with s:
        fl = 1.0 / (0.8 * rc.half_band(prob))   # the band's outer bins are evanescent
        k = rc.bins(prob.L)
        dead = (fl * fl * (k[:, None] ** 2 + k[None, :] ** 2) > 1.0) & rc.band_mask(prob.L, rc.band_of(prob))
        assert dead.any() and (objF[:, dead] != 0).all()
        planes, _ = s.refocus(zl, fl, sums=False)
        assert planes.shape == (len(zl), B, prob.L, prob.L) and planes.dtype == np.complex64
        crop = s.download(objF=False, pupil=False, support=False)["objCrop"]
    want = rc.planes(objF, zl, fl)
    worst = 0.0
    for i, z in enumerate(zl):
        for b in range(B):
            e = rc.rel_l2(planes[i, b], want[i, b])
            worst = max(worst, e)
            assert e <= rc.PLANE_BOUND, (cid, z, b, e)
        if z == 0.0:
            # launched on the stored spectrum itself: objCrop's bits, evanescent bins and all
            assert planes[i].tobytes() == crop.tobytes()
    print(f"{cid}: worst relative L2 {worst:.3e} = {worst / rc.PLANE_BOUND:.3f} of the bound")


# ---- 2. a z per patch, the neighbours in the list, host and device output -------------
@pytest.mark.parametrize("cid", ["L96", "L360", "L96h"])
def test_per_patch_z_and_list_independence(cid):
    import torch
    s, prob, objF = _solver(cid, 3, 77)
    with s:
        B, L = 3, prob.L
        fl = 1.0 / (0.8 * rc.half_band(prob))
        zpp = np.array([[7.25, -3.5, 12.0], [1.0, 7.25, -1000.5], [0.0, 0.0, 0.0]])
        per, _ = s.refocus(zpp, fl, sums=False)
        shared = {z: s.refocus([z], fl, sums=False)[0][0] for z in sorted(set(zpp.ravel()))}
        for i in range(len(zpp)):
            for b in range(B):
                assert per[i, b].tobytes() == shared[zpp[i, b]][b].tobytes(), (i, b)
        assert per[2].tobytes() == s.download(objF=False, pupil=False, support=False)["objCrop"].tobytes()
        # a plane does not depend on its neighbours in the list or on nz
        three, sums3 = s.refocus([7.25, -3.5, 12.0], fl, margin=3)
        other, sums_o = s.refocus([99.0, 12.0, 7.25], fl, margin=3)
        one, sums1 = s.refocus([7.25], fl, margin=3)
        assert three[0].tobytes() == one[0].tobytes() == other[2].tobytes() == shared[7.25].tobytes()
        assert three[2].tobytes() == other[1].tobytes()
        for k in ("sum_a", "sum_a2", "sum_g"):
            assert sums3[k][0].tobytes() == sums1[k][0].tobytes() == sums_o[k][2].tobytes()
            assert sums3[k][2].tobytes() == sums_o[k][1].tobytes()
        # device output: the transform stores straight into the caller's memory
        dev = torch.full((len(zpp), B, L, L, 2), float("nan"), dtype=torch.float32, device="cuda")
        none, dsums = s.refocus(zpp, fl, margin=3, device_ptr=dev.data_ptr())
        torch.cuda.synchronize()
        assert none is None
        assert dev.cpu().numpy().tobytes() == per.tobytes()
        _, hsums = s.refocus(zpp, fl, margin=3)
        for k in hsums:
            assert dsums[k].tobytes() == hsums[k].tobytes()
        # two calls on the same state return the same bytes
        again, _ = s.refocus(zpp, fl, sums=False)
        assert again.tobytes() == per.tobytes()


# ---- 3. the sums ----------------------------------------------------------------------
@pytest.mark.parametrize("cid", rc.SUM_CONTEXTS)
def test_sums(cid):
    s, prob, objF = _solver(cid, 3, rc.SUM_SEED[cid])
    with s:
        L, fl = prob.L, 0.5 / rc.half_band(prob)
        for margin in rc.sum_margins(L):
            planes, sums = s.refocus(rc.SUM_ZL, fl, margin=margin)
            want = dict(zip(("sum_a", "sum_a2", "sum_g"), rc.sums(planes, margin)))
            assert (want["sum_g"] / want["sum_a2"] >= rc.GRAD_CONDITION).all()   # the sum_g bound's condition
            for k, bound in (("sum_a", rc.SUM_BOUND), ("sum_a2", rc.SUM_BOUND), ("sum_g", rc.GRAD_BOUND)):
                assert sums[k].shape == (len(rc.SUM_ZL), 3)
                err = np.abs(sums[k] / want[k] - 1).max()
                print(f"{cid} margin {margin} {k}: {err:.3e} = {err / bound:.3f} of the bound")
                assert err <= bound, (cid, margin, k, err)
            # without planes: the same sums bit for bit
            none, only = s.refocus(rc.SUM_ZL, fl, margin=margin, planes=False)
            assert none is None
            for k in sums:
                assert only[k].tobytes() == sums[k].tobytes(), (margin, k)
            # any sum pointer NULL leaves the others unchanged
            for drop in range(3):
                want_ptr = tuple(i != drop for i in range(3))
                _, out = _raw(s, rc.SUM_ZL, fl, margin, want_ptr)
                for i, k in enumerate(("sum_a", "sum_a2", "sum_g")):
                    assert (out[i] is None) == (i == drop)
                    if out[i] is not None:
                        assert out[i].tobytes() == sums[k].tobytes(), (margin, drop, k)
            _, out = _raw(s, rc.SUM_ZL, fl, margin, (False, False, True))
            assert out[2].tobytes() == sums["sum_g"].tobytes()


# ---- 4. energy ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["L96", "L512"])
def test_energy_is_conserved(cid):
    s, prob, objF = _solver(cid, 3, 31)
    with s:
        _, sums = s.refocus(rc.PARITY_ZL, 0.5 / rc.half_band(prob), margin=0, planes=False)
    e = sums["sum_a2"]
    dev = np.abs(e / e[:1] - 1).max()
    print(f"{cid}: sum_a2 varies by {dev:.3e} across the planes")
    assert dev <= 1e-5
    # Parseval against the state itself
    want = (np.abs(objF.astype(np.complex128)) ** 2).sum((1, 2)) / prob.L ** 2
    np.testing.assert_allclose(e[0], want, rtol=1e-5)


# ---- 5. autofocus end to end ----------------------------------------------------------
Z_STAR = (8.0, 12.0, -16.0)
Z_PLANES = np.arange(-24.0, 24.0 + 1, 4.0)


@functools.lru_cache(maxsize=None)
def _autofocus_scene():
    Np, L, r, step, B = 64, 192, 10, 6, 3
    x0, y0, order = grid_geometry(Np, L, 3, step)
    prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=B)
    fl = 0.5 / rc.half_band(prob)
    pairs = [rc.scene(L, rc.band_of(prob), z, fl, seed=20 + b) for b, z in enumerate(Z_STAR)]
    objF = np.stack([p[0] for p in pairs]).astype(np.complex64)
    sharp = np.stack([p[1] for p in pairs])
    return prob, fl, objF, sharp


@pytest.mark.parametrize("measure", rc.MEASURES)
def test_autofocus_end_to_end(measure):
    prob, fl, objF, sharp = _autofocus_scene()
    lam = 0.5                                  # any unit: z = zl * lam, ps from fl = lam / (L ps)
    ps = lam / (prob.L * fl)
    assert focus.bin_frequency(lam, prob.L, ps) == pytest.approx(fl, rel=1e-15)
    with fpm_amd.Solver(prob) as s:
        s.set_state(objF, np.ones((prob.np_, prob.np_), np.complex64))
        got = focus.autofocus(s, Z_PLANES * lam, lam, ps, measure=measure, margin=8)
        idx = [int(np.flatnonzero(Z_PLANES == z)[0]) for z in Z_STAR]
        np.testing.assert_array_equal(got["index"], idx)
        np.testing.assert_allclose(got["z"], np.array(Z_STAR) * lam)
        assert got["field"].shape == (3, prob.L, prob.L) and got["field"].dtype == np.complex64
        for b in range(3):
            e = rc.rel_l2(got["field"][b], sharp[b])
            print(f"{measure} patch {b}: relative L2 to the sharp object {e:.3e} = {e / (2 * rc.PLANE_BOUND):.3f} "
                  f"of the bound")
            assert e <= 2 * rc.PLANE_BOUND, (b, e)
        # the device's sums make the yardstick's measures
        want = rc.measures(got["sums"]["sum_a"], got["sums"]["sum_a2"], got["sums"]["sum_g"], prob.L, 8)[measure]
        np.testing.assert_allclose(got["values"], want, rtol=1e-12)


# ---- 6. read-only, accounting, errors ---------------------------------------------------
def _run_case(B=3):
    Np, L, r = 32, 96, 6
    x0, y0, order = grid_geometry(Np, L, 5, 4)
    stack = make_stack(Np, L, r, x0, y0, n_patch=B, seed=7)
    return fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=B), stack


def _fields(struct):
    return {f: getattr(struct, f) for f, _ in struct._fields_}


def test_refocus_is_read_only_and_counts_its_scratch():
    prob, stack = _run_case()
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(2)
        before, timing, clock = s.download(), _fields(s.timing()), _fields(s.clock())
        gains, crops, meas = s.gains(), s.crops(), s.download_stack()
        b0 = s.info().device_bytes
        fl = 0.5 / rc.half_band(prob)
        s.refocus([0.0, 5.5], fl, margin=2)
        b1 = s.info().device_bytes
        B, L = prob.n_patch, prob.L
        assert b1 - b0 >= B * L * L * 8      # the fp32 scratch of objF H, and the small buffers
        s.refocus([[3.0, -2.0, 1.0]], fl, planes=False)
        s.refocus([1.0] * 70, fl, margin=1, planes=False)   # more planes than one piece holds
        s.refocus([5.5, 0.0], fl, sums=False)   # the staging ends on a z = 0 plane: kept as objCrop, and it is
        assert s.info().device_bytes == b1
        after = s.download()
        for k in before:
            assert after[k].tobytes() == before[k].tobytes(), k
        assert _fields(s.timing()) == timing and _fields(s.clock()) == clock
        assert s.gains().tobytes() == gains.tobytes() and s.download_stack().tobytes() == meas.tobytes()
        for a, b in zip(s.crops(), crops):
            np.testing.assert_array_equal(a, b)
        # the run goes on as if nothing had happened
        s.run(1)
        mine = s.download()
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(2)
        s.run(1)
        ref = s.download()
    for k in ref:
        assert mine[k].tobytes() == ref[k].tobytes(), k


def test_seventy_planes_match_single_calls():
    s, prob, objF = _solver("L96", 2, 5)
    with s:
        fl = 0.5 / rc.half_band(prob)
        zl = np.linspace(-30, 30, 70)
        _, sums = s.refocus(zl, fl, margin=4, planes=False)
        for i in (0, 63, 64, 69):   # either side of the piece boundary
            _, one = s.refocus(zl[i:i + 1], fl, margin=4, planes=False)
            for k in sums:
                assert one[k][0].tobytes() == sums[k][i].tobytes(), (i, k)


def test_errors():
    prob, stack = _run_case()
    fl = 0.03
    with fpm_amd.Solver(prob) as s:
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.refocus([0.0], fl)
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        s.upload(stack)
        with pytest.raises(fpm_amd.FpmError) as ei:
            s.refocus([0.0], fl)
        assert ei.value.code == fpm_amd.FPM_ERR_STATE
        s.init()
        s.refocus([0.0], fl)
        L = prob.L
        lib, dp = fpm_amd._lib, C.POINTER(C.c_double)
        z = np.array([1.0, 2.0, 3.0])
        out = np.empty((3, prob.n_patch))
        zp, op = z.ctypes.data_as(dp), out.ctypes.data_as(dp)

        def refused(name, *args):
            assert lib.fpm_refocus(s._h, *args) == fpm_amd.FPM_ERR_INVAL, name
            msg = lib.fpm_last_error().decode()
            assert name in msg, (name, msg)

        refused("zl", None, 3, fl, 0, 0, None, op, None, None, None)
        refused("nz", zp, 0, fl, 0, 0, None, op, None, None, None)
        refused("nz", zp, -1, fl, 0, 0, None, op, None, None, None)
        for bad in (float("nan"), float("inf"), 0.0, -0.01):
            refused("fl", zp, 3, bad, 0, 0, None, op, None, None, None)
        refused("margin", zp, 3, fl, -1, 0, None, op, None, None, None)
        refused("margin", zp, 3, fl, (L - 2) // 2 + 1, 0, None, op, None, None, None)
        refused("flag", zp, 3, fl, 0, 4, None, op, None, None, None)
        refused("flag", zp, 3, fl, 0, 0x80000000, None, op, None, None, None)
        refused("output", zp, 3, fl, 0, 0, None, None, None, None, None)
        for bad, i in ((float("nan"), 1), (float("-inf"), 2), (1.0000001e6, 0), (-1.0000001e6, 2)):
            zz = z.copy()
            zz[i] = bad
            refused(f"zl[{i}]", zz.ctypes.data_as(dp), 3, fl, 0, 0, None, op, None, None, None)
        zz = np.ones((2, prob.n_patch))
        zz[1, 2] = float("nan")
        refused(f"zl[{prob.n_patch + 2}]", zz.ctypes.data_as(dp), 2, fl, 0, fpm_amd.REFOCUS_Z_PER_PATCH, None, op, None,
                None, None)
        # the limits themselves are legal
        s.refocus([1e6, -1e6], fl, margin=(L - 2) // 2, planes=False)
        with pytest.raises(ValueError):
            s.refocus(np.zeros((2, prob.n_patch + 1)), fl)


def test_refocus_on_a_capturing_stream_is_refused():
    import torch
    prob, stack = _run_case()
    with fpm_amd.Solver(prob) as s:
        s.upload(stack)
        s.init()
        s.run(1)
        fl = 0.03
        want, wsums = s.refocus([2.5], fl, margin=1)
        cs = torch.cuda.Stream()
        s.set_stream(cs.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(fpm_amd.FpmError) as ei:
            with torch.cuda.graph(g, stream=cs, capture_error_mode="relaxed"):
                s.refocus([2.5], fl, margin=1)
        assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "capturing" in str(ei.value)
        got, gsums = s.refocus([2.5], fl, margin=1)   # on the caller's stream, no longer capturing
        assert got.tobytes() == want.tobytes() and gsums["sum_g"].tobytes() == wsums["sum_g"].tobytes()
        s.set_stream(None)
        assert s.refocus([2.5], fl, margin=1)[0].tobytes() == want.tobytes()


# ---- 7. CLI ---------------------------------------------------------------------------
def test_cli_refocus(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    outs = {}
    for tag, extra in (("refocus", ["--refocus", "-4:4:3", "--write-refocus", "--focus-measure", "grad"]),
                       ("without", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([BIN, ds["json"], "2", "--out", str(out)] + extra, capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = out
    plain = json.loads((outs["without"] / "result.json").read_text())
    assert "refocus" not in plain and not (outs["without"] / "objCrop_focus.npy").exists()
    meta = json.loads((outs["refocus"] / "result.json").read_text())
    assert set(meta) - {"refocus"} == set(plain)
    for f in ("objCrop.npy", "objF.npy", "pupil.npy"):
        assert (outs["refocus"] / f).read_bytes() == (outs["without"] / f).read_bytes(), f
    rf, L = meta["refocus"], meta["nlarge"]
    lam = ds["keys"]["lambda"]
    assert rf["z"] == [-4.0, 0.0, 4.0] and rf["measure"] == "grad" and rf["pick"] == "max" and rf["ms"] > 0
    np.testing.assert_allclose(rf["zl"], np.array(rf["z"]) / np.float32(lam), rtol=1e-12)
    assert rf["fl"] > 0 and rf["margin"] == 8
    for k in ("sum_a", "sum_a2", "sum_g"):
        assert np.array(rf[k]).shape == (3, 1) and (np.array(rf[k]) > 0).all()
    planes = np.load(outs["refocus"] / "refocus.npy")
    crop = np.load(outs["refocus"] / "objCrop.npy")
    assert planes.dtype == np.complex64 and planes.shape == (3, 1, L, L)
    assert planes[1, 0].tobytes() == crop.tobytes()          # z = 0: objCrop's bits
    grad = focus.measures(rf, L, rf["margin"])["grad"]
    assert rf["plane"] == [int(grad[:, 0].argmax())] and rf["z_best"] == [rf["z"][rf["plane"][0]]]
    best = np.load(outs["refocus"] / "objCrop_focus.npy")
    assert best.shape == (1, L, L) and best.tobytes() == planes[rf["plane"][0]].tobytes()
    # the sums are those of the planes written
    want = rc.sums(planes, rf["margin"])
    for k, w, bound in zip(("sum_a", "sum_a2", "sum_g"), want, (rc.SUM_BOUND, rc.SUM_BOUND, rc.GRAD_BOUND)):
        np.testing.assert_allclose(np.array(rf[k]), w, rtol=bound)
    r = subprocess.run([BIN, ds["json"], "1", "--refocus", "0:1"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 2 and "Z0:DZ:N" in r.stderr
    r = subprocess.run([BIN, ds["json"], "1", "--focus-pick", "min"], capture_output=True, text=True, env=env,
                       timeout=60)
    assert r.returncode == 2 and "need --refocus" in r.stderr


def test_cli_refocus_with_overlap(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([BIN, ds["json"], "1", "--out", str(out), "--grid", "2x2", "--overlap", "8", "--write-tiles",
                        "--refocus", "-6:6:3", "--write-refocus", "--focus-margin", "5"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    meta = json.loads((out / "result.json").read_text())
    rf, L = meta["refocus"], meta["nlarge"]
    assert rf["margin"] == 5 and len(rf["plane"]) == 4 and np.array(rf["sum_g"]).shape == (3, 4)
    planes = np.load(out / "refocus.npy")
    best = np.load(out / "objCrop_focus.npy")
    assert planes.shape == (3, 4, L, L) and best.shape == (4, L, L)
    for b in range(4):
        assert best[b].tobytes() == planes[rf["plane"][b], b].tobytes(), b
    assert planes[1].tobytes() == np.load(out / "objCrop_tiles.npy").tobytes()
    # the field is the stitch of the focused tiles
    st = meta["stitch"]
    field, fac = fpm_amd.stitch_tiles(best, (2, 2), st["stride"], align=st["align"])
    assert np.load(out / "objCrop_field.npy").tobytes() == field.tobytes()
    np.testing.assert_array_equal(np.array(st["factors"]), np.stack([fac.real, fac.imag], 1))


def test_cli_refocus_places_the_focused_tiles_without_overlap(tmp_path):
    from dataset_fixture import make_dataset
    ds = make_dataset(str(tmp_path / "data"))
    env = dict(os.environ, OPENCV_OPENCL_DEVICE="GPU:0")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([BIN, ds["json"], "1", "--out", str(out), "--grid", "2x2", "--write-tiles", "--refocus", "3:6:2"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    meta = json.loads((out / "result.json").read_text())
    L = meta["nlarge"]
    assert meta["refocus"]["z"] == [3.0, 9.0] and "stitch" not in meta
    best, tiles, field = (np.load(out / f) for f in ("objCrop_focus.npy", "objCrop_tiles.npy", "objCrop_field.npy"))
    assert best.shape == tiles.shape == (4, L, L) and field.shape == (2 * L, 2 * L)
    assert not np.array_equal(best, tiles)   # no plane at z = 0: the focused tiles are not objCrop
    for b in range(4):
        i, j = divmod(b, 2)
        assert field[i * L:(i + 1) * L, j * L:(j + 1) * L].tobytes() == best[b].tobytes(), b
