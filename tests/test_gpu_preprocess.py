"""Loader preprocessing on the GPU (fpm_upload_frames, fpmMain.cpp:124-144)
vs the oracle's numpy restatement, bit-exact (integer work), for several
patches cut from each full frame, host and device frame sources (GPU only).

The second half runs the tables of tests/preprocess_cases.py: the arithmetic's
edge cases at the three smallest sizes (Np 32 fused, Np 90 fused, Np 64
general; the 64-bit sums at Np 1024 only) and one row per stack layout through
all three upload routes.  Every comparison is an equality.  Deliberate breaks
of csrc/preprocess.hip, each run once on an MI355X against this file (the three
tests that were here before pass under all of them):
  rint -> round in k_crop_patches      dark_tie_even, dark_tie_odd and every row's frames upload
  round -> rint in bg_value            bg_tie (3 sizes), bg_tie_nonpow2
  32-bit window sums in k_bg_sums      sum_over_32_bits-np1024, the np1024 row's frames uploads
  one pass of k_crop_patches' loop     the general320 and np1024 rows, sum_over_32_bits-np1024
  the v > 65535 clamp removed          bg_negative_threshold, bg_negative_half_threshold (3 sizes each)
"""
import numpy as np
import pytest

import fpm_oracle as oracle
import fpm_amd
from tools.synth import grid_geometry

pytestmark = pytest.mark.gpu

NP, L, R = 32, 96, 6
H, W = 300, 280
PATCHES = [(0, 0), (37, 11), (248, 268), (120, 90)]   # (x0, y0): includes the frame corner
BK1, BK2 = (5, 250), (200, 3)


def _frames(n, seed=1):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 4000, (n, H, W)) + rng.integers(0, 2000, (n, 1, 1))
    f[:, 100:200, 50:150] += rng.integers(0, 60000, (n, 100, 100))   # saturating pixels
    return np.clip(f, 0, 65535).astype(np.uint16)


def _expected(frames, dark, thresh, mult):
    n = len(frames)
    want = np.zeros((n, len(PATCHES), NP, NP), np.uint16)
    bgs = np.zeros(n, np.int64)
    for i in range(n):
        for b, (x, y) in enumerate(PATCHES):
            want[i, b], bgs[i] = oracle.preprocess_frame(frames[i], NP, (x, y), BK1, BK2, thresh, mult, bool(dark[i]))
    return want, bgs


def _solver(n):
    x0, y0, order = grid_geometry(NP, L, 3, 4)
    x0, y0 = x0[:n], y0[:n]
    order = np.arange(n)
    prob = fpm_amd.Problem(NP, L, order, x0, y0, R, 5, 10, n_patch=len(PATCHES))
    return fpm_amd.Solver(prob)


@pytest.mark.parametrize("thresh,mult", [(1000, 1.0), (2500, 3.0), (40000, 2.5)])
def test_frames_host_upload_matches_oracle(thresh, mult):
    n = 6
    frames = _frames(n)
    dark = np.array([1, 0, 1, 1, 0, 0], np.uint8)
    want, bgs = _expected(frames, dark, thresh, mult)
    with _solver(n) as s:
        bg = s.upload_frames(frames, [p[0] for p in PATCHES], [p[1] for p in PATCHES], BK1, BK2, thresh, mult, dark)
        got = s.download_stack()
    np.testing.assert_array_equal(bg, bgs)
    np.testing.assert_array_equal(got, want)


def test_frames_device_upload_and_solve():
    import torch
    n = 6
    frames = _frames(n, seed=4)
    dark = np.zeros(n, np.uint8)
    want, _ = _expected(frames, dark, 1000, 1.0)
    dev = torch.from_numpy(frames.view(np.int16)).cuda()
    with _solver(n) as s:
        s.upload_frames(None, [p[0] for p in PATCHES], [p[1] for p in PATCHES], BK1, BK2, 1000, 1.0, dark,
                        device_ptr=dev.data_ptr(), shape=(H, W))
        np.testing.assert_array_equal(s.download_stack(), want)
        s.init()
        s.run(1)
        out = s.download()
    # the same stack through the host upload gives the same reconstruction
    x0, y0, _ = grid_geometry(NP, L, 3, 4)
    prob = fpm_amd.Problem(NP, L, np.arange(n), x0[:n], y0[:n], R, 5, 10, n_patch=len(PATCHES))
    ref = fpm_amd.run_fpm(prob, want, 1)
    np.testing.assert_array_equal(out["objCrop"], ref["objCrop"])


def test_frames_reject_patch_outside():
    with _solver(6) as s:
        with pytest.raises(fpm_amd.FpmError, match="outside"):
            s.upload_frames(_frames(6), [0, 0, 0, W - NP + 1], [0, 0, 0, 0], BK1, BK2)


# ---- the case tables of tests/preprocess_cases.py -------------------------------------
# Edge cases: rounding ties of the divide and of bg_val, both saturation clamps,
# bg_val over the int16 range it is defined on, coinciding windows, 64-bit window
# sums -- each checked on the CPU to reach what it names (test_preprocess_cases.py).
# Layout rows: every stack permutation a context can have (meas_layout), through
# fpm_upload_frames from host and device memory, fpm_upload_stack and
# fpm_upload_stack_device.  All integer work: equality, no tolerance.
import preprocess_cases as pc  # noqa: E402

EDGE_RUNS = pc.edge_runs()


def _row_solver(row, monkeypatch, n_patch=None):
    """The row's context, after checking that it holds the layout the row names."""
    for knob in pc.KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    s = fpm_amd.Solver(row.problem(n_patch))
    try:
        assert s.debug_plan()["meas_g"] == row.meas_g, (row.id, row.kernel)
    except BaseException:
        s.close()
        raise
    return s


def _upload_frames(s, inp, device=False):
    args = (inp.px, inp.py, inp.bk1, inp.bk2, inp.bg_threshold, inp.dark_mult, inp.darkfield)
    if not device:
        return s.upload_frames(inp.frames, *args)
    import torch
    dev = torch.from_numpy(np.array(inp.frames).view(np.int16)).cuda()   # a writable copy: the table's is read-only
    bg = s.upload_frames(None, *args, device_ptr=dev.data_ptr(), shape=inp.frames.shape[1:])
    torch.cuda.synchronize()
    return bg


@pytest.mark.parametrize("case,row", EDGE_RUNS, ids=[f"{c.name}-{r.id}" for c, r in EDGE_RUNS])
def test_edge_case_matches_oracle(case, row, monkeypatch):
    inp = case.inputs(row.Np, row.n)
    want, bgs = pc.expected(inp, row.Np)
    with _row_solver(row, monkeypatch, n_patch=len(inp.patches)) as s:
        bg = _upload_frames(s, inp)
        got = s.download_stack()
    np.testing.assert_array_equal(bg, bgs)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", pc.LAYOUTS, ids=lambda r: r.id)
def test_layout_frames_upload_matches_oracle(row, device, monkeypatch):
    inp = pc.layout_inputs(row.id)
    want, bgs = pc.layout_expected(row.id)
    with _row_solver(row, monkeypatch) as s:
        bg = _upload_frames(s, inp, device)
        got = s.download_stack()
        again = s.download_stack()      # the download un-permutes and re-permutes in place
    np.testing.assert_array_equal(bg, bgs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(again, want)


@pytest.mark.parametrize("row", pc.LAYOUTS, ids=lambda r: r.id)
def test_layout_stack_uploads_round_trip(row, monkeypatch):
    """fpm_upload_stack and fpm_upload_stack_device; the device route copies and
    permutes in one pass at g = 16 and g = 10 and falls back to copy plus
    in-place permutation for g = 9 and the transposes."""
    import torch
    want, _ = pc.layout_expected(row.id)
    dev = torch.from_numpy(np.array(want).view(np.int16)).cuda()
    with _row_solver(row, monkeypatch) as s:
        s.upload(want)
        np.testing.assert_array_equal(s.download_stack(), want)
        np.testing.assert_array_equal(s.download_stack(), want)
        s.upload(np.zeros_like(want))       # so the device route cannot pass on what the host route left
        s.upload_device(dev.data_ptr())
        np.testing.assert_array_equal(s.download_stack(), want)
        np.testing.assert_array_equal(s.download_stack(), want)
        torch.cuda.synchronize()


@pytest.mark.parametrize("row", [r for r in pc.LAYOUTS if r.solve], ids=lambda r: r.id)
def test_layout_solve_after_frames_upload(row, monkeypatch):
    """The kernels read the stack where the frames upload left it: one iteration
    gives the bits of a host upload of the oracle's stack.  Np 1024 leaves this
    out (its solve is tests/test_gpu_np1024.py's; the stack equality above pins
    the device bytes, the un-permutation being a fixed bijection)."""
    inp = pc.layout_inputs(row.id)
    want, _ = pc.layout_expected(row.id)
    with _row_solver(row, monkeypatch) as s:
        _upload_frames(s, inp)
        s.init()
        s.run(1)
        out = s.download(objF=False, support=False)
    ref = fpm_amd.run_fpm(row.problem(), want, 1)
    for k in ("objCrop", "pupil"):
        assert np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, k
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def _bad_frames(row, inp, kind):
    """(frames, keyword changes) of an upload fpm_upload_frames must refuse."""
    H, W = inp.frames.shape[1:]
    if kind == "window_outside":
        return inp.frames, dict(bk2=(W - row.Np + 1, 0))
    if kind == "frame_smaller_than_np":
        return np.ascontiguousarray(inp.frames[:, :row.Np - 1, :]), {}
    return inp.frames, dict(mult={"multiplier_zero": 0.0, "multiplier_negative": -2.0}[kind])


@pytest.mark.parametrize("kind", ["window_outside", "frame_smaller_than_np", "multiplier_zero", "multiplier_negative"])
def test_frames_rejections_leave_the_context_usable(kind, monkeypatch):
    row = pc.LAYOUT["small32"]
    inp = pc.layout_inputs(row.id)
    want, bgs = pc.layout_expected(row.id)
    frames, change = _bad_frames(row, inp, kind)
    with _row_solver(row, monkeypatch) as s:
        with pytest.raises(fpm_amd.FpmError) as e:
            s.upload_frames(frames, inp.px, inp.py, inp.bk1, change.get("bk2", inp.bk2), inp.bg_threshold,
                            change.get("mult", inp.dark_mult), inp.darkfield)
        assert e.value.code == fpm_amd.FPM_ERR_INVAL
        np.testing.assert_array_equal(_upload_frames(s, inp), bgs)
        np.testing.assert_array_equal(s.download_stack(), want)
