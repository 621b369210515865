"""The carried max|objF| / max|P| bookkeeping (fpm_debug_get_maxima) against
the downloaded fp32 state, magnitudes in float64: the check of
tests/test_gpu_schedules.py (whose docstring states the invariant), shared
with tests/test_gpu_sizes.py.  Needs a live context; plain numpy otherwise.

`case` names the context: case.row.B, case.row.fp16, case.row.kernel (the
fpm_info.fused_kernel it reports) and case.band(), the live band
(sy0, sy1, sx0, sx1) inclusive."""
import numpy as np

import fpm_amd

ULP4 = 4.0


def tile_max(mag):
    """[B][L][L] magnitudes -> [B][nty][ntx] maxima over 16 x 16 tiles (the last partial)."""
    B, L, _ = mag.shape
    nt = (L + 15) // 16
    pad = np.zeros((B, nt * 16, nt * 16))
    pad[:, :L, :L] = mag
    return pad.reshape(B, nt, 16, nt, 16).max(axis=(2, 4))


def check_maxima(s, case, where):
    row = case.row
    before = s.download(objCrop=False, support=False)
    mx = s.debug_maxima()
    again = s.debug_maxima()
    after = s.download(objCrop=False, support=False)
    for k in ("tmax", "dirty", "pmax") + (("rmax",) if mx["rmax"] is not None else ()):
        np.testing.assert_array_equal(mx[k], again[k], err_msg=f"{where}: {k} differs between two read-backs")
    for k in ("objF", "pupil"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=f"{where}: the read-back changed {k}")

    spec = np.fft.fftshift(before["objF"], axes=(-2, -1))
    true = tile_max(np.hypot(spec.real.astype(np.float64), spec.imag.astype(np.float64)))
    tmax, dirty = mx["tmax"].astype(np.float64), mx["dirty"]
    assert tmax.shape == true.shape == dirty.shape, (tmax.shape, true.shape)

    def tol(v):  # of a float64 magnitude v
        ulp = ULP4 * np.spacing(np.asarray(v, np.float32)).astype(np.float64)
        return ulp + (np.asarray(v) * 2.0 ** -10 if row.fp16 else 0.0)

    bad = ~dirty & (np.abs(tmax - true) > tol(true))
    assert not bad.any(), (where, "clean tile maximum", np.argwhere(bad)[:4].tolist(), tmax[bad][:4], true[bad][:4])
    low = dirty & (tmax < true - tol(true))
    assert not low.any(), (where, "dirty tile below its maximum", np.argwhere(low)[:4].tolist(), tmax[low][:4],
                           true[low][:4])
    for b in range(row.B):
        gmax = true[b].max()
        cmax = tmax[b][~dirty[b]].max()
        assert abs(cmax - gmax) <= tol(gmax), (where, b, "max over the clean tiles", cmax, gmax)
        pm = np.abs(before["pupil"][b].astype(np.complex128)).max()
        assert abs(float(mx["pmax"][b].max()) - pm) <= ULP4 * float(np.spacing(np.float32(pm))), \
            (where, b, "max|P|", mx["pmax"][b].max(), pm)
    if row.kernel == fpm_amd.KERNEL_GENERAL:
        assert not dirty.any(), where
        np.testing.assert_array_equal(mx["rmax"], mx["tmax"].max(axis=2), err_msg=f"{where}: rmax")
    else:
        assert mx["rmax"] is None
        sy0, sy1, sx0, sx1 = case.band()
        out = np.ones(dirty.shape[1:], bool)
        out[sy0 // 16:sy1 // 16 + 1, sx0 // 16:sx1 // 16 + 1] = False
        assert not dirty[:, out].any() and not mx["tmax"][:, out].any(), (where, "tiles outside the band")
    return int(dirty.sum())
