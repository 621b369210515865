"""The yardstick of the fpm_predict tests (tests/test_gpu_predict.py): a float64
numpy evaluation of the DOWNLOADED state, as tests/residual_check.py's,
    a_ref = |ifft2(ifftshift(O[y:y+Np, x:x+Np]) P)|,  O = fftshift(objF), P = ifftshift(pupil),
per entry and patch, the bounds and the comparisons.  Plain numpy, no GPU.

Bounds, per (entry, patch) image, norms over its Np^2 pixels:
  AMPLITUDE  ||a_gpu - a_ref|| <= EPS ||a_ref||, EPS = 1e-5: the amplitude error
             the residual's own bound 2e-5 sqrt(E Q) assumes (residual_check.bound,
             derived in tests/test_gpu_residual.py).  Where the window misses the
             support a_ref = 0 and the bound is 0: the image must be exactly 0.
  DIFF       d = a - g sqrt(I): the amplitude bound plus the fp32 rounding of
             g sqrt(I) (one rounding of the root, one of the product):
             ||d_gpu - d_ref|| <= EPS ||a_ref|| + 2^-23 ||g sqrt(I)||.
             sum d^2 (float64) against fpm_residual's E: residual_check.bound(E, Q).
             Where the window misses the support (Q = 0) that bound is 0, which
             no float32 d can meet: there d = -fl(g fl(sqrt(I))), whose square
             is not the g^2 I the sweep adds up.  Such an image is required to
             be exactly that float32 value instead.
  COUNTS     c = min(rint((a / g)^2), 65535).  Rounding moves a pixel by at
             most 1/2 (||.|| <= Np / 2 over the image) and the amplitude error
             da changes (a / g)^2 by 2 a da / g^2 to first order:
             ||c_gpu - min(a_ref^2 / g^2, 65535)|| <= Np / 2 + 2 EPS max(a_ref) ||a_ref|| / g^2.
             Per pixel: within 1 count of rint(a_ref^2 / g^2) (the two roundings
             can fall on either side of a half), or within what the amplitude
             bound allows that pixel: |da| <= EPS ||a_ref|| gives
             |c_gpu - a_ref^2 / g^2| <= 1/2 + (2 a_ref da + da^2) / g^2.
Each check prints the measured ratio to its bound before it asserts."""
import numpy as np

EPS = 1e-5
SAT = 65535.0


def amplitudes(state, prob, pos=None, dx=None, dy=None):
    """float64 a_ref [n][B][Np][Np] of the downloaded state: the identity list
    (pos None: row i is order[i]'s LED with its own window) or the probe
    entries (pos[k], dx[k], dy[k])."""
    Np, B = prob.np_, prob.n_patch
    order = [int(v) for v in prob.order]
    if pos is None:
        pos = range(len(order))
    pos = [int(p) for p in pos]
    dx = [0] * len(pos) if dx is None else [int(v) for v in dx]
    dy = [0] * len(pos) if dy is None else [int(v) for v in dy]
    out = np.empty((len(pos), B, Np, Np))
    for b in range(B):
        O = np.fft.fftshift(state["objF"][b].astype(np.complex128))
        P = np.fft.ifftshift(state["pupil"][b].astype(np.complex128))
        for k, p in enumerate(pos):
            led = order[p]
            xs, ys = int(prob.x0[led]) + dx[k], int(prob.y0[led]) + dy[k]
            out[k, b] = np.abs(np.fft.ifft2(np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np]) * P))
    return out


def _norm(a):
    """L2 norm of every (entry, patch) image, float64 [n][B]."""
    a = np.asarray(a, np.float64)
    return np.sqrt((a * a).sum(axis=(-2, -1)))


def _ratio(delta, bnd):
    return np.divide(delta, bnd, out=np.where(delta > 0, np.inf, 0.0), where=bnd > 0)


def amplitude_bound(a_ref):
    return EPS * _norm(a_ref)


def counts_reference(a_ref, g):
    """(a_ref / g)^2 saturated, float64: what COUNTS rounds.  g [n][B]."""
    return np.minimum(a_ref ** 2 / np.asarray(g, np.float64)[..., None, None] ** 2, SAT)


def counts_bound(a_ref, g):
    Np = a_ref.shape[-1]
    g = np.asarray(g, np.float64)
    return 0.5 * Np + 2.0 * EPS * a_ref.max(axis=(-2, -1)) * _norm(a_ref) / g ** 2


def diff_reference(a_ref, stack_rows, g):
    """a_ref - g sqrt(I), float64; stack_rows uint16 [n][B][Np][Np] (row k = the entry's image)."""
    return a_ref - np.asarray(g, np.float64)[..., None, None] * np.sqrt(stack_rows.astype(np.float64))


def diff_bound(a_ref, stack_rows, g):
    gs = np.asarray(g, np.float64)[..., None, None] * np.sqrt(stack_rows.astype(np.float64))
    return amplitude_bound(a_ref) + 2.0 ** -23 * _norm(gs)


def check_amplitude(tag, a_gpu, a_ref):
    assert a_gpu.dtype == np.float32 and a_gpu.shape == a_ref.shape, (a_gpu.dtype, a_gpu.shape)
    delta, bnd = _norm(a_gpu.astype(np.float64) - a_ref), amplitude_bound(a_ref)
    ratio = _ratio(delta, bnd)
    print(f"predict {tag} amplitude: max ||da||/bound {ratio.max():.3e}  "
          f"({int((bnd == 0).sum())} of {bnd.size} images with a_ref = 0)")
    assert np.all(np.isfinite(a_gpu)) and np.all(delta <= bnd), (tag, float(ratio.max()))
    dark = bnd == 0
    assert not np.any(a_gpu[dark]), tag  # exactly 0 where the window misses the support


def check_counts(tag, c_gpu, a_ref, g):
    assert c_gpu.dtype == np.uint16 and c_gpu.shape == a_ref.shape, (c_gpu.dtype, c_gpu.shape)
    c, q = c_gpu.astype(np.float64), counts_reference(a_ref, g)
    delta, bnd = _norm(c - q), counts_bound(a_ref, g)
    ratio = _ratio(delta, bnd)
    # per pixel: one count, or what the amplitude bound allows this pixel
    g2 = np.asarray(g, np.float64)[..., None, None] ** 2
    da = amplitude_bound(a_ref)[..., None, None]
    allowed = 0.5 + (2.0 * a_ref * da + da * da) / g2
    off = np.abs(c - np.rint(q))
    bad = (off > 1) & (np.abs(c - q) > allowed)
    print(f"predict {tag} counts: max ||dc||/bound {ratio.max():.3e}, pixels off by one {int((off == 1).sum())}, "
          f"by more {int((off > 1).sum())}, unexplained {int(bad.sum())} of {c.size}; max count {int(c_gpu.max())}")
    assert np.all(delta <= bnd), (tag, float(ratio.max()))
    assert not bad.any(), (tag, int(bad.sum()))


def check_diff(tag, d_gpu, a_ref, stack_rows, g, err=None, E=None, Q=None):
    """err: fpm_residual's E of the same rows (GPU); E, Q: the float64 reference's, for its bound."""
    assert d_gpu.dtype == np.float32 and d_gpu.shape == a_ref.shape, (d_gpu.dtype, d_gpu.shape)
    d = d_gpu.astype(np.float64)
    delta, bnd = _norm(d - diff_reference(a_ref, stack_rows, g)), diff_bound(a_ref, stack_rows, g)
    ratio = _ratio(delta, bnd)
    msg = f"predict {tag} diff: max ||dd||/bound {ratio.max():.3e}"
    r2 = None
    if err is not None:
        import residual_check
        lit = np.asarray(Q) > 0
        gap, b2 = np.abs((d * d).sum(axis=(-2, -1)) - err)[lit], residual_check.bound(E, Q)[lit]
        r2 = _ratio(gap, b2)
        msg += f", max |sum d^2 - E|/bound {r2.max() if r2.size else 0.0:.3e} ({int((~lit).sum())} images with Q = 0)"
    print(msg)
    assert np.all(np.isfinite(d_gpu)) and np.all(delta <= bnd), (tag, float(ratio.max()))
    if r2 is not None:
        assert np.all(gap <= b2), (tag, float(r2.max()))
        # a dark image: exactly the float32 -g sqrt(I)
        s32 = np.asarray(g, np.float32)[..., None, None] * np.sqrt(stack_rows.astype(np.float32))
        assert s32.dtype == np.float32
        np.testing.assert_array_equal(d_gpu[~lit], -s32[~lit], err_msg=tag)


def residual_sums(a_ref, stack_rows, g):
    """float64 E = sum (a - g sqrt(I))^2 and Q = sum a^2 [n][B] of the reference."""
    d = diff_reference(a_ref, stack_rows, g)
    return (d * d).sum(axis=(-2, -1)), (a_ref * a_ref).sum(axis=(-2, -1))
