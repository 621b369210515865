"""The yardstick of the fpm_residual tests (tests/test_gpu_residual.py, whose
docstring derives the bound, and tests/test_gpu_ladder.py): a float64 numpy
evaluation of the DOWNLOADED state, the bound on |E_gpu - E_ref| and the
comparison.  Plain numpy, no GPU."""
import numpy as np


def reference(state, stack, prob):
    """float64 E, Q [n_order][B] and the integer S of the downloaded state."""
    Np, B = prob.np_, prob.n_patch
    n = len(prob.order)
    E, Q, S = np.empty((n, B)), np.empty((n, B)), np.empty((n, B))
    for b in range(B):
        O = np.fft.fftshift(state["objF"][b].astype(np.complex128))
        P = np.fft.ifftshift(state["pupil"][b].astype(np.complex128))
        for i, led in enumerate(prob.order):
            xs, ys = int(prob.x0[led]), int(prob.y0[led])
            a = np.abs(np.fft.ifft2(np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np]) * P))
            I = stack[led, b].astype(np.float64)
            E[i, b] = ((a - np.sqrt(I)) ** 2).sum()
            Q[i, b] = (a * a).sum()
            S[i, b] = float(stack[led, b].astype(np.int64).sum())
    return E, Q, S


def bound(E, Q):
    return 2e-5 * np.sqrt(E * Q) + 1e-10 * Q


def check(tag, d, ref):
    E, Q, S = ref
    delta, bnd = np.abs(d["err"] - E), bound(E, Q)
    # a window that misses the spectrum's support for good has psi = 0: Q = 0, the bound is 0 and E = S exactly
    ratio = np.divide(delta, bnd, out=np.zeros_like(delta), where=bnd > 0)
    print(f"residual {tag}: max |dE|/bound {ratio.max():.3e}  ({int((bnd == 0).sum())} of {bnd.size} with Q = 0; "
          f"E/S {d['err'].sum() / S.sum():.3e}, sweep {d['ms']:.3f} ms)")
    assert np.all(np.isfinite(d["err"])) and np.all(delta <= bnd), (tag, float(ratio.max()), float(delta.max()))
    np.testing.assert_array_equal(d["ref"], S)
