"""The row-pair decomposition of the Np 256 fused kernel's row passes
(fpm_fused.hip with two column halves, fused256.hpp "row pairs"), restated in
numpy with exactly the kernel's index maps and checked against numpy.fft.

The halves of T are cut on the LOW digit of the column: x = x1 + 16 x2, half h
holds x1 in [8h, 8h+8).  Spectral index k = kb + 16 ka; only ka in SK can lie
in the support.  A 16-lane group serves its two FFT rows j = 0, 1 with one
four-step transform per pass and half:

  pass A (inverse)   lane kb: per row j the in-6 DFT16 over ka, outputs x1 of
                     the half, times W256^{-x1 kb} (= conj of the lane's own
                     twiddle set w[8h + i], tw2[(8h + i) * 16 + kb]), written to
                     tile position i' = 8 j + (x1 - 8h).
                     exchange: lane t' reads position t' of every lane kb.
                     lane t' = (row t' >> 3, x1 = 8h + (t' & 7)): dense DFT16
                     over kb -> the 16 x2, stored at xl = (x1 - 8h) + 8 x2.
  pass C (forward)   lane t' reads its 16 x2 at xl = (t' & 7) + 8 x2, dense
                     DFT16 over x2 -> kb, times W256^{x1 kb} = tw2[kb * 16 + x1]
                     (the set of the lane's x1, not of t'), written to tile
                     position kb.
                     exchange: lane kb reads position kb of every lane t'.
                     lane kb: per row j the in-half (x1 = 8h + i from lane
                     8 j + i), out-6 DFT16 -> F[j][s] += X_j[kb + 16 SK[s]].

Everything that turns a half-T slot into an image column uses
x = 8h + (xl & 7) + 16 (xl >> 3); the tail-pixel sums of pass C walk
xl = t + 16 m, i.e. x = x(t) + 32 m.
"""
import numpy as np
import pytest

NP = 256
SK = (0, 1, 2, 13, 14, 15)
W256 = np.exp(-2j * np.pi * np.arange(NP) / NP)
TW2 = np.array([W256[((i >> 4) * (i & 15)) & 255] for i in range(256)])  # [m * 16 + t] = W256^{m t}
W16 = np.exp(-2j * np.pi / 16)


def xcol(xl, h):
    """image column of slot xl of half h"""
    return 8 * h + (xl & 7) + 16 * (xl >> 3)


def exchange(y):
    """four-step exchange: y[lane][position] -> z[lane][j] = y[j][lane]"""
    return y.T.copy()


def _rows(seed):
    """two rows whose spectrum lives on the six-slot support |kx| <= 47"""
    rng = np.random.default_rng(seed)
    X = np.zeros((2, NP), complex)
    for ka in SK:
        X[:, 16 * ka:16 * ka + 16] = rng.standard_normal((2, 16)) + 1j * rng.standard_normal((2, 16))
    return X


def pass_a(X, h):
    """half-T rows [j][xl] of the unscaled inverse transforms of X[j]"""
    y = np.zeros((16, 16), complex)  # [lane kb][tile position]
    for kb in range(16):
        for j in range(2):
            for i in range(8):
                x1 = 8 * h + i
                s1 = sum(X[j, kb + 16 * ka] * W16 ** (-x1 * ka) for ka in SK)
                y[kb, 8 * j + i] = s1 * np.conj(TW2[(8 * h + i) * 16 + kb])
    z = exchange(y)
    T = np.zeros((2, 128), complex)
    for t in range(16):
        j, i = t >> 3, t & 7
        for x2 in range(16):
            T[j, i + 8 * x2] = sum(z[t, kb] * W16 ** (-x2 * kb) for kb in range(16))
    return T


def pass_c(T, h):
    """F[j][kb][s]: the half's contribution to X_j[kb + 16 SK[s]]"""
    y = np.zeros((16, 16), complex)  # [lane t][tile position kb]
    for t in range(16):
        j, x1 = t >> 3, 8 * h + (t & 7)
        v = [T[j, (t & 7) + 8 * x2] for x2 in range(16)]
        for kb in range(16):
            y[t, kb] = sum(v[x2] * W16 ** (x2 * kb) for x2 in range(16)) * TW2[kb * 16 + x1]
    z = exchange(y)
    F = np.zeros((2, 16, 6), complex)
    for kb in range(16):
        for j in range(2):
            for s, ka in enumerate(SK):
                F[j, kb, s] = sum(z[kb, 8 * j + i] * W16 ** ((8 * h + i) * ka) for i in range(8))
    return F


def test_column_map_is_a_bijection_per_half_and_covers_the_row():
    cols = [sorted(xcol(xl, h) for xl in range(128)) for h in range(2)]
    for h in range(2):
        assert cols[h] == [x for x in range(NP) if x % 16 // 8 == h]
    assert sorted(cols[0] + cols[1]) == list(range(NP))
    # the tail-pixel walk: lane t, term m -> slot t + 16 m, column x(t) + 32 m
    for h in range(2):
        for t in range(16):
            for m in range(8):
                assert xcol(t + 16 * m, h) == xcol(t, h) + 32 * m


@pytest.mark.parametrize("h", [0, 1])
def test_pass_a_gives_the_half_of_the_inverse_transform(h):
    X = _rows(1)
    ref = np.fft.ifft(X, axis=1) * NP  # unscaled
    T = pass_a(X, h)
    for xl in range(128):
        np.testing.assert_allclose(T[:, xl], ref[:, xcol(xl, h)], rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("h", [0, 1])
def test_pass_c_gives_the_half_input_transform_on_the_support(h):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, NP)) + 1j * rng.standard_normal((2, NP))
    T = np.array([[x[j, xcol(xl, h)] for xl in range(128)] for j in range(2)])
    xh = np.zeros_like(x)
    cols = [xcol(xl, h) for xl in range(128)]
    xh[:, cols] = x[:, cols]
    ref = np.fft.fft(xh, axis=1)
    F = pass_c(T, h)
    for kb in range(16):
        for s, ka in enumerate(SK):
            np.testing.assert_allclose(F[:, kb, s], ref[:, kb + 16 * ka], rtol=0, atol=1e-12 * np.abs(ref).max())


def test_summed_halves_round_trip_on_the_support():
    """A then C over both halves returns Np X on the SK outputs, and the sum
    of the two half transforms of a dense row is its transform."""
    X = _rows(3)
    F = sum(pass_c(pass_a(X, h), h) for h in range(2))
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, NP)) + 1j * rng.standard_normal((2, NP))
    G = sum(pass_c(np.array([[x[j, xcol(xl, h)] for xl in range(128)] for j in range(2)]), h) for h in range(2))
    ref = np.fft.fft(x, axis=1)
    for kb in range(16):
        for s, ka in enumerate(SK):
            np.testing.assert_allclose(F[:, kb, s], NP * X[:, kb + 16 * ka], rtol=0, atol=1e-12 * NP * np.abs(X).max())
            np.testing.assert_allclose(G[:, kb, s], ref[:, kb + 16 * ka], rtol=0, atol=1e-12 * np.abs(ref).max())
