"""The yardstick of the fpm_gradient tests (tests/test_gradient_check.py,
tests/test_gpu_gradient.py): a float64 numpy evaluation of the DOWNLOADED state,
as tests/predict_check.py's, of
    psi_i = ifft2(ifftshift(W_i) P),  W_i = O[y:y+Np, x:x+Np],  O = fftshift(objF),  P = ifftshift(pupil)
    f     = sum_i sum_yx (|psi_i| - g_i sqrt(I_i))^2
    rho_i = psi_i - g_i sqrt(I_i) psi_i / |psi_i|       (0 where |psi_i| = 0)
    R_i   = fft2(rho_i) / Np^2
    G_O[window_i] += 2 fftshift(conj(P) R_i)            G_objF  = ifftshift(G_O)
    G_P           += 2 conj(ifftshift(W_i)) R_i         G_pupil = fftshift(G_P) support
G = df/dRe(z) + i df/dIm(z), so df = sum Re(conj(G) dz); the two M maps of the
majorised steps; the bound; the comparisons.  Plain numpy, no GPU.

The bound, per patch and output, on ||G_gpu - G_ref|| over the array.  With the
project's amplitude error EPS = 1e-5 (predict_check.EPS) taken as the norm-wise
error of psi:
  an entry's  ||d rho|| <= EPS ||a_ref|| max_px c + 2^-23 ||g sqrt(I)||, where
              c = |1 - s/a| + s/a is the pixel's conditioning from the reference
              (rho = psi (1 - s/a): an error of psi enters through psi itself and
              through a), and the second term is the fp32 rounding of g sqrt(I);
  ||d R||     = ||d rho|| / Np, by Parseval (R = fft2(rho) / Np^2);
  ||d G_objF|| <= 2 max|P| sum_i ||d R_i|| + 2^-23 sum_i ||term_i||: the terms
              2 conj(P) R_i are added one by one in fp32;
  ||d G_pupil|| the same with max|W_i| per entry.
"""
import numpy as np

EPS = 1e-5
U = 2.0 ** -23


def support(Np, r):
    ky, kx = np.mgrid[-(Np // 2):Np - Np // 2, -(Np // 2):Np - Np // 2]
    return (ky * ky + kx * kx <= r * r).astype(np.float64)


def entries(prob, pos=None, dx=None, dy=None):
    """[(led, xs, ys)] of the identity list (pos None) or of the probe entries."""
    order = [int(v) for v in prob.order]
    pos = list(range(len(order))) if pos is None else [int(p) for p in pos]
    dx = [0] * len(pos) if dx is None else [int(v) for v in dx]
    dy = [0] * len(pos) if dy is None else [int(v) for v in dy]
    return [(order[p], int(prob.x0[order[p]]) + dx[k], int(prob.y0[order[p]]) + dy[k]) for k, p in enumerate(pos)]


def cost(objF, pupil, prob, stack, gains=None, pos=None, dx=None, dy=None):
    """float64 E [n][B] of the state (objF [B][L][L] un-centred, pupil [B][Np][Np] centred)."""
    Np, B = prob.np_, prob.n_patch
    ent = entries(prob, pos, dx, dy)
    E = np.empty((len(ent), B))
    for b in range(B):
        O = np.fft.fftshift(np.asarray(objF[b], np.complex128))
        P = np.fft.ifftshift(np.asarray(pupil[b], np.complex128))
        for k, (led, xs, ys) in enumerate(ent):
            a = np.abs(np.fft.ifft2(np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np]) * P))
            g = 1.0 if gains is None else float(gains[led, b])
            E[k, b] = ((a - g * np.sqrt(stack[led, b].astype(np.float64))) ** 2).sum()
    return E


def gradient(state, prob, stack, gains=None, pos=None, dx=None, dy=None):
    """The float64 yardstick: dict(objF complex128 [B][L][L] un-centred, pupil
    complex128 [B][Np][Np] centred, err / ref float64 [n][B], Q [n][B] = sum
    |psi|^2, bound_objF / bound_pupil [B], acc_objF / acc_pupil [B] = the
    accumulation-rounding term of each bound alone)."""
    Np, B, L, r = prob.np_, prob.n_patch, prob.L, prob.radius
    ent = entries(prob, pos, dx, dy)
    n = len(ent)
    S = support(Np, r)
    out = dict(objF=np.zeros((B, L, L), np.complex128), pupil=np.zeros((B, Np, Np), np.complex128),
               err=np.empty((n, B)), ref=np.empty((n, B)), Q=np.empty((n, B)), bound_objF=np.zeros(B),
               bound_pupil=np.zeros(B), acc_objF=np.zeros(B), acc_pupil=np.zeros(B))
    for b in range(B):
        O = np.fft.fftshift(np.asarray(state["objF"][b], np.complex128))
        P = np.fft.ifftshift(np.asarray(state["pupil"][b], np.complex128) * S)
        GO, GP = np.zeros((L, L), np.complex128), np.zeros((Np, Np), np.complex128)
        pmax = np.abs(P).max()
        for k, (led, xs, ys) in enumerate(ent):
            W = np.fft.ifftshift(O[ys:ys + Np, xs:xs + Np])
            psi = np.fft.ifft2(W * P)
            a = np.abs(psi)
            g = 1.0 if gains is None else float(gains[led, b])
            s = g * np.sqrt(stack[led, b].astype(np.float64))
            lit = a > 0
            ratio = np.divide(s, a, out=np.zeros_like(a), where=lit)
            rho = np.where(lit, psi * (1.0 - ratio), 0.0)
            R = np.fft.fft2(rho) / (Np * Np)
            tO, tP = 2.0 * np.conj(P) * R, 2.0 * np.conj(W) * R
            GO[ys:ys + Np, xs:xs + Np] += np.fft.fftshift(tO)
            GP += tP
            out["err"][k, b] = ((a - s) ** 2).sum()
            out["ref"][k, b] = float(stack[led, b].astype(np.int64).sum())
            out["Q"][k, b] = (a * a).sum()
            if lit.any():
                c = (np.abs(1.0 - ratio) + ratio)[lit].max()
                d_rho = EPS * np.linalg.norm(a) * c + U * np.linalg.norm(s)
                d_R = d_rho / Np
                out["bound_objF"][b] += 2.0 * pmax * d_R
                out["bound_pupil"][b] += 2.0 * np.abs(W).max() * d_R
            out["acc_objF"][b] += U * np.linalg.norm(tO)
            out["acc_pupil"][b] += U * np.linalg.norm(tP * np.fft.ifftshift(S))
        out["bound_objF"][b] += out["acc_objF"][b]
        out["bound_pupil"][b] += out["acc_pupil"][b]
        out["objF"][b] = np.fft.ifftshift(GO)
        out["pupil"][b] = np.fft.fftshift(GP) * S
    return out


def coverage(prob, pupil, pos=None, dx=None, dy=None):
    """M_k = sum_i |P(k - c_i)|^2, float64 [B][L][L] in objF's un-centred layout."""
    Np, L = prob.np_, prob.L
    w = np.abs(np.asarray(pupil, np.complex128)) ** 2
    M = np.zeros((w.shape[0], L, L))
    for _, xs, ys in entries(prob, pos, dx, dy):
        M[:, ys:ys + Np, xs:xs + Np] += w
    return np.fft.ifftshift(M, axes=(-2, -1))


def object_coverage(prob, objF, pos=None, dx=None, dy=None):
    """M_k = sum_i |O(c_i + k)|^2, float64 [B][Np][Np] in the pupil's centred layout."""
    Np = prob.np_
    w = np.abs(np.fft.fftshift(np.asarray(objF, np.complex128), axes=(-2, -1))) ** 2
    M = np.zeros((w.shape[0], Np, Np))
    for _, xs, ys in entries(prob, pos, dx, dy):
        M += w[:, ys:ys + Np, xs:xs + Np]
    return M


def majorised(z, G, M, Np):
    """z - Np^2 G / (2 M) where M > 0, float64."""
    step = np.zeros(np.shape(z), np.complex128)
    np.divide(Np * Np * np.asarray(G, np.complex128), 2.0 * M, out=step, where=M > 0)
    return np.asarray(z, np.complex128) - step


def union_of_disks(prob, pos=None, dx=None, dy=None):
    """bool [L][L], objF's un-centred layout: the pixels some entry's support disk covers."""
    Np, L = prob.np_, prob.L
    S = support(Np, prob.radius) > 0
    m = np.zeros((L, L), bool)
    for _, xs, ys in entries(prob, pos, dx, dy):
        m[ys:ys + Np, xs:xs + Np] |= S
    return np.fft.ifftshift(m)


def check(tag, got, ref, cap=1e-2):
    """got: Solver.gradient's dict (complex64); ref: gradient()'s.  Prints the
    measured ratio to the bound per output, asserts the bound and its cap
    bound <= cap ||G_ref||; returns the ratios {name: max over patches}."""
    ratios = {}
    for name in ("objF", "pupil"):
        if name not in got:
            continue
        g = got[name]
        assert g.dtype == np.complex64 and g.shape == ref[name].shape, (name, g.dtype, g.shape)
        assert np.all(np.isfinite(g.view(np.float32))), (tag, name)
        B = g.shape[0]
        delta = np.array([np.linalg.norm(g[b].astype(np.complex128) - ref[name][b]) for b in range(B)])
        norm = np.array([np.linalg.norm(ref[name][b]) for b in range(B)])
        bnd = ref["bound_" + name]
        ratio = np.divide(delta, bnd, out=np.where(delta > 0, np.inf, 0.0), where=bnd > 0)
        capr = np.divide(bnd, norm, out=np.zeros_like(bnd), where=norm > 0)
        print(f"gradient {tag} {name}: max ||dG||/bound {ratio.max():.3e}, ||dG||/||G|| "
              f"{np.divide(delta, norm, out=np.zeros_like(delta), where=norm > 0).max():.3e}, bound/||G|| {capr.max():.3e}")
        assert np.all(bnd <= cap * norm), (tag, name, "the bound hides a failure", float(capr.max()))
        assert np.all(delta <= bnd), (tag, name, float(ratio.max()))
        ratios[name] = float(ratio.max())
    return ratios
