"""Descent on the data-fidelity cost f = sum (|psi| - g sqrt(I))^2 with
Solver.gradient (fpm_gradient).

The amplitude cost is majorised by sum |psi - g sqrt(I) e^{i theta}|^2 with the
current phases theta.  psi is linear in the object, psi = A objF, and A^H A is
diagonal: M_k / Np^2 with M_k = sum_i |P(k - c_i)|^2 (c_i the window's
position), so the majoriser's minimiser is per pixel
    objF <- objF - Np^2 G_objF / (2 M)      where M > 0
and it never increases f with the pupil held fixed (object_step).  The same
holds for the pupil with the object fixed and M_k = sum_i |O(c_i + k)|^2
(pupil_step).  G is Solver.gradient's, df/dRe + i df/dIm.

fpm_set_state's band rule: the spectrum it is given must stay exactly zero
outside the context's live band (the support boxes of the init placement and
of the used LEDs).  The gradient of the context's own list already is, so a
step of this module keeps the rule; a regulariser or an optimiser of the
caller's must mask its update the same way.

CostFunction makes f a differentiable function of device tensors for
torch.optim (Adam, L-BFGS): nothing leaves the device but the sums.
"""
from __future__ import annotations

import numpy as np


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _entries(prob, pos, dx, dy):
    order = [int(v) for v in prob.order]
    pos = range(len(order)) if pos is None else [int(p) for p in pos]
    pos = list(pos)
    dx = [0] * len(pos) if dx is None else [int(v) for v in dx]
    dy = [0] * len(pos) if dy is None else [int(v) for v in dy]
    return [(int(prob.x0[order[p]]) + dx[k], int(prob.y0[order[p]]) + dy[k]) for k, p in enumerate(pos)]


def coverage(prob, pupil, pos=None, dx=None, dy=None):
    """M_k = sum_i |P(k - c_i)|^2 of the object step, [n_patch][L][L] in objF's
    (un-centred) layout.  pupil: download()'s centred [n_patch][Np][Np], numpy
    or a torch tensor (then M is a tensor on its device).  The entries are
    Solver.gradient's (default: order[] with its own windows)."""
    Np, L = prob.np_, prob.L
    if _is_torch(pupil):
        import torch
        w = pupil.real ** 2 + pupil.imag ** 2
        M = torch.zeros((w.shape[0], L, L), dtype=w.dtype, device=w.device)
        for xs, ys in _entries(prob, pos, dx, dy):
            M[:, ys:ys + Np, xs:xs + Np] += w
        return torch.fft.ifftshift(M, dim=(-2, -1))
    p = np.asarray(pupil)
    w = p.real.astype(np.float64) ** 2 + p.imag.astype(np.float64) ** 2
    M = np.zeros((w.shape[0], L, L))
    for xs, ys in _entries(prob, pos, dx, dy):
        M[:, ys:ys + Np, xs:xs + Np] += w
    return np.fft.ifftshift(M, axes=(-2, -1))


def object_coverage(prob, objF, pos=None, dx=None, dy=None):
    """M_k = sum_i |O(c_i + k)|^2 of the pupil step, [n_patch][Np][Np] in the
    pupil's (centred) layout.  objF: download()'s un-centred [n_patch][L][L],
    numpy or a torch tensor."""
    Np = prob.np_
    if _is_torch(objF):
        import torch
        O = torch.fft.fftshift(objF, dim=(-2, -1))
        w = O.real ** 2 + O.imag ** 2
        M = torch.zeros((w.shape[0], Np, Np), dtype=w.dtype, device=w.device)
        for xs, ys in _entries(prob, pos, dx, dy):
            M += w[:, ys:ys + Np, xs:xs + Np]
        return M
    O = np.fft.fftshift(np.asarray(objF), axes=(-2, -1))
    w = O.real.astype(np.float64) ** 2 + O.imag.astype(np.float64) ** 2
    M = np.zeros((w.shape[0], Np, Np))
    for xs, ys in _entries(prob, pos, dx, dy):
        M += w[:, ys:ys + Np, xs:xs + Np]
    return M


def majorised(z, G, M, Np: int):
    """z - Np^2 G / (2 M) where M > 0, z elsewhere; float64 arithmetic, z's dtype."""
    z = np.asarray(z)
    step = np.zeros(z.shape, np.complex128)
    np.divide(Np * Np * np.asarray(G, np.complex128), 2.0 * M, out=step, where=M > 0)
    return (z.astype(np.complex128) - step).astype(z.dtype)


def object_step(solver):
    """One majorised step of the spectrum with the pupil held fixed: gradient,
    M, set_state.  Never increases f.  A host round trip: the state and the
    gradient are downloaded, M and the step are formed in numpy float64 and the
    new spectrum is uploaded again (CostFunction keeps everything on the device)."""
    prob = solver.prob
    st = solver.download(objCrop=False, support=False)
    G = solver.gradient(pupil=False)["objF"]
    solver.set_state(objF=majorised(st["objF"], G, coverage(prob, st["pupil"]), prob.np_))


def pupil_step(solver):
    """One majorised step of the pupil with the spectrum held fixed; a host round
    trip as object_step."""
    prob = solver.prob
    st = solver.download(objCrop=False, support=False)
    G = solver.gradient(objF=False)["pupil"]
    solver.set_state(pupil=majorised(st["pupil"], G, object_coverage(prob, st["objF"]), prob.np_))


def _cost_function():
    import torch

    class CostFunction(torch.autograd.Function):
        """f(objF, pupil) = sum E of a Solver with a stack uploaded, for device
        tensors in download()'s layouts (complex64, contiguous, on the
        solver's device): CostFunction.apply(objF, pupil, solver).  forward
        installs the pair with fpm_set_state(FPM_STATE_DEVICE) and returns
        f = sum of fpm_residual's E (float64, on the device); backward installs
        it again (the context may have moved since) and returns the two
        gradients from one fpm_gradient(FPM_GRAD_DEVICE) call, times grad_out:
        the product is formed in float64 and rounded once to complex64, so
        grad_out = 1 returns fpm_gradient's bits."""

        @staticmethod
        def forward(ctx, objF, pupil, solver):
            objF, pupil = objF.detach().contiguous(), pupil.detach().contiguous()
            ctx.solver = solver
            ctx.save_for_backward(objF, pupil)
            torch.cuda.current_stream(objF.device).synchronize()
            solver.set_state_device(objF.data_ptr(), pupil.data_ptr())
            return torch.tensor(float(solver.residual()["err"].sum()), dtype=torch.float64, device=objF.device)

        @staticmethod
        def backward(ctx, grad_out):
            objF, pupil = ctx.saved_tensors
            gO, gP = torch.empty_like(objF), torch.empty_like(pupil)
            torch.cuda.current_stream(objF.device).synchronize()
            ctx.solver.set_state_device(objF.data_ptr(), pupil.data_ptr())
            ctx.solver.gradient(device_ptrs=(gO.data_ptr(), gP.data_ptr()))
            s = grad_out.to(torch.float64)
            return (gO * s).to(gO.dtype), (gP * s).to(gP.dtype), None

    return CostFunction


def __getattr__(name):  # CostFunction needs torch: made on first use
    if name == "CostFunction":
        cls = _cost_function()
        globals()["CostFunction"] = cls
        return cls
    raise AttributeError(name)
