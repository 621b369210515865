"""tests/gradient_check.py's own arithmetic, without a GPU: the float64 numpy
yardstick of fpm_gradient against torch.autograd of the same forward model in
complex128 and against central finite differences, the majorised steps it
promises, and an entry that misses the spectrum's support.  Np 16, L 48, r 4,
four overlapping windows (and a fifth LED whose window is dark), gains != 1."""
import types

import numpy as np
import pytest

import gradient_check as gc

NP, L, R, B = 16, 48, 4, 2


def _example(seed=3):
    rng = np.random.default_rng(seed)
    # four windows 4 apart (disks of radius 4 around (22 | 26, 22 | 26) overlap); LED 4's disk
    # (centre 8, 8) lies where the spectrum is zero
    x0, y0 = [14, 18, 14, 18, 0], [14, 14, 18, 18, 0]
    prob = types.SimpleNamespace(np_=NP, L=L, n_patch=B, order=[2, 0, 3, 1], x0=x0, y0=y0, radius=R)
    O = (rng.normal(size=(B, L, L)) + 1j * rng.normal(size=(B, L, L))) * 300.0
    O[:, :14, :] = 0
    O[:, :, :14] = 0
    objF = np.fft.ifftshift(O, axes=(-2, -1))
    pupil = (rng.normal(size=(B, NP, NP)) + 1j * rng.normal(size=(B, NP, NP)) + 2.0) * gc.support(NP, R)
    gains = rng.uniform(0.6, 1.7, size=(5, B))
    # the images of a nearby state (the spectrum perturbed by 30 %), as a camera with these gains records them
    near = objF * (1 + 0.3 * (rng.normal(size=objF.shape) + 1j * rng.normal(size=objF.shape)))
    stack = rng.integers(0, 4000, size=(5, B, NP, NP)).astype(np.uint16)
    for b in range(B):
        On, P = np.fft.fftshift(near[b]), np.fft.ifftshift(pupil[b])
        for led in range(4):
            a = np.abs(np.fft.ifft2(np.fft.ifftshift(On[y0[led]:y0[led] + NP, x0[led]:x0[led] + NP]) * P))
            stack[led, b] = np.minimum(np.rint((a / gains[led, b]) ** 2), 65535)
    return prob, dict(objF=objF, pupil=pupil), stack, gains


def _f(prob, objF, pupil, stack, gains, **kw):
    return gc.cost(objF, pupil, prob, stack, gains, **kw).sum()


def test_yardstick_matches_autograd():
    torch = pytest.importorskip("torch")
    prob, st, stack, gains = _example()
    ref = gc.gradient(st, prob, stack, gains)
    zO = torch.tensor(st["objF"], dtype=torch.complex128, requires_grad=True)
    zP = torch.tensor(st["pupil"], dtype=torch.complex128, requires_grad=True)
    O = torch.fft.fftshift(zO, dim=(-2, -1))
    P = torch.fft.ifftshift(zP * torch.tensor(gc.support(NP, R)), dim=(-2, -1))  # P = ifftshift(pupil support)
    f = 0.0
    for led, xs, ys in gc.entries(prob):
        psi = torch.fft.ifft2(torch.fft.ifftshift(O[:, ys:ys + NP, xs:xs + NP], dim=(-2, -1)) * P)
        s = torch.tensor(gains[led][:, None, None] * np.sqrt(stack[led].astype(np.float64)))
        f = f + ((psi.abs() - s) ** 2).sum()
    f.backward()
    assert abs(float(f.detach()) - ref["err"].sum()) <= 1e-12 * float(f.detach())
    for name, z in (("objF", zO), ("pupil", zP)):
        rel = np.linalg.norm(z.grad.numpy() - ref[name]) / np.linalg.norm(ref[name])
        print(f"yardstick vs autograd, {name}: {rel:.2e}")
        assert rel <= 1e-12, (name, rel)


def test_yardstick_matches_finite_differences():
    prob, st, stack, gains = _example()
    ref = gc.gradient(st, prob, stack, gains)
    rng = np.random.default_rng(11)
    for trial in range(4):
        dO = (rng.normal(size=st["objF"].shape) + 1j * rng.normal(size=st["objF"].shape)) * gc.union_of_disks(prob)
        dP = (rng.normal(size=st["pupil"].shape) + 1j * rng.normal(size=st["pupil"].shape)) * gc.support(NP, R)
        for name, dz in (("objF", dO), ("pupil", dP)):
            h = 1e-6 * np.linalg.norm(st[name]) / np.linalg.norm(dz)
            hi, lo = dict(st), dict(st)
            hi[name], lo[name] = st[name] + h * dz, st[name] - h * dz
            fd = (_f(prob, hi["objF"], hi["pupil"], stack, gains) - _f(prob, lo["objF"], lo["pupil"], stack, gains)) / (2 * h)
            an = (np.conj(ref[name]) * dz).real.sum()
            print(f"finite difference {name} trial {trial}: {abs(fd - an) / abs(an):.2e}")
            assert abs(fd - an) <= 1e-6 * abs(an), (name, trial, fd, an)


def test_probe_lists_moved_windows_and_repeats():
    prob, st, stack, gains = _example()
    ref = gc.gradient(st, prob, stack, gains)
    same = gc.gradient(st, prob, stack, gains, pos=[0, 1, 2, 3])
    np.testing.assert_array_equal(same["objF"], ref["objF"])
    # additive over the list; a repeated entry counts twice
    a, b = gc.gradient(st, prob, stack, gains, pos=[0, 1]), gc.gradient(st, prob, stack, gains, pos=[2, 3, 3])
    both = gc.gradient(st, prob, stack, gains, pos=[0, 1, 2, 3, 3])
    np.testing.assert_allclose(both["objF"], a["objF"] + b["objF"], rtol=0, atol=1e-9 * np.abs(both["objF"]).max())
    np.testing.assert_allclose(both["pupil"], a["pupil"] + b["pupil"], rtol=0, atol=1e-9 * np.abs(both["pupil"]).max())
    moved = gc.gradient(st, prob, stack, gains, pos=[0], dx=[1], dy=[-2])
    assert moved["objF"].shape == ref["objF"].shape and not np.array_equal(moved["objF"], a["objF"])
    # exactly zero outside the disks and outside the support
    for g in (ref, moved):
        assert not np.any(g["pupil"][:, gc.support(NP, R) == 0])
    assert not np.any(ref["objF"][:, ~gc.union_of_disks(prob)])
    assert not np.any(moved["objF"][:, ~gc.union_of_disks(prob, [0], [1], [-2])])


def test_majorised_steps_never_increase_the_cost():
    prob, st, stack, gains = _example()
    objF, pupil = st["objF"].copy(), st["pupil"].copy()
    f = [_f(prob, objF, pupil, stack, gains)]
    for _ in range(6):
        G = gc.gradient(dict(objF=objF, pupil=pupil), prob, stack, gains)["objF"]
        objF = gc.majorised(objF, G, gc.coverage(prob, pupil), NP)
        f.append(_f(prob, objF, pupil, stack, gains))
    for _ in range(6):
        G = gc.gradient(dict(objF=objF, pupil=pupil), prob, stack, gains)["pupil"]
        pupil = gc.majorised(pupil, G, gc.object_coverage(prob, objF), NP)
        f.append(_f(prob, objF, pupil, stack, gains))
    print("majorised steps:", " -> ".join(f"{v:.6g}" for v in f))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(f, f[1:])), f
    assert f[1] < f[0] and f[7] < f[6]


def test_a_window_off_the_support_adds_nothing():
    prob, st, stack, gains = _example()
    prob.order = [2, 0, 3, 1, 4]
    ref = gc.gradient(st, prob, stack, gains, pos=[0, 1, 2, 3])
    dark = gc.gradient(st, prob, stack, gains, pos=[0, 1, 2, 3, 4])
    assert dark["Q"][4].max() == 0 and np.all(dark["err"][4] > 0)  # psi = 0: E = g^2 S
    np.testing.assert_array_equal(dark["objF"], ref["objF"])
    np.testing.assert_array_equal(dark["pupil"], ref["pupil"])
    np.testing.assert_array_equal(dark["bound_objF"], ref["bound_objF"])


def test_check_accepts_fp32_rounding_and_refuses_a_wrong_gradient():
    prob, st, stack, gains = _example()
    ref = gc.gradient(st, prob, stack, gains)
    good = dict(objF=ref["objF"].astype(np.complex64), pupil=ref["pupil"].astype(np.complex64))
    gc.check("example", good, ref)
    for name, bad in (("objF", good["objF"] * np.complex64(1.02)), ("pupil", np.conj(good["pupil"])),
                      ("objF", np.ascontiguousarray(good["objF"].transpose(0, 2, 1)))):
        with pytest.raises(AssertionError):
            gc.check("example, wrong", {name: bad}, ref)
