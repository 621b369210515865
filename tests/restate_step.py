"""The loop body of oracle/fpm_oracle.py::run_fpm restated from a GIVEN state:
the yardstick for what the oracle cannot express, a crop table that changes
in the middle of a run (fpm_set_crops).  `iterate` continues from any (objF,
pupil) -- a downloaded one, say -- with any table; started from the oracle's
own initial state (`initial_state`) it reproduces run_fpm bit for bit in
float64 (tests/test_probe.py), which is what makes it a yardstick.  Plain
numpy, no GPU.

Line numbers are the reference's (fpmMain.cpp), as in the oracle.
"""
import numpy as np

from fpm_oracle import disk_support, fftshift2


def initial_state(stack, order, np_, L, radius, init_pos=1, dtype=np.complex128):
    """(objF un-centred [L][L], pupil CENTRED [Np][Np]) after :302-343, in the
    conventions of run_fpm's result and of Solver.download()."""
    ct = np.dtype(dtype)
    rt = np.float64 if ct == np.complex128 else np.float32
    support = disk_support(np_, radius).astype(ct)
    amp0 = np.sqrt(np.asarray(stack)[int(order[init_pos])].astype(rt))
    ci = fftshift2(np.fft.fft2(amp0.astype(ct)).astype(ct, copy=False) * support)
    objF = np.zeros((L, L), ct)
    c0 = L // 2 - np_ // 2
    objF[c0:c0 + np_, c0:c0 + np_] = ci
    return fftshift2(objF), fftshift2(support)


def iterate(objF, pupil, stack, order, x0, y0, np_, L, radius, delta1, delta2, iters=1,
            eps=float(np.float32(1e-10)), all_channels=True, dtype=np.complex128, record=None, objf_max=None,
            objcrop=True):
    """`iters` passes over order[] (:345-482) from the state (objF un-centred,
    pupil centred, as downloaded) with the crop table (x0, y0).  Returns
    dict(objF, objCrop, pupil, support) like run_fpm.

    The three last arguments leave the results bit for bit as they are without
    them (tests/test_probe.py).  `record`: a list that receives one dict per
    LED step: led, psi_min = min |psi + eps cs| (the divisor of the amplitude
    replacement), psi_max = max |psi|, objf_max and objf_argmax = max|objF|
    after the step's object update and its (y, x) in the CENTRED spectrum.
    `objf_max(objF_c, led)`
    replaces max|objF| in the pupil update's coefficient (objF_c: the centred
    spectrum after the object update): what a kernel with a wrong maximum would
    compute.  objcrop=False skips the final L x L transform (objCrop is None)."""
    ct = np.dtype(dtype)
    rt = np.float64 if ct == np.complex128 else np.float32
    stack = np.asarray(stack)
    cs = (1 + 1j) if all_channels else 1.0
    support = disk_support(np_, radius).astype(ct)
    objF = np.asarray(objF).astype(ct)
    pupil = fftshift2(np.asarray(pupil).astype(ct))      # un-centred inside the loop
    assert objF.shape == (L, L) and pupil.shape == (np_, np_)
    for _ in range(iters):
        for led in (int(i) for i in order):
            xs, ys = int(x0[led]), int(y0[led])
            objF_c = fftshift2(objF)                                    # :358
            objfcrop = fftshift2(objF_c[ys:ys + np_, xs:xs + np_])      # :361
            objfcropP = objfcrop * pupil                                # :364
            objcropP = np.fft.ifft2(objfcropP).astype(ct, copy=False)   # :365
            object_amp = np.sqrt(stack[led].astype(rt))                 # :378-387
            tmp1 = objcropP + eps * cs                                  # :390
            tmp3 = np.abs(tmp1)                                         # :391
            psi = (float(tmp3.min()), float(np.abs(objcropP).max())) if record is not None else None
            tmp1 = objcropP / tmp3                                      # :392
            tmp3 = tmp1 * object_amp                                    # :393
            objfup = np.fft.fft2(tmp3).astype(ct, copy=False)           # :394
            pupil_abs = np.abs(pupil)
            numerator = (objfup - objfcropP) * (pupil_abs * np.conj(pupil))
            denom = (pupil_abs * pupil_abs + delta2 * cs) * pupil_abs.max()  # :415-418
            tmp2 = numerator / denom                                    # :419
            objF_c = fftshift2(objF)                                    # :427
            objF_c[ys:ys + np_, xs:xs + np_] = fftshift2(tmp2) + objF_c[ys:ys + np_, xs:xs + np_]  # :432-444
            objF = fftshift2(objF_c)                                    # :447
            objfcrop_abs = np.abs(objfcrop)
            objf_abs_max = np.abs(objF).max()                           # :460,467
            if record is not None:
                m = np.abs(fftshift2(objF))
                record.append(dict(led=led, psi_min=psi[0], psi_max=psi[1], objf_max=float(objf_abs_max),
                                   objf_argmax=tuple(int(v) for v in np.unravel_index(int(np.argmax(m)), m.shape))))
            if objf_max is not None:
                objf_abs_max = rt(objf_max(fftshift2(objF), led))
            numerator = (objfup - objfcropP) * (objfcrop_abs * np.conj(objfcrop))
            denom = (objfcrop_abs * objfcrop_abs + delta1 * cs) * objf_abs_max  # :469-470
            pupil = pupil + (numerator / denom) * support               # :471-475
    return dict(objF=objF, objCrop=np.fft.ifft2(objF).astype(ct, copy=False) if objcrop else None,
                pupil=fftshift2(pupil), support=support)
