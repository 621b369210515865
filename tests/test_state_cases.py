"""tests/state_cases.py holds cases (CPU only): from the seeded state fp32
carries two iterations with a tenth of the parity bound to spare on every
kernel row, the support mask the library applies to a given pupil changes the
result far beyond the bound, and fpmMain refuses an --init-pupil / --init-objf
file it cannot use by naming it, before it needs a GPU.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import state_cases as sc
from dataset_fixture import KEYS, make_dataset
from fpm_oracle import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fpm-opencv_amd", "bin", "fpmMain")
KEYS3 = ("objF", "objCrop", "pupil")


def _shape_key(case):
    r = case.row
    return (r.Np, r.L, r.r, case.x0, case.y0)


@functools.lru_cache(maxsize=2)
def _runs(key):
    """Patch 0 of the rows of one shape: complex128 and complex64 from the masked seed, complex128 from the unmasked."""
    case = next(c for c in sc.CASES if _shape_key(c) == key)
    row = case.row
    objF, P = sc.seed_spectrum(case, 0), sc.seed_pupil(row.Np, row.r)
    masked = P * sc.support_centred(row.Np, row.r)
    return (sc.iterate(case, objF, masked, case.iters), sc.iterate(case, objF, masked, case.iters, dtype=np.complex64),
            sc.iterate(case, objF, P, case.iters))


def test_rows_are_the_issue_s():
    assert sc.ROWS == ("general_lds", "general_lds_L90", "fused_small", "fused_small_L90", "fused_np90", "fused_np200",
                       "fused_np256", "fused_np256_split", "fused_np256_dist", "general_reg256", "general_reg1024",
                       "general_reg1024_fp16")
    assert all(len(c.order) == 11 and c.iters == 2 for c in sc.CASES)


@pytest.mark.parametrize("name", sc.ROWS)
def test_seed_is_a_case(name):
    case = sc.BY_ROW[name]
    row = case.row
    P, S = sc.seed_pupil(row.Np, row.r), sc.support_centred(row.Np, row.r)
    assert P.dtype == np.complex64 and np.abs(P[~S]).min() > 0           # nonzero outside the disk
    y, x = np.unravel_index(int(np.argmax(np.abs(P * S))), P.shape)
    assert (y, x) != (row.Np // 2, row.Np // 2) and abs(np.abs(P * S).max() - 1) > 0.05
    spec = np.fft.fftshift(sc.seed_spectrum(case, 0))
    sy0, sy1, sx0, sx1 = case.band()
    live = np.zeros(spec.shape, bool)
    live[sy0:sy1 + 1, sx0:sx1 + 1] = True
    assert spec.dtype == np.complex64 and not live.all()
    assert np.count_nonzero(spec[~live]) == 0 and np.count_nonzero(spec[live]) == live.sum()
    if row.fp16:   # inside the fp16 storage range (fpm_state.hpp: hscale = 2^-ceil(log2 Np^2))
        assert max(np.abs(spec.real).max(), np.abs(spec.imag).max()) / row.Np ** 2 < 65504


@pytest.mark.parametrize("name", sc.ROWS)
def test_fp32_headroom_and_mask(name):
    case = sc.BY_ROW[name]
    r128, r64, unmasked = _runs(_shape_key(case))
    e = {k: rel_l2(r64[k], r128[k]) for k in KEYS3}
    d = rel_l2(unmasked["objF"], r128["objF"])
    print(f"{name}: complex64 vs complex128 {max(e.values()):.1e}; unmasked vs masked objF {d:.2f}")
    assert max(e.values()) < 5e-5 / 10, e
    assert d > 1e-2, d


# ---- fpmMain --init-pupil / --init-objf: files checked before the GPU -------------------------
NP = KEYS["cropSizeX"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(str(tmp_path_factory.mktemp("state_ds")), leds=range(1, 4))


def _fpm(dataset, *extra):
    e = dict(os.environ)
    e.pop("OPENCV_OPENCL_DEVICE", None)
    return subprocess.run([BIN, dataset["json"], "1", "--out", os.path.dirname(dataset["json"]), *extra],
                          capture_output=True, text=True, env=e, timeout=120)


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


P32 = np.ones((NP, NP), np.complex64)
BAD = [
    ("fortran.npy", sc.npy_bytes(P32, fortran=True), "Fortran"),
    ("dtype.npy", sc.npy_bytes(P32.astype(np.complex128)), "<c16"),
    ("real.npy", sc.npy_bytes(P32.real.copy()), "<f4"),
    ("shape.npy", sc.npy_bytes(np.ones((NP, NP + 2), np.complex64)), f"expected ({NP}, {NP})"),
    ("patches.npy", sc.npy_bytes(np.ones((3, NP, NP), np.complex64)), f"(1, {NP}, {NP})"),
    ("short.npy", sc.npy_bytes(P32)[:-8], "fewer values"),
    # a header that claims 2^62 values is refused by its shape, before a byte is allocated for them
    ("huge.npy", sc.npy_bytes(P32, shape=(2 ** 31, 2 ** 31)), f"shape ({2 ** 31}, {2 ** 31}), expected ({NP}, {NP})"),
    ("huge3.npy", sc.npy_bytes(P32, shape=(1, 2 ** 17, 2 ** 17)), f"expected ({NP}, {NP})"),
    ("v3.npy", sc.npy_bytes(P32, version=(1, 0)).replace(b"NUMPY\x01", b"NUMPY\x03"), "version"),
    ("text.npy", b"not an array", "not a .npy"),
]


@pytest.mark.parametrize("name,data,match", BAD, ids=[b[0] for b in BAD])
def test_bad_init_pupil_names_the_file(dataset, tmp_path, name, data, match):
    path = _write(tmp_path, name, data)
    r = _fpm(dataset, "--init-pupil", path)
    assert r.returncode != 0, r.stdout
    assert path in r.stderr and match in r.stderr, r.stderr
    assert "Loading Images" not in r.stdout          # refused before the loader and the GPU


def test_bad_init_objf_names_the_file_and_the_shape(dataset, tmp_path):
    path = _write(tmp_path, "objf.npy", sc.npy_bytes(P32))
    r = _fpm(dataset, "--init-objf", path)
    assert r.returncode != 0 and path in r.stderr and "[Nlarge][Nlarge]" in r.stderr, r.stderr
    r = _fpm(dataset, "--init-objf", path, "--grid", "2x1")
    assert r.returncode != 0 and path in r.stderr and "single-patch" in r.stderr, r.stderr
    r = _fpm(dataset, "--init-objf", str(tmp_path / "missing.npy"))
    assert r.returncode != 0 and "missing.npy" in r.stderr and "cannot open" in r.stderr, r.stderr


@pytest.mark.parametrize("version", [(1, 0), (2, 0)])
def test_good_headers_pass_the_file_check(dataset, tmp_path, version):
    """Version 1.0 and 2.0 headers, [Np][Np] and [patches][Np][Np]: the run gets
    past the file check to the loader (and ends wherever a machine without a GPU ends)."""
    for tag, a, extra in (("shared", P32, []), ("per_patch", np.ones((2, NP, NP), np.complex64), ["--grid", "2x1"])):
        path = _write(tmp_path, f"{tag}.npy", sc.npy_bytes(a, version=version))
        r = _fpm(dataset, "--init-pupil", path, *extra)
        assert "Loading Images" in r.stdout and "--init-pupil" not in r.stderr, r.stderr
        assert np.array_equal(np.load(path), a)    # the hand-written header is one numpy reads too
