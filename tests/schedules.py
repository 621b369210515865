"""Case table of the LED-schedule tests: plain data and builders, no GPU.

tests/test_schedules.py (CPU) checks that every case is a case -- the signal
reaches the corner, the maximum moves, fp32 is precise enough -- and
tests/test_gpu_schedules.py runs the same table on the device.

KERNELS   one row per LED-update kernel, at the smallest shape at which the
          kernel still has its structure (partial 16 x 16 tiles at L 90 / 180 /
          600, tail rows and `towner` pixels at Np 256 / r 33).
S1        a chain of LEDs from the centre to the corner (x0, y0) = (0, L - Np)
          of the spectrum, one LED at odd offsets with x != y, one stack entry
          that is never used at the opposite corner; two iterations.
S2        a 3 x 3 grid walked in an order with immediate and later repeats,
          two LEDs never used, n_order 11 > n_stack 9; init_pos 0 / 1 / last,
          both readings of the cv::add scalar; two iterations.
S3        a phase grating without DC on a 5 x 5 grid, small delta2: the
          maximum of |objF| moves between tiles and decreases; three iterations.

The spectrum's last, partial tile (rows and columns from 16 floor(L / 16) on)
can only be touched by a window that reaches row y0 + Np / 2 + r with
y0 <= L - Np, i.e. row L - Np / 2 + r at the most:
  L 90  / Np 30 / r 5    row 80 = 16 * 5: touched by the corner LED
  L 180 / Np 90 / r 10   row 145 < 176: out of reach; r >= 41 reaches it, so the
                         Np 90 kernel has a second S1 row at r 42 (rows .. 177)
  L 600 / Np 200         the kernel takes r <= 29: row 529 < 592 at the most, so
                         no valid problem reaches the partial tile
                         (PARTIAL_TILE_UNREACHABLE)
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import fpm_amd
from tools.synth import forward_intensities, grid_geometry, make_stack

S2_ORDER = (8, 4, 4, 0, 5, 4, 2, 8, 3, 3, 1)
S2_INIT_POS = (0, 1, 10)
S2_FLAGS = (0, fpm_amd.FLAG_SCALAR_RE_ONLY)
# positions of S2_ORDER that name the same LED: fpm_residual's rows there are bit-equal
S2_REPEATS = ((0, 7), (1, 2, 5), (8, 9))


@dataclass(frozen=True)
class KernelRow:
    name: str
    Np: int
    L: int
    r: int
    B: int
    kernel: int                 # fpm_info.fused_kernel the context must report
    path: int
    env: tuple = ()             # environment switches at fpm_create
    wg: int = 1                 # fpm_info.wg_per_patch
    general_kind: int = -1      # fpm_debug_get_plan (general path)
    flags: int = 0
    schedules: tuple = ("S1", "S2", "S3")
    s2_step: int = 0            # S2 grid step (0: r)
    ledtab: bool = False        # the kernel has the LED-table fallback (ledtab.hpp)
    # S3 tuning (per shape, found on the CPU with run_fpm's record=): grating
    # orders, delta2, seed
    s3: tuple = (0, 0, 0.01, 1)
    # S1's delta2: 10, larger where the complex64 oracle drifts too far with it (test_fp32_headroom)
    s1_delta2: float = 10

    @property
    def fp16(self):
        return bool(self.flags & fpm_amd.FLAG_SPEC_FP16)


_G, _F = fpm_amd.PATH_GENERAL, fpm_amd.PATH_FUSED
_NP256 = dict(Np=256, L=512, r=33, B=2, path=_F, ledtab=True, s3=(20, 15, 0.01, 1))
KERNELS = (
    KernelRow("general_lds", 32, 96, 6, 3, fpm_amd.KERNEL_GENERAL, _G, general_kind=fpm_amd.GENERAL_LDS,
              s3=(4, 3, 0.01, 1)),
    KernelRow("general_lds_L90", 30, 90, 5, 3, fpm_amd.KERNEL_GENERAL, _G, general_kind=fpm_amd.GENERAL_LDS,
              s3=(3, 3, 0.01, 1)),
    KernelRow("fused_small", 32, 96, 6, 2, fpm_amd.KERNEL_FUSED_SMALL, _F, s3=(4, 3, 0.01, 1)),
    KernelRow("fused_small_L90", 30, 90, 5, 2, fpm_amd.KERNEL_FUSED_SMALL, _F, s3=(3, 3, 0.01, 1)),
    KernelRow("fused_np90", 90, 180, 10, 2, fpm_amd.KERNEL_FUSED_NP90, _F, ledtab=True, s3=(6, 6, 0.01, 1)),
    # the radius from which the Np 90 kernel's window reaches the partial tile of L 180 (module docstring)
    KernelRow("fused_np90_r42", 90, 180, 42, 2, fpm_amd.KERNEL_FUSED_NP90, _F, schedules=("S1",)),
    KernelRow("fused_np200", 200, 600, 12, 2, fpm_amd.KERNEL_FUSED_NP200, _F, ledtab=True, s3=(8, 6, 0.01, 1),
              s1_delta2=100),   # 27 LEDs of r 12 in the chain: delta2 10 drifts 1.7e-5 in complex64, 100 3.4e-7
    KernelRow("fused_np256", kernel=fpm_amd.KERNEL_FUSED_NP256, env=(("FPM_NO_SPLIT", "1"), ("FPM_NO_DIST", "1")),
              **_NP256),
    KernelRow("fused_np256_split", kernel=fpm_amd.KERNEL_FUSED_NP256, wg=2,
              env=(("FPM_SPLIT", "2"), ("FPM_NO_DIST", "1")), **_NP256),
    KernelRow("fused_np256_dist", kernel=fpm_amd.KERNEL_FUSED_NP256_DIST, wg=4, env=(("FPM_DIST", "4"),), **_NP256),
    # the geometry of test_unsupported_fused_radius_falls_back_to_general
    KernelRow("general_reg256", 256, 512, 40, 2, fpm_amd.KERNEL_GENERAL, _G, general_kind=fpm_amd.GENERAL_REG256,
              s3=(24, 18, 0.01, 1)),
    KernelRow("general_reg1024", 1024, 2048, 100, 2, fpm_amd.KERNEL_GENERAL, _G,
              general_kind=fpm_amd.GENERAL_REG1024, schedules=("S2",), s2_step=60),
    KernelRow("general_reg1024_fp16", 1024, 2048, 100, 2, fpm_amd.KERNEL_GENERAL, _G,
              general_kind=fpm_amd.GENERAL_REG1024, flags=fpm_amd.FLAG_SPEC_FP16, schedules=("S2",), s2_step=60),
)
ROWS = {k.name: k for k in KERNELS}

# rows whose corner LED must touch the spectrum's partial tile, and the one
# kernel no valid problem brings there: (row, largest radius the kernel takes)
PARTIAL_TILE = ("general_lds_L90", "fused_small_L90", "fused_np90_r42")
PARTIAL_TILE_UNREACHABLE = (("fused_np200", 29),)   # fused_mr.hip fm::RMAX


@dataclass(frozen=True)
class Case:
    """One (kernel row, schedule) pair: what fpm_amd.Problem and the oracles take."""
    row: KernelRow
    sched: str
    tag: str
    x0: tuple
    y0: tuple
    order: tuple
    iters: int
    delta1: float
    delta2: float
    init_pos: int = 1
    flags: int = 0              # besides the row's
    unused: tuple = ()          # stack entries no order[] position names

    @property
    def id(self):
        return f"{self.row.name}-{self.tag}"

    @property
    def all_channels(self):
        return not (self.flags & fpm_amd.FLAG_SCALAR_RE_ONLY)

    @property
    def tol(self):
        """The project's parity bound: relative L2 against
        the fp64 oracle by iterations; fp16 spectrum storage has its own."""
        if self.row.fp16:
            return 1e-2
        return 1e-5 if self.iters <= 1 else 5e-5

    def problem(self):
        r = self.row
        return fpm_amd.Problem(r.Np, r.L, np.array(self.order), np.array(self.x0), np.array(self.y0), r.r,
                               self.delta1, self.delta2, n_patch=r.B, init_pos=self.init_pos, path=r.path,
                               flags=r.flags | self.flags)

    def stack(self):
        return _stack(self)

    def used(self):
        return sorted(set(self.order))

    def box(self, led):
        """(y0, y1, x0, x1), inclusive: the LED's (2r+1)^2 support box in the centred spectrum."""
        r = self.row
        yc, xc = self.y0[led] + r.Np // 2, self.x0[led] + r.Np // 2
        return yc - r.r, yc + r.r, xc - r.r, xc + r.r

    def band(self):
        """(sy0, sy1, sx0, sx1), inclusive: the live band (fpm_state.hpp) of the used LEDs."""
        r = self.row
        b = [r.L // 2 - r.r, r.L // 2 + r.r, r.L // 2 - r.r, r.L // 2 + r.r]
        for led in self.used():
            y0, y1, x0, x1 = self.box(led)
            b = [min(b[0], y0), max(b[1], y1), min(b[2], x0), max(b[3], x1)]
        return max(b[0], 0), min(b[1], r.L - 1), max(b[2], 0), min(b[3], r.L - 1)


def s1_geometry(Np, L, r):
    """Chain to the corner: (x0, y0, order, unused index)."""
    c = L // 2 - Np // 2
    s = max(1, round(r / 1.5))
    assert s * math.sqrt(2) < 2 * r      # neighbouring disks overlap
    K = -(-c // s)
    x0 = [max(c - k * s, 0) for k in range(K + 1)]
    y0 = [min(c + k * s, L - Np) for k in range(K + 1)]
    assert (x0[-1], y0[-1]) == (0, L - Np)
    x0 += [c + 3, L - Np]               # odd offsets, x != y, not tile aligned; the unused corner
    y0 += [c - 7, 0]
    used = range(len(x0) - 1)
    order = sorted(used, key=lambda i: ((x0[i] - c) ** 2 + (y0[i] - c) ** 2, i))
    return tuple(x0), tuple(y0), tuple(order), len(x0) - 1


def grating_stack(Np, L, r, x0, y0, B, kx, ky, seed):
    """S3's measurements: the forward model of a phase grating whose carrier
    has no DC (J0(2.4048) = 0), scaled to a 40000 peak and rounded, no noise."""
    yy, xx = np.mgrid[0:L, 0:L]
    stack = np.empty((len(x0), B, Np, Np), np.uint16)
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        o = np.exp(1j * (2.4048 * np.cos(2 * np.pi * (kx * xx + ky * yy) / L) + 0.2 * rng.standard_normal((L, L))))
        inten = forward_intensities(o, Np, r, list(x0), list(y0))
        stack[:, b] = np.clip(np.rint(inten * (40000.0 / inten.max())), 0, 65535).astype(np.uint16)
    return stack


def _stack(case):
    r = case.row
    return _stack_of(case.sched, r.Np, r.L, r.r, r.B, case.x0, case.y0, r.s3 if case.sched == "S3" else None)


@functools.lru_cache(maxsize=4)
def _stack_of(sched, Np, L, r, B, x0, y0, s3):
    """One stack per (schedule, shape): S2's variants, the Np 256 kernel's three
    modes and the fp16-storage row read the same measurements."""
    if sched == "S3":
        kx, ky, _, seed = s3
        st = grating_stack(Np, L, r, x0, y0, B, kx, ky, seed)
    else:
        st = make_stack(Np, L, r, x0, y0, n_patch=B, seed={"S1": 51, "S2": 52}[sched])
    st.setflags(write=False)
    return st


def _cases():
    out = []
    for row in KERNELS:
        if "S1" in row.schedules:
            x0, y0, order, unused = s1_geometry(row.Np, row.L, row.r)
            out.append(Case(row, "S1", "S1", x0, y0, order, 2, 5, row.s1_delta2, unused=(unused,)))
        if "S2" in row.schedules:
            x0, y0, _ = grid_geometry(row.Np, row.L, 3, row.s2_step or row.r)
            for ip in S2_INIT_POS:
                for fl in S2_FLAGS:
                    out.append(Case(row, "S2", f"S2-init{ip}-{'reonly' if fl else 'cv'}", tuple(int(v) for v in x0),
                                    tuple(int(v) for v in y0), S2_ORDER, 2, 5, 10, init_pos=ip, flags=fl,
                                    unused=(6, 7)))
        if "S3" in row.schedules:
            x0, y0, order = grid_geometry(row.Np, row.L, 5, max(1, round(row.r / 1.5)))
            out.append(Case(row, "S3", "S3", tuple(int(v) for v in x0), tuple(int(v) for v in y0), tuple(order), 3,
                            1, row.s3[2]))
    return tuple(out)


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ---- the oracle's per-step trace of max|objF| (S3) ---------------------------------
def argmax_trace(case, patch=0):
    """The fp64 Python oracle's max|objF| after fpm_init and after every LED
    step of `case`: a list of (led, max, (ty, tx) of the argmax tile), entry 0
    (led -1) the init state."""
    from fpm_oracle import fftshift2, run_fpm
    r = case.row
    st = case.stack()[:, patch]
    kw = dict(all_channels=case.all_channels, init_pos=case.init_pos)
    rec = []
    init = run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, 0, **kw)
    run_fpm(st, case.order, case.x0, case.y0, r.Np, r.L, r.r, case.delta1, case.delta2, case.iters, record=rec, **kw)
    out = []
    for led, objF in [(-1, init["objF"])] + [(led, oF) for led, oF, _ in rec]:
        m = np.abs(fftshift2(objF))
        y, x = np.unravel_index(int(np.argmax(m)), m.shape)
        out.append((led, float(m[y, x]), (y >> 4, x >> 4)))
    return out


def trace_counts(case, trace):
    """(steps where the argmax tile changed, steps where the maximum decreased
    and the new argmax tile lies outside the tile window of the LED just
    processed, steps where it decreased and stayed in its tile)."""
    moved = left = stayed = 0
    for (_, m0, t0), (led, m1, t1) in zip(trace, trace[1:]):
        y0, y1, x0, x1 = case.box(led)
        inside = (y0 >> 4) <= t1[0] <= (y1 >> 4) and (x0 >> 4) <= t1[1] <= (x1 >> 4)
        moved += t1 != t0
        left += m1 < m0 and not inside
        stayed += m1 < m0 and t1 == t0
    return moved, left, stayed
