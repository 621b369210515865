"""Case tables of the loader-preprocessing tests: plain data and builders, no GPU.

fpm_upload_frames (csrc/preprocess.hip, csrc/transfer.cpp) and the host loader
(host/dataset.cpp) restate fpmMain.cpp:124-144: crop, darkfield divide
(cv::divide: round half to even, saturate), bg = (mean1 + mean2) / 2 of the
undivided frame clamped to bgThresh and rounded half away from zero to int16,
saturating subtract.  The GPU then applies the stack permutation of whichever
kernel the context selected (meas_layout).  Two tables:

CASES    edge cases of the arithmetic.  Each is a frame builder plus its
         parameters (Inputs), the branches it claims to reach (BRANCHES) and,
         where the case names one, the bg_val it must give.  reach() counts the
         branches in exact integer / rational arithmetic, independent of the
         oracle's doubles; tests/test_preprocess_cases.py (CPU) checks every
         claim and runs the cases the dataset JSON can express through
         libfpm_host, tests/test_gpu_preprocess.py runs all of them on the device.
LAYOUTS  one row per stack layout a context can have, with the meas_g that
         Solver.debug_plan() must report, so a row that silently selects another
         kernel fails instead of passing on the wrong path.

Contract: bg_val is defined for bg <= 32767.  Above it the reference's
(int16_t)round(bg) is undefined behaviour, as is the host's and the kernel's
cast; every case here stays at or below 32767 (bg_max_int16 sits on it).

Edge-case frames are Np + 40 rows by 2 Np + 33 columns (odd width: rows are
2-byte aligned only), wide enough for two disjoint background windows;
frame_is_patch is Np x Np and sum_over_32_bits uses the layout rows' shape.
Layout frames are Np + 40 rows by Np + 33 columns, odd wherever Np is even.
"""
from __future__ import annotations

import functools
import zlib
from collections import Counter
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import fpm_amd
import fpm_oracle as oracle
from tools.synth import grid_geometry

# every knob fpm_create reads that could move a row to another kernel or layout
KNOBS = ("FPM_NO_S90", "FPM_NO_REG1024", "FPM_NO_REG256", "FPM_NO_SPLIT", "FPM_NO_DIST", "FPM_SPLIT", "FPM_DIST",
         "FPM_PATCH_GROUPS", "FPM_T32")


# ---- inputs --------------------------------------------------------------------------
@dataclass(frozen=True)
class Inputs:
    frames: np.ndarray          # uint16 [n][H][W], read-only
    patches: tuple              # ((x0, y0), ...) one per patch
    bk1: tuple
    bk2: tuple
    bg_threshold: float
    dark_mult: float
    darkfield: np.ndarray       # uint8 [n]
    bg_want: tuple | None = None    # the bg_val per frame the case names (None: whatever the arithmetic gives)
    pins: tuple = ()            # (frame, patch, y, x, value): output pixels the case names

    @property
    def px(self):
        return [p[0] for p in self.patches]

    @property
    def py(self):
        return [p[1] for p in self.patches]


def default_dark(n):
    """Darkfield flags of a case that does not care: both values, first frame dark."""
    return (np.arange(n) % 3 != 1).astype(np.uint8)


def edge_shape(Np):
    return Np + 40, 2 * Np + 33


def edge_windows(Np):
    """Two disjoint background windows of an edge_shape frame; the columns
    Np + 1 .. Np + 29 between them belong to neither."""
    return (1, 3), (Np + 30, 37)


def edge_patches(Np):
    """(0, 0), the far corner, and one with odd x0 and y0."""
    H, W = edge_shape(Np)
    return (0, 0), (W - Np, H - Np), ((Np // 2) | 1, 17)


def _rng(name, Np):
    return np.random.default_rng(zlib.crc32(f"{name}-{Np}".encode()))


def _noise(name, Np, n, hi, shape=None):
    H, W = shape or edge_shape(Np)
    return _rng(name, Np).integers(0, hi + 1, (n, H, W)).astype(np.int64)


def _fill(f, win, Np, value):
    """Set the window of every frame; value is a scalar, [n] or [n][Np][Np]."""
    x, y = win
    v = np.asarray(value)
    f[:, y:y + Np, x:x + Np] = v.reshape(v.shape + (1,) * (3 - v.ndim)) if v.ndim < 3 else v


def _done(f):
    assert f.min() >= 0 and f.max() <= 65535
    f = f.astype(np.uint16)
    f.setflags(write=False)
    return f


def _pin(f, i, Np, y, k, value, want):
    """Put `value` into frame i between the background windows, at row y and
    column 2 + k of the gap as the odd-origin patch sees it; returns the pin."""
    px, py = edge_patches(Np)[2]
    x = Np + 3 + k - px
    assert 0 <= x < Np and 0 <= y < Np and 0 <= k < 27
    f[i, py + y, px + x] = value
    return int(i), 2, y, x, want


# ---- builders: (Np, n, dark) -> Inputs ------------------------------------------------
def _dark_tie(mult, table):
    def build(Np, n, dark):
        f = _noise(f"dark_tie{mult}", Np, n, 4000)
        patches = edge_patches(Np)
        pins = []
        for i in np.flatnonzero(dark):
            pins += [_pin(f, i, Np, 2, k, v, q) for k, (v, q) in enumerate(table)]
        b1, b2 = edge_windows(Np)
        return Inputs(_done(f), patches, b1, b2, 0, mult, dark, bg_want=(0,) * n, pins=tuple(pins))
    return build


def _dark_saturate(Np, n, dark):
    f = _noise("dark_saturate", Np, n, 65535)
    patches = edge_patches(Np)
    pins = []
    for i in np.flatnonzero(dark):
        pins += [_pin(f, i, Np, 1, k, v, q)
                 for k, (v, q) in enumerate(((40000, 65535), (32768, 65535), (32767, 65534), (30000, 60000)))]
    b1, b2 = edge_windows(Np)
    return Inputs(_done(f), patches, b1, b2, 0, 0.5, dark, bg_want=(0,) * n, pins=tuple(pins))


def _bg_case(name, c1, c2, thresh, want, mult=2.0, hi=6000, pins=()):
    """Background windows filled per frame with c1(i), c2(i) ([n] or [n][Np][Np]) over noise."""
    def build(Np, n, dark):
        f = _noise(name, Np, n, hi)
        i = np.arange(n)
        b1, b2 = edge_windows(Np)
        _fill(f, b1, Np, c1(i, Np))
        _fill(f, b2, Np, c2(i, Np))
        patches = edge_patches(Np)
        out = [_pin(f, fr, Np, 4, k, v, q) for fr in range(n) for k, (v, q) in enumerate(pins)]
        return Inputs(_done(f), patches, b1, b2, thresh, mult, dark if mult != 1 else np.zeros(n, np.uint8),
                      bg_want=tuple(int(v) for v in want(i)), pins=tuple(out))
    return build


def _checker(c):
    """Half the window at c, half at c + 1: its mean is c + 0.5 exactly when Np^2 is even."""
    def fill(i, Np):
        assert Np % 2 == 0, "the half-and-half window needs an even Np^2"
        yy, xx = np.mgrid[0:Np, 0:Np]
        return c(i)[:, None, None] + ((yy + xx) & 1)[None]
    return fill


def _const(c):
    return lambda i, Np: c(i)


def _dark_flags(Np, n, dark):
    f = _noise("dark_flags", Np, n, 60000)
    flags = np.resize(np.array([0, 1, 2, 255, 0, 128, 1, 0, 3], np.uint8), n)
    b1, b2 = edge_windows(Np)
    return Inputs(_done(f), edge_patches(Np), b1, b2, 0, 3.0, flags, bg_want=(0,) * n)


def _dark_mult_one(Np, n, dark):
    f = _noise("dark_mult_one", Np, n, 4000)
    b1, b2 = edge_windows(Np)
    return Inputs(_done(f), edge_patches(Np), b1, b2, 1000, 1.0, np.ones(n, np.uint8))


def _levels(n):
    """Per-frame background levels on both sides of a 2500 threshold."""
    return 400 + 2600 * (np.arange(n) % 2) + 37 * np.arange(n)


def _windows_overlap(Np, n, dark):
    H, W = edge_shape(Np)
    f = _noise("windows_overlap", Np, n, 3000) + _levels(n)[:, None, None]
    f[:, H - 30:, W - 50:] += _rng("windows_overlap_hot", Np).integers(0, 60000, (n, 30, 50))   # clear of the window
    bk = (5, 7)
    patches = (bk, bk, (W - Np, H - Np), (0, 0), ((Np // 2) | 1, 9))
    return Inputs(_done(np.minimum(f, 65535)), patches, bk, bk, 2500, 2.0, dark)


def _frame_is_patch(Np, n, dark):
    f = _noise("frame_is_patch", Np, n, 3000, shape=(Np, Np)) + _levels(n)[:, None, None]
    return Inputs(_done(f), ((0, 0),) * 3, (0, 0), (0, 0), 2500, 2.0, dark)


def layout_shape(Np):
    return Np + 40, Np + 33


def _sum_over_32_bits(Np, n, dark):
    H, W = layout_shape(Np)
    f = _noise("sum_over_32_bits", Np, n, 10000, shape=(H, W)) + 15000 + 100 * np.arange(n)[:, None, None]
    b1, b2 = (1, 3), (W - Np - 2, H - Np - 1)
    for i in range(n):
        for x, y in (b1, b2):
            s = int(f[i, y:y + Np, x:x + Np].sum())
            assert s >= 2 ** 32, (Np, s)
    return Inputs(_done(f), ((W - Np, H - Np), (0, 0)), b1, b2, 30000, 2.0, dark)


# ---- the table -----------------------------------------------------------------------
BRANCHES = (
    "dark_tie_even", "dark_tie_odd",    # exact x.5 quotients, by the parity of floor(v / mult)
    "dark_clamp",                       # quotient above 65535
    "dark_flag_other",                  # a frame divided on a flag other than 1
    "dark_mult_one",                    # a flagged frame that is not divided (multiplier 1)
    "dark_divides", "dark_passes",      # divided / undivided frames
    "bg_tie",                           # unclamped bg = k + 0.5 exactly
    "bg_tie_nonpow2",                   # the same with Np^2 no power of two
    "bg_at_threshold",                  # bg == bgThresh: not clamped
    "bg_clamped", "bg_unclamped",
    "bg_threshold_tie",                 # clamped to a threshold of k + 0.5
    "bg_negative", "bg_negative_tie",   # bg_val < 0; clamped to -(k + 0.5)
    "bg_max_int16", "bg_zero",
    "image_unchanged",                  # bg_val 0 and no divide: the patch is the crop
    "sub_clamp_low", "sub_clamp_high",  # the saturating subtract at 0 / at 65535
    "sum_over_32_bits",                 # both window sums >= 2^32
    "windows_coincide", "patch_is_window", "patches_identical", "patch_at_far_corner", "patch_at_origin",
    "patch_odd_origin", "odd_width", "frame_is_patch",
)

EDGE_LAYOUTS = ("small32", "np90", "general64")


@dataclass(frozen=True)
class EdgeCase:
    name: str
    build: object
    reaches: tuple              # branches reach() must count above zero
    layouts: tuple = EDGE_LAYOUTS
    host: bool = True           # the dataset JSON can express it (integer multiplier and threshold, NA flags)

    def inputs(self, Np, n, dark=None):
        dark = default_dark(n) if dark is None else np.asarray(dark, np.uint8)
        inp = self.build(Np, n, dark)
        assert inp.frames.shape[0] == n and len(inp.darkfield) == n
        return inp


def _i(v):
    return lambda i: np.full(len(i), v, np.int64)


CASES = (
    # the two multipliers of the tie cases; each frame set holds ties of both parities of floor(v / mult)
    # multiplier 2: 5/2 -> 2, 7/2 -> 4 (and 1/2 -> 0, 3/2 -> 2): every odd pixel is a tie
    EdgeCase("dark_tie_even", _dark_tie(2.0, ((5, 2), (7, 4), (1, 0), (3, 2), (65535, 32768))),
             ("dark_tie_even", "dark_tie_odd", "dark_divides", "dark_passes")),
    # multiplier 4: 6/4 -> 2, 10/4 -> 2, 14/4 -> 4: every pixel = 2 mod 4 is a tie
    EdgeCase("dark_tie_odd", _dark_tie(4.0, ((6, 2), (10, 2), (14, 4), (2, 0), (7, 2), (9, 2))),
             ("dark_tie_even", "dark_tie_odd", "dark_divides", "dark_passes")),
    EdgeCase("dark_saturate", _dark_saturate, ("dark_clamp", "dark_divides"), host=False),
    EdgeCase("bg_tie", _bg_case("bg_tie", _const(lambda i: 1000 + 3 * i), _const(lambda i: 1001 + 5 * i), 30000,
                                lambda i: 1001 + 4 * i),
             ("bg_tie", "bg_unclamped", "sub_clamp_low", "dark_divides")),
    EdgeCase("bg_tie_nonpow2", _bg_case("bg_tie_nonpow2", _checker(lambda i: 700 + 2 * i),
                                        _checker(lambda i: 900 + 4 * i), 30000, lambda i: 801 + 3 * i),
             ("bg_tie", "bg_tie_nonpow2", "bg_unclamped"), layouts=("np90",)),
    EdgeCase("bg_at_threshold", _bg_case("bg_at_threshold", _const(lambda i: 1500 - 100 * (i % 2)),
                                         _const(lambda i: 1500 + 100 * (i % 2)), 1500, _i(1500)),
             ("bg_at_threshold", "bg_unclamped")),
    EdgeCase("bg_over_threshold", _bg_case("bg_over_threshold", _const(lambda i: 2000 + i), _const(_i(1800)), 1500,
                                           _i(1500)),
             ("bg_clamped",)),
    EdgeCase("bg_fraction_threshold", _bg_case("bg_fraction_threshold", _const(_i(2000)), _const(lambda i: 1900 + i),
                                               999.5, _i(1000)),
             ("bg_clamped", "bg_threshold_tie"), host=False),
    # v + 7 passes 65535 from 65529 on
    EdgeCase("bg_negative_threshold",
             _bg_case("bg_negative_threshold", _const(_i(300)), _const(lambda i: 10 * i), -7, _i(-7), mult=1.0,
                      hi=65535, pins=((65535, 65535), (65529, 65535), (65528, 65535), (65527, 65534), (0, 7))),
             ("bg_clamped", "bg_negative", "sub_clamp_high")),
    # out of the JSON's contract (bgThresh is asInt), in the C ABI's (a double): std::round(-7.5) = -8
    EdgeCase("bg_negative_half_threshold",
             _bg_case("bg_negative_half_threshold", _const(_i(300)), _const(lambda i: 10 * i), -7.5, _i(-8), mult=1.0,
                      hi=65535, pins=((65535, 65535), (65528, 65535), (65527, 65535), (65526, 65534), (0, 8))),
             ("bg_clamped", "bg_negative", "bg_negative_tie", "sub_clamp_high"), host=False),
    EdgeCase("bg_max_int16", _bg_case("bg_max_int16", _const(lambda i: 40000 + i), _const(_i(33000)), 32767,
                                      _i(32767), hi=65535),
             ("bg_clamped", "bg_max_int16", "sub_clamp_low")),
    EdgeCase("bg_zero", _bg_case("bg_zero", _const(_i(0)), _const(_i(0)), 1000, _i(0), mult=1.0),
             ("bg_zero", "bg_unclamped", "image_unchanged")),
    EdgeCase("dark_flags", _dark_flags, ("dark_flag_other", "dark_divides", "dark_passes"), host=False),
    EdgeCase("dark_mult_one", _dark_mult_one, ("dark_mult_one", "dark_passes")),
    EdgeCase("windows_overlap", _windows_overlap,
             ("windows_coincide", "patch_is_window", "patches_identical", "patch_at_far_corner", "patch_at_origin",
              "patch_odd_origin", "odd_width", "bg_clamped", "bg_unclamped", "dark_divides", "dark_passes")),
    EdgeCase("frame_is_patch", _frame_is_patch, ("frame_is_patch", "windows_coincide", "patch_is_window",
                                                 "bg_clamped", "bg_unclamped")),
    EdgeCase("sum_over_32_bits", _sum_over_32_bits, ("sum_over_32_bits", "bg_unclamped", "dark_divides",
                                                     "dark_passes", "odd_width"),
             layouts=("np1024",), host=False),
)
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


# ---- exact restatement: which branches an input reaches -------------------------------
def _round_half_away(q: Fraction) -> int:
    a = abs(q)
    r = a.numerator // a.denominator
    if 2 * (a - r) >= 1:
        r += 1
    return r if q >= 0 else -r


def reach(inp: Inputs, Np: int):
    """(Counter of BRANCHES, want uint16 [n][P][Np][Np], bg_val [n]) in integer and
    rational arithmetic: no double, no oracle."""
    f = inp.frames.astype(np.int64)
    n, H, W = f.shape
    c = Counter()
    m = Fraction(inp.dark_mult)
    thr = Fraction(inp.bg_threshold)
    num, den = m.numerator, m.denominator
    want = np.zeros((n, len(inp.patches), Np, Np), np.uint16)
    bgs = np.zeros(n, np.int64)

    def window(i, w):
        assert 0 <= w[0] <= W - Np and 0 <= w[1] <= H - Np, (w, H, W)
        return f[i, w[1]:w[1] + Np, w[0]:w[0] + Np]

    c["windows_coincide"] = int(inp.bk1 == inp.bk2)
    c["patch_is_window"] = sum(p in (inp.bk1, inp.bk2) for p in inp.patches)
    c["patches_identical"] = len(inp.patches) - len(set(inp.patches))
    c["patch_at_far_corner"] = sum(p == (W - Np, H - Np) and p != (0, 0) for p in inp.patches)
    c["patch_at_origin"] = sum(p == (0, 0) for p in inp.patches)
    c["patch_odd_origin"] = sum(p[0] % 2 == 1 and p[1] % 2 == 1 for p in inp.patches)
    c["odd_width"] = W % 2
    c["frame_is_patch"] = int(H == Np and W == Np)
    for i in range(n):
        s1, s2 = int(window(i, inp.bk1).sum()), int(window(i, inp.bk2).sum())
        c["sum_over_32_bits"] += s1 >= 2 ** 32 and s2 >= 2 ** 32
        bg = Fraction(s1 + s2, 2 * Np * Np)
        tie = bg.denominator == 2
        if bg > thr:
            bg = thr
            c["bg_clamped"] += 1
            c["bg_threshold_tie"] += thr.denominator == 2
            c["bg_negative_tie"] += thr.denominator == 2 and thr < 0
        else:
            c["bg_unclamped"] += 1
            c["bg_at_threshold"] += bg == thr
            c["bg_tie"] += tie
            c["bg_tie_nonpow2"] += tie and (Np & (Np - 1)) != 0
        bgv = _round_half_away(bg)
        assert -32768 <= bgv <= 32767, "bg above int16 is out of contract"
        bgs[i] = bgv
        c["bg_negative"] += bgv < 0
        c["bg_max_int16"] += bgv == 32767
        c["bg_zero"] += bgv == 0
        flag = int(inp.darkfield[i])
        divides = flag != 0 and m != 1
        c["dark_divides"] += divides
        c["dark_passes"] += not divides
        c["dark_flag_other"] += divides and flag != 1
        c["dark_mult_one"] += flag != 0 and m == 1
        for b, p in enumerate(inp.patches):
            v = window(i, p)
            if divides:         # q = v den / num, round half to even, saturate
                a = v * den
                fl, rem2 = a // num, 2 * (a % num)
                tie_px = rem2 == num
                c["dark_tie_even"] += int(np.count_nonzero(tie_px & (fl % 2 == 0)))
                c["dark_tie_odd"] += int(np.count_nonzero(tie_px & (fl % 2 == 1)))
                v = fl + ((rem2 > num) | (tie_px & (fl % 2 == 1)))
                c["dark_clamp"] += int(np.count_nonzero(v > 65535))
                v = np.minimum(v, 65535)
            d = v - bgv
            c["sub_clamp_low"] += int(np.count_nonzero(d < 0))
            c["sub_clamp_high"] += int(np.count_nonzero(d > 65535))
            want[i, b] = np.clip(d, 0, 65535)
            c["image_unchanged"] += bgv == 0 and not divides and np.array_equal(want[i, b], window(i, p))
    return c, want, bgs


def expected(inp: Inputs, Np: int):
    """The oracle's stack uint16 [n][P][Np][Np] and bg_val [n] (fpm_oracle.preprocess_frame)."""
    n = len(inp.frames)
    want = np.zeros((n, len(inp.patches), Np, Np), np.uint16)
    bgs = np.zeros(n, np.int64)
    for i in range(n):
        for b, p in enumerate(inp.patches):
            want[i, b], bgs[i] = oracle.preprocess_frame(inp.frames[i], Np, p, inp.bk1, inp.bk2, inp.bg_threshold,
                                                         inp.dark_mult, bool(inp.darkfield[i]))
    want.setflags(write=False)
    return want, bgs


# ---- stack layouts -------------------------------------------------------------------
@dataclass(frozen=True)
class Layout:
    id: str
    Np: int
    L: int
    r: int
    meas_g: int                 # what Solver.debug_plan() must report
    kernel: str                 # the permutation after an upload
    step: int = 20              # of the LED grid
    n_side: int = 3
    n_patch: int = 3
    path: int = fpm_amd.PATH_AUTO
    env: dict = field(default_factory=dict)     # environment at fpm_create
    solve: bool = True          # init(); run(1) after the frames upload is compared too

    @property
    def n(self):
        return self.n_side ** 2

    def problem(self, n_patch=None):
        x0, y0, order = grid_geometry(self.Np, self.L, self.n_side, self.step)
        return fpm_amd.Problem(self.Np, self.L, order, x0, y0, self.r, 5, 10,
                               n_patch=self.n_patch if n_patch is None else n_patch, path=self.path)

    @property
    def crop_passes(self):
        """Times the x += 256 loops of k_bg_sums / k_crop_patches go round."""
        return -(-self.Np // 256)


GENERAL = fpm_amd.PATH_GENERAL
LAYOUTS = (
    Layout("small32", 32, 96, 6, 32, "k_meas_transpose", step=4),
    Layout("small96", 96, 288, 20, 96, "k_meas_transpose, the largest Np"),
    Layout("small90", 90, 360, 20, 90, "k_meas_transpose, non-power-of-two", env={"FPM_NO_S90": "1"}),
    Layout("np90", 90, 360, 20, 9, "k_meas_layout<90,9>"),
    Layout("np200", 200, 600, 20, 10, "k_meas_layout<200,10>"),
    Layout("np256", 256, 512, 20, 16, "k_meas_layout<256,16>, 132 KB of LDS"),
    # tests/test_gpu_np256.py r35_3patches: beyond the fused kernels' radius, two patch groups
    Layout("reg256", 256, 768, 35, 16, "k_meas_layout<256,16> on a general-path context", step=60),
    Layout("general64", 64, 256, 20, 0, "none", path=GENERAL),
    Layout("general320", 320, 640, 20, 0, "none; the second pass of the x += 256 loops is partial", path=GENERAL),
    Layout("np1024", 1024, 2048, 120, 1024, "k_meas_transpose_tiles; the crop loops take four passes", step=100,
           n_side=2, n_patch=2, solve=False),
)
LAYOUT = {r.id: r for r in LAYOUTS}
assert len(LAYOUT) == len(LAYOUTS)


def edge_runs():
    """(case, layout) of every edge case on the device, in table order."""
    return [(c, LAYOUT[l]) for c in CASES for l in c.layouts]


@functools.lru_cache(maxsize=2)
def layout_inputs(row_id):
    """One random frame set per row: some darkfield frames at multiplier 2, bg on
    both sides of the threshold, windows that overlap the patches and each
    other.  Pixels are A u^3, u uniform: mean A / 4 with a long tail, so a
    divided frame keeps a fifth of its pixels above the undivided frame's bg.
    Even frames have A near 6000 (bg near 1500, unclamped), odd frames A =
    65535 (clamped at 2500)."""
    row = LAYOUT[row_id]
    Np, n = row.Np, row.n
    H, W = layout_shape(Np)
    amp = np.where(np.arange(n) % 2, 65535, 6000 + 100 * np.arange(n))[:, None, None]
    f = np.floor(amp * _rng(f"layout-{row_id}", Np).random((n, H, W)) ** 3).astype(np.int64)
    patches = ((W - Np, H - Np), (0, 0), (17, 21))[:row.n_patch]
    return Inputs(_done(f), patches, (1, 3), (W - Np - 2, H - Np - 1), 2500, 2.0, default_dark(n))


@functools.lru_cache(maxsize=2)
def layout_expected(row_id):
    return expected(layout_inputs(row_id), LAYOUT[row_id].Np)
