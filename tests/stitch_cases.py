"""Cases and the float64 restatement of fpm_stitch_tiles (include/fpm_hip.h;
DESIGN.md section 4.9): the feather weights, the alignment factors and the
blend, written from the definition and sharing no code with the library.

A case is (gy, gx, L, sy, sx): gy x gx tiles of L x L at strides (sy, sx).  Each
carries two inputs from a fixed seed:
  consistent   tiles cut from one random complex field and divided by known
               factors (phases in (-pi, pi), scales in [0.5, 2]): aligned and
               blended they must give truth / f_true[0] (a grid whose neighbours
               share no pixel carries one factor for all its tiles);
  independent  unrelated random tiles: only the restatement says what is right.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

ALIGNS = ("none", "phase", "complex")

#        gy gx   L  sy  sx
CASES = {
    "single": (1, 1, 32, 32, 32),             # a single tile
    "max_overlap": (1, 3, 30, 15, 15),        # every interior pixel is shared
    "v1": (3, 1, 32, 31, 32),                 # V = 1
    "unequal_odd": (3, 3, 40, 28, 33),        # unequal overlaps, odd stride, odd W
    "unequal_strides": (2, 3, 34, 17, 20),    # maximum overlap on one axis
    "odd_tile": (2, 2, 33, 20, 21),           # odd L
    "big_pairs": (2, 2, 192, 96, 96),         # pair regions larger than one workgroup's share
    "placement": (2, 3, 32, 32, 32),          # plain placement
}


def shape(gy, gx, L, sy, sx):
    return (gy - 1) * sy + L, (gx - 1) * sx + L


def axis_weights(k: int, n: int, L: int, s: int) -> np.ndarray:
    """Weights [L] of tile k of n along one axis, stride s (overlap V = L - s)."""
    V = L - s
    w = np.ones(L, np.float64)
    for u in range(L):
        if k > 0 and u < V:
            w[u] = (u + 1) / (V + 1)
        elif k < n - 1 and u >= s:
            w[u] = (L - u) / (V + 1)
    return w


def tile_weights(i, j, gy, gx, L, sy, sx) -> np.ndarray:
    return np.outer(axis_weights(i, gy, L, sy), axis_weights(j, gx, L, sx))


def pair_sums(T, gy, gx, L, sy, sx):
    """{(n, t): (c, a, b)} over the pixels neighbours n (left or upper) and t share, unweighted."""
    T = np.asarray(T).astype(np.complex128)
    out = {}
    for i in range(gy):
        for j in range(gx):
            t = i * gx + j
            if j > 0:
                A, B = T[t - 1][:, sx:], T[t][:, :L - sx]
                out[(t - 1, t)] = ((A * B.conj()).sum(), (np.abs(A) ** 2).sum(), (np.abs(B) ** 2).sum())
            if i > 0:
                A, B = T[t - gx][sy:, :], T[t][:L - sy, :]
                out[(t - gx, t)] = ((A * B.conj()).sum(), (np.abs(A) ** 2).sum(), (np.abs(B) ** 2).sum())
    return out


def solve(sums, gy, gx, align):
    """Factors complex128 [gy*gx] from pair_sums' dict, and per tile
    (|z| + sum_n |f[n] c|) / |z|: what an error of the sums, relative to |z| + sum
    |terms|, becomes relative to f[t] = z / |z| (times a scale).  0 where nothing
    is solved."""
    f = np.ones(gy * gx, np.complex128)
    mag = np.zeros(gy * gx)
    if align == "none":
        return f, mag
    for i in range(gy):
        for j in range(gx):
            t = i * gx + j
            nbrs = ([t - 1] if j > 0 else []) + ([t - gx] if i > 0 else [])
            if not nbrs:
                continue
            z = sum(f[n] * sums[(n, t)][0] for n in nbrs)
            num = sum(abs(f[n]) ** 2 * sums[(n, t)][1] for n in nbrs)
            den = sum(sums[(n, t)][2] for n in nbrs)
            if abs(z) == 0 or den == 0:
                continue
            mag[t] = (abs(z) + sum(abs(f[n] * sums[(n, t)][0]) for n in nbrs)) / abs(z)
            f[t] = z / abs(z) * (np.sqrt(num / den) if align == "complex" else 1.0)
    return f, mag


def factors(T, gy, gx, L, sy, sx, align):
    return solve(pair_sums(T, gy, gx, L, sy, sx), gy, gx, align)[0]


def blend(T, f, gy, gx, L, sy, sx):
    """(field complex128 [H][W], bound float64 [H][W] = sum_t w_t |f32(f_t) T_t|): the
    factors enter as the library uses them, rounded to complex64."""
    T = np.asarray(T)
    f32 = np.asarray(f, np.complex128).astype(np.complex64).astype(np.complex128)
    H, W = shape(gy, gx, L, sy, sx)
    out = np.zeros((H, W), np.complex128)
    bound = np.zeros((H, W), np.float64)
    for i in range(gy):
        for j in range(gx):
            t = i * gx + j
            w = tile_weights(i, j, gy, gx, L, sy, sx)
            v = f32[t] * T[t].astype(np.complex128)
            out[i * sy:i * sy + L, j * sx:j * sx + L] += w * v
            bound[i * sy:i * sy + L, j * sx:j * sx + L] += w * np.abs(v)
    return out, bound


def cover_count(gy, gx, L, sy, sx) -> np.ndarray:
    """Tiles over each field pixel, int [H][W]."""
    H, W = shape(gy, gx, L, sy, sx)
    n = np.zeros((H, W), np.int64)
    for i in range(gy):
        for j in range(gx):
            n[i * sy:i * sy + L, j * sx:j * sx + L] += 1
    return n


@dataclass(frozen=True)
class Inputs:
    tiles: np.ndarray          # complex64 [gy*gx][L][L]
    truth: np.ndarray | None   # complex64 [H][W] (consistent)
    f_true: np.ndarray | None  # complex128 [gy*gx]: tiles = cut(truth) / f_true


def _rng(name, kind):
    return np.random.default_rng(zlib.crc32(f"{name}/{kind}".encode()))


@functools.lru_cache(maxsize=None)
def consistent(name: str) -> Inputs:
    gy, gx, L, sy, sx = CASES[name]
    rng = _rng(name, "consistent")
    H, W = shape(gy, gx, L, sy, sx)
    truth = (rng.normal(size=(H, W)) + 1j * rng.normal(size=(H, W))).astype(np.complex64)
    ft = np.exp(1j * rng.uniform(-3.1, 3.1, gy * gx)) * rng.uniform(0.5, 2.0, gy * gx)
    if (gx > 1 and sx == L) or (gy > 1 and sy == L):
        ft[:] = ft[0]   # neighbours that share no pixel cannot be aligned: one factor for every tile
    tiles = np.stack([(truth[i * sy:i * sy + L, j * sx:j * sx + L] / ft[i * gx + j]).astype(np.complex64)
                      for i in range(gy) for j in range(gx)])
    for a in (tiles, truth, ft):
        a.setflags(write=False)
    return Inputs(tiles, truth, ft)


@functools.lru_cache(maxsize=None)
def independent(name: str) -> Inputs:
    gy, gx, L, sy, sx = CASES[name]
    rng = _rng(name, "independent")
    tiles = (rng.normal(size=(gy * gx, L, L)) + 1j * rng.normal(size=(gy * gx, L, L))).astype(np.complex64)
    tiles.setflags(write=False)
    return Inputs(tiles, None, None)


INPUTS = {"consistent": consistent, "independent": independent}


@functools.lru_cache(maxsize=None)
def expected(name: str, kind: str, align: str):
    """(factors, mag, field, bound) of the restatement for one case, input and alignment."""
    g = CASES[name]
    T = INPUTS[kind](name).tiles
    f, mag = solve(_sums(name, kind), g[0], g[1], align)
    field, bound = blend(T, f, *g)
    for a in (f, mag, field, bound):
        a.setflags(write=False)
    return f, mag, field, bound


@functools.lru_cache(maxsize=None)
def _sums(name, kind):
    return pair_sums(INPUTS[kind](name).tiles, *CASES[name])
