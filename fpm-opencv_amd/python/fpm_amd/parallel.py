"""Patch sharding, the final objCrop gather and stitching.

Patches are independent FPM problems (the per-LED crop offsets depend only on
the LED position, fpmMain.cpp:146-168), so a field of P patches is split into
contiguous blocks, one per rank, with no collective inside an iteration.  The
only exchange is one gather of every rank's high-resolution tiles to rank 0
after the last iteration, followed by placing tile i at its (row, column) of
the patch grid.  Tiles cut at a stride of a whole tile do not overlap, so
stitching them is pure placement (stitch); tiles cut with an overlap are
brought to a common phase and feathered together on the GPU (stitch_blend,
fpm_stitch_tiles).  The reference processes a single patch, so stitching is
new here.

torch.distributed carries the gather (backend "nccl" = RCCL over xGMI on the
GPU box, "gloo" in the CPU tests); nothing here touches the solver itself.
"""
from __future__ import annotations

import numpy as np


def shard_range(total: int, world: int, rank: int) -> tuple[int, int]:
    """Half-open patch range [lo, hi) owned by `rank`: contiguous blocks of
    ceil(total/world), the last rank taking the remainder (possibly empty)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    per = -(-total // world)
    lo = min(total, rank * per)
    return lo, min(total, lo + per)


def gather_tiles(tiles, dist, dst: int = 0):
    """Gather every rank's [n_local, L, L, 2] float32 tiles onto `dst`.

    Ranks may own different patch counts (the last shard can be short), so the
    local tensor is padded to the largest shard; rank `dst` returns the
    concatenation in rank order with the padding dropped, other ranks None."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    n = torch.tensor([tiles.shape[0]], dtype=torch.int64, device=tiles.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n)
    counts = [int(c.item()) for c in counts]
    nmax = max(counts)
    if tiles.shape[0] < nmax:
        pad = torch.zeros((nmax - tiles.shape[0],) + tuple(tiles.shape[1:]), dtype=tiles.dtype, device=tiles.device)
        tiles = torch.cat([tiles, pad])
    bufs = [torch.empty_like(tiles) for _ in range(world)] if rank == dst else None
    dist.gather(tiles.contiguous(), bufs, dst=dst)
    if rank != dst:
        return None
    return torch.cat([b[:c] for b, c in zip(bufs, counts)])


def field_grid(total: int) -> tuple[int, int]:
    """(gy, gx) of the most nearly square grid with gy * gx == total, gy <= gx
    (1024 patches -> 32 x 32)."""
    gy = int(total ** 0.5)
    while gy > 1 and total % gy:
        gy -= 1
    return max(gy, 1), total // max(gy, 1)


def stitch(tiles, grid: tuple[int, int]):
    """Place tiles [P, L, L(, 2)] (row-major patch order) on a grid (gy, gx):
    tile i lands at rows (i // gx)*L and columns (i % gx)*L.  numpy arrays
    and torch tensors (e.g. the gathered tiles still on rank 0's GPU) alike."""
    gy, gx = grid
    P, L = tiles.shape[0], tiles.shape[1]
    if P != gy * gx:
        raise ValueError(f"{P} tiles for a {gy}x{gx} grid")
    rest = tuple(tiles.shape[3:])
    out = tiles.reshape((gy, gx, L, L) + rest).swapaxes(1, 2).reshape((gy * L, gx * L) + rest)
    return np.ascontiguousarray(out) if isinstance(out, np.ndarray) else out.contiguous()


def stitch_blend(tiles, grid: tuple[int, int], stride, align: str = "none"):
    """Blend OVERLAPPING tiles [P, L, L(, 2)] (row-major patch order) cut at
    strides `stride` (an int or (stride_y, stride_x), ceil(L/2) .. L) into one
    field: neighbours are brought to a common phase (align="phase") or phase
    and scale ("complex") from the pixels they share and feathered together
    (fpm_stitch_tiles, fpm_hip.h).  Returns (field,
    factors), factors complex128 [P].

    A torch tensor on the GPU (e.g. the gathered tiles on rank 0) is read in
    place and the field is a torch tensor on the same device, of the tiles'
    layout (complex64 [H, W] or float32 [H, W, 2]); a numpy array goes through
    the host path.  At stride L without alignment the field is stitch()'s."""
    import fpm_amd
    gy, gx = grid
    if tiles.shape[0] != gy * gx:
        raise ValueError(f"{tiles.shape[0]} tiles for a {gy}x{gx} grid")
    if isinstance(tiles, np.ndarray):
        return fpm_amd.stitch_tiles(tiles, grid, stride, align)
    import torch
    if not tiles.is_cuda:
        raise ValueError("stitch_blend: a torch tensor must be on the GPU (numpy arrays take the host path)")
    pairs = not tiles.is_complex()
    if (tiles.dtype != (torch.float32 if pairs else torch.complex64) or tiles.dim() != (4 if pairs else 3)
            or (pairs and tiles.shape[-1] != 2) or tiles.shape[1] != tiles.shape[2]):
        raise ValueError(f"tiles {tiles.dtype} {tuple(tiles.shape)}: want complex64 [P, L, L] or float32 [P, L, L, 2]")
    t = tiles.contiguous()
    L = t.shape[1]
    H, W = fpm_amd.stitch_shape(grid, L, stride)
    field = torch.empty((H, W, 2) if pairs else (H, W), dtype=t.dtype, device=t.device)
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(t.device).cuda_stream
    fac, _ = fpm_amd.stitch_tiles_device(t.data_ptr(), field.data_ptr(), grid, L, stride, align, dev, stream)
    return field, fac
