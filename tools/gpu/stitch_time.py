"""What the last step of a field costs: fpm_stitch_tiles on a 16 x 16 grid of
768^2 tiles in device memory (the bench shape's objCrop tiles, gathered);
prints one JSON line.  No effect on bench.py.

(a) placement  stride L, no alignment, against parallel.stitch on the same
               tensor (torch's copy of the same bytes): bytes moved (tiles read
               once, field written once) over the median time.
(b) overlap    a high-resolution overlap of 96 (stride 672) with alignment
               none, phase and complex: the blend's bytes (every tile pixel read
               once, the field written once) and the pair pass's (both sides of
               every shared region read once).

A round times every variant once, one after the other, so the rounds alternate
them; the line carries every round's value, the median and the spread (max -
min).  Ours is the library's event-to-event time of its kernels (elapsed_ms)
and, beside it, the wall clock of the blocking call; torch's copy is timed by
events around it.

usage: python tools/gpu/stitch_time.py [--rounds 9] [--grid 16] [--tile 768] [--overlap 96]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fpm-opencv_amd", "python")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--tile", type=int, default=768)
    ap.add_argument("--overlap", type=int, default=96)
    a = ap.parse_args()

    import torch
    import fpm_amd
    from fpm_amd import parallel

    G, L, V = a.grid, a.tile, a.overlap
    s = L - V
    gen = torch.Generator(device="cuda").manual_seed(1)
    tiles = torch.randn((G * G, L, L, 2), dtype=torch.float32, device="cuda", generator=gen)
    Hb, Wb = fpm_amd.stitch_shape((G, G), L, s)
    field_a = torch.empty((G * L, G * L, 2), dtype=torch.float32, device="cuda")
    field_b = torch.empty((Hb, Wb, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.cuda.current_device()

    names = ["placement", "torch_placement", "overlap_none", "overlap_phase", "overlap_complex"]
    kernel_ms = {k: [] for k in names}
    wall_ms = {k: [] for k in names if k != "torch_placement"}

    def ours(key, field, stride, align):
        t0 = time.perf_counter()
        _, ms = fpm_amd.stitch_tiles_device(tiles.data_ptr(), field.data_ptr(), (G, G), L, stride, align, dev, stream)
        wall_ms[key].append((time.perf_counter() - t0) * 1e3)
        kernel_ms[key].append(ms)

    def torch_copy():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = parallel.stitch(tiles, (G, G))
        e1.record()
        torch.cuda.synchronize()
        kernel_ms["torch_placement"].append(e0.elapsed_time(e1))
        return out

    def one_round():
        ours("placement", field_a, L, "none")
        ref = torch_copy()
        ours("overlap_none", field_b, s, "none")
        ours("overlap_phase", field_b, s, "phase")
        ours("overlap_complex", field_b, s, "complex")
        return ref

    ref = one_round()  # warm-up: code objects, allocator
    same = bool(torch.equal(ref, field_a))
    del ref
    for v in list(kernel_ms.values()) + list(wall_ms.values()):
        v.clear()
    for _ in range(a.rounds):
        one_round()

    def stat(v):
        return dict(median=statistics.median(v), spread=max(v) - min(v), values=[round(x, 4) for x in v])

    tile_bytes = G * G * L * L * 8
    pairs = 2 * G * (G - 1)
    pair_bytes = pairs * 2 * L * V * 8
    out = dict(shape=dict(grid=[G, G], tile=L, overlap=V, stride=s, field_overlap=[Hb, Wb]), rounds=a.rounds,
               placement_equals_torch=same, tile_bytes=tile_bytes,
               placement_bytes=2 * tile_bytes, blend_bytes=tile_bytes + Hb * Wb * 8, pair_bytes=pair_bytes)
    out["kernel_ms"] = {k: stat(v) for k, v in kernel_ms.items()}
    out["wall_ms"] = {k: stat(v) for k, v in wall_ms.items()}
    km = {k: out["kernel_ms"][k]["median"] for k in names}
    out["placement_tb_per_s"] = 2 * tile_bytes / (km["placement"] * 1e-3) / 1e12
    out["torch_placement_tb_per_s"] = 2 * tile_bytes / (km["torch_placement"] * 1e-3) / 1e12
    out["blend_tb_per_s"] = out["blend_bytes"] / (km["overlap_none"] * 1e-3) / 1e12
    out["align_pass_ms"] = dict(phase=km["overlap_phase"] - km["overlap_none"],
                                complex=km["overlap_complex"] - km["overlap_none"])
    out["pair_tb_per_s"] = pair_bytes / (max(out["align_pass_ms"]["phase"], 1e-9) * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
