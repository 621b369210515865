"""What installing a state costs: fpm_set_state from host and from device
memory, fpm_download_state_device, and fpm_init on the same context for scale,
at the bench shape (bench.config_geometry("metric", 256): Np 256 / L 768 /
r 33, 256 patches); prints one JSON line.  No effect on bench.py.

The state installed is the one fpm_init leaves (its download), so every call
of a round starts from and ends in the same state.  A round times the four
calls one after the other (wall clock around the blocking call; fpm_init is
followed by a synchronize), the rounds alternate them, and the line carries
every round's value, the median and the spread (max - min).

For the device path the line also gives the bytes the call must move --
the spectrum read once by the check and once by the place and written once,
the live band's tiles read once for the maxima, the pupils read twice and the
boxes written -- and that figure over the median time.

usage: python tools/gpu/state_time.py [--rounds 7] [--patches 256]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--patches", type=int, default=256)
    a = ap.parse_args()

    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench

    geo = bench.config_geometry("metric", 256)
    Np, L, r, B, n = geo["np_"], geo["L"], geo["r"], a.patches, int(geo["n_led"])
    # fpm_init reads one image per patch: any stack times it
    stack = torch.randint(0, 30000, (n, B, Np, Np), dtype=torch.int16, device="cuda")
    tF = torch.empty((B, L, L, 2), dtype=torch.float32, device="cuda")
    tP = torch.empty((B, Np, Np, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    prob = fpm_amd.Problem(Np, L, np.arange(n), geo["x0"], geo["y0"], r, geo["d1"], geo["d2"], n_patch=B)
    times = dict(set_state_host_ms=[], set_state_device_ms=[], download_state_device_ms=[], init_ms=[])

    def timed(key, call):
        t0 = time.perf_counter()
        call()
        times[key].append((time.perf_counter() - t0) * 1e3)

    with fpm_amd.Solver(prob) as s:
        info = s.info()
        s.upload_device(stack.data_ptr())
        s.init()
        s.synchronize()
        host = s.download(objCrop=False, support=False)
        # warm-up: the first call allocates the check scratch
        s.download_state_device(tF.data_ptr(), tP.data_ptr())
        s.set_state_device(tF.data_ptr(), tP.data_ptr())
        for _ in range(a.rounds):
            timed("set_state_host_ms", lambda: s.set_state(host["objF"], host["pupil"]))
            timed("set_state_device_ms", lambda: s.set_state_device(tF.data_ptr(), tP.data_ptr()))
            timed("download_state_device_ms", lambda: s.download_state_device(tF.data_ptr(), tP.data_ptr()))
            timed("init_ms", lambda: (s.init(), s.synchronize()))
        same = all(np.array_equal(s.download(objCrop=False, support=False)[k], host[k]) for k in ("objF", "pupil"))
        # the pixels of the band's tile rectangle (what the maxima pass reads), from the context's own band
        sy0, sy1, sx0, sx1 = s.debug_band()
        band_px = (min(L, (sy1 // 16 + 1) * 16) - sy0 // 16 * 16) * (min(L, (sx1 // 16 + 1) * 16) - sx0 // 16 * 16)

    spec_bytes = B * L * L * 8
    nb = 2 * r + 1
    must = 3 * spec_bytes + B * band_px * 8 + 2 * B * nb * nb * 8 + B * nb * nb * 8
    out = dict(shape=dict(np=Np, L=L, r=r, patches=B), kernel=fpm_amd.KERNEL_NAMES[info.fused_kernel], rounds=a.rounds,
               state_unchanged=bool(same), spectrum_bytes=spec_bytes, device_path_bytes=must)
    for k, v in times.items():
        out[k] = dict(median=statistics.median(v), spread=max(v) - min(v), values=[round(x, 4) for x in v])
    out["device_path_gb_per_s"] = must / (out["set_state_device_ms"]["median"] * 1e-3) / 1e9
    out["download_gb_per_s"] = (2 * spec_bytes) / (out["download_state_device_ms"]["median"] * 1e-3) / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
