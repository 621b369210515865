"""What fpm_refocus costs per plane beside the objCrop transform it launches,
and whether adding it moved that transform: prints one JSON line.
predict_time.py's sibling; no effect on bench.py.

Shape: the bench shape (metric geometry: 256 patches of 256^2, L 768, the
register objCrop of L = 256 M).  After fpm_init and --reps iterations of one
fpm_run(ctx, 1) each, in one process:
  objcrop_ms       fpm_timing's objCrop time of an iteration (median): the same
                   transform without the new kernels
  sums_only_ms     per plane, planes == NULL (multiply, transform, sums): the
                   autofocus sweep
  device_ms        per plane into device memory, with sums
  device_nosum_ms  the same without sums (multiply, transform)
  z0_ms            per plane at z = 0 without sums: the transform alone,
                   through fpm_refocus
  mul_ms           device_nosum_ms - z0_ms;  sums_ms = device_ms - device_nosum_ms
  copy_mul_ms      a device-to-device copy of the live band's bytes (it reads and
                   writes what the multiply reads and writes)
  copy_sums_ms     a device-to-device copy of half a plane list's bytes (its
                   traffic is the one read of every plane)
  host_ms, host_wall_ms   per plane into host memory: the kernels' event time
                   and the wall time with the copies (2 planes)
all medians over --reps calls of --planes planes after one warm-up call, event
times of the library (elapsed_ms), with the shader clock of the iteration that
preceded them.

With --parent-lib / --parent-python objcrop_ms is also measured on a build of
the parent commit: a round is one child process per library, this tree and the
parent alternating, each child under a time limit; a child that fails ends the
measurement.  The gate: this tree's median objcrop_ms is at most the parent's
median plus the parent's own spread (max - min of its rounds).

usage: python tools/gpu/refocus_time.py [--reps 5] [--planes 8] [--parent-lib SO --parent-python DIR [--rounds 3]]
       python tools/gpu/refocus_time.py --one   (a child: the shape on the library FPM_HIP_LIB names)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# a child of the parent library imports the parent commit's mirror of it
sys.path[:0] = [ROOT, os.environ.get("REFOCUS_TIME_PYTHON") or os.path.join(ROOT, "fpm-opencv_amd", "python")]

NAME, CONFIG, NP, PATCHES = "bench_np256", "metric", 256, 256


def one(reps, nz):
    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench
    from tools.synth_torch import make_stack

    geo = bench.config_geometry(CONFIG, NP)
    stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], PATCHES, device="cuda")
    torch.cuda.synchronize()
    n, L, B = int(geo["n_led"]), int(geo["L"]), PATCHES
    prob = fpm_amd.Problem(geo["np_"], L, np.arange(n), geo["x0"], geo["y0"], geo["r"], geo["d1"], geo["d2"], n_patch=B)
    with fpm_amd.Solver(prob) as s:
        s.upload_device(stack.data_ptr())
        del stack
        s.init()
        crop = []
        for _ in range(reps + 1):
            s.run(1)
            crop.append(s.timing().objcrop_ms)
        out = dict(name=NAME, np=geo["np_"], L=L, r=geo["r"], patches=B, leds=n, planes=nz,
                   kernel=fpm_amd.KERNEL_NAMES[s.info().fused_kernel], objcrop_kind=s.debug_objcrop_plan()["kind"],
                   clock_mhz=s.clock().clock_mhz, objcrop_ms=statistics.median(crop[1:]))
        if hasattr(s, "refocus"):
            sy0, sy1, sx0, sx1 = s.debug_band()
            hb = max(L // 2 - sy0, sy1 - L // 2, L // 2 - sx0, sx1 - L // 2)
            fl, margin = 0.5 / hb, 8
            zl = np.linspace(-14.0, 14.0, nz) + 0.25   # no plane at z = 0
            dst = torch.empty((nz, B, L, L, 2), dtype=torch.float32, device="cuda")

            def per_plane(**kw):
                ms = []
                for _ in range(reps + 1):
                    s.refocus(kw.pop("zl", zl), fl, margin=margin, **kw)
                    ms.append(s.refocus_ms / nz)
                return statistics.median(ms[1:])

            out["sums_only_ms"] = per_plane(planes=False)
            out["device_ms"] = per_plane(device_ptr=dst.data_ptr())
            out["device_nosum_ms"] = per_plane(device_ptr=dst.data_ptr(), sums=False)
            ms = []
            for _ in range(reps + 1):
                s.refocus(np.zeros(nz), fl, margin=margin, device_ptr=dst.data_ptr(), sums=False)
                ms.append(s.refocus_ms / nz)
            out["z0_ms"] = statistics.median(ms[1:])
            out["mul_ms"] = out["device_nosum_ms"] - out["z0_ms"]
            out["sums_ms"] = out["device_ms"] - out["device_nosum_ms"]

            def copy_ms(nbytes):
                flat = dst.view(-1).view(torch.uint8)
                a, b = flat[:nbytes], flat[flat.numel() // 2:flat.numel() // 2 + nbytes]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ms = []
                for _ in range(reps + 1):
                    ev[0].record()
                    b.copy_(a)
                    ev[1].record()
                    torch.cuda.synchronize()
                    ms.append(ev[0].elapsed_time(ev[1]))
                return statistics.median(ms[1:])

            band_bytes = B * (sy1 - sy0 + 1) * (sx1 - sx0 + 1) * 8
            plane_bytes = B * L * L * 8
            out.update(band=[sy0, sy1, sx0, sx1], band_mb=band_bytes / 1e6, plane_mb=plane_bytes / 1e6,
                       copy_mul_ms=copy_ms(band_bytes), copy_sums_ms=copy_ms(plane_bytes // 2))
            del dst
            torch.cuda.empty_cache()
            s.refocus(zl[:2], fl, margin=margin)  # warm-up
            t0 = time.perf_counter()
            s.refocus(zl[:2], fl, margin=margin)
            out["host_wall_ms"] = (time.perf_counter() - t0) * 1e3 / 2
            out["host_ms"] = s.refocus_ms / 2
            s.run(1)
            out["objcrop_after_ms"] = s.timing().objcrop_ms
            out["device_mb"] = s.info().device_bytes / 1e6
    print(json.dumps(out), flush=True)


def child(env, reps, nz, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--reps", str(reps), "--planes", str(nz)],
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=limit)
    if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"child exited {r.returncode}")
    return [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-python", default="")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    a = ap.parse_args()
    if a.one:
        return one(a.reps, a.planes)
    if bool(a.parent_lib) != bool(a.parent_python):
        raise SystemExit("--parent-lib and --parent-python: a build and the Python mirror of the parent commit")
    if not a.parent_lib:
        print(json.dumps(child({}, a.reps, a.planes, a.limit)))
        return
    envs = {"tree": {}, "parent": {"FPM_HIP_LIB": os.path.abspath(a.parent_lib),
                                   "REFOCUS_TIME_PYTHON": os.path.abspath(a.parent_python)}}
    runs = {w: [] for w in envs}
    for _ in range(a.rounds):
        for who, env in envs.items():
            runs[who].append(child(env, a.reps, a.planes, a.limit))
    t, p = [x["objcrop_ms"] for x in runs["tree"]], [x["objcrop_ms"] for x in runs["parent"]]
    mt, mp, spread = statistics.median(t), statistics.median(p), max(p) - min(p)
    d = dict(runs["tree"][-1])
    for k in ("sums_only_ms", "device_ms", "device_nosum_ms", "z0_ms", "mul_ms", "sums_ms", "copy_mul_ms",
              "copy_sums_ms", "host_ms", "host_wall_ms"):
        d[k] = statistics.median(x[k] for x in runs["tree"])
    d.update(rounds=a.rounds, objcrop_tree=t, objcrop_parent=p, objcrop_ms=mt, objcrop_parent_ms=mp,
             parent_spread=spread, tree_over_parent=mt / mp, passes=bool(mt <= mp + spread),
             clock_mhz=[x["clock_mhz"] for x in runs["tree"]], clock_mhz_parent=[x["clock_mhz"] for x in runs["parent"]])
    print(json.dumps(d))


if __name__ == "__main__":
    main()
