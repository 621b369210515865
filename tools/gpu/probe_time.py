"""Times of the window search (fpm_residual_at) beside the sweep it is made of;
prints one JSON line.  No effect on bench.py.

At the metric geometry (bench.config_geometry("metric"): 256 patches, 293 LEDs,
Np 256, r 33), after two run(1):
  sweep         fpm_residual's elapsed_ms on this tree
  sweep_parent  the same on a built checkout of the parent commit
                (--parent-lib its fpm-opencv_amd/lib/libfpm_hip.so,
                --parent-python its fpm-opencv_amd/python, which finds the host
                library beside it): one load per entry against two dependent ones
  probe         a radius-1 search of all LEDs: fpm_residual_at over
                calibrate.probe_list (9 candidates per LED, fewer where a window
                would leave the spectrum), and the same context's sweep
Every measurement runs in a child process of its own (one warm-up, then the
measured call), alternating rounds, each under a time limit.

usage: python tools/gpu/probe_time.py [--rounds 3] [--patches 256] [--parent-lib SO --parent-python DIR]
       python tools/gpu/probe_time.py --one sweep|sweep_parent|probe   (a child)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# a child of sweep_parent imports the parent commit's mirror of its own library
sys.path[:0] = [ROOT, os.environ.get("PROBE_TIME_PYTHON") or os.path.join(ROOT, "fpm-opencv_amd", "python")]


def one(mode, patches):
    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench
    from tools.synth_torch import make_stack

    geo = bench.config_geometry("metric")
    stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], patches, device="cuda")
    torch.cuda.synchronize()
    order = np.arange(geo["n_led"])
    prob = fpm_amd.Problem(geo["np_"], geo["L"], order, geo["x0"], geo["y0"], geo["r"], geo["d1"], geo["d2"],
                           n_patch=patches)
    with fpm_amd.Solver(prob) as s:
        s.upload_device(stack.data_ptr())
        s.init()
        s.run(1)  # warm-up
        s.run(1)
        s.residual()  # warm-up (allocates the scratch)
        d = s.residual()
        out = dict(mode=mode, patches=patches, leds=int(geo["n_led"]), kernel=fpm_amd.KERNEL_NAMES[s.info().fused_kernel],
                   led_ms=s.timing().led_ms, sweep_ms=d["ms"], e_over_s=float(d["err"].sum() / d["ref"].sum()))
        if mode == "probe":
            from fpm_amd import calibrate
            pos, dx, dy, _ = calibrate.probe_list(s.crops(), order, geo["L"], geo["np_"], calibrate.neighbourhood(1))
            s.residual_at(pos, dx, dy)  # warm-up
            p = s.residual_at(pos, dx, dy)
            centre = (dx == 0) & (dy == 0)
            assert np.array_equal(p["err"][centre], d["err"])  # the search's (0, 0) entries are the sweep's rows
            out.update(probe_ms=p["ms"], entries=int(len(pos)))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-python", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.patches)
    parent = bool(a.parent_lib and a.parent_python)
    modes = ["sweep"] + (["sweep_parent"] if parent else []) + ["probe"]
    envs = {"sweep_parent": {"FPM_HIP_LIB": os.path.abspath(a.parent_lib),
                             "PROBE_TIME_PYTHON": os.path.abspath(a.parent_python)}} if parent else {}
    runs = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", m, "--patches", str(a.patches)],
                               capture_output=True, text=True, env=dict(os.environ, **envs.get(m, {})), timeout=a.limit)
            if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{m}: child exited {r.returncode}")
            runs[m].append(json.loads(r.stdout.strip().splitlines()[-1]))

    def med(m, key):
        return statistics.median(x[key] for x in runs[m])

    res = dict(rounds=a.rounds, patches=a.patches, sweep_ms=med("sweep", "sweep_ms"), probe_ms=med("probe", "probe_ms"),
               probe_entries=runs["probe"][0]["entries"], probe_sweep_ms=med("probe", "sweep_ms"),
               fused_led_ms=med("sweep", "led_ms"))
    res["probe_over_sweep"] = res["probe_ms"] / res["probe_sweep_ms"]
    res["probe_entries_over_leds"] = res["probe_entries"] / runs["probe"][0]["leds"]
    if parent:
        p = [x["sweep_ms"] for x in runs["sweep_parent"]]
        res.update(sweep_parent_ms=statistics.median(p), sweep_parent_spread_ms=max(p) - min(p))
        res["sweep_minus_parent_ms"] = res["sweep_ms"] - res["sweep_parent_ms"]
        res["sweep_not_slower_than_parent"] = res["sweep_minus_parent_ms"] <= res["sweep_parent_spread_ms"]
        res["same_bits_as_parent"] = {x["e_over_s"] for x in runs["sweep"]} == {x["e_over_s"] for x in runs["sweep_parent"]}
    res["runs"] = runs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
