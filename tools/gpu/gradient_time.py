"""What fpm_gradient costs beside the residual sweep whose kernels it shares and
beside one iteration of the general path's LED steps, and whether adding it
moved the sweep: prints one JSON line.  predict_time.py's sibling; no effect on
bench.py.

Shape: the bench shape (metric geometry: 256 patches of 256^2, 293 LEDs, the
Np 256 register pair).  After fpm_init and one iteration, in one process:
fpm_residual's event time and, on a library that has it, the event time of
fpm_gradient into device memory with both outputs, with the object only and
with the sums (the median of --reps calls after one warm-up call each), then
the LED-step time of one fpm_run iteration of a general-path context of the
same shape (fpm_timing.led_ms).

With --parent-lib / --parent-python the sweep is also measured on a build of
the parent commit: a round is one child process per library, this tree and the
parent alternating, each child under a time limit; a child that fails ends the
measurement.  same_bits_as_parent: both libraries' sweeps return the same E and
S bytes.  The gate: this tree's median is at most the parent's median plus the
parent's own spread (max - min of its rounds).

usage: python tools/gpu/gradient_time.py [--reps 5] [--parent-lib SO --parent-python DIR [--rounds 3]]
       python tools/gpu/gradient_time.py --one   (a child: the shape on the library FPM_HIP_LIB names)
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# a child of the parent library imports the parent commit's mirror of it
sys.path[:0] = [ROOT, os.environ.get("GRADIENT_TIME_PYTHON") or os.path.join(ROOT, "fpm-opencv_amd", "python")]

NAME, CONFIG, NP, PATCHES = "bench_np256", "metric", 256, 256


def one(reps):
    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench
    from tools.synth_torch import make_stack

    geo = bench.config_geometry(CONFIG, NP)
    stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], PATCHES, device="cuda")
    torch.cuda.synchronize()
    n = int(geo["n_led"])

    def problem(path):
        return fpm_amd.Problem(geo["np_"], geo["L"], np.arange(n), geo["x0"], geo["y0"], geo["r"], geo["d1"], geo["d2"],
                               n_patch=PATCHES, path=path)

    with fpm_amd.Solver(problem(fpm_amd.PATH_AUTO)) as s:
        s.upload_device(stack.data_ptr())
        s.init()
        s.run(1)
        s.residual()  # warm-up (allocates the scratch)
        sweeps = [s.residual() for _ in range(reps)]
        bits = hashlib.sha256(sweeps[0]["err"].tobytes() + sweeps[0]["ref"].tobytes()).hexdigest()
        out = dict(name=NAME, np=geo["np_"], r=geo["r"], L=geo["L"], patches=PATCHES, leds=n,
                   kernel=fpm_amd.KERNEL_NAMES[s.info().fused_kernel], residual_kind=s.debug_plan()["residual_kind"],
                   clock_mhz=s.clock().clock_mhz, sweep_ms=statistics.median(d["ms"] for d in sweeps), sweep_bits=bits)
        if hasattr(s, "gradient"):
            gO = torch.empty((PATCHES, geo["L"], geo["L"], 2), dtype=torch.float32, device="cuda")
            gP = torch.empty((PATCHES, geo["np_"], geo["np_"], 2), dtype=torch.float32, device="cuda")
            for key, ptrs, sums in (("gradient_ms", (gO.data_ptr(), gP.data_ptr()), False),
                                    ("gradient_object_ms", (gO.data_ptr(), None), False),
                                    ("gradient_sums_ms", (gO.data_ptr(), gP.data_ptr()), True)):
                ms = []
                for _ in range(reps + 1):
                    s.gradient(device_ptrs=ptrs, sums=sums)
                    ms.append(s.gradient_ms)
                out[key] = statistics.median(ms[1:])
            out["sweep_after_ms"] = s.residual()["ms"]
            del gO, gP
    if hasattr(fpm_amd.Solver, "gradient"):  # one iteration of the general path's LED steps at the same shape
        with fpm_amd.Solver(problem(fpm_amd.PATH_GENERAL)) as s:
            s.upload_device(stack.data_ptr())
            s.init()
            s.run(1)
            led = []
            for _ in range(min(reps, 3)):
                s.run(1)
                led.append(s.timing().led_ms)
            out["general_iteration_led_ms"] = statistics.median(led)
    del stack
    torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def child(env, reps, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--reps", str(reps)], capture_output=True,
                       text=True, env=dict(os.environ, **env), timeout=limit)
    if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"child exited {r.returncode}")
    return [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-python", default="")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    a = ap.parse_args()
    if a.one:
        return one(a.reps)
    if bool(a.parent_lib) != bool(a.parent_python):
        raise SystemExit("--parent-lib and --parent-python: a build and the Python mirror of the parent commit")
    if not a.parent_lib:
        print(json.dumps(child({}, a.reps, a.limit)))
        return
    envs = {"tree": {}, "parent": {"FPM_HIP_LIB": os.path.abspath(a.parent_lib),
                                   "GRADIENT_TIME_PYTHON": os.path.abspath(a.parent_python)}}
    runs = {w: [] for w in envs}
    for _ in range(a.rounds):
        for who, env in envs.items():
            runs[who].append(child(env, a.reps, a.limit))
    t, p = [x["sweep_ms"] for x in runs["tree"]], [x["sweep_ms"] for x in runs["parent"]]
    mt, mp, spread = statistics.median(t), statistics.median(p), max(p) - min(p)
    d = dict(runs["tree"][-1])
    for key in ("gradient_ms", "gradient_object_ms", "gradient_sums_ms", "general_iteration_led_ms"):
        d[key] = statistics.median(x[key] for x in runs["tree"])
    same = {x["sweep_bits"] for x in runs["tree"]} == {x["sweep_bits"] for x in runs["parent"]}
    d.update(rounds=a.rounds, sweep_tree=t, sweep_parent=p, sweep_ms=mt, sweep_parent_ms=mp, parent_spread=spread,
             tree_over_parent=mt / mp, same_bits_as_parent=same, passes=bool(mt <= mp + spread and same),
             clock_mhz=[x["clock_mhz"] for x in runs["tree"]], clock_mhz_parent=[x["clock_mhz"] for x in runs["parent"]])
    print(json.dumps(d))


if __name__ == "__main__":
    main()
