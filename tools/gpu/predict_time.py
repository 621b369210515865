"""What fpm_predict costs beside the residual sweep whose kernels it shares, and
whether adding it moved the sweep: prints one JSON line.  gains_time.py's
sibling; no effect on bench.py.

Shapes: the bench shape (metric geometry: 256 patches of 256^2, 293 LEDs, the
Np 256 register pair) and config 2 (Np 90, 64 patches: general.hip's column
kernels on the g = 9 stack layout).  Per shape, after fpm_init and one
iteration, in one process: fpm_residual's event time and, on a library that has
it, the event time of each kind of fpm_predict into device memory (the median
of --reps calls after one warm-up call each), with the shader clock of the
iteration that preceded them.

With --parent-lib / --parent-python the sweep is also measured on a build of
the parent commit: a round is one child process per library, this tree and the
parent alternating, each child under a time limit; a child that fails ends the
measurement.  same_bits_as_parent: both libraries' sweeps return the same E and
S bytes.  The gate: this tree's median is at most the parent's median plus the
parent's own spread (max - min of its rounds).

usage: python tools/gpu/predict_time.py [--reps 5] [--parent-lib SO --parent-python DIR [--rounds 3]]
       python tools/gpu/predict_time.py --one   (a child: every shape on the library FPM_HIP_LIB names)
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
sys.path[:0] = [ROOT, os.environ.get("PREDICT_TIME_PYTHON") or os.path.join(ROOT, "fpm-opencv_amd", "python")]

CASES = [  # name, config, Np, patches
    ("bench_np256", "metric", 256, 256),
    ("config2_np90", "c2", 90, 64),
]


def one(reps):
    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench
    from tools.synth_torch import make_stack

    for name, config, np_, patches in CASES:
        geo = bench.config_geometry(config, np_)
        stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], patches, device="cuda")
        torch.cuda.synchronize()
        n = int(geo["n_led"])
        prob = fpm_amd.Problem(geo["np_"], geo["L"], np.arange(n), geo["x0"], geo["y0"], geo["r"], geo["d1"], geo["d2"],
                               n_patch=patches)
        with fpm_amd.Solver(prob) as s:
            s.upload_device(stack.data_ptr())
            s.init()
            s.run(1)
            s.residual()  # warm-up (allocates the scratch)
            sweeps = [s.residual() for _ in range(reps)]
            bits = hashlib.sha256(sweeps[0]["err"].tobytes() + sweeps[0]["ref"].tobytes()).hexdigest()
            out = dict(name=name, np=geo["np_"], r=geo["r"], patches=patches, leds=n,
                       kernel=fpm_amd.KERNEL_NAMES[s.info().fused_kernel], residual_kind=s.debug_plan()["residual_kind"],
                       clock_mhz=s.clock().clock_mhz, sweep_ms=statistics.median(d["ms"] for d in sweeps),
                       sweep_bits=bits)
            if hasattr(s, "predict"):
                dst = torch.empty((n, patches, geo["np_"], geo["np_"]), dtype=torch.float32, device="cuda")
                out["out_mb"] = dict(amplitude=dst.numel() * 4 / 1e6, counts=dst.numel() * 2 / 1e6,
                                     diff=dst.numel() * 4 / 1e6)
                for kind in ("amplitude", "counts", "diff"):
                    ms = []
                    for _ in range(reps + 1):
                        s.predict(kind, device_ptr=dst.data_ptr())
                        ms.append(s.predict_ms)
                    out[f"{kind}_ms"] = statistics.median(ms[1:])
                out["sweep_after_ms"] = s.residual()["ms"]
                del dst
        del stack
        torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


def child(env, reps, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--reps", str(reps)], capture_output=True,
                       text=True, env=dict(os.environ, **env), timeout=limit)
    if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"child exited {r.returncode}")
    return {d["name"]: d for d in (json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{"))}


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
        print(json.dumps(dict(shapes=list(child({}, a.reps, a.limit).values()))))
        return
    envs = {"tree": {}, "parent": {"FPM_HIP_LIB": os.path.abspath(a.parent_lib),
                                   "PREDICT_TIME_PYTHON": os.path.abspath(a.parent_python)}}
    runs = {w: [] for w in envs}
    for _ in range(a.rounds):
        for who, env in envs.items():
            runs[who].append(child(env, a.reps, a.limit))
    shapes, ok = [], True
    for name, *_ in CASES:
        t, p = [x[name]["sweep_ms"] for x in runs["tree"]], [x[name]["sweep_ms"] for x in runs["parent"]]
        mt, mp, spread = statistics.median(t), statistics.median(p), max(p) - min(p)
        d = dict(runs["tree"][-1][name])
        for kind in ("amplitude", "counts", "diff"):
            d[f"{kind}_ms"] = statistics.median(x[name][f"{kind}_ms"] for x in runs["tree"])
        same = {x[name]["sweep_bits"] for x in runs["tree"]} == {x[name]["sweep_bits"] for x in runs["parent"]}
        d.update(sweep_tree=t, sweep_parent=p, sweep_ms=mt, sweep_parent_ms=mp, parent_spread=spread,
                 tree_over_parent=mt / mp, same_bits_as_parent=same, passes=bool(mt <= mp + spread and same),
                 clock_mhz=[x[name]["clock_mhz"] for x in runs["tree"]],
                 clock_mhz_parent=[x[name]["clock_mhz"] for x in runs["parent"]])
        ok = ok and d["passes"]
        shapes.append(d)
    print(json.dumps(dict(rounds=a.rounds, all_pass=ok, shapes=shapes)))


if __name__ == "__main__":
    main()
