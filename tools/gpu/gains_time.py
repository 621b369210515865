"""What the LED gains cost a context that sets none: the times of every LED-update
kernel and of the residual sweep on this tree beside a build of the parent
commit, on one box; prints one JSON line per kernel and one summary line.
probe_time.py's sibling; no effect on bench.py.

Per kernel, at its bench geometry (bench.config_geometry), after one warm-up
iteration:
  fused kernels   cycles_per_launch (fpm_get_clock, block 0's shader cycles: a
                  slower clock does not change them) of two iterations:
                  metric at 256 patches (one workgroup per patch) and its 128 /
                  64 / 32-patch shards (split and distributed modes), config 2
                  (Np 90, 64 patches), config 3 (Np 200, 256 patches)
  general path    led_ms of one iteration: config 5 (Np 1024, fp16 storage, 8
                  patches) and Np 256 / r 84 (config 2's optics at Np 256, 64
                  patches)
  sweep           fpm_residual's ms at the metric geometry, and on this tree the
                  moments sweep's (fpm_moments) beside it
A round is one child process per library that measures every kernel, this tree
and the parent alternating, each child under a time limit; a child that fails
ends the measurement.  The gate (issue "LED gains", section 4): a kernel passes
if this tree's median is at most the parent's median plus the parent's own
spread (max - min of its rounds).

usage: python tools/gpu/gains_time.py --parent-lib SO --parent-python DIR [--rounds 3] [--only NAME,...]
       python tools/gpu/gains_time.py --one      (a child: every kernel on the library FPM_HIP_LIB names)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# a child of the parent library imports the parent commit's mirror of it
sys.path[:0] = [ROOT, os.environ.get("GAINS_TIME_PYTHON") or os.path.join(ROOT, "fpm-opencv_amd", "python")]

CASES = [  # name, config, patches, figure
    ("metric_256", "metric", 256, "cycles"),
    ("metric_128", "metric", 128, "cycles"),
    ("metric_64", "metric", 64, "cycles"),
    ("metric_32", "metric", 32, "cycles"),
    ("config2_np90", "c2", 64, "cycles"),
    ("config3_np200", "c3", 256, "cycles"),
    ("config5_np1024_fp16", "c5", 8, "led_ms"),
    ("np256_r84", "c2np256", 64, "led_ms"),
]


def one(only):
    import numpy as np
    import torch
    import fpm_amd  # before bench, which puts this tree's package first on sys.path
    import bench
    from tools.synth_torch import make_stack

    for name, config, patches, figure in CASES:
        if only and name not in only:
            continue
        geo = bench.config_geometry("c2", 256) if config == "c2np256" else bench.config_geometry(
            config, 90 if config == "c2" else 256)
        stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], patches, device="cuda")
        torch.cuda.synchronize()
        prob = fpm_amd.Problem(geo["np_"], geo["L"], np.arange(geo["n_led"]), geo["x0"], geo["y0"], geo["r"], geo["d1"],
                               geo["d2"], n_patch=patches, flags=fpm_amd.FLAG_SPEC_FP16 if config == "c5" else 0)
        with fpm_amd.Solver(prob) as s:
            s.upload_device(stack.data_ptr())
            s.init()
            s.run(1)  # warm-up
            iters = 2 if figure == "cycles" else 1
            s.run(iters)
            info, t, k = s.info(), s.timing(), s.clock()
            out = dict(name=name, patches=patches, leds=int(geo["n_led"]), kernel=fpm_amd.KERNEL_NAMES[info.fused_kernel],
                       wg_per_patch=info.wg_per_patch, led_ms=t.led_ms / iters, cycles_per_launch=k.cycles_per_launch,
                       clock_mhz=k.clock_mhz, figure=figure)
            if name == "metric_256":
                s.residual()  # warm-up (allocates the scratch)
                d = s.residual()
                out.update(sweep_ms=d["ms"], e_over_s=float(d["err"].sum() / d["ref"].sum()))
                if hasattr(s, "moments"):
                    s.moments()
                    out.update(moments_ms=s.moments()["ms"])
        del stack
        torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-python", default="")
    ap.add_argument("--limit", type=int, default=400, help="seconds per child")
    a = ap.parse_args()
    only = [v for v in a.only.split(",") if v]
    if a.one:
        return one(only)
    if not (a.parent_lib and a.parent_python):
        raise SystemExit("--parent-lib and --parent-python: a build and the Python mirror of the parent commit")
    envs = {"tree": {}, "parent": {"FPM_HIP_LIB": os.path.abspath(a.parent_lib),
                                   "GAINS_TIME_PYTHON": os.path.abspath(a.parent_python)}}
    runs = {w: {} for w in envs}
    for _ in range(a.rounds):
        for who, env in envs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--only", a.only], capture_output=True,
                               text=True, env=dict(os.environ, **env), timeout=a.limit)
            if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{who}: child exited {r.returncode}")
            for line in r.stdout.strip().splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    runs[who].setdefault(d["name"], []).append(d)

    def gate(name, key, rows_t, rows_p):
        t, p = [x[key] for x in rows_t], [x[key] for x in rows_p]
        mt, mp, spread = statistics.median(t), statistics.median(p), max(p) - min(p)
        return dict(name=name, figure=key, kernel=rows_t[0]["kernel"], wg_per_patch=rows_t[0]["wg_per_patch"],
                    patches=rows_t[0]["patches"], tree=t, parent=p, tree_median=mt, parent_median=mp,
                    parent_spread=spread, tree_over_parent=mt / mp, passes=mt <= mp + spread)

    lines = []
    for name, _, _, figure in CASES:
        if name not in runs["tree"]:
            continue
        lines.append(gate(name, "cycles_per_launch" if figure == "cycles" else "led_ms", runs["tree"][name],
                          runs["parent"][name]))
        if name == "metric_256":
            g = gate("sweep_metric_256", "sweep_ms", runs["tree"][name], runs["parent"][name])
            g["moments_ms"] = [x["moments_ms"] for x in runs["tree"][name]]
            g["same_bits_as_parent"] = ({x["e_over_s"] for x in runs["tree"][name]} ==
                                        {x["e_over_s"] for x in runs["parent"][name]})
            lines.append(g)
    for g in lines:
        print(json.dumps(g))
    print(json.dumps(dict(rounds=a.rounds, all_pass=all(g["passes"] for g in lines),
                          failed=[g["name"] for g in lines if not g["passes"]])))


if __name__ == "__main__":
    main()
