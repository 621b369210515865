"""Times of the residual sweep (fpm_residual) beside the LED updates it
monitors; prints one JSON line.  No effect on bench.py.

At the metric geometry (bench.metric_geometry(): 256 patches, 293 LEDs, Np 256,
r 33), after one run(1):
  reg      fpm_residual's elapsed_ms with the register kernel pair, and the same
           context's timing().led_ms of one fused iteration with its clock
  lds      the same with FPM_RES_LDS=1 (the LDS kernel pair, wave-private columns)
  lds_tiled  and with FPM_NO_WAVE_COLS=1 as well (its tiled column kernel)
  general  PATH_GENERAL's led_ms of one iteration of THIS tree (not a build of
           an earlier commit: the residual adds kernels and leaves the step
           kernels' assembly as it was, tools/cmp_asm.py); at this geometry
           that is the Np 256 register kernels, and general_lds is the same
           with FPM_NO_REG256=1 (the LDS step kernels K1-K3)
and at config 5 (Np 1024, L 4096 fp16, 8 patches, 512 LEDs):
  c5       the sweep with the default batching, c5b1 with FPM_RES_BATCH=1.
Every measurement runs in a child process of its own (one warm-up, then the
measured call), three alternating rounds, each under a time limit.

usage: python tools/gpu/residual_time.py [--rounds 3] [--patches 256] [--skip-c5]
       python tools/gpu/residual_time.py --one reg|lds|lds_tiled|general|general_lds|c5|c5b1   (a child)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fpm-opencv_amd", "python")]

ENV = {"lds": {"FPM_RES_LDS": "1"}, "lds_tiled": {"FPM_RES_LDS": "1", "FPM_NO_WAVE_COLS": "1"}, "c5b1": {"FPM_RES_BATCH": "1"}, "general_lds": {"FPM_NO_REG256": "1"}}


def one(mode, patches):
    import numpy as np
    import torch
    import bench
    import fpm_amd
    from tools.synth_torch import make_stack

    c5 = mode.startswith("c5")
    geo = bench.config_geometry("c5" if c5 else "metric")
    B = 8 if c5 else patches
    stack = make_stack(geo["np_"], geo["L"], geo["r"], geo["x0"], geo["y0"], B, device="cuda")
    torch.cuda.synchronize()
    prob = fpm_amd.Problem(geo["np_"], geo["L"], np.arange(geo["n_led"]), geo["x0"], geo["y0"], geo["r"],
                           geo["d1"], geo["d2"], n_patch=B,
                           path=fpm_amd.PATH_GENERAL if mode.startswith("general") else fpm_amd.PATH_AUTO,
                           flags=fpm_amd.FLAG_SPEC_FP16 if c5 else 0)
    with fpm_amd.Solver(prob) as s:
        s.upload_device(stack.data_ptr())
        s.init()
        s.run(1)  # warm-up
        s.run(1)
        t, k = s.timing(), s.clock()
        out = dict(mode=mode, patches=B, leds=int(geo["n_led"]), kernel=fpm_amd.KERNEL_NAMES[s.info().fused_kernel],
                   led_ms=t.led_ms, clock_mhz=k.clock_mhz)
        if not mode.startswith("general"):
            s.residual()  # warm-up (allocates the scratch)
            d = s.residual()
            out.update(sweep_ms=d["ms"], e_over_s=float(d["err"].sum() / d["ref"].sum()))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.patches)
    modes = ["reg", "lds", "lds_tiled", "general", "general_lds"] + ([] if a.skip_c5 else ["c5", "c5b1"])
    runs = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            env = dict(os.environ, **ENV.get(m, {}))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", m, "--patches", str(a.patches)],
                               capture_output=True, text=True, env=env, timeout=a.limit)
            if r.returncode != 0:  # a failed child ends the measurement: nothing more is started
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{m}: child exited {r.returncode}")
            runs[m].append(json.loads(r.stdout.strip().splitlines()[-1]))

    def med(m, key):
        return statistics.median(x[key] for x in runs[m])

    res = dict(rounds=a.rounds, patches=a.patches,
               sweep_reg_ms=med("reg", "sweep_ms"), sweep_lds_ms=med("lds", "sweep_ms"),
               sweep_lds_tiled_ms=med("lds_tiled", "sweep_ms"),
               fused_led_ms=med("reg", "led_ms"), fused_clock_mhz=med("reg", "clock_mhz"),
               general_led_ms=med("general", "led_ms"), general_lds_led_ms=med("general_lds", "led_ms"))
    res["sweep_reg_over_fused_iteration"] = res["sweep_reg_ms"] / res["fused_led_ms"]
    res["sweep_reg_under_general_iteration"] = res["sweep_reg_ms"] < res["general_led_ms"]
    res["sweep_lds_under_general_iteration"] = res["sweep_lds_ms"] < res["general_led_ms"]
    if not a.skip_c5:
        res.update(c5_sweep_ms=med("c5", "sweep_ms"), c5_sweep_batch1_ms=med("c5b1", "sweep_ms"),
                   c5_led_ms=med("c5", "led_ms"))
    res["runs"] = runs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
