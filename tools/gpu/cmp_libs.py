"""Bit-identity of two builds of libfpm_hip.so on the same inputs (same-box
checks of changes that must not move a bit, e.g. a reduction rewritten with
DPP moves).  Each library runs in its own process (FPM_HIP_LIB is read at
import); the outputs, the context's fpm_info (the kernel selection and the
device bytes allocated) and the residual sweep's err / ref (fpm_residual after
the run: read-only, so it disturbs nothing before it; its scratch is part of
device_bytes, read after it) are compared exactly.

usage: python tools/gpu/cmp_libs.py [--allow-bytes] [--python-a DIR] <lib_a.so> <lib_b.so>
  --python-a DIR  lib_a is an older commit's build whose exports this tree's
                  Python mirror no longer matches: DIR is that commit's
                  fpm-opencv_amd/python
  --allow-bytes   a change that adds a device buffer (the LED gain table): the
                  device_bytes may differ (the difference is printed), every
                  other figure and every output bit may not
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

G256 = (256, 768, 33, 3, 60)  # Np, L, r, LED grid side, step: metric-like, tail rows and tail pixels
CASES = [  # (name, environment, geometry)
    ("one_workgroup", {"FPM_NO_DIST": "1", "FPM_NO_SPLIT": "1"}, G256),
    ("split_ks2", {"FPM_NO_DIST": "1", "FPM_SPLIT": "2"}, G256),
    ("split_ks4", {"FPM_NO_DIST": "1", "FPM_SPLIT": "4"}, G256),
    ("dist_ks4", {"FPM_DIST": "4"}, G256),
    ("dist_ks8", {"FPM_DIST": "8"}, G256),
    ("np90_s90", {}, (90, 360, 30, 5, 24)),       # k_fused_s90 (configs 1 / 2)
    ("np90_small", {"FPM_NO_S90": "1"}, (90, 360, 30, 5, 24)),  # k_fused_small<90>
    ("np64_small", {}, (64, 256, 20, 3, 16)),     # k_fused_small<0>, the runtime plan
    ("np200_mr", {}, (200, 600, 26, 5, 40)),      # k_fused_mr (config 3)
    # the general path's Np 1024 register kernels + K4 + the L 4096 objCrop
    # passes (config 5 shape at L 2048 / 4096, fp16 spectrum storage: flag 2)
    ("np1024_fp16", {"CMP_FLAGS": "2", "CMP_NPATCH": "1"}, (1024, 4096, 333, 3, 200)),
    ("np1024_fp32", {"CMP_NPATCH": "2"}, (1024, 2048, 120, 3, 100)),
    # the general path's LDS kernels and its launch plan (CMP_PATH: the requested path)
    ("np32_wave_cols", {"CMP_PATH": "general", "CMP_NPATCH": "2"}, (32, 96, 6, 5, 4)),  # tiled rows, wave columns,
                                                                                         # batched objCrop
    ("np32_tiled_cols", {"CMP_PATH": "general", "CMP_NPATCH": "2", "FPM_NO_WAVE_COLS": "1"}, (32, 96, 6, 5, 4)),
    ("np256_reg", {"CMP_NPATCH": "2"}, (256, 768, 84, 3, 60)),                          # Np 256 register kernels
    ("np256_lds", {"CMP_NPATCH": "2", "FPM_NO_REG256": "1"}, (256, 768, 84, 3, 60)),    # LDS kernels at Np 256
    ("np256_direct", {"CMP_NPATCH": "2", "FPM_NO_GRAPH": "1", "FPM_PATCH_GROUPS": "2"},  # direct launches across groups
     (256, 768, 84, 3, 60)),
    ("np1024_lds", {"CMP_NPATCH": "1", "FPM_NO_REG1024": "1"}, (1024, 2048, 120, 3, 100)),  # LDS kernels at Np 1024
    # the one-sequence row kernels (two box rows do not fit a 256-thread tile)
    ("np2700_one_seq", {"CMP_PATH": "general", "CMP_NPATCH": "1"}, (2700, 3000, 4, 2, 100)),
    # the residual sweep's other kernel pairs and batching (the cases above run its default)
    ("res_lds_metric", {"FPM_RES_LDS": "1"}, G256),                                      # LDS pair, wave columns, g 16
    ("res_one_seq_np32", {"CMP_PATH": "general", "CMP_NPATCH": "2", "FPM_RES_ONE_SEQ": "1"}, (32, 96, 6, 5, 4)),
    ("res_batch1_np32", {"CMP_PATH": "general", "CMP_NPATCH": "2", "FPM_RES_BATCH": "1"}, (32, 96, 6, 5, 4)),
    ("res_lds_np256_reg", {"CMP_NPATCH": "2", "FPM_RES_LDS": "1"}, (256, 768, 84, 3, 60)),
]

CHILD = r"""
import sys, numpy as np
import os
sys.path.insert(0, os.environ.get('CMP_PYTHON') or 'fpm-opencv_amd/python'); sys.path.insert(0, '.')
import fpm_amd
from tools.synth import grid_geometry, make_stack
Np, L, r, nside, step = (int(v) for v in sys.argv[2:7])
x0, y0, order = grid_geometry(Np, L, nside, step)
import os
npatch = int(os.environ.get("CMP_NPATCH", "4"))
stack = make_stack(Np, L, r, x0, y0, n_patch=npatch, seed=7)
path = {"auto": fpm_amd.PATH_AUTO, "general": fpm_amd.PATH_GENERAL, "fused": fpm_amd.PATH_FUSED}[
    os.environ.get("CMP_PATH", "auto")]
prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 5, 10, n_patch=npatch, path=path,
                       flags=int(os.environ.get("CMP_FLAGS", "0")))
with fpm_amd.Solver(prob) as s:
    s.upload(stack)
    s.init()
    s.run(2)
    out = s.download()
    res = s.residual()
    i = s.info()  # device_bytes now counts the sweep's scratch
info = np.array([i.path, i.box, i.support_px, i.device_bytes, i.wg_per_patch, i.fused_kernel, i.threads_per_wg],
                dtype=np.int64)  # the plan and the allocation total
np.savez(sys.argv[1], info=info, err=np.asarray(res["err"]), ref=np.asarray(res["ref"]),
         **{k: np.asarray(out[k]) for k in ("objF", "objCrop", "pupil")})
"""


def run(lib, env, geo, path, python=""):
    e = dict(os.environ, FPM_HIP_LIB=os.path.abspath(lib), **env)
    if python:
        e["CMP_PYTHON"] = os.path.abspath(python)
    subprocess.run([sys.executable, "-c", CHILD, path, *map(str, geo)], check=True, env=e, timeout=300)


def main():
    argv = [v for v in sys.argv[1:] if v != "--allow-bytes"]
    allow_bytes = len(argv) != len(sys.argv) - 1
    python_a = ""
    if "--python-a" in argv:
        i = argv.index("--python-a")
        python_a = argv[i + 1]
        del argv[i:i + 2]
    a, b = argv[0], argv[1]
    ok = True
    with tempfile.TemporaryDirectory() as d:
        for name, env, geo in CASES:
            pa, pb = os.path.join(d, f"{name}_a.npz"), os.path.join(d, f"{name}_b.npz")
            run(a, env, geo, pa, python_a)
            run(b, env, geo, pb)
            za, zb = dict(np.load(pa)), dict(np.load(pb))
            extra = ""
            if allow_bytes and za["info"][3] != zb["info"][3]:
                extra = f" (device_bytes {int(za['info'][3])} -> {int(zb['info'][3])})"
                zb["info"][3] = za["info"][3]
            same = all(np.array_equal(za[k], zb[k]) for k in za)
            ok = ok and same
            if same:
                print(f"{name}: bit-identical{extra}")
            else:  # which outputs moved, by how much (relative L2)
                rel = {k: float(np.linalg.norm(za[k] - zb[k]) / max(np.linalg.norm(za[k]), 1e-30))
                       for k in za if not np.array_equal(za[k], zb[k])}
                if "info" in rel:
                    print(f"{name}: info {za['info'].tolist()} != {zb['info'].tolist()}")
                print(f"{name}: DIFFERENT " + " ".join(f"{k} rel {v:.2e}" for k, v in rel.items()))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
