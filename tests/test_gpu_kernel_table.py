"""fpm_info of every kernel selection: the kernel code, its threads per
workgroup and the workgroups per patch, one row per selection (the table
ctx.hpp keeps per kernel), and the path, which follows from the kernel."""
import pytest

import fpm_amd
from tools.synth import grid_geometry

pytestmark = pytest.mark.gpu

CASES = [  # id, Np, L, r, path, env, (fused_kernel, threads_per_wg, wg_per_patch)
    ("np256", 256, 512, 20, fpm_amd.PATH_AUTO, {"FPM_NO_SPLIT": "1", "FPM_NO_DIST": "1"},
     (fpm_amd.KERNEL_FUSED_NP256, 512, 1)),
    ("split2", 256, 512, 20, fpm_amd.PATH_AUTO, {"FPM_SPLIT": "2", "FPM_NO_DIST": "1"},
     (fpm_amd.KERNEL_FUSED_NP256, 512, 2)),
    ("dist4", 256, 512, 20, fpm_amd.PATH_AUTO, {"FPM_DIST": "4"}, (fpm_amd.KERNEL_FUSED_NP256_DIST, 512, 4)),
    ("np200", 200, 600, 20, fpm_amd.PATH_AUTO, {}, (fpm_amd.KERNEL_FUSED_NP200, 768, 1)),
    ("np90", 90, 360, 20, fpm_amd.PATH_AUTO, {}, (fpm_amd.KERNEL_FUSED_NP90, 1024, 1)),
    ("np90_small", 90, 360, 20, fpm_amd.PATH_AUTO, {"FPM_NO_S90": "1"}, (fpm_amd.KERNEL_FUSED_SMALL, 1024, 1)),
    ("np64", 64, 256, 20, fpm_amd.PATH_AUTO, {}, (fpm_amd.KERNEL_FUSED_SMALL, 1024, 1)),
    ("general", 64, 256, 20, fpm_amd.PATH_GENERAL, {}, (fpm_amd.KERNEL_GENERAL, 0, 1)),
]


@pytest.mark.parametrize("Np,L,r,path,env,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_info_reports_the_selected_kernel(Np, L, r, path, env, want, monkeypatch):
    x0, y0, order = grid_geometry(Np, L, 3, 20)
    prob = fpm_amd.Problem(Np, L, order, x0, y0, r, 10, 3, n_patch=2, path=path)
    for knob in ("FPM_NO_SPLIT", "FPM_SPLIT", "FPM_NO_DIST", "FPM_DIST", "FPM_NO_S90"):
        monkeypatch.delenv(knob, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with fpm_amd.Solver(prob) as s:
        info = s.info()
    assert (info.fused_kernel, info.threads_per_wg, info.wg_per_patch) == want
    assert (info.path == fpm_amd.PATH_FUSED) == (info.fused_kernel != fpm_amd.KERNEL_GENERAL)


def test_fused_path_with_fp16_storage_is_refused_before_anything_is_created():
    """PATH_FUSED with fp16 spectrum storage has no kernel: fpm_create refuses
    it while planning the context; PATH_AUTO takes the general path."""
    Np, L, r = 64, 256, 20
    x0, y0, order = grid_geometry(Np, L, 3, 20)

    def problem(path):
        return fpm_amd.Problem(Np, L, order, x0, y0, r, 10, 3, n_patch=2, path=path, flags=fpm_amd.FLAG_SPEC_FP16)

    with pytest.raises(fpm_amd.FpmError) as ei:
        fpm_amd.Solver(problem(fpm_amd.PATH_FUSED))
    assert ei.value.code == fpm_amd.FPM_ERR_INVAL and "fused path unsupported" in str(ei.value)
    with fpm_amd.Solver(problem(fpm_amd.PATH_AUTO)) as s:
        assert s.info().fused_kernel == fpm_amd.KERNEL_GENERAL
