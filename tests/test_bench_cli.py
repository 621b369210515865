"""bench.py's launcher contract on the CPU (no GPU call is reached):
`--gpus N` without a launcher re-launches itself under torch.distributed.run
with N ranks (one per GPU) as a child process and exits with its status; under
a launcher whose WORLD_SIZE differs from --gpus it refuses to run.  A 1-GPU
number must never be labelled N GPUs (round-2 review)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_main(monkeypatch, argv, env):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    calls = []
    import subprocess
    monkeypatch.setattr(subprocess, "call", lambda cmd, *a, **k: calls.append(cmd) or 7)
    with pytest.raises(SystemExit) as e:
        bench.main()
    return e.value.code, calls


def test_gpus_n_spawns_one_rank_per_gpu(monkeypatch):
    code, calls = _run_main(monkeypatch, ["--gpus", "8", "--steps", "3", "--warmup", "1"], {})
    assert code == 7 and len(calls) == 1              # the child's exit status is returned
    cmd = calls[0]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"]


def test_gpus_mismatch_under_launcher_refuses(monkeypatch):
    code, calls = _run_main(monkeypatch, ["--gpus", "8"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert calls == [] and "WORLD_SIZE=2" in str(code)


class _FakeSolver:
    """download() of a 3-patch context, filled with known values."""

    def __init__(self):
        import numpy as np
        rng = np.random.default_rng(7)

        def c(*shape):
            return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
        self.out = dict(objF=c(3, 24, 24), objCrop=c(3, 24, 24), pupil=c(3, 8, 8), support=None)

    def synchronize(self):
        pass

    def download(self, **kw):
        assert kw == {"support": False}
        return self.out


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: an array within its byte share is written whole as
    float32 [..., 2]; a larger one as the seeded sample of its elements, the
    same elements on every call."""
    import numpy as np
    import bench
    s = _FakeSolver()
    monkeypatch.setattr(bench, "DUMP_BYTES", {"objCrop": 8 * 100, "objF": 10 ** 6, "pupil": 10 ** 6})
    bench.dump_outputs(s, str(tmp_path / "a"))
    bench.dump_outputs(s, str(tmp_path / "b"))
    for name in ("objCrop", "objF", "pupil"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
        full = s.out[name]
        if name == "objCrop":
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, full.size, 100))
            assert a.shape == (100, 2) and np.array_equal(a[:, 0] + 1j * a[:, 1], full.reshape(-1)[idx])
        else:
            assert a.shape == full.shape + (2,) and np.array_equal(a[..., 0] + 1j * a[..., 1], full)


def test_dump_budget():
    """The dumped arrays stay within 64 MB in all."""
    import bench
    assert sum(bench.DUMP_BYTES.values()) <= 64 * 10 ** 6


@pytest.mark.gpu
def test_plain_run_dumps_repeatable_outputs(tmp_path, monkeypatch, capsys):
    """A plain run (2 patches of config 2) times exactly --steps steps, leaves
    cpu_baseline out, and two runs with the same arguments dump identical
    arrays: the seeded inputs and the solver are deterministic."""
    import json
    import numpy as np
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    lines = []
    for d in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "c2",
                                          "--patches", "2", "--dump-outputs", str(tmp_path / d)])
        bench.main()
        lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    for ln in lines:
        assert ln["steps"] == 2 and ln["ms_per_step"] > 0 and ln["cpu_baseline"] is None
        assert ln["value"] == pytest.approx(2 * 193 / (ln["ms_per_step"] * 1e-3), rel=5e-3)
    for name, shape in (("objCrop", (2, 360, 360, 2)), ("objF", (2, 360, 360, 2)), ("pupil", (2, 90, 90, 2))):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))


def test_general_path_traffic_counts_every_patch_group(tmp_path):
    """The general path runs each per-LED kernel once per patch group, so a
    counter file's per-dispatch bytes cover one group: bench.load_pmc scales
    them by the kernel's dispatches over the profiled run's LED steps (the
    rounds 5-6 config 5 figure of 2.80x was one group's)."""
    import json
    import bench
    from tools.srchash import src_hash
    per = {"k_rows256_inv": 1.0e6, "k_cols256": 2.0e6, "k_rows256_fwd": 3.0e6, "k_pupil_commit": 0.5e6}
    disp = {"k_rows256_inv": 386, "k_cols256": 386, "k_rows256_fwd": 386, "k_pupil_commit": 2}
    p = tmp_path / "pmc.json"
    p.write_text(json.dumps({"src_hash": src_hash(), "per_launch_hbm_bytes": per, "dispatches": disp,
                             "derived": {}}))
    tot, _, note = bench.load_pmc(str(p), "general_led_step", n_led=193)
    assert tot == pytest.approx(2 * (1.0e6 + 2.0e6 + 3.0e6) + 0.5e6 * 2 / 193)
    assert "dispatches" in note
    # a file without dispatch counts (older tools) keeps the one-group sum and says so
    p.write_text(json.dumps({"src_hash": src_hash(), "per_launch_hbm_bytes": per, "derived": {}}))
    tot, _, note = bench.load_pmc(str(p), "general_led_step", n_led=193)
    assert tot == pytest.approx(6.5e6) and "one patch group" in note
    # a fused kernel: one dispatch per iteration, the per-dispatch bytes as they are
    p.write_text(json.dumps({"src_hash": src_hash(), "per_launch_hbm_bytes": {"k_fused_s90": 4.0e8},
                             "dispatches": {"k_fused_s90": 1}, "derived": {}}))
    tot, _, _ = bench.load_pmc(str(p), "k_fused_s90", n_led=193)
    assert tot == 4.0e8
