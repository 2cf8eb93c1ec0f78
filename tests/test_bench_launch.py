"""bench.py --gpus N outside torchrun must start its own N ranks as a child job (never re-exec, never touch
the GPU in the parent) and pass the child's exit code on; a plain run makes only the headline, --full the rest."""
import os
import sys

import helpers as H


def test_self_launch_builds_a_torchrun_child(monkeypatch):
    sys.path.insert(0, H.ROOT)
    import bench

    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = bench._parse()
    assert bench._self_launch(args) == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr" in cmd and "127.0.0.1" in cmd
    i = cmd.index(os.path.join(H.ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert "torch" not in getattr(bench, "__dict__", {}), "bench.py must not import torch at module level"


def test_workload_table_covers_the_survey_configs():
    import bench

    wl = bench.build_workload("C4", 2000, 0)
    assert wl["cfg"].is_dual and wl["algo_bytes"] == 174 and wl["outputs"] == ("bc1", "bc2", "keep_start", "keep_end")
    wl = bench.build_workload("C5", 50, 0)
    assert wl["algo_bytes"] == 212 and wl["survey_bytes"] == 10012 and len(wl["seq"]) == 50 * 10000
    wl = bench.build_workload("C2d", 1000, 0)
    assert wl["cfg"].max_error_rate == 0.2 and wl["algo_bytes"] == 162


def test_steps_must_be_positive(monkeypatch):
    import pytest

    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench._parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", "d"])
    args = bench._parse()
    assert args.steps == 3 and args.dump_outputs == "d"


def test_plain_run_makes_only_the_headline(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench._parse()
    assert not args.full and bench.full_legs(args, 1) == set()


def test_full_run_keeps_every_leg(monkeypatch):
    import bench

    def legs(*argv, world=1):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--full", *argv])
        return bench.full_legs(bench._parse(), world)

    assert legs() == {"host_path", "cpu_baseline", "other_configs"}
    assert legs("--no-cpu-baseline", "--no-host-path") == {"other_configs"}
    assert legs("--no-other-configs") == {"host_path", "cpu_baseline"}
    # the short legs and the end-to-end figure belong to the default C2 workload only
    assert legs("--config", "C4") == legs("--reads", "1000") == legs("--max-error-rate", "0.2") == {"host_path", "cpu_baseline"}
    # and every leg to a single rank
    assert legs(world=2) == set()


def test_dump_outputs_whole_vectors_when_they_fit(tmp_path):
    import numpy as np

    import bench

    v = np.arange(-1, 999, dtype=np.int32)
    counts = np.array([1000, 990, 9, 1], dtype=np.int64)
    s = bench.dump_outputs(str(tmp_path), {"bc1": v}, counts, seed=1)
    assert s["files"] == ["bc1.npy", "counts.npy"] and s["reads_written"] == 1000
    got = np.load(tmp_path / "bc1.npy")
    assert got.dtype == np.float32 and np.array_equal(got, v)
    c = np.load(tmp_path / "counts.npy")
    assert c.dtype == np.float64 and np.array_equal(c, counts)


def test_dump_outputs_samples_the_same_reads_under_the_size_cap(tmp_path, monkeypatch):
    import numpy as np

    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    n = 100_000
    out = {k: (np.arange(n, dtype=np.int32) * (i + 1)) % 10_000 - 1 for i, k in enumerate(("bc1", "bc2", "keep_start", "keep_end"))}
    a, b = tmp_path / "a", tmp_path / "b"
    sa = bench.dump_outputs(str(a), out, np.zeros(8, dtype=np.int64), seed=5)
    sb = bench.dump_outputs(str(b), out, np.zeros(8, dtype=np.int64), seed=5)
    assert sa["bytes"] <= 200_000 and 0 < sa["reads_written"] < n and sa["files"] == sb["files"]
    idx = np.load(a / "read_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(b / "read_index.npy"))
    assert np.all(np.diff(idx) > 0)
    for k, v in out.items():
        assert np.array_equal(np.load(a / f"{k}.npy"), v[idx.astype(np.int64)])
    # a later dump that fits whole leaves no stale sample index behind
    bench.dump_outputs(str(a), {"bc1": out["bc1"][:10]}, np.zeros(8, dtype=np.int64), seed=5)
    assert not (a / "read_index.npy").exists()
