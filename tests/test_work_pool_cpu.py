"""The host worker pool (csrc/bdx_pool.h) under many short back-to-back sections of differing size: every index runs
exactly once and the pool never stalls (tests/work_pool_driver.cpp), also under ThreadSanitizer where it runs here."""
import os
import subprocess

import pytest

import helpers as H

DRIVER = os.path.join(H.ROOT, "tests", "work_pool_driver.cpp")
CSRC = os.path.join(H.ROOT, "biodemux.jl_amd", "csrc")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-pthread", "-I", CSRC, "-o", exe, DRIVER])
    return exe


def test_pool_runs_every_index_once_without_stalling(tmp_path):
    exe = _build(tmp_path, "pool_driver", ["-O2"])
    out = subprocess.run([exe, "3000000", "20"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "work pool ok" in out.stdout


def test_pool_under_thread_sanitizer(tmp_path):
    probe = tmp_path / "tsan_probe.cpp"
    probe.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n")
    try:
        subprocess.check_call(["g++", "-fsanitize=thread", "-pthread", "-o", str(tmp_path / "tsan_probe"), str(probe)])
        usable = subprocess.run([str(tmp_path / "tsan_probe")], capture_output=True, timeout=60).returncode == 0
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired):
        usable = False
    if not usable:
        pytest.skip("ThreadSanitizer does not run on this machine")
    exe = _build(tmp_path, "pool_driver_tsan", ["-fsanitize=thread", "-g", "-O1"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe, "20000", "20"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "work pool ok" in out.stdout
