"""The sweep set-up helpers of the wave kernel's LEAN forms (csrc/bdx_sweep_col.h): tests/sweep_setup_host.cpp — a program of
its own, built here with the host compiler under ASan / UBSan — holds the junk-column mask of a word (one clamp, one 64-bit
shift) and the start value of Pv (one shift) to the expressions they replace: every window remainder -40 .. 72 in every word,
every barcode length 1 .. 32.  (No Python process loads sanitised code.)"""
import os
import subprocess

import plan_cases as PC
from test_sanitizers import ENV, SAN


def test_sweep_setup_helpers_equal_the_expressions_they_replace(tmp_path):
    exe = str(tmp_path / "sweep_setup_host")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", PC.CSRC, "-o", exe, os.path.join(PC.HERE, "sweep_setup_host.cpp")])
    out = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.startswith("sweep setup driver ok:"), out.stdout
    masks, shortcuts, pvs = (int(x.split()[0]) for x in out.stdout.split(":")[1].split(","))
    assert masks == 113 * 4 and shortcuts == 49 and pvs == 32
