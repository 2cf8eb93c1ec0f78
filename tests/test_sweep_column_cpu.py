"""The column code of the wave kernel's sweeps (csrc/bdx_sweep_col.h): tests/sweep_column_host.cpp — a program of its own, built
here with the host compiler under ASan / UBSan — checks the nibble -> byte-field expansion over every word of codes 0 .. 4, with
and without junk nibbles, the add-with-carry score update against the carry-free arithmetic, and both forms of the column
step against a plain DP.  (No Python process loads sanitised code.)"""
import os
import subprocess

import plan_cases as PC
from test_sanitizers import ENV, SAN


def test_sweep_column_helpers_against_each_other_and_a_plain_dp(tmp_path):
    exe = str(tmp_path / "sweep_column_host")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", PC.CSRC, "-o", exe, os.path.join(PC.HERE, "sweep_column_host.cpp")])
    out = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.startswith("sweep column driver ok:"), out.stdout
    words, pairs, cols = (int(x.split()[0]) for x in out.stdout.split(":")[1].split(","))
    assert words == 5 ** 8 and pairs >= 1000004 and cols == 2000 * 64
