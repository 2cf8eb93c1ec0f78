"""The wave kernel's hit -> read mapping for tiles of equal-length reads (csrc/bdx_read_index.h): tests/read_index_host.cpp — a
program of its own, built here with the host compiler under ASan / UBSan — checks the multiply-high against x / len for every
length and position a 32-read tile of 5 KiB can hold, at the largest x with x * len < 2^32 for a few hundred lengths, and that a
position in front of the tile's first base comes out beyond any tile's read count.  (No Python process loads sanitised code.)"""
import os
import subprocess

import plan_cases as PC
from test_sanitizers import ENV, SAN


def test_read_index_by_multiply_high_against_division(tmp_path):
    exe = str(tmp_path / "read_index_host")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", PC.CSRC, "-o", exe, os.path.join(PC.HERE, "read_index_host.cpp")])
    out = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.startswith("read index driver ok:"), out.stdout
    exhaustive, lens, edges, heads = (int(x.split()[0]) for x in out.stdout.split(":")[1].split(","))
    assert exhaustive == 5136 * 5136 and lens >= 300 and edges >= 64 * 300 and heads == 16 * 10256
