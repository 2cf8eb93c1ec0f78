"""The context's buffers free themselves (DevBuf / PinnedBuf, csrc/bdx_ctx.h): tests/buf_host.cpp — a program of its own, built
here under ASan / UBSan over a stub of hipMalloc / hipFree / hipHostMalloc / hipHostFree that counts calls and knows the live
pointers — moves, move-assigns onto live buffers, grows a std::vector of them, grows and fails `ensure`, and destroys; every
allocation is freed exactly once, none twice, none by the other kind's call.  (No Python process loads sanitised code.)"""
import os
import subprocess

import plan_cases as PC
from test_sanitizers import ENV, SAN


def test_buffers_free_every_allocation_exactly_once(tmp_path):
    exe = str(tmp_path / "buf_host")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", PC.CSRC, "-o", exe,
                           os.path.join(PC.HERE, "buf_host.cpp")])
    out = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    dev_alloc, dev_free, pin_alloc, pin_free = map(int, out.stdout.split(":")[1].split())
    assert out.stdout.startswith("buffer driver ok:") and dev_alloc == dev_free >= 100 and pin_alloc == pin_free >= 100
