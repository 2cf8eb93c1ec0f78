"""The stream inflate (csrc/bdx_inflate_stream_core.h as plain C++) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/inflate_stream_host.cpp built with its own main is a stand-alone driver that runs every
case of tests/inflate_stream_cases.py at its chunk sizes, every prefix of the small ones and some ten thousand corrupted
files, with the compressed file, the 16-bit staging image and the output as exact-size heap blocks.  This is where the
bounds handling of bad input is proven: a read one byte outside the file or a write one byte outside the output is the
sanitizer's to report."""
import os
import subprocess

import helpers as H
import inflate_stream_cases as SC
from test_sanitizers import ENV, SAN


def test_stream_inflate_under_asan_ubsan(tmp_path):
    files = [(c.name, c.data, plain, SC.CHUNKS) for c, plain in SC.derived_cases()]
    for name, data in SC.arbiter_cases():
        files.append((name, data, SC.arbiter(data), (64, 0)))
    small = sum(len(data) <= 1500 for _, data, _, _ in files)
    assert small >= 70
    for k, (_, data, plain, chunks) in enumerate(files):
        (tmp_path / ("case_%d.gz" % k)).write_bytes(data)
        (tmp_path / ("case_%d.plain" % k)).write_bytes(plain or b"")
        (tmp_path / ("case_%d.info" % k)).write_text("%d %s\n" % (plain is not None, " ".join(map(str, chunks))))
    exe = str(tmp_path / "stream_driver")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-DINFS_HOST_MAIN", "-o", exe, os.path.join(H.ROOT, "tests", "inflate_stream_host.cpp")])
    out = subprocess.run([exe, str(tmp_path), str(len(files))], env=ENV, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    good = sum(plain is not None for _, _, plain, _ in files)
    assert "stream inflate driver ok: %d good, %d bad" % (good, len(files) - good) in out.stdout
    words = out.stdout.split()
    assert int(words[-2]) >= 150 * small >= 10000 and int(words[-4]) >= sum(len(d) for _, d, _, _ in files if len(d) <= 1500)
