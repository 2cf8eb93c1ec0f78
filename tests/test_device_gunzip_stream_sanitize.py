"""The stream inflate (csrc/bdx_inflate_stream_core.h as plain C++) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/inflate_stream_host.cpp built with its own main is a stand-alone driver that runs every
case of tests/inflate_stream_cases.py at its chunk sizes, every prefix of the small ones and some ten thousand corrupted
files, with the compressed file, the 16-bit staging image and the output as exact-size heap blocks.  This is where the
bounds handling of bad input is proven: a read one byte outside the file or a write one byte outside the output is the
sanitizer's to report.

The fixed slice of the seeded corpus (tests/inflate_stream_fuzz.py: 100 good files, 300 bit-flipped and truncated ones)
goes through the same driver as it is, and the driver runs a second time the way the device starts its workgroups: every
one from a state full of one byte, 16 of them dealing the items among themselves.  The GPU runs these very files."""
import os
import subprocess

import helpers as H
import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ
from test_sanitizers import ENV, SAN

LAUNCH = ("165", "16")  # the second run: fill byte 0xA5, a grid of 16 workgroups


def test_stream_inflate_under_asan_ubsan(tmp_path):
    files = [(c.name, c.data, plain, SC.CHUNKS) for c, plain in SC.derived_cases()]
    for name, data in SC.arbiter_cases():
        files.append((name, data, SC.arbiter(data), (64, 0)))
    small = sum(len(data) <= 1500 for _, data, _, _ in files)
    assert small >= 70
    hand = len(files)  # the slice behind them: as it is, without prefixes and further corruption
    files += FZ.slice_files()
    assert len(files) - hand >= 400 and sum(plain is None for _, _, plain, _ in files[hand:]) >= 100
    for k, (_, data, plain, chunks) in enumerate(files):
        (tmp_path / ("case_%d.gz" % k)).write_bytes(data)
        (tmp_path / ("case_%d.plain" % k)).write_bytes(plain or b"")
        (tmp_path / ("case_%d.info" % k)).write_text("%d %s\n" % ((plain is not None) + 2 * (k >= hand), " ".join(map(str, chunks))))
    exe = str(tmp_path / "stream_driver")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-DINFS_HOST_MAIN", "-o", exe, os.path.join(H.ROOT, "tests", "inflate_stream_host.cpp")])
    good = sum(plain is not None for _, _, plain, _ in files)
    for launch in ((), LAUNCH):
        out = subprocess.run([exe, str(tmp_path), str(len(files)), *launch], env=ENV, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (launch, out.stderr[-3000:])
        assert "stream inflate driver ok: %d good, %d bad" % (good, len(files) - good) in out.stdout
        words = out.stdout.split()
        assert int(words[-2]) >= 150 * small >= 10000 and int(words[-4]) >= sum(len(d) for _, d, _, _ in files[:hand] if len(d) <= 1500)
