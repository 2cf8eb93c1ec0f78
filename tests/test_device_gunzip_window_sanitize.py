"""The windowed stream inflate (csrc/bdx_inflate_window_core.h as plain C++) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/inflate_window_host.cpp built with its own main is a stand-alone program that takes
every file through a window object under a seeded schedule of window sizes, and the small files at every cut, with the
carried state, each window's compressed bytes, its staging image and its output as exact-size heap blocks (every window
is first fed without room and says what it needs).  A read one byte outside a window, or a write one byte outside its
text or the carried state, is the sanitizer's to report.

The files are the small files and the small good and bad members (every cut), and the fixed slice of the seeded corpus
(one schedule each).  The program runs a second time the way the device starts its workgroups: every one from a state
full of the byte 0xA5, 16 of them dealing the items among themselves."""
import os
import subprocess

import helpers as H
import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ
from test_sanitizers import ENV, SAN

LAUNCH = ("165", "16")


def test_window_inflate_under_asan_ubsan(tmp_path):
    files = [(name, data, SC.arbiter(data), 2) for name, data in SC.small_files()]
    files += [(name, data, SC.arbiter(data), 2) for name, data in SC.arbiter_cases() if len(data) <= 1500]
    cuts = sum(len(data) + 1 for _, data, _, _ in files)
    assert len(files) >= 70 and cuts >= 50000
    sliced = FZ.slice_files()
    assert len(sliced) >= 400 and sum(plain is None for _, _, plain, _ in sliced) >= 100
    files += [(name, data, plain, 0) for name, data, plain, _ in sliced]
    for k, (_, data, plain, every_cut) in enumerate(files):
        (tmp_path / ("case_%d.gz" % k)).write_bytes(data)
        (tmp_path / ("case_%d.plain" % k)).write_bytes(plain or b"")
        (tmp_path / ("case_%d.info" % k)).write_text("%d %d\n" % ((plain is not None) + every_cut, FZ.ODD[k % len(FZ.ODD)] if k % 2 else 64))
    exe = str(tmp_path / "window_driver")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-DINFW_HOST_MAIN", "-o", exe, os.path.join(H.ROOT, "tests", "inflate_window_host.cpp")])
    good = sum(plain is not None for _, _, plain, _ in files)
    for launch in ((), LAUNCH):
        out = subprocess.run([exe, str(tmp_path), str(len(files)), *launch], env=ENV, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, (launch, out.stderr[-3000:])
        assert "window inflate driver ok: %d good, %d bad, %d cuts" % (good, len(files) - good, cuts) in out.stdout
