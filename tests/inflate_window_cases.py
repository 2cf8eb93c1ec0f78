"""Windows over the .gz files of tests/inflate_stream_cases.py and tests/inflate_stream_fuzz.py for the windowed stream
inflate (csrc/bdx_inflate_window_core.h), shared by its CPU, sanitizer and GPU tests: the plain C++ build
(tests/inflate_window_host.cpp), seeded window schedules, and the cuts at the edges the format has — derived from the
files' bytes, never from the code under test.  zlib is the arbiter (SC.arbiter)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import inflate_cases as IC
import inflate_stream_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
SPACE, STATE, CONTRACT = -5, -3, -9
SEED = 20261
BETWEEN, INSIDE, TRAILER, IGNORE = 0, 1, 2, 3


# ---- the core as plain C++ ----
class Host:
    """the windowed core and, in the same library, the whole-file one"""

    def __init__(self, directory, flags=(), name="libinfw_host.so"):
        so = os.path.join(str(directory), name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-o", so, os.path.join(HERE, "inflate_window_host.cpp")])
        L = self.L = C.CDLL(so)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        L.infs_host_set_launch.restype = None
        L.infs_host_set_launch.argtypes = [C.c_int, C.c_int]
        L.infs_host_inflate.restype = i32
        L.infs_host_inflate.argtypes = [C.c_char_p, i64, i32, vp, i64, vp, vp, vp, vp, i64]
        L.infw_host_open.restype = vp
        L.infw_host_close.argtypes = [vp]
        L.infw_host_state.argtypes = [vp, vp]
        L.infw_host_feed.restype = i32
        L.infw_host_feed.argtypes = [vp, C.c_char_p, i64, i32, i32, vp, i64, vp, vp, vp, vp, vp, i64]
        L.infw_host_run.restype = i32
        L.infw_host_run.argtypes = [C.c_char_p, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, i64]
        self.set_launch = L.infs_host_set_launch
        self.shared_bytes = int(L.infw_host_shared_bytes())

    def whole(self, data: bytes, chunk: int, cap: int):
        """the whole-file build -> (rc, member, at)"""
        out = np.zeros(cap + 1, dtype=np.uint8)
        plen, member, at = C.c_int64(-1), C.c_int32(-1), C.c_int64(-1)
        rc = self.L.infs_host_inflate(data, len(data), chunk, out.ctypes.data, cap, C.byref(plen), None, C.byref(member), C.byref(at), 4)
        return rc, member.value, at.value

    def run(self, data: bytes, sizes, chunk: int, cap: int, seg_room: int = 4):
        """a whole file under a schedule -> (rc, bytes or None, member, at, windows)"""
        out = np.full(cap + 64, 0xC5, dtype=np.uint8)
        sz = np.asarray(list(sizes), dtype=np.int64)
        plen, member, at, wins = C.c_int64(-1), C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
        rc = self.L.infw_host_run(data, len(data), sz.ctypes.data, len(sz), chunk, out.ctypes.data, cap, C.byref(plen), C.byref(member),
                                  C.byref(at), C.byref(wins), seg_room)
        assert (out[cap:] == 0xC5).all()
        return rc, (out[:plen.value].tobytes() if rc == 0 else None), member.value, at.value, wins.value

    def open(self):
        return HostWindow(self)


class HostWindow:
    def __init__(self, host):
        self.L, self.h = host.L, host.L.infw_host_open()

    def feed(self, data: bytes, last: int, chunk: int, cap: int, fill: int = 0xC5):
        """-> (rc, consumed, plain_len, bytes, member, at, every byte of the buffer beyond the text still `fill`)"""
        out = np.full(cap + 64, fill, dtype=np.uint8)
        used, plen, member, at = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1), C.c_int64(-1)
        info = np.full(8, -1, dtype=np.int64)
        rc = self.L.infw_host_feed(self.h, data, len(data), last, chunk, out.ctypes.data, cap, C.byref(used), C.byref(plen), info.ctypes.data,
                                   C.byref(member), C.byref(at), 4)
        n = plen.value if rc == 0 else 0
        return rc, used.value, plen.value, out[:n].tobytes(), member.value, at.value, bool((out[n:] == fill).all())

    def state(self):
        six = np.zeros(6, dtype=np.int64)
        self.L.infw_host_state(self.h, six.ctypes.data)
        return dict(zip(("where", "bit", "member", "member_n", "comp_abs", "plain_abs"), six.tolist()))

    def close(self):
        if self.h:
            self.L.infw_host_close(self.h)
        self.h = None


# ---- schedules ----
def schedule(seed: int, n: int, lo: int = 64, hi=None):
    """window sizes drawn from lo .. hi (the whole file), enough of them for n bytes (what is left goes in one window)"""
    rng = np.random.default_rng(seed)
    hi = max(lo, n if hi is None else hi)
    out, left = [], n
    while left > 0:
        s = int(rng.integers(lo, hi + 1)) if rng.integers(4) else int(rng.integers(lo, min(hi, 4 * lo) + 1))
        out.append(s)
        left -= s
    return out


def verdict_ok(want, rc, got, member, at, n):
    """accepted exactly when zlib accepts, with zlib's bytes; a refusal has a reason, a member and a place in the file"""
    if want is not None:
        return rc == 0 and got == want
    return 1 <= rc <= 11 and member >= 0 and 0 <= at <= n


# ---- the edges of a file, from its bytes ----
def edge_cuts(case):
    """{edge name: [cuts]} for a derived case (SC.Case with members): a cut c ends the first window behind byte c - 1"""
    cuts = {}

    def add(name, c):
        if 0 <= c <= len(case.data):
            cuts.setdefault(name, []).append(c)

    blocks = SC.file_blocks(case)
    for m, (off, body, plain) in enumerate(case.members):
        end = off + len(body)  # the trailer's first byte
        for i in range(8):  # the window ends in front of the trailer's byte i
            add("inside the trailer", end + i)
        add("right behind the trailer", end + 8)
        if m + 1 < len(case.members):
            add("between two members", end + 8)
            add("inside the next header", end + 8 + 5)
        for b in blocks[m]:
            add("on a block's first bit", b.bit // 8)
            add("on a block's first bit", b.bit // 8 + 1)
            add("on a block's last bit", (b.end - 1) // 8)
            add("on a block's last bit", (b.end - 1) // 8 + 1)
            if b.btype == 2:
                add("inside a dynamic header", b.bit // 8 + 3)
                add("inside a dynamic header", b.bit // 8 + 12)
            if b.btype == 0:
                p = (b.bit + 3 + 7) // 8
                for i in (1, 2, 3):
                    add("inside LEN/NLEN", p + i)
    return cuts


def with_fname(case, name=b"reads.fastq\0"):
    """the case's first member with an FNAME field; -> (data, [cuts inside the name])"""
    off, body, plain = case.members[0]
    hdr = b"\x1f\x8b\x08\x08\0\0\0\0\0\xff" + name
    data = hdr + case.data[off:]
    return data, list(range(10, len(hdr) + 1))


# ---- files built for the history ----
def _member(body, plain):
    return SC.HDR + body + IC.trailer(plain)


@functools.lru_cache(maxsize=1)
def history_file():
    """One member of stored blocks and fixed blocks with matches whose sources lie far back: (data, plain, marks), marks
    naming the byte of the file each block with a far match begins at.  Block A: 40 000 bytes stored in pieces of 10 000.
    Block B (fixed): a match of length 258 at distance 32 768, then one of length 5 at distance 1.  Then two short stored
    blocks (100 and 1 byte, then none), and block C (fixed): a match at distance 32 768 again, whose source lies three
    blocks back."""
    s = SC.Stream()
    marks = {}
    for _ in range(4):
        s.stored(s.text(10000))
    marks["far"] = s.byte()
    s.fixed([(258, 32768), (5, 1)])
    marks["short"] = s.byte()
    s.stored(s.text(100))
    marks["one"] = s.byte()
    s.stored(s.text(1))
    marks["zero"] = s.byte()
    s.stored(b"")
    marks["far2"] = s.byte()
    s.fixed([(200, 32768), (3, 1)])
    marks["tail"] = s.byte()
    s.stored(s.text(50), final=True)
    header, body, plain = s.member()
    data = _member(body, plain)
    assert SC.arbiter(data) == plain
    return data, plain, marks


def history_cuts():
    """absolute cuts that put every marked block of history_file() at a window's front: the far matches then read the
    carried 32 KiB, the second one through windows of 100, 1 and 0 plain bytes; and the plain bytes of each window"""
    data, plain, marks = history_file()
    return [marks[k] for k in ("far", "short", "one", "zero", "far2", "tail")], [40000, 263, 100, 1, 0, 203, 50]


def feed_cuts(win, data: bytes, cuts, chunk: int, cap: int):
    """data through the window object `win` (its feed as HostWindow.feed), a window ending at each cut (absolute), the
    last at the file's end; a window without progress is offered again up to the next cut.
    -> (rc, text, [(first byte, bytes offered, consumed, plain bytes)], member, at)"""
    pos, text, log = 0, [], []
    for cut in sorted(set(c for c in cuts if c < len(data))) + [len(data)]:
        if cut < pos:
            continue
        last = int(cut == len(data))
        rc, used, plen, got, member, at, clean = win.feed(data[pos:cut], last, chunk, cap)
        assert clean, "bytes beyond the text were written"
        log.append((pos, cut - pos, used, plen))
        if rc != 0:
            return rc, None, log, member, at
        assert 0 <= used <= cut - pos and (not last or used == cut - pos), log[-1]
        text.append(got)
        pos += used
    return 0, b"".join(text), log, -1, -1


def run_schedule(win, data: bytes, sizes, chunk: int, cap: int):
    """What infw_host_run does, over any window object with HostWindow's feed: window i is offered sizes[i] bytes (behind
    the list: all that is left), one without progress again twice as long.  -> (rc, text or None, member, at, windows)"""
    pos = total = i = grow = wins = 0
    text = []
    while True:
        want = min(grow or (sizes[i] if i < len(sizes) else len(data) - pos), len(data) - pos)
        last = int(pos + want == len(data))
        rc, used, plen, got, member, at, clean = win.feed(data[pos:pos + want], last, chunk, cap - total)
        wins += 1
        assert clean, "bytes beside the window's text were written"
        if rc != 0:
            return rc, None, member, at, wins
        assert 0 <= used <= want and (not last or used == want), (pos, want, used)
        text.append(got)
        total += plen
        if last:
            return 0, b"".join(text), -1, -1, wins
        if used == 0 and plen == 0:
            grow = 64 if want < 32 else 2 * want
            continue
        pos, grow, i = pos + used, 0, i + 1
