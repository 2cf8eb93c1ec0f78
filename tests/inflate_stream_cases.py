"""Whole .gz files for the stream inflate (csrc/bdx_inflate_stream_core.h), shared by its CPU, sanitizer and GPU tests.
Built from tests/inflate_cases.py and tests/inflate_edge_cases.py: zlib streams, and files written block by block
(stored_block, fixed_block, dynamic_block) so that block starts, matches and false candidates lie where a chunk size
of 64 or 4096 bytes makes them matter.

Nothing about a case is typed in.  What the file inflates to comes from zlib (`arbiter`, which follows zlib's gzread:
members back to back, what does not begin with 1f 8b behind a member is ignored).  What `info` must say comes from
`expected_info`: the block positions that `anatomy` reads from the file's bytes, a Python restatement of the candidate
rule (`is_candidate`) and of the chain.  `features` says which edges a case reaches, again read from its bytes."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

import inflate_cases as IC
import inflate_edge_cases as EC

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNKS = (64, 4096, 0)  # 0: the default
DEFAULT_CHUNK = 131072
HDR = b"\x1f\x8b\x08\0\0\0\0\0\0\xff"
SPACE = -5  # BDX_E_SPACE

# members: [(offset of the deflate body in data, body, plain)] for the files whose info is derived (None: not derived)
Case = namedtuple("Case", "name data members")


# ---- zlib is the arbiter ----
def arbiter(data: bytes):
    """what zlib's gzread gives for the file, None when it fails (a truncated member is refused here, as gunzip does)"""
    out, rest = [], data
    try:
        while True:
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
            if not d.eof:
                return None
            rest = d.unused_data
            if not (len(rest) >= 2 and rest[:2] == b"\x1f\x8b"):
                return b"".join(out)
    except zlib.error:
        return None


# ---- the candidate rule, restated ----
def is_candidate(data: bytes, bit: int) -> bool:
    """BTYPE 2, HLIT <= 29, HDIST <= 29, a complete code-length code, exactly nl + nd lengths, both code sets taken by
    zlib's rule, a code for symbol 256 — all of it inside the file"""
    r = EC._Reader(data)
    r.pos = bit
    try:
        r.get(1)
        if r.get(2) != 2:
            return False
        nl, nd, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
        if nl > 286 or nd > 30:
            return False
        cl = [0] * 19
        for i in range(hclen):
            cl[EC.ORDER[i]] = r.get(3)
        h = EC._huff(cl, True)
        lens = []
        while len(lens) < nl + nd:
            s = r.sym(h)
            if s < 16:
                lens.append(s)
            elif s == 16:
                if not lens:
                    return False
                lens += [lens[-1]] * (3 + r.get(2))
            else:
                lens += [0] * ((3 if s == 17 else 11) + r.get(3 if s == 17 else 7))
        if len(lens) > nl + nd or lens[256] == 0:
            return False
        EC._huff(lens[:nl])
        EC._huff(lens[nl:])
        return True
    except EC.Refused:
        return False


def _prefiltered(data: bytes) -> np.ndarray:
    """the bit offsets that pass the cheap part of the rule (header fields and the code-length code's Kraft sum), by numpy"""
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")
    n = len(bits)
    b = np.concatenate([bits, np.zeros(96, dtype=np.uint8)]).astype(np.int32)

    def field(off, k):
        v = np.zeros(n, dtype=np.int32)
        for i in range(k):
            v |= b[off + i:off + i + n] << i
        return v

    ok = (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    hclen = field(13, 4) + 4
    kraft = np.zeros(n, dtype=np.int32)
    for i in range(19):
        l = field(17 + 3 * i, 3)
        kraft += np.where((i < hclen) & (l > 0), 128 >> l, 0)
    ok &= kraft == 128
    ok &= np.arange(n) + 17 + 3 * hclen <= n
    return np.flatnonzero(ok)


@functools.lru_cache(maxsize=None)
def all_candidates(data: bytes):
    return tuple(int(p) for p in _prefiltered(data) if is_candidate(data, int(p)))


def first_candidates(data: bytes, chunk: int):
    """{k: s_k} for the chunks k >= 1 that have a candidate"""
    out = {}
    for p in all_candidates(data):
        k = p // (8 * chunk)
        if k >= 1 and k not in out:
            out[k] = p
    return out


# ---- the blocks of a file and the chain, restated ----
PBlock = namedtuple("PBlock", "bit end btype final nbytes tokens")


@functools.lru_cache(maxsize=None)
def _body_blocks(body: bytes, plain: bytes):
    blocks, got, why = EC.anatomy(IC.wrap(body, IC.trailer(plain), tag="DX"), strict=False)
    assert why is None and got == plain, why
    out = []
    for B in blocks:
        n = B.stored if B.btype == 0 else sum(1 if isinstance(t, int) else t[0] for t in B.tokens)
        out.append(PBlock(B.bit, B.end_bit, B.btype, B.final, n, B.tokens))
    return tuple(out)


def file_blocks(case):
    """per member the blocks with absolute bit positions"""
    return [[b._replace(bit=8 * off + b.bit, end=8 * off + b.end) for b in _body_blocks(body, plain)] for off, body, plain in case.members]


Segment = namedtuple("Segment", "s e off n member guessed blocks")


def chain(case, chunk: int):
    """the segments the chain must arrive at, and info[0:6]"""
    chunk = chunk or DEFAULT_CHUNK
    c8 = 8 * chunk
    data = case.data
    n_chunks = -(-len(data) // chunk)
    s = first_candidates(data, chunk)
    segs, total = [], 0
    for m, blocks in enumerate(file_blocks(case)):
        s0 = {0: blocks[0].bit} if m == 0 else {}
        i = 0
        while True:
            cur, k, first = blocks[i].bit, blocks[i].bit // c8, i
            landed = s.get(k) == cur or s0.get(k) == cur
            while True:
                b = blocks[i]
                i += 1
                if b.final or (landed and b.end >= (k + 1) * c8) or (not landed and s.get(b.end // c8) == b.end):
                    break
            n = sum(x.nbytes for x in blocks[first:i])
            segs.append(Segment(cur, b.end, total, n, m, landed and k > 0, tuple(blocks[first:i])))
            total += n
            if b.final:
                break
    confirmed = sum(g.guessed for g in segs)
    info = [len(case.members), n_chunks, confirmed, len(s) - confirmed, n_chunks - 1 - len(s), max((g.e + 7) // 8 - g.s // 8 for g in segs)]
    return segs, info


def expected_info(case, chunk: int):
    return chain(case, chunk)[1] + [0, 0]


def features(case, chunk: int):
    """the edges the case reaches at this chunk size, read from its bytes"""
    chunk = chunk or DEFAULT_CHUNK
    c8 = 8 * chunk
    segs, info = chain(case, chunk)
    f = set()
    first = {}
    for blocks in file_blocks(case):
        for b in blocks:
            first.setdefault(b.bit // c8, b)
            if b.end // c8 - b.bit // c8 >= 3:
                f.add("block spans 3 chunks")
            if b.bit % c8 == 0 and b.bit:
                f.add("block start on a chunk's first bit")
            if b.bit % c8 == c8 - 1:
                f.add("block start on a chunk's last bit")
    for k, b in first.items():
        if k >= 1:
            f.add("first block start of a chunk: " + ("stored", "fixed", "dynamic")[b.btype] + (", final" if b.final else ""))
    if info[3]:
        f.add("candidate discarded")
    if len(case.data) % chunk == 0:
        f.add("comp_len a multiple of the chunk")
    if len(case.data) < chunk:
        f.add("smaller than one chunk")
    for j, g in enumerate(segs):
        if g.n <= 1:
            f.add("segment of %d bytes" % g.n)
        pos = 0
        for b in g.blocks:
            for t in b.tokens:
                if isinstance(t, int):
                    pos += 1
                    continue
                length, dist = t
                if dist > pos and j > 0:  # its source begins in front of the segment
                    back = dist - pos
                    if dist == 1:
                        f.add("distance 1 into the previous segment")
                    if dist == 32768:
                        f.add("distance 32768 into an earlier segment")
                    if length == 258:
                        f.add("length 258 from in front of the segment")
                    reach, crossed = 0, 0  # how many earlier segments the source touches
                    for h in reversed(segs[:j]):
                        lo, hi = reach, reach + h.n  # bytes in front of the segment this one covers
                        if h.n and lo < back and hi > back - min(length, dist):
                            crossed += 1
                        reach = hi
                    if crossed >= 2:
                        f.add("source straddles %d earlier segments" % min(crossed, 3))
                pos += length
            if b.btype == 0:
                pos += b.nbytes
    return f


# ---- writing files block by block ----
TEXT = IC.fastq_text(60000, 77)
LL = [8] * 226 + [9] * 60      # a complete literal/length code over all 286 symbols
DD = [4] * 2 + [5] * 28        # a complete distance code over all 30
SEQ = EC.rle(LL + DD)          # its code-length sequence with repeats: a header of some 40 bytes


class Stream:
    """a deflate body written block by block; `origin`: the byte of the file its first byte will be"""

    def __init__(self, origin=len(HDR), at=0):
        self.w, self.plain, self.origin, self.at = EC.W(), b"", origin, at

    def text(self, n):
        self.at += n
        return (TEXT[(self.at - n) % 50000:] + TEXT * (n // len(TEXT) + 1))[:n]

    def lits(self, n):
        return list(self.text(n))

    def byte(self):
        return self.origin + (self.w.pos() + 7) // 8

    def stored(self, data, final=False):
        EC.stored_block(self.w, data, final)
        self.plain += data
        return self

    def fixed(self, tokens, final=False):
        EC.fixed_block(self.w, tokens, final)
        self.plain = EC.apply(tokens, self.plain)
        return self

    def dyn(self, tokens, final=False, fat=False):
        """fat: one code-length symbol per length, no repeats: a header of some 90 bytes"""
        EC.dynamic_block(self.w, LL, DD, tokens, final, cl_sequence=None if fat else SEQ)
        self.plain = EC.apply(tokens, self.plain)
        return self

    def pad_to(self, byte):
        """stored blocks of text up to where the next block begins at `byte` of the file, on its first bit"""
        while True:
            room = byte - (self.origin + (self.w.pos() + 3 + 7) // 8 + 4)
            assert room >= 0, "pad_to: too close"
            n = room if room <= 65535 else min(65535, room - 5)
            self.stored(self.text(n))
            if n == room:
                assert self.w.pos() % 8 == 0 and self.origin + self.w.pos() // 8 == byte
                return self

    def member(self, header=HDR):
        return header, self.w.bytes(), self.plain


def case(name, *members):
    """members: (header, body, plain)"""
    data, table = b"", []
    for header, body, plain in members:
        table.append((len(data) + len(header), body, plain))
        data += header + body + IC.trailer(plain)
    return Case(name, data, tuple(table))


def zcase(name, plain, level):
    return case(name, (HDR, IC.raw_deflate(plain, level=level), plain))


def _repairs():
    out = []
    s = Stream()  # every block type, in turns: at 64 bytes a chunk nearly every block start is the first of its chunk
    for r in range(12):
        s.dyn(s.lits(30) + [(20, 25)]).stored(s.text(70 + r)).fixed(s.lits(40) + [(9, 60)]).dyn(s.lits(50), fat=r % 3 == 0)
    s.pad_to((s.byte() // 64 + 2) * 64).fixed(s.lits(3), final=True)  # a final block on a chunk's first bit
    out.append(case("every_block_type", s.member()))
    s = Stream()  # blocks that span three chunks and more: a stored one and a dynamic one
    s.dyn(s.lits(20)).stored(s.text(300)).dyn(s.lits(400)).dyn(s.lits(10)).stored(s.text(9000)).dyn(s.lits(30), final=True)
    out.append(case("long_blocks", s.member()))
    s = Stream()  # block starts on a chunk's first and last bit, dynamic and not
    s.dyn(s.lits(10)).pad_to(256).dyn(s.lits(10)).pad_to(512 - 7).fixed([200, 201, 202, 203, 204])  # 3 + 5 * 9 + 7 = 55 bits
    s.dyn(s.lits(10)).pad_to(4096).dyn(s.lits(10)).pad_to(8192 - 7).fixed([200, 201, 202, 203, 204]).dyn(s.lits(10))
    s.pad_to(8192 + 256).stored(s.text(5)).pad_to(8192 + 512 - 7).fixed([200, 201, 202, 203, 204]).fixed(s.lits(10))
    s.dyn(s.lits(5), final=True)
    s.w.align()
    tail = -(len(HDR) + len(s.w.bytes()) + 8) % 4096  # ... and a file that is a multiple of the chunk: a second member pads it
    assert tail >= 30
    pad = b"p" * (tail - len(HDR) - 5 - 8)  # (a final stored block: 5 bytes in front of its payload)
    out.append(case("first_and_last_bit", s.member(), Stream().stored(pad, final=True).member()))
    assert len(out[-1].data) % 4096 == 0
    out.append(case("tiny", Stream().fixed(list(b"hello"), final=True).member()))
    s = Stream()  # a guess that holds at the default chunk size: a dynamic block is the first block start of chunk 1
    s.dyn(s.lits(40)).pad_to(DEFAULT_CHUNK + 100).dyn([(258, 32768), (3, 1)] + s.lits(30)).dyn(s.lits(20), final=True)
    out.append(case("default_chunk_guess", s.member()))
    return out


def _windows():
    out = []
    s = Stream()  # sources in the previous segment: distance 1, length 258, distance 32768
    s.dyn(s.lits(60)).pad_to(33000).dyn([(258, 1), (3, 32768), (258, 32768)] + s.lits(40), fat=True)
    s.pad_to(33000 + 4096).dyn([(258, 1), (258, 32768), (5, 32768)] + s.lits(40), fat=True).dyn(s.lits(3), final=True)
    out.append(case("far_sources", s.member()))
    s = Stream()  # short segments; sources that straddle several of them; a copy of a copy of a copy
    s.dyn(s.lits(300), fat=True)
    for r in range(8):
        s.dyn(s.lits(10) + [(200, 250)] + s.lits(5) + [(30, 205 + r)], fat=True)
    for r in range(6):
        s.dyn([(120, 130)] + s.lits(6), fat=True)  # what the block before copied, copied again
    for r in range(6):
        s.dyn(s.lits(20), fat=True)  # segments of 20 bytes ...
    s.dyn([(100, 110)] + s.lits(4), fat=True)  # ... and a source that runs over five of them
    s.dyn(s.lits(3), final=True)
    out.append(case("short_segments", s.member()))
    s = Stream()  # segments of 0 bytes and of 1 byte: a fat empty block on a chunk's first bit is a segment of its own
    s.dyn(s.lits(50)).pad_to(256).dyn([], fat=True).pad_to(512).dyn([65], fat=True).pad_to(768).dyn([(40, 30)] + s.lits(4), fat=True)
    s.pad_to(4096).dyn([], fat=True).pad_to(4096 + 256).dyn([(4, 1)], final=True)
    out.append(case("empty_segments", s.member()))
    return out


def _planted_block():
    """the bytes of a complete dynamic block with text tokens, none of them zero (it has to live in an FNAME too)"""
    for seed in range(200):
        w = EC.W()
        toks = list(IC.fastq_text(60, 300 + seed))
        EC.dynamic_block(w, LL, DD, toks, False, cl_sequence=SEQ)
        w.align()
        if 0 not in w.bytes():
            assert is_candidate(w.bytes(), 0)
            return w.bytes()
    raise AssertionError("no planted block without a zero byte")


def _planted():
    fake = _planted_block()
    out = []
    for name, at in (("planted_in_stored_4096", 4096), ("planted_in_stored_default", DEFAULT_CHUNK)):
        s = Stream()
        s.dyn(s.lits(40)).pad_to(at - 5).stored(fake + s.text(300)).dyn(s.lits(30) + [(50, 300)], final=True)
        c = case(name, s.member())
        assert c.data[at:at + len(fake)] == fake
        out.append(c)
    s = Stream()  # in the FNAME of the second member's header, which begins a chunk of 64 and of 4096 bytes
    s.dyn(s.lits(40)).pad_to(4096 - 10 - 8 - 5).stored(b"", final=True)
    first = s.member()
    assert len(HDR) + len(first[1]) + 8 == 4096 - 10
    header = b"\x1f\x8b\x08\x08\0\0\0\0\0\xff" + fake + b"\0"
    t = Stream(origin=4096 - 10 + len(header))
    t.dyn(t.lits(80)).dyn([(30, 40)] + t.lits(9), final=True)
    c = case("planted_in_fname", first, t.member(header))
    assert c.data[4096:4096 + len(fake)] == fake
    out.append(c)
    return out


def _members():
    out = []
    text = IC.fastq_text(3000, 5)
    out.append(case("three_members", Stream().fixed([], final=True).member(), Stream().fixed([65], final=True).member(),
                    (HDR, IC.raw_deflate(text), text)))
    d = IC.dressed_header_member()
    body = IC.raw_deflate(d.plain)
    head = d.comp[:len(d.comp) - 8 - len(body)]
    assert d.comp == head + body + IC.trailer(d.plain)
    s = Stream()
    s.dyn(s.lits(100)).dyn(s.lits(100), final=True)
    out.append(case("dressed_later_member", s.member(), (head, body, d.plain), (HDR, IC.raw_deflate(text), text)))
    bg = []
    for k in range(40):
        plain = IC.fastq_text(50 + 37 * k, 100 + k)
        m = IC.zmember("m", plain, tag="BC", level=k % 10)
        bg.append((m.comp[:18], m.comp[18:-8], plain))
    bg.append((IC.zmember("eof", b"", tag="BC").comp[:18], IC.zmember("eof", b"", tag="BC").comp[18:-8], b""))
    out.append(case("bgzf_chain", *bg))
    return out


def _reach_back():
    """member 2 copies from member 1's bytes: from its first segment, and from a later one.  zlib refuses both."""
    s = Stream()
    s.dyn(s.lits(300), final=True)
    first = s.member()
    out = []
    for name, lead in (("reach_back_first_segment", 0), ("reach_back_later_segment", 3)):
        t = Stream(origin=len(HDR) + len(first[1]) + 8 + len(HDR))
        for _ in range(lead):
            t.dyn(t.lits(40), fat=True)
        n = len(t.plain)
        EC.dynamic_block(t.w, LL, DD, t.lits(2) + [(10, n + 2 + 5)] + t.lits(2), True)  # 5 bytes in front of the member's first
        header, body, plain = t.member()  # (the text stops in front of that block: no decoder gets as far as the trailer)
        data = b"".join((first[0], first[1], IC.trailer(first[2]), header, body, IC.trailer(plain)))
        assert arbiter(data) is None
        out.append(Case(name, data, None))
    return out


@functools.lru_cache(maxsize=1)
def derived_cases():
    """good files whose info is derived: (Case, plain)"""
    zl = [zcase("zlib_level_%d" % lv, IC.fastq_text(300000, 40 + lv), lv) for lv in (1, 6, 9)]
    zl.append(zcase("zlib_random", IC.random_bytes(150000, 3), 6))
    out = []
    for c in zl + _repairs() + _windows() + _planted() + _members():
        plain = b"".join(p for _, _, p in c.members)
        assert arbiter(c.data) == plain and len(plain) < 400000, c.name
        out.append((c, plain))
    return tuple(out)


ZLIB_CASES = ("zlib_level_1", "zlib_level_6", "zlib_level_9", "zlib_random")
WANTED = {  # every edge the issue names, and the chunk sizes at which some case has to reach it
    "first block start of a chunk: stored": (64, 4096), "first block start of a chunk: fixed": (64,),
    "first block start of a chunk: dynamic": (64, 4096, 0), "first block start of a chunk: dynamic, final": (64, 4096),
    "first block start of a chunk: fixed, final": (64,),
    "block spans 3 chunks": (64,), "block start on a chunk's first bit": (64, 4096), "block start on a chunk's last bit": (64, 4096),
    "comp_len a multiple of the chunk": (64, 4096), "smaller than one chunk": (64, 4096, 0),
    "distance 1 into the previous segment": (64, 4096), "distance 32768 into an earlier segment": (64, 4096, 0),
    "length 258 from in front of the segment": (64, 4096, 0), "source straddles 2 earlier segments": (64,),
    "source straddles 3 earlier segments": (64,), "segment of 0 bytes": (64, 4096), "segment of 1 bytes": (64,),
    "candidate discarded": (64, 4096, 0),
}


@functools.lru_cache(maxsize=1)
def arbiter_cases():
    """[(name, data)]: every good and bad member of inflate_cases and inflate_edge_cases alone and behind a good member,
    flipped CRC and ISIZE, trailing zeros and junk, the files that reach back; zlib says what each gives"""
    good = list(IC.good_members()) + list(EC.good_edge_members())
    bad = list(IC.bad_members()) + [m for m, _ in EC.bad_edge_members()]
    lead = IC.zmember("lead", IC.fastq_text(700, 1)).comp
    out = []
    for m in good + bad:
        out.append((m.name, m.comp))
        out.append(("lead+" + m.name, lead + m.comp))
    base = dict((c.name, c.data) for c, _ in derived_cases())["every_block_type"]
    for name, at in (("crc", -8), ("isize", -4)):
        out.append(("flipped_" + name, base[:at] + bytes([base[at] ^ 1]) + base[at:][1:]))
    two = lead + lead
    mid = len(lead) - 8
    out.append(("flipped_crc_first_member", two[:mid] + bytes([two[mid] ^ 4]) + two[mid + 1:]))
    for name, tail in (("zeros", b"\0" * 9), ("one_byte", b"\x1f"), ("junk", b"junk!"), ("junk_with_magic", b"\x1f\x8bjunk"),
                       ("magic_alone", b"\x1f\x8b")):
        out.append(("trailing_" + name, base + tail))
    out += [(c.name, c.data) for c in _reach_back()]
    return tuple(out)


def small_files():
    """the files every prefix of which is tried"""
    return [(c.name, c.data) for c, _ in derived_cases() if len(c.data) <= 1500]


# ---- the core as plain C++ (tests/inflate_stream_host.cpp) ----
def build_host(directory, flags=(), name="libinfs_host.so"):
    """flags: further compiler flags (another INFS_REBASE, say), for a second library beside the first: give it a `name`"""
    import ctypes as C
    import subprocess

    so = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-o", so, os.path.join(HERE, "inflate_stream_host.cpp")])
    L = C.CDLL(so)
    L.infs_host_set_launch.restype = None
    L.infs_host_set_launch.argtypes = [C.c_int, C.c_int]
    L.infs_host_inflate.restype = C.c_int32
    L.infs_host_inflate.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int64]

    def inflate(data: bytes, chunk: int, cap: int, seg_room: int = 4):
        """-> (rc, bytes or None, plain_len, info, member, at, the output buffer beyond what was asked for untouched)"""
        out = np.full(cap + 64, 0xC5, dtype=np.uint8)
        plen, info, member, at = C.c_int64(-1), np.full(8, -1, dtype=np.int64), C.c_int32(-1), C.c_int64(-1)
        rc = L.infs_host_inflate(data, len(data), chunk, out.ctypes.data, cap, C.byref(plen), info.ctypes.data, C.byref(member), C.byref(at),
                                 seg_room)
        used = plen.value if rc == 0 else 0
        return rc, (out[:used].tobytes() if rc == 0 else None), plen.value, info.tolist(), member.value, at.value, bool((out[used:] == 0xC5).all())

    inflate.chunk_default = int(L.infs_host_chunk_default())
    inflate.set_launch = L.infs_host_set_launch  # (fill, grid): how a workgroup starts, see inflate_stream_host.cpp; (-1, 0) is the default
    return inflate
