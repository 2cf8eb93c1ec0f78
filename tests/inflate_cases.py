"""Gzip members for the device inflate (csrc/bdx_inflate_core.h), shared by its CPU and GPU tests: raw deflate bodies
from zlib (wbits = -15) or written bit by bit here, inside a hand-written BGZF ('B','C') or 'D','X' header.  zlib is the
arbiter: every good member gunzips to its text, every bad one is refused by gzip.decompress — checked when the lists
are built."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import tempfile
import zlib
from collections import namedtuple

import numpy as np

import deflate_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
MEMBER_MAX = 65536
STATUS = {0: "ok", 1: "bad header", 2: "bad block type", 3: "bad stored lengths", 4: "bad code set", 5: "bad symbol",
          6: "distance too far", 7: "output overrun", 8: "output short", 9: "input exhausted", 10: "CRC mismatch",
          11: "ISIZE mismatch"}

# plain: what the member inflates to (None: zlib refuses it); plen: the ISIZE its trailer states (the slot it is given)
Member = namedtuple("Member", "name comp plain plen")


# ---- texts ----
def fastq_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        ln = int(rng.integers(30, 151))
        rec = (b"@A00123:45:HXXXXXXX:1:1101:%d:%d 1:N:0:ACGT\n" % tuple(rng.integers(1000, 32000, 2))
               + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ln).tobytes() + b"\n+\n"
               + rng.choice(np.frombuffer(b"FFFFFF:,#", dtype=np.uint8), ln).tobytes() + b"\n")
        out.append(rec)
        size += len(rec)
    return b"".join(out)[:n]


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- members ----
def trailer(plain: bytes) -> bytes:
    return zlib.crc32(plain).to_bytes(4, "little") + (len(plain) & 0xFFFFFFFF).to_bytes(4, "little")


def wrap(body: bytes, tail: bytes, tag: str = "auto") -> bytes:
    """a size-tagged gzip member around a raw deflate body: BGZF when it fits 64 KiB (or asked for), else 'D','X'"""
    if tag == "auto":
        tag = "BC" if 18 + len(body) + 8 <= 65536 else "DX"
    if tag == "BC":
        total = 18 + len(body) + 8
        assert total <= 65536
        return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (total - 1).to_bytes(2, "little") + body + tail
    total = 20 + len(body) + 8
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x08\0DX\x04\0" + total.to_bytes(4, "little") + body + tail


def raw_deflate(plain: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None:
        return z.compress(plain) + z.flush()
    return z.compress(plain[:flush_at]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(plain[flush_at:]) + z.flush()


def zmember(name, plain, tag="auto", **kw) -> Member:
    return Member(name, wrap(raw_deflate(plain, **kw), trailer(plain), tag), plain, len(plain))


class Bits:
    """deflate's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, val, nbits):
        self.acc |= val << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def fixed_lit(self, sym):
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def fixed_match(self, length, dist):
        lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
        lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
        dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                 8193, 12289, 16385, 24577]
        ls = max(i for i in range(29) if lbase[i] <= length) if length < 258 else 28
        self.fixed_lit(257 + ls)
        self.put(length - lbase[ls], lext[ls])
        ds = max(i for i in range(30) if dbase[i] <= dist)
        self.code(ds, 5)
        self.put(dist - dbase[ds], 0 if ds < 4 else (ds - 2) >> 1)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


def far_match_member() -> Member:
    """a match at distance 32768, the farthest there is (zlib itself stops at 32506): a stored block of 32768 bytes,
    then a fixed block whose only token copies 258 bytes from the member's first byte"""
    head = random_bytes(32768, 91)
    b = Bits()
    b.put(0, 3)  # not final, stored
    body = b.bytes() + (32768).to_bytes(2, "little") + (32768 ^ 0xFFFF).to_bytes(2, "little") + head
    b = Bits()
    b.put(1 | (1 << 1), 3)
    b.fixed_match(258, 32768)
    b.fixed_lit(256)
    plain = head + head[:258]
    return Member("far_match_32768", wrap(body + b.bytes(), trailer(plain)), plain, len(plain))


def dressed_header_member() -> Member:
    """FEXTRA with a foreign subfield in front of the tag, FNAME, FCOMMENT and FHCRC"""
    plain = fastq_text(3001, 17)
    body = raw_deflate(plain)
    extra_wo = b"ZZ\x03\0abc" + b"DX\x04\0"
    rest = b"reads.fastq\0" + b"a comment\0"
    total = 10 + 2 + len(extra_wo) + 4 + len(rest) + 2 + len(body) + 8
    head = b"\x1f\x8b\x08" + bytes([4 | 8 | 16 | 2]) + b"\0\0\0\0\0\xff" + (len(extra_wo) + 4).to_bytes(2, "little") + extra_wo \
        + total.to_bytes(4, "little") + rest
    head += (zlib.crc32(head) & 0xFFFF).to_bytes(2, "little")
    return Member("dressed_header", head + body + trailer(plain), plain, len(plain))


def encoder_members(encode=None):
    """members of the device encoder itself (its plain C++ build): dynamic blocks, a stored one, one distance code"""
    encode = encode or DC.host_encoder()
    out = []
    for name, plain in (("enc_text", fastq_text(2 * DC.CH + 1, 23)), ("enc_random", random_bytes(5000, 24)),
                        ("enc_one_distance", b"ab" * 2000)):  # (one distance code: a single one-bit code, an incomplete set zlib accepts)
        p = 0
        for k, m in enumerate(DC.split_members(encode(plain))):
            n = int.from_bytes(m[-4:], "little")
            out.append(Member("%s_%d" % (name, k), m, plain[p:p + n], n))
            p += n
        assert p == len(plain)
    return out


@functools.lru_cache(maxsize=1)
def good_members():
    out = []
    for n in (0, 1, 2, 3, 257, 258, 259, 32768, 65535, 65536):
        out.append(zmember("text_%d" % n, fastq_text(n, n + 1)))
    for n in (258, 259, 65536):
        out.append(zmember("rle_%d" % n, b"G" * n, level=9))  # length-258 matches at distance 1
    for n in (257, 32768, 65536):
        out.append(zmember("random_%d" % n, random_bytes(n, n)))  # stored blocks; 65536: more than one
    out.append(zmember("level0_60000", fastq_text(60000, 5), level=0))
    out.append(zmember("level1_65536", fastq_text(65536, 6), level=1))
    out.append(zmember("level9_65536", fastq_text(65536, 7), level=9))
    out.append(zmember("fixed_40000", fastq_text(40000, 8), strategy=zlib.Z_FIXED))
    out.append(zmember("huffman_only_40000", fastq_text(40000, 9), strategy=zlib.Z_HUFFMAN_ONLY))
    out.append(zmember("rle_strategy_40000", fastq_text(40000, 10), strategy=zlib.Z_RLE))
    out.append(zmember("full_flush_30000", fastq_text(30000, 11), flush_at=12345))
    out.append(zmember("text_dx_tag_5000", fastq_text(5000, 12), tag="DX"))
    out.append(far_match_member())
    out.append(dressed_header_member())
    out += encoder_members()
    for m in out:
        assert gzip.decompress(m.comp) == m.plain and m.plen == len(m.plain) <= MEMBER_MAX, m.name
    kinds = {(m.comp[member_body(m.comp)] >> 1) & 3 for m in out if m.comp[3] == 4}
    assert kinds == {0, 1, 2}
    return tuple(out)


def member_body(comp: bytes) -> int:
    """offset of the deflate body of a member without FNAME / FCOMMENT / FHCRC"""
    return 12 + int.from_bytes(comp[10:12], "little")


def _retag(comp: bytes) -> bytes:
    """the member with its size tag set to its length (after bytes were cut off)"""
    if comp[12:14] == b"BC":
        return comp[:16] + (len(comp) - 1).to_bytes(2, "little") + comp[18:]
    return comp[:16] + len(comp).to_bytes(4, "little") + comp[20:]


@functools.lru_cache(maxsize=1)
def bad_members():
    plain = fastq_text(5000, 31)
    good = zmember("base", plain).comp
    b0 = member_body(good)
    out = []

    def add(name, comp, plen=None):
        out.append(Member(name, comp, None, int.from_bytes(comp[-4:], "little") if plen is None else plen))

    add("crc_bit", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:])
    add("isize_small", good[:-4] + (len(plain) - 1).to_bytes(4, "little"))
    add("isize_large", good[:-4] + (len(plain) + 1).to_bytes(4, "little"))
    add("btype_3", good[:b0] + bytes([good[b0] | 6]) + good[b0 + 1:])
    mid = (b0 + len(good) - 8) // 2
    add("body_bit", good[:mid] + bytes([good[mid] ^ 0x10]) + good[mid + 1:])
    stored = zmember("s", plain, level=0).comp
    s0 = member_body(stored)
    add("stored_nlen", stored[:s0 + 3] + bytes([stored[s0 + 3] ^ 0x40]) + stored[s0 + 4:])
    b = Bits()  # 1 10 0000001 00000 0000000: final, fixed; length 3 at distance 1 as the first symbol; end of block
    b.put(1 | (1 << 1), 3)
    b.fixed_match(3, 1)
    b.fixed_lit(256)
    assert b.bytes() == bytes([0x03, 0x02, 0x00])
    add("distance_before_start", wrap(b.bytes(), zlib.crc32(b"\0\0\0").to_bytes(4, "little") + (3).to_bytes(4, "little")))
    add("truncated_9", _retag(good[:-9]), plen=len(plain))  # (the slot the whole member had)
    b = Bits()  # dynamic block, 19 code-length code lengths of 1: over-subscribed
    b.put(1 | (2 << 1), 3)
    b.put(0, 5)
    b.put(0, 5)
    b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    b.put(0, 32)
    add("oversubscribed_code_lengths", wrap(b.bytes(), trailer(b"")))
    for m in out:
        try:
            gzip.decompress(m.comp)
        except Exception:  # noqa: BLE001 - zlib.error, EOFError, gzip.BadGzipFile: refused, which is the point
            continue
        raise AssertionError("gzip.decompress accepts " + m.name)
    return tuple(out)


# ---- the decoder as plain C++ (tests/inflate_core_host.cpp) ----
def build_host_decoder(directory):
    """g++ build of tests/inflate_core_host.cpp in `directory`; returns decode(comp, plen, fresh=False) -> (status, bytes).
    All calls share ONE InfShared, as the members of a persistent workgroup do; fresh=True zeroes it first."""
    so = os.path.join(str(directory), "libinf_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "inflate_core_host.cpp")])
    L = C.CDLL(so)
    L.inf_host_decode.restype = C.c_int32
    L.inf_host_decode.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    L.inf_host_reset.restype = None
    assert L.inf_host_member_max() == MEMBER_MAX

    def decode(comp: bytes, plen: int, fresh=False):
        if fresh:
            L.inf_host_reset()
        src = np.frombuffer(comp, dtype=np.uint8).copy()
        out = np.full(max(plen, 1), 0xEE, dtype=np.uint8)
        st = L.inf_host_decode(src.ctypes.data if len(comp) else None, len(comp), out.ctypes.data, plen)
        return int(st), out[:max(plen, 0)].tobytes()

    decode.shared_bytes = int(L.inf_host_shared_bytes())
    return decode


@functools.lru_cache(maxsize=1)
def host_decoder():
    host_decoder.dir = tempfile.TemporaryDirectory(prefix="inf_host_")
    return build_host_decoder(host_decoder.dir.name)


def chain(members) -> bytes:
    return b"".join(m.comp for m in members)


if __name__ == "__main__":
    dec = host_decoder()
    print("InfShared: %d bytes" % dec.shared_bytes)
    for m in good_members():
        st, got = dec(m.comp, m.plen)
        print("%-28s %6d -> %6d bytes  btype %d  status %d%s" % (m.name, len(m.comp), m.plen, (m.comp[member_body(m.comp)] >> 1) & 3,
                                                                 st, "" if st == 0 and got == m.plain else "  WRONG"))
    for m in bad_members():
        st, _ = dec(m.comp, m.plen)
        print("%-28s %6d bytes, slot %6d: status %d (%s)" % (m.name, len(m.comp), m.plen, st, STATUS.get(st, "?")))
