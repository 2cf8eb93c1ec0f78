"""A seeded corpus of .gz files for the stream inflate (csrc/bdx_inflate_stream_core.h), shared by its CPU, sanitizer and
GPU tests.  Nothing is typed in: zlib (`SC.arbiter`) says what every file gives, and for the files whose block positions
are known (`case` is set) `SC.expected_info` says what the counters must be.

  zlib family     levels 0-9, memLevel 1/2/8/9, every strategy, wbits 9-15, up to 40 sync and full flushes, 1-3 members,
                  FASTQ text, random bytes and a short repeated piece, sizes 0 .. 120 000
  pigz-like       pieces of 8-32 KB deflated on their own with the 32 KiB in front as dictionary, each closed by a sync
                  flush, concatenated and closed by the empty final fixed block 03 00: one member
  block writer    random sequences of dynamic, fixed and stored blocks (SC.Stream) with random tokens whose sources reach
                  into earlier segments, block starts padded onto a chunk's first or last bit
  named           memlevel1_l6, memlevel1_l1 (hundreds of small dynamic blocks), many_members (1100 members: the segment
                  list outgrows its first room at the default chunk size and at 4096)
  mutants         1-2 flipped bits, and truncations, of every file

Every file carries its own chunk sizes: 64, one of 65..300, one of 300..5000, one of ODD, and 0 (the default)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import inflate_cases as IC
import inflate_stream_cases as SC

SEED = 20260
ODD = (65, 127, 129, 1000, 4097)
SIZES = (0, 1, 50, 700, 5000, 40000, 120000)
N_ZLIB, N_PIGZ, N_BLOCKS = 250, 14, 40
MUTANTS_PER_FILE = 5
TAG = "@%d" % SEED  # every name ends with it: two lists of files with the same names are the same files

# case: an SC.Case with its members' bodies when the block positions can be derived, else None
Good = namedtuple("Good", "name data plain case chunks")
# want: what zlib gives, None when it refuses; chunks: 64, the source's random one, the default
Mutant = namedtuple("Mutant", "name data want chunks")


def _chunks(rng):
    return (64, int(rng.integers(65, 301)), int(rng.integers(300, 5001)), ODD[int(rng.integers(len(ODD)))], 0)


def _text(rng, n):
    kind, seed = int(rng.integers(3)), int(rng.integers(1 << 30))
    if kind == 0:
        return IC.fastq_text(n, seed)
    if kind == 1:
        return IC.random_bytes(n, seed)
    piece = IC.fastq_text(int(rng.integers(40, 400)), seed)  # long matches at a distance far below 32768
    return (piece * (n // len(piece) + 1))[:n]


# ---- zlib family ----
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY,) * 4 + (zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def _zlib_body(rng, plain):
    z = zlib.compressobj(int(rng.integers(0, 10)), zlib.DEFLATED, -(9, 10, 12, 15)[int(rng.integers(4))], (1, 1, 2, 8, 9)[int(rng.integers(5))],
                         STRATEGIES[int(rng.integers(len(STRATEGIES)))])
    n_flush = int(rng.integers(0, 41)) if rng.integers(3) else 0
    cuts = sorted(int(c) for c in rng.integers(0, len(plain) + 1, n_flush))
    out, p = [], 0
    for c in cuts:
        out.append(z.compress(plain[p:c]))
        out.append(z.flush(zlib.Z_SYNC_FLUSH if rng.integers(2) else zlib.Z_FULL_FLUSH))
        p = c
    out.append(z.compress(plain[p:]))
    out.append(z.flush())
    return b"".join(out)


def _zlib_file(rng, k):
    members = []
    for _ in range(int(rng.integers(1, 4))):
        plain = _text(rng, SIZES[int(rng.integers(len(SIZES)))])
        members.append((SC.HDR, _zlib_body(rng, plain), plain))
    c = SC.case("zlib_%d%s" % (k, TAG), *members)
    return Good(c.name, c.data, b"".join(m[2] for m in members), None, _chunks(rng))


# ---- pigz-like ----
def pigz_body(rng, plain):
    out, p = [], 0
    while p < len(plain):
        n = int(rng.integers(8192, 32769))
        zdict = plain[max(0, p - 32768):p]
        level = int(rng.integers(1, 10))
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(z.compress(plain[p:p + n]) + z.flush(zlib.Z_SYNC_FLUSH))
        p += n
    return b"".join(out) + b"\x03\x00"


def _pigz_file(rng, k):
    plain = _text(rng, (40000, 40000, 120000)[int(rng.integers(3))])
    c = SC.case("pigz_%d%s" % (k, TAG), (SC.HDR, pigz_body(rng, plain), plain))
    return Good(c.name, c.data, plain, c, _chunks(rng))


# ---- block writer ----
def _tokens(rng, s, n, p_match):
    """n random tokens behind s.plain; a match: length 3..258, distance 1, 2, the length, any, or all the history there is"""
    toks, hist = [], len(s.plain)
    lits = s.lits(n) if rng.integers(2) else [int(v) for v in rng.integers(0, 256, n)]
    for i in range(n):
        if hist and rng.random() < p_match:
            length = int(rng.integers(3, 259))
            far = min(hist, 32768)
            dist = (1, 2, length, int(rng.integers(1, far + 1)), far)[int(rng.integers(5))]
            toks.append((length, min(dist, far)))
            hist += length
        else:
            toks.append(lits[i])
            hist += 1
    return toks


def _block_member(rng, origin, chunk, fake, style):
    s = SC.Stream(origin=origin)
    n_blocks = int(rng.integers(2, 14)) if style != 1 else int(rng.integers(20, 50))
    for b in range(n_blocks):
        final = b == n_blocks - 1
        what = int(rng.integers(10))
        if not final and what == 0:  # the next block starts on a chunk's first bit
            s.pad_to((s.byte() // chunk + 2) * chunk)
            continue
        if not final and what == 1:  # ... on a chunk's last bit: 3 + 5 * 9 + 7 = 55 bits in front of it
            s.pad_to((s.byte() // chunk + 2) * chunk - 7).fixed([200, 201, 202, 203, 204])
            continue
        if style == 1:  # many short fat dynamic blocks: at 64 bytes a chunk each is a segment, and sources run over several
            s.dyn(_tokens(rng, s, int(rng.integers(0, 12)), 0.4), final=final, fat=True)
            continue
        if what <= 3:
            n = (0, 1, 5, 70, 300, 9000, 33000)[int(rng.integers(7))] if style == 2 else (0, 1, 5, 70, 300)[int(rng.integers(5))]
            data = s.text(n)
            if n >= 300 and rng.integers(2):
                data = data[:100] + fake + data[100 + len(fake):]  # a false candidate inside a stored block
                assert len(data) == n
            s.stored(data, final=final)
        elif what <= 5:
            s.fixed(_tokens(rng, s, int(rng.integers(0, 40)), 0.3), final=final)
        else:
            s.dyn(_tokens(rng, s, int(rng.integers(0, 60)), 0.3), final=final, fat=bool(rng.integers(2)))
    return s.member()


def _block_file(rng, k, fake):
    chunks = _chunks(rng)
    chunk = chunks[int(rng.integers(3))]  # the chunk size the padding is meant for
    members, at = [], 0
    for _ in range(int(rng.integers(1, 3))):
        m = _block_member(rng, at + len(SC.HDR), chunk, fake, k % 3)
        members.append(m)
        at += len(m[0]) + len(m[1]) + 8
    c = SC.case("blocks_%d%s" % (k, TAG), *members)
    return Good(c.name, c.data, b"".join(m[2] for m in members), c, chunks)


# ---- named ----
@functools.lru_cache(maxsize=None)
def memlevel1(level, n=200000):
    """FASTQ text at memLevel 1: hundreds of small dynamic blocks"""
    plain = IC.fastq_text(n, 600 + level)
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 1)
    c = SC.case("memlevel1_l%d" % level + ("" if n == 200000 else "_%d" % n), (SC.HDR, z.compress(plain) + z.flush(), plain))
    return Good(c.name, c.data, plain, c, (64, 256, 129))


@functools.lru_cache(maxsize=1)
def many_members():
    """1100 members of 20-70 bytes of text: more segments than the chain's first room at the default chunk size and at 4096"""
    rng = np.random.default_rng(SEED + 1)
    members = []
    for k in range(1100):
        plain = IC.fastq_text(int(rng.integers(20, 71)), 9000 + k)
        members.append((SC.HDR, IC.raw_deflate(plain, level=1 + k % 9), plain))
    c = SC.case("many_members", *members)
    return Good(c.name, c.data, b"".join(m[2] for m in members), c, (0, 4096, 64))


def named():
    return (memlevel1(6), memlevel1(1), many_members())


# ---- the corpus ----
@functools.lru_cache(maxsize=1)
def good_files():
    rng = np.random.default_rng(SEED)
    fake = SC._planted_block()
    out = [_zlib_file(rng, k) for k in range(N_ZLIB)]
    out += [_pigz_file(rng, k) for k in range(N_PIGZ)]
    out += [_block_file(rng, k, fake) for k in range(N_BLOCKS)]
    for g in out:
        assert SC.arbiter(g.data) == g.plain, g.name
    return tuple(out)


def _mutants_of(rng, g):
    out, n = [], len(g.data)
    for j in range(MUTANTS_PER_FILE):
        if j == MUTANTS_PER_FILE - 1:  # a truncation: mostly near the end, where the trailer and the last block are
            cut = int(rng.integers(max(0, n - 40), n)) if rng.integers(2) else int(rng.integers(0, n))
            data, kind = g.data[:cut], "cut%d" % cut
        else:
            b = bytearray(g.data)
            for _ in range(int(rng.integers(1, 3))):  # anywhere, or in the first header and block header: MTIME, XFL and OS are free
                b[int(rng.integers(n if rng.integers(2) else min(n, 16)))] ^= 1 << int(rng.integers(8))
            data, kind = bytes(b), "flip%d" % j
        out.append(Mutant("%s/%s" % (g.name, kind), data, SC.arbiter(data), (64, g.chunks[1 + int(rng.integers(3))], 0)))
    return out


@functools.lru_cache(maxsize=1)
def mutants():
    rng = np.random.default_rng(SEED + 2)
    out = []
    for g in good_files():
        out += _mutants_of(rng, g)
    return tuple(out)


@functools.lru_cache(maxsize=1)
def fixed_slice():
    """(100 good files, 300 mutants): what the launch-independence, rebase, sanitizer and GPU tests all run"""
    good, bad = good_files()[::3][:100], mutants()[::4][:300]  # (4 and MUTANTS_PER_FILE coprime: every kind of mutant)
    assert len(good) == 100 and len(bad) == 300
    return good, bad


def slice_chunks(g):
    """the chunk sizes a good file of the slice runs at: 64, one of ODD, the default (its mutants: 64)"""
    return (64, g.chunks[3], 0)


def slice_files():
    """the slice as the sanitizer driver and the GPU take it: [(name, data, zlib's text or None, chunk sizes)]"""
    good, bad = fixed_slice()
    return [(g.name, g.data, g.plain, slice_chunks(g)) for g in good] + [(m.name, m.data, m.want, (64,)) for m in bad]


def known(goods):
    """the files whose info is derived"""
    return [g for g in goods if g.case is not None]
