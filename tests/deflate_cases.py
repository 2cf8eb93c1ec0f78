"""The inputs that hold the device DEFLATE encoder (csrc/bdx_deflate_core.h, csrc/bdx_deflate.hip) to its plain C++ build
byte for byte: the host build and its ctypes wrapper, a small inflate parser that states what a member is made of, and
named, deterministic cases, each with a predicate over that anatomy which proves the input reaches the edge it is named
for.  test_device_gzip_cpu.py asserts the predicates on the host build; test_device_gzip_bytes_gpu.py compares the
device's bytes with the host build's on the same cases."""
import collections
import ctypes as C
import functools
import heapq
import itertools
import gzip
import os
import subprocess
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CH = 32768        # DFL_CHUNK (build_host_encoder checks it against the header's)
SUB = 256         # DFL_THREADS: positions of a sub-block; the hash table holds earlier sub-blocks only
TAB_BYTES = 32764  # (DFL_TAB - 1) * 4: the bit buffer less its last word
SEARCH_CAP = 400  # host encodes a boundary search may take (a condition, not a tuning knob)
ALPHABET = np.frombuffer(b"ACGTN\n@+FFFF:,I#0123 ", dtype=np.uint8)  # the 21 letters of the older tests


# ---- the host build ----
def build_host_encoder(directory):
    """g++ build of tests/deflate_core_host.cpp in `directory`; returns encode(data, fresh=False) -> bytes.  The input
    goes in as an exact-size copy (no pad byte behind it).  All calls share ONE DflShared, as the chunks of a persistent
    workgroup do; fresh=True zeroes it first.  encode.last_dynamic_bytes() is dfl_host_last_dynamic_bytes, encode.encodes
    counts the calls."""
    so = os.path.join(str(directory), "libdfl_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "deflate_core_host.cpp")])
    L = C.CDLL(so)
    L.dfl_host_encode.restype = C.c_int64
    L.dfl_host_encode.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.dfl_host_last_dynamic_bytes.restype = C.c_int64
    L.dfl_host_reset.restype = None
    ch = L.dfl_host_chunk()
    assert ch == CH

    def raw(data: bytes, fresh=False) -> bytes:
        if fresh:
            L.dfl_host_reset()
        src = np.frombuffer(data, dtype=np.uint8).copy()  # exactly len(data) bytes of its own
        cap = len(data) + 33 * -(-len(data) // ch) + 64
        out = np.zeros(cap, dtype=np.uint8)
        n = L.dfl_host_encode(src.ctypes.data if len(data) else None, len(data), out.ctypes.data, cap)
        assert 0 <= n <= cap - 64
        encode.encodes += 1
        return out[:n].tobytes()

    def encode(data: bytes, fresh=False) -> bytes:
        comp = raw(data, fresh)
        assert gzip.decompress(comp) == data if data else comp == b""
        assert len(split_members(comp)) == -(-len(data) // ch)
        return comp

    encode.raw = raw  # without the checks: the boundary searches and the large mixes
    encode.chunk = ch
    encode.encodes = 0
    encode.last_dynamic_bytes = lambda: int(L.dfl_host_last_dynamic_bytes())
    return encode


@functools.lru_cache(maxsize=1)
def host_encoder():
    """one host build per process, in a temporary directory of its own"""
    host_encoder.dir = tempfile.TemporaryDirectory(prefix="dfl_host_")
    return build_host_encoder(host_encoder.dir.name)


def split_members(block: bytes):
    """the members of a class block by their 'D','X' sizes; they must land on the block's end"""
    out, p = [], 0
    while p < len(block):
        assert block[p:p + 4] == b"\x1f\x8b\x08\x04" and block[p + 9] == 255, "FEXTRA gzip header with OS = 255"
        assert block[p + 10:p + 16] == b"\x08\x00DX\x04\x00"
        s = int.from_bytes(block[p + 16:p + 20], "little")
        assert s >= 28
        out.append(block[p:p + s])
        p += s
    assert p == len(block)
    return out


# ---- anatomy: a bit-by-bit inflate of one member (RFC 1951 / 1952), with the checks zlib does not make ----
def _len_base(i):  # length symbol 257 + i -> (base, extra bits)
    if i < 8:
        return 3 + i, 0
    if i == 28:
        return 258, 0
    e = (i - 4) >> 2
    return 3 + ((4 + (i & 3)) << e), e


def _dist_base(s):
    if s < 4:
        return s + 1, 0
    e = (s - 2) >> 1
    return 1 + ((2 + (s & 1)) << e), e


def dist_symbol(d):
    return max(s for s in range(30) if _dist_base(s)[0] <= d)


class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def take(self, n):  # n bits, least significant first
        v = 0
        for i in range(n):
            p = self.pos + i
            assert (p >> 3) < len(self.d), "the stream ends inside the block"
            v |= ((self.d[p >> 3] >> (p & 7)) & 1) << i
        self.pos += n
        return v


def _kraft(lengths):
    return sum(1 << (15 - l) for l in lengths if l)  # in units of 2^-15


def _decoder(lengths):
    """canonical Huffman code of RFC 1951 3.2.2: {(bits, code): symbol}"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)  # Huffman codes arrive most significant bit first
        s = table.get((n, code))
        if s is not None:
            return s
    raise AssertionError("no code of at most 15 bits matches")


def anatomy(member: bytes) -> dict:
    """What one member is made of.  Keys: n, data, btype, body_bytes; for a dynamic block also hlit, hdist, ll_lengths,
    d_lengths, tokens ((byte,) or (length, distance, position)), eob_bit (where the end-of-block code starts), end_bit
    (the first bit after it), pad_bits."""
    assert member[:4] == b"\x1f\x8b\x08\x04" and member[4:10] == b"\0\0\0\0\0\xff", "gzip header: FEXTRA only, OS = 255"
    assert member[10:16] == b"\x08\x00DX\x04\x00", "XLEN = 8, subfield 'D','X' of 4 bytes"
    assert int.from_bytes(member[16:20], "little") == len(member), "the 'D','X' size is the member's"
    body = member[20:-8]
    bits = _Bits(body)
    assert bits.take(1) == 1, "one block, BFINAL set"
    btype = bits.take(2)
    a = dict(btype=btype, body_bytes=len(body), tokens=[])
    out = bytearray()
    if btype == 0:
        assert bits.take(5) == 0, "padding bits are zero"
        ln, nl = bits.take(16), bits.take(16)
        assert ln ^ nl == 0xFFFF and len(body) == 5 + ln
        out += body[5:]
    else:
        assert btype == 2, "stored or dynamic, never fixed"
        hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
        assert hlit <= 286 and hdist <= 30
        cl = [0] * 19
        for i in range(hclen):
            cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits.take(3)
        assert _kraft(cl) == 1 << 15, "the code-length code is complete"
        clt, lens = _decoder(cl), []
        while len(lens) < hlit + hdist:
            s = _symbol(bits, clt)
            if s < 16:
                lens.append(s)
            elif s == 16:
                assert lens
                lens += [lens[-1]] * (3 + bits.take(2))
            else:
                lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
        assert len(lens) == hlit + hdist
        ll, dl = lens[:hlit], lens[hlit:]
        assert max(lens) <= 15 and ll[256] > 0
        assert _kraft(ll) == 1 << 15, "the literal/length code is complete (Kraft sum exactly 1)"
        used = [l for l in dl if l]
        assert not used or used == [1] or _kraft(dl) == 1 << 15, "the distance code is empty, one 1-bit code, or complete"
        llt, dt = _decoder(ll), _decoder(dl)
        while True:
            at = bits.pos
            s = _symbol(bits, llt)
            if s == 256:
                break
            if s < 256:
                a["tokens"].append((s,))
                out.append(s)
                continue
            base, e = _len_base(s - 257)
            length = base + bits.take(e)
            base, e = _dist_base(_symbol(bits, dt))
            dist = base + bits.take(e)
            assert 4 <= length <= 258 and 1 <= dist <= len(out), (length, dist, len(out))
            a["tokens"].append((length, dist, len(out)))
            for _ in range(length):
                out.append(out[-dist])
        a.update(hlit=hlit, hdist=hdist, ll_lengths=ll, d_lengths=dl, eob_bit=at, end_bit=bits.pos)
        pad = -bits.pos % 8
        assert bits.take(pad) == 0, "padding bits are zero"
        assert bits.pos == 8 * len(body), "the body ends with the block"
        a["pad_bits"] = pad
        assert len(body) < len(out) + 5 and len(body) <= TAB_BYTES, "a dynamic body is smaller than stored and fits the bit buffer"
    assert 1 <= len(out) <= CH
    assert int.from_bytes(member[-8:-4], "little") == zlib.crc32(bytes(out)), "CRC-32"
    assert int.from_bytes(member[-4:], "little") == len(out), "ISIZE"
    a.update(n=len(out), data=bytes(out))
    return a


# ---- what the predicates ask ----
def _matches(a):
    return [t for t in a["tokens"] if len(t) == 3]


def _dynamic(A):
    return all(a["btype"] == 2 for a in A)


def _stored(A):
    return all(a["btype"] == 0 for a in A)


def _d_used(a):
    return [l for l in a["d_lengths"] if l]


def _earlier_sub_blocks_only(A):
    """every candidate lies in an earlier sub-block than its match: the table is consulted before this sub-block's inserts"""
    return all((p - d) // SUB < p // SUB for a in A for (_, d, p) in _matches(a))


def _has_258(A):
    return _dynamic(A) and any(l == 258 for a in A for (l, _, _) in _matches(a)) and all(a["ll_lengths"][285] > 0 for a in A if _matches(a))


def _all_literals_no_distance_code(A):
    return _dynamic(A) and not _matches(A[0]) and A[0]["hdist"] == 1 and not _d_used(A[0])


def _period_256(A):
    m = _matches(A[0])
    return _dynamic(A) and m and all(d == 256 for (_, d, _) in m) and _d_used(A[0]) == [1]


def _period_255(A):
    m = _matches(A[0])
    # position 255 repeats position 0 inside sub-block 0: no match may start there; the matches begin in sub-block 1
    return (_dynamic(A) and any(d == 255 for (_, d, _) in m) and _earlier_sub_blocks_only(A)
            and min(p for (_, _, p) in m) >= SUB)


def _far(A):
    return _dynamic(A) and any(d >= 24577 for (_, d, _) in _matches(A[0])) and A[0]["d_lengths"][29] > 0


def _ends_with_match(k):
    def pred(A):
        a = A[0]
        t = a["tokens"][-1]
        return _dynamic(A) and len(t) == 3 and t[0] == 40 + k and t[2] + t[0] == a["n"] and t[2] == 300
    return pred


def _huffman_depth(counts):
    """the longest code of an unrestricted Huffman code over `counts`"""
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]


def _len_symbol(length):
    return max(i for i in range(29) if _len_base(i)[0] <= length) + 257 if length < 258 else 285


def _some_length_15(A):
    """a literal/length code of 15 bits where the unrestricted code is deeper: the limit was at work"""
    hist = collections.Counter([256] + [t[0] if len(t) == 1 else _len_symbol(t[0]) for t in A[0]["tokens"]])
    return _dynamic(A) and max(A[0]["ll_lengths"]) == 15 and _huffman_depth(hist.values()) > 15


def _one_distance_symbol(A):
    return _dynamic(A) and len(_d_used(A[0])) == 1 and _d_used(A[0]) == [1] and len(_matches(A[0])) >= 1


def _all_30_distance_symbols(A):
    a = A[0]
    return _dynamic(A) and {dist_symbol(d) for (_, d, _) in _matches(a)} == set(range(30)) and all(a["d_lengths"])


def _members(k):
    return lambda A: len(A) == k


# ---- the cases ----
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def text(n, name):
    return _rng(name).choice(ALPHABET, n).tobytes()


def _hash(w4: bytes) -> int:  # dfl_ph_find's
    return ((int.from_bytes(w4, "little") * 2654435761) & 0xFFFFFFFF) >> 19


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


def _far_match():
    rng = _rng("far")
    d = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), CH).tobytes())
    block = rng.integers(128, 256, 64, dtype=np.uint8).tobytes()
    d[0:64] = block
    d[CH - 64:CH] = block
    d[CH - 4:CH] = block[:4]
    return bytes(d)


def _end_clamp(k):
    block = text(300, "clamp%d" % k)
    return block + block[:40 + k]  # the copy starts sub-block 1 at position 300 and ends the chunk


def _all_distance_symbols():
    """random ACGT (256 four-grams: few table slots taken, many natural matches) with one planted six-byte match per
    distance symbol at the symbol's base distance.  Every plant's four-gram hashes to a slot no other gram of the text
    uses, so the candidate survives until its match; the short distances straddle a sub-block boundary."""
    rng = _rng("dist30")
    d = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), CH).tobytes())
    taken = {_hash(bytes(g)) for g in itertools.product(b"ACGT", repeat=4)}
    used = []  # [lo, hi) of what was planted

    def free(lo, hi):
        return lo >= 0 and hi <= CH and all(hi <= a or lo >= b for a, b in used)

    for s in range(30):
        dist = _dist_base(s)[0]
        sub = 97 + s  # sub-blocks 97 .. 126: far enough in for distance 24 577
        for offs in ([0] if dist < SUB else range(8, 240, 8)):
            p = SUB * sub + offs
            src = (p - dist, p - dist + min(dist, 6))
            if free(p, p + 6) and free(*src) and (src[1] <= p):
                break
        else:
            raise AssertionError("no room for the plant of distance symbol %d" % s)
        while True:
            pat = rng.integers(128, 256, 6, dtype=np.uint8).tobytes()
            seq = bytearray(pat[:min(dist, 6)])
            while len(seq) < dist + 6 and dist < 6:
                seq.append(seq[-dist])
            grams = [bytes(seq[i:i + 4]) for i in range(len(seq) - 3)] if dist < 6 else [pat[i:i + 4] for i in range(3)]
            hs = {_hash(g) for g in grams}
            if not (hs & taken):
                taken |= hs
                break
        d[src[0]:src[1]] = pat[:min(dist, 6)]
        for i in range(6):
            d[p + i] = d[p + i - dist]
        used += [(p, p + 6), src]
    return bytes(d)


def _deep_code(seed=0):
    """A chunk whose TOKEN histogram is a Fibonacci-like chain of 17 symbols (every count at least the sum of the two
    below it), so that an unrestricted Huffman code is 16 deep and the encoder has to limit it.  Byte counts alone do
    not do that: the matches take most of the frequent bytes away (the Fibonacci byte counts of the older tests end at
    code lengths of 10 to 13).  Sub-block 0 is literals whatever it holds: ten letters with counts 1, 2, 3, 5, 8, 13, 21,
    34, 59, 110 (and the end-of-block symbol's 1), the last 39 bytes being six words of 4 .. 9 distinct letters.  The
    rest is those words again, 2 150 / 1 320 / 810 / 490 / 300 / 175 times from the shortest: each is one match of its
    own length, because the word that follows differs in its first letter from the one that followed the candidate
    (the word's latest occurrence in an earlier sub-block)."""
    letters = b"abcdefghij"
    counts = dict(zip(letters, (1, 2, 3, 5, 8, 13, 21, 34, 59, 110)))
    sets = {9: b"ebcdfghij", 8: b"fcdeghij", 7: b"gdefhij", 6: b"hefgij", 5: b"ifghj", 4: b"jghi"}  # first letters differ
    want = {4: 2150, 5: 1320, 6: 810, 7: 490, 8: 300, 9: 175}
    rng = np.random.default_rng(1000 + seed)
    words = {L: w[:1] + bytes(rng.permutation(np.frombuffer(w[1:], dtype=np.uint8))) for L, w in sets.items()}
    for w in words.values():
        for b in w:
            counts[b] -= 1
    assert min(counts.values()) >= 0
    text = bytearray(b"".join(bytes([b]) * counts[b] for b in letters))  # sorted runs: no four distinct letters in a row
    occ = {L: [] for L in words}  # [start, length of the word that followed]
    last = None

    def put(L):
        nonlocal last
        if last is not None:
            last[1] = L
        last = [len(text), None]
        occ[L].append(last)
        text.extend(words[L])

    for L in (9, 8, 7, 6, 5, 4):
        put(L)
    assert len(text) == SUB
    left = dict(want)
    cur = 4
    while True:
        put(cur)
        left[cur] -= 1
        sub = last[0] // SUB
        cand = [o for o in occ[cur] if o[0] // SUB < sub][-1]
        pick = [L for L in left if left[L] > 0 and L != cand[1]]
        if not pick:
            break
        cur = max(pick, key=lambda L: left[L] / want[L])
    assert len(text) <= CH and sum(left.values()) <= 8, left
    grams = {bytes(text[i:i + 4]) for i in range(len(text) - 3)}
    heads = {w[:4] for w in words.values()}
    if any(_hash(g) == _hash(h) for h in heads for g in grams if g != h):
        return _deep_code(seed + 1)  # a word's first four bytes share their table slot with another gram: other words
    return bytes(text)


class Case:
    def __init__(self, name, data, pred, why):
        self.name, self.data, self.pred, self.why = name, data, pred, why
        self.tries = None  # boundary cases: host encodes their search took

    def __repr__(self):
        return self.name


def _plain_cases():
    out = []
    for n in [*range(1, 9), 255, 256, 257, *range(258, 263), 511, 512, 513, *range(CH - 3, CH + 2)]:
        out.append(Case("text_%d" % n, text(n, "text%d" % n), _members(2 if n > CH else 1), "random text over 21 letters"))
    for n in (4, 5, 259, 262, 516, CH):
        pred = _has_258 if n >= 516 else _all_literals_no_distance_code if n == 259 else _members(1)
        out.append(Case("byte_%d" % n, b"G" * n, pred, "one byte repeated; 516 and up: length 258, symbol 285; 259: no distance code"))
    for p in (1, 2, 255, 256, 257, 258, 512):
        pred = {256: _period_256, 255: _period_255}.get(p, _earlier_sub_blocks_only)
        out.append(Case("period_%d" % p, (text(p, "period%d" % p) * (2048 // p + 1))[:2048], pred, "period-p text of 2 048 bytes"))
    out.append(Case("far_match", _far_match(), _far, "distance symbol 29 with 13 extra bits"))
    for k in range(9):
        out.append(Case("end_clamp_%d" % k, _end_clamp(k), _ends_with_match(k), "a match of 40 + k clamped by the chunk's end"))
    out.append(Case("no_repeated_triple", b"aaababbbaa", _stored, "ten bytes: stored"))
    out.append(Case("ab_x40", b"ab" * 40, _stored, "eighty bytes: stored"))
    for k in (21, 22):
        data = np.repeat(np.arange(65, 65 + k, dtype=np.uint8), _fib(k))
        # (byte counts; the matches flatten the token histogram, the longest code is 10 to 13 bits: no length limit here)
        out.append(Case("fib%d_sorted" % k, data.tobytes(), _dynamic, "Fibonacci byte counts"))
        out.append(Case("fib%d_shuffled" % k, np.random.default_rng(11).permutation(data).tobytes(), _dynamic,
                        "Fibonacci byte counts, shuffled"))
    out.append(Case("fib_tokens", _deep_code(), _some_length_15, "Fibonacci-like token counts, 17 symbols: lengths limited to 15"))
    out.append(Case("one_distance_symbol", b"ab" * 258, _one_distance_symbol, "one match: a single 1-bit distance code"))
    out.append(Case("all_distance_symbols", _all_distance_symbols(), _all_30_distance_symbols, "all 30 distance symbols in use"))
    return out


# ---- the stored / dynamic boundary: bytes >= n + 5 || bytes > 32 764 ----
def _probe(enc, data):
    comp = enc.raw(data, fresh=True)
    return enc.last_dynamic_bytes(), comp


def _search_small(enc, want, name):
    """n with dynamic bytes == n + want over one fixed random stream: the excess over n falls by about 1 - H/8 bytes per
    byte of text (H: the alphabet's bits), so bisect on n for the crossing and then walk to the exact value"""
    rng = _rng(name)
    stream = rng.integers(0, 128, 3200, dtype=np.uint8).tobytes()  # a 128-letter alphabet
    tries, seen = 0, {}

    def excess(n):
        nonlocal tries
        if n not in seen:
            tries += 1
            if tries > SEARCH_CAP:
                raise RuntimeError("boundary search %s: not found within %d host encodes" % (name, SEARCH_CAP))
            seen[n] = _probe(enc, stream[:n])[0] - n
        return seen[n]

    lo, hi = 200, 3200
    assert excess(lo) > want > excess(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if excess(mid) > want:
            lo = mid
        else:
            hi = mid
    for step in range(0, 3000):  # outwards from the crossing
        for n in (hi + step, hi - step):
            if 200 <= n <= 3200 and excess(n) == want:
                return stream[:n], tries
    raise RuntimeError("boundary search %s: no n in 200..3200 has dynamic bytes n + %d" % (name, want))


def _search_full(enc, want, name):
    """CH random bytes whose first `pre` are 'A', with dynamic bytes == want: a byte more of the run saves about a byte,
    so move `pre` by the miss, and walk on from the nearest untried value when that returns to a tried one"""
    body = _rng("boundary_full").integers(0, 256, CH, dtype=np.uint8).tobytes()  # (c) and (d) share the random bytes
    pre, tries, seen = 400, 0, {}
    while tries < SEARCH_CAP:
        data = b"A" * pre + body[pre:]
        seen[pre] = got = _probe(enc, data)[0]
        tries += 1
        if got == want:
            return data, tries
        step = got - want
        nxt = pre + step
        while nxt in seen or not 0 <= nxt <= CH:
            nxt += 1 if step > 0 else -1
            if not -CH <= nxt <= 2 * CH:
                raise RuntimeError("boundary search %s: ran out of prefixes" % name)
        pre = nxt
    raise RuntimeError("boundary search %s: not found within %d host encodes" % (name, SEARCH_CAP))


def _boundary_cases(enc):
    out = []
    for tag, search, want, dynamic, why in (
            ("a", _search_small, 4, True, "dynamic bytes n + 4: the last size that stays dynamic"),
            ("b", _search_small, 5, False, "dynamic bytes n + 5: stored"),
            ("c", _search_full, TAB_BYTES, True, "dynamic bytes 32 764 at n = CH: the last free word of the bit buffer"),
            ("d", _search_full, TAB_BYTES + 1, False, "dynamic bytes 32 765 at n = CH: stored although < n + 5")):
        name = "boundary_" + tag
        data, tries = search(enc, want, name)
        c = Case(name, data, _dynamic if dynamic else _stored, why)
        c.tries = tries
        c.dynamic_bytes = want + (len(data) if search is _search_small else 0)  # what dfl_host_last_dynamic_bytes must say
        out.append(c)
    return out


CASES = _plain_cases() + _boundary_cases(host_encoder())
assert len({c.name for c in CASES}) == len(CASES)


# ---- many classes of one chunk each ----
def _fastq_like(rng, n):
    rec = (b"@A00123:45:HXXXXXXX:1:1101:%d:%d 1:N:0:ACGT\n" % tuple(rng.integers(1000, 32000, 2))
           + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150).tobytes() + b"\n+\n"
           + rng.choice(np.frombuffer(b"F:,#FFFF", dtype=np.uint8), 150).tobytes() + b"\n")
    return (rec * (n // len(rec) + 1))[:n]


def persistent_mix(n_chunks, grid):
    """`n_chunks` class texts of one chunk each for a persistent grid of `grid` workgroups.  Chunk c's kind is
    (c + c // grid) % 4 — tiny (1-40 B), FASTQ-like (300-900 B), full dynamic chunk, full stored chunk — so a workgroup
    meets another kind on every iteration.  Full chunks are one class in 16 ((c // 4) % 8 == (c // grid) % 8); the other
    classes of the two full kinds are 300-900 B of the same nature (FASTQ-like: dynamic; random bytes: stored)."""
    rng = np.random.default_rng(20260 + n_chunks + 7 * grid)
    out = []
    for c in range(n_chunks):
        kind = (c + c // grid) % 4
        full = (c // 4) % 8 == (c // grid) % 8
        if kind == 0:
            out.append(rng.choice(ALPHABET, int(rng.integers(1, 41))).tobytes())
        elif kind == 1 or (kind == 2 and not full):
            out.append(_fastq_like(rng, int(rng.integers(300, 901))))
        elif kind == 2:
            out.append(_fastq_like(rng, CH))
        else:
            out.append(rng.integers(0, 256, CH if full else int(rng.integers(300, 901)), dtype=np.uint8).tobytes())
    return out


SCAN_NCH = (1, 255, 256, 257, 511, 513, 768)  # dfl_scan_kernel: runs of 1, 2 and 3 members per thread, empty tail threads


def scan_mix(nch):
    rng = np.random.default_rng(777 + nch)
    return [rng.choice(ALPHABET, int(rng.integers(1, 41))).tobytes() for _ in range(nch)]


def coverage_lines(enc=None):
    """one line per case for profiles/deflate_case_coverage.txt (host build: needs no GPU); of an input of two chunks
    the dynamic bytes are the last chunk's, the other figures are over both members"""
    enc = enc or host_encoder()
    lines = []
    for c in CASES:
        comp = enc(c.data, fresh=True)
        dyn = enc.last_dynamic_bytes()
        A = [anatomy(m) for m in split_members(comp)]
        a = A[-1]
        m = [t for x in A for t in _matches(x)]
        lines.append("%-22s n %6d  %-7s dynamic bytes %6d  tokens %6d  max distance %6d  max length %4d  max code length %2d%s" % (
            c.name, len(c.data), "+".join("stored" if x["btype"] == 0 else "dynamic" for x in A), dyn, sum(len(x["tokens"]) for x in A),
            max([d for (_, d, _) in m], default=0), max([l for (l, _, _) in m], default=0),
            max([max(x["ll_lengths"] + x["d_lengths"]) for x in A if x["btype"] == 2], default=0),
            "  search: %d host encodes" % c.tries if c.tries else ""))
    return lines


if __name__ == "__main__":
    print("\n".join(coverage_lines()))
