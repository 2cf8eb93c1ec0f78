"""The inputs that hold level 2 of the device DEFLATE encoder (csrc/bdx_deflate2_core.h, dfl2_encode_kernel) to its
plain C++ build byte for byte, after the pattern of deflate_cases.py: the host build of tests/deflate2_core_host.cpp and
its ctypes wrapper, a parser of the run-length coded block header, and named, deterministic cases, each with a predicate
that proves on the host build that the input reaches the edge it is named for.  A predicate sees the members' anatomy
(deflate_cases.anatomy), their tokens by position, their header symbols and — for the lazy and bucket edges, where the
match that gave way is in no token — every position's best match before the walk (dfl2_host_records).
test_device_gzip_level_cpu.py asserts the predicates; test_device_gzip_level_gpu.py compares the device's bytes with the
host build's on the same cases.  ratio_report() writes profiles/r07_deflate_level2_ratio_host_build.txt, coverage_lines()
profiles/deflate2_case_coverage.txt."""
import collections
import ctypes as C
import functools
import gzip
import os
import subprocess
import tempfile
import zlib

import numpy as np

import deflate_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
CH, SUB = DC.CH, DC.SUB
K = 8            # DFL2_K: positions a hash keeps (build_host_encoder checks both against the header's)
HASH_BITS = 11   # DFL2_HASH_BITS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- the host build ----
def build_host_encoder(directory, flags=()):
    """g++ build of tests/deflate2_core_host.cpp in `directory` (flags: -DDFL2_... of the ablation); returns
    encode(data, level=2, fresh=False) -> bytes, checked to gunzip to data.  All calls and both levels share ONE
    Dfl2Shared; fresh=True zeroes it first.  encode.raw skips the checks, encode.records(chunk) is dfl2_host_records,
    encode.last_dynamic_bytes() and encode.last_cl_lengths() read what the last level-2 chunk left."""
    tag = "".join(c for c in "_".join(flags) if c.isalnum() or c == "_")
    so = os.path.join(str(directory), "libdfl2_host%s.so" % tag)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-o", so, os.path.join(HERE, "deflate2_core_host.cpp")])
    L = C.CDLL(so)
    L.dfl2_host_encode.restype = C.c_int64
    L.dfl2_host_encode.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.dfl2_host_last_dynamic_bytes.restype = C.c_int64
    L.dfl2_host_last_cl_lengths.restype = None
    L.dfl2_host_last_cl_lengths.argtypes = [C.c_void_p]
    L.dfl2_host_records.restype = None
    L.dfl2_host_records.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dfl2_host_reset.restype = None
    ch = L.dfl2_host_chunk()
    assert ch == CH
    if not flags:
        assert (L.dfl2_host_k(), L.dfl2_host_hash_bits()) == (K, HASH_BITS)

    def raw(data: bytes, level=2, fresh=False) -> bytes:
        if fresh:
            L.dfl2_host_reset()
        src = np.frombuffer(data, dtype=np.uint8).copy()  # exactly len(data) bytes of its own
        cap = len(data) + 33 * -(-len(data) // ch) + 64
        out = np.zeros(cap, dtype=np.uint8)
        n = L.dfl2_host_encode(level, src.ctypes.data if len(data) else None, len(data), out.ctypes.data, cap)
        if level not in (1, 2):
            assert n == -1
            return None
        assert 0 <= n <= cap - 64
        return out[:n].tobytes()

    def encode(data: bytes, level=2, fresh=False) -> bytes:
        comp = raw(data, level, fresh)
        assert gzip.decompress(comp) == data if data else comp == b""
        assert len(DC.split_members(comp)) == -(-len(data) // ch)
        return comp

    def records(chunk: bytes):
        assert 1 <= len(chunk) <= ch
        src = np.frombuffer(chunk, dtype=np.uint8).copy()
        ln, ds = np.zeros(len(chunk), dtype=np.uint16), np.zeros(len(chunk), dtype=np.uint16)
        L.dfl2_host_records(src.ctypes.data, len(chunk), ln.ctypes.data, ds.ctypes.data)
        return ln.astype(int), ds.astype(int)

    def last_cl_lengths():
        out = np.zeros(19, dtype=np.uint8)
        L.dfl2_host_last_cl_lengths(out.ctypes.data)
        return [int(v) for v in out]

    encode.raw, encode.records, encode.chunk = raw, records, ch
    encode.last_dynamic_bytes = lambda: int(L.dfl2_host_last_dynamic_bytes())
    encode.last_cl_lengths = last_cl_lengths
    return encode


@functools.lru_cache(maxsize=1)
def host_encoder():
    """one host build per process, in a temporary directory of its own"""
    host_encoder.dir = tempfile.TemporaryDirectory(prefix="dfl2_host_")
    return build_host_encoder(host_encoder.dir.name)


# ---- the header of a dynamic block, symbol by symbol ----
def header_anatomy(member: bytes) -> dict:
    """hclen, cl_lengths (19, by symbol) and symbols [(code-length symbol, repeat count or None, index of the first
    length it stands for)] of a member's dynamic block; {} for a stored one"""
    bits = DC._Bits(member[20:-8])
    assert bits.take(1) == 1
    if bits.take(2) != 2:
        return {}
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = bits.take(3)
    assert hclen == 4 or cl[CL_ORDER[hclen - 1]] > 0, "HCLEN is trimmed"
    assert max(cl) <= 7 and DC._kraft(cl) == 1 << 15
    table, lens, syms = DC._decoder(cl), [], []
    while len(lens) < hlit + hdist:
        s = DC._symbol(bits, table)
        at = len(lens)
        if s < 16:
            lens.append(s)
            syms.append((s, None, at))
            continue
        cnt = 3 + bits.take(2) if s == 16 else 3 + bits.take(3) if s == 17 else 11 + bits.take(7)
        lens += [lens[-1] if s == 16 else 0] * cnt
        syms.append((s, cnt, at))
    assert len(lens) == hlit + hdist
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=cl, symbols=syms, lengths=lens, bits=bits.pos)


def runs(lengths):
    """[(value, run length, first index)] of a code-length sequence"""
    out, i = [], 0
    while i < len(lengths):
        j = i
        while j < len(lengths) and lengths[j] == lengths[i]:
            j += 1
        out.append((lengths[i], j - i, i))
        i = j
    return out


def expected_header_symbols(lengths):
    """the run-length coding the issue words: zeros as 18s of at most 138, then a 17 for 3 to 10, then plain; a length
    once plain, then 16s of 3 to 6, then plain"""
    out = []
    for v, run, at in runs(lengths):
        if v == 0:
            while run >= 11:
                c = min(run, 138)
                out.append((18, c, at))
                run, at = run - c, at + c
            if run >= 3:
                out.append((17, run, at))
                run, at = 0, at + run
        else:
            out.append((v, None, at))
            run, at = run - 1, at + 1
            while run >= 3:
                c = min(run, 6)
                out.append((16, c, at))
                run, at = run - c, at + c
        for _ in range(run):
            out.append((v, None, at))
            at += 1
    return out


def tokens_by_position(a):
    """{position: (match length or 0, distance or 0)} of one member's tokens"""
    out, pos = {}, 0
    for t in a["tokens"]:
        if len(t) == 1:
            out[pos] = (0, 0)
            pos += 1
        else:
            assert t[2] == pos
            out[pos] = (t[0], t[1])
            pos += t[0]
    return out


class View:
    """what a predicate sees of a case on the host build"""
    def __init__(self, enc, data, comp):
        self.data = data
        self.members = DC.split_members(comp)
        self.A = [DC.anatomy(m) for m in self.members]
        self.T = [tokens_by_position(a) for a in self.A]
        self.H = [header_anatomy(m) for m in self.members]
        self.rec_len, self.rec_dist = enc.records(data[:CH])  # (leaves the shared state as after these phases)
        self.matches = [(p, l, d) for p, (l, d) in sorted(self.T[0].items()) if l]
        self.dynamic = all(a["btype"] == 2 for a in self.A)
        self.lengths = self.H[0].get("lengths", [])
        self.zero_runs = [r for v, r, _ in runs(self.lengths) if v == 0]
        self.rep_runs = [r for v, r, _ in runs(self.lengths) if v != 0]


def hash2(w4: bytes) -> int:  # dfl2_ph_hash's
    return ((int.from_bytes(w4, "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def _hash_counts(data, lo, hi):
    return collections.Counter(hash2(data[p:p + 4]) for p in range(lo, min(hi, len(data) - 3)))


# ---- texts ----
def filler(n, name):
    """n bytes of 128 .. 255: the plants below are lower-case letters, a filler never matches into one"""
    return DC._rng("fill" + name).integers(128, 256, n, dtype=np.uint8).tobytes()


def _plant(n, name, plants, alone=None):
    """a filler with `plants` [(position, bytes)] in it; `alone`: a 4-gram whose hash no other position may have"""
    d = bytearray(filler(n, name))
    for at, s in plants:
        assert 0 <= at and at + len(s) <= n
        d[at:at + len(s)] = s
    if alone is not None:
        planted = {q for at, s in plants for q in range(at, at + len(s))}
        for p in range(n - 3):
            while bytes(d[p:p + 4]) != alone and hash2(d[p:p + 4]) == hash2(alone):
                q = max(q for q in range(p, p + 4) if q not in planted)
                d[q] = 128 + (d[q] + 1) % 128
    return bytes(d)


def _de_bruijn(k, n):
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def _in_block(d):
    if d == 255:
        return _plant(600, "inb255", [(0, bytes(range(32, 32 + 30))), (255, bytes(range(32, 32 + 30)))])
    unit = b"abcd"[:d]
    return _plant(600, "inb%d" % d, [(300, unit * (40 // d))])


def _in_block_pred(d):
    def pred(x):
        hit = [(p, l, dd) for p, l, dd in x.matches if dd == d and (p - dd) // SUB == p // SUB]
        return x.dynamic and bool(hit) and (d != 255 or hit[0][0] == 255)
    return pred


def _run_across(x):  # one distance-1 match that begins in sub-block 0 and ends in sub-block 1
    return x.dynamic and any(d == 1 and p < SUB < p + l for p, l, d in x.matches)


def _source_last_position(x):
    return x.dynamic and any((p - d) % SUB == SUB - 1 and (p - d) // SUB == p // SUB - 1 for p, l, d in x.matches)


def _lazy_text(at, taken):
    first = b"abcdQ" if taken else b"abcdefghij"
    return _plant(1200, "lazy%d%d" % (at, taken), [(10, first), (30, b"bcdefghijR"), (at, b"abcdefghij")])


def _lazy_taken_at(at):
    def pred(x):
        return (x.dynamic and x.rec_len[at] == 4 and x.rec_len[at + 1] == 9 and x.T[0].get(at) == (0, 0)
                and x.T[0].get(at + 1, (0, 0))[0] == 9)
    return pred


def _lazy_refused_at(at):
    def pred(x):
        return x.dynamic and x.rec_len[at] == 10 and 0 < x.rec_len[at + 1] <= 10 and x.T[0].get(at) == (10, at - 10)
    return pred


def _lazy_end_text(taken):
    n = 700
    if taken:  # "abcd" (4, from the first plant) at n - 6 gives way to "bcdef" (5, clamped by the end) at n - 5
        return _plant(n, "lazyend1", [(10, b"abcdQ"), (30, b"bcdefR"), (n - 6, b"abcdef")])
    return _plant(n, "lazyend0", [(10, b"abcdQ"), (n - 4, b"abcd")])  # no record behind n - 4: the match stands


def _lazy_end(taken):
    def pred(x):
        n = len(x.data)
        if taken:
            return x.dynamic and x.rec_len[n - 6] == 4 and x.T[0].get(n - 6) == (0, 0) and x.T[0].get(n - 5) == (5, n - 5 - 30)
        return x.dynamic and x.T[0].get(n - 4) == (4, n - 4 - 10) and not any(x.rec_len[n - 3:])
    return pred


def _lazy_258_text():
    z = DC._rng("z258").integers(0, 64, 300, dtype=np.uint8).tobytes()
    return _plant(1500, "lazy258", [(10, b"abcdQ"), (100, b"bcd" + z), (800, b"abcd" + z)])


def _lazy_258(x):
    return x.dynamic and x.rec_len[800] == 4 and x.T[0].get(800) == (0, 0) and x.T[0].get(801) == (258, 701)


def _period4(x):
    per_block = max(_hash_counts(x.data, 0, SUB).values())
    return x.dynamic and per_block == 64 > K and x.matches and all(d == 4 for _, _, d in x.matches) and x.matches[0][0] == 4


def _spread_text(shorts_after, name):
    """"abcdEFGHIJKL" in sub-block 1, then `shorts_after` sub-blocks with one "abcd" + another byte each, then the
    long text again: its hash's bucket keeps K positions"""
    plants = [(SUB + 40, b"abcdEFGHIJKL")]
    for i in range(shorts_after):
        plants.append((SUB * (2 + i) + 40, b"abcd" + bytes([48 + i])))
    plants.append((SUB * (2 + shorts_after) + 40, b"abcdEFGHIJKL"))
    return _plant(SUB * (3 + shorts_after), name, plants, alone=b"abcd")


def _spread(shorts_after, kept):
    def pred(x):
        q = SUB * (2 + shorts_after) + 40
        h = hash2(b"abcd")
        same = [p for p in range(q) if hash2(x.data[p:p + 4]) == h]
        if len({p // SUB for p in same}) != len(same) or len(same) != 1 + shorts_after:
            return False  # one position of the hash per sub-block
        if kept:  # the long plant is the oldest of the K kept
            return len(same) == K and (x.rec_len[q], x.rec_dist[q]) == (12, q - same[0]) and x.T[0].get(q) == (12, q - same[0])
        return len(same) == K + 1 and (x.rec_len[q], x.rec_dist[q]) == (4, q - same[-1])  # evicted: the nearest short one
    return pred


def _more_than_k_spread(x):
    h = hash2(b"abcd")
    same = [p for p in range(len(x.data) - 3) if hash2(x.data[p:p + 4]) == h]
    return x.dynamic and len(same) > K + 2 and len({p // SUB for p in same}) == len(same)


@functools.lru_cache(maxsize=1)
def _colliding_grams():
    seen = {}
    for a in range(97, 123):
        for b in range(97, 123):
            g = bytes([a, b, 113, 122])
            h = hash2(g)
            if h in seen:
                return seen[h], g
            seen[h] = g
    raise AssertionError("no two of 676 four-grams share one of 2 048 hashes")


def _collision_text():
    g1, g2 = _colliding_grams()
    return _plant(SUB * 5, "collide", [(40, g1 + b"WXYZ"), (2 * SUB + 40, g2 + b"WXYZ"), (4 * SUB + 40, g1 + b"WXYZ")])


def _collision(x):
    g1, g2 = _colliding_grams()
    q2, q = 2 * SUB + 40, 4 * SUB + 40
    return (g1 != g2 and hash2(g1) == hash2(g2) and x.rec_len[q2] == 0  # the bucket held g1's position: other bytes
            and x.T[0].get(q) == (8, q - 40))                            # g2's is nearer and skipped


def _gaps_text(values, name, n=900):
    return DC._rng(name).choice(np.array(values, dtype=np.uint8), n).tobytes()


def _zero_run(r, want):
    def pred(x):
        if not x.dynamic or r not in x.zero_runs:
            return False
        got = [[(s, c) for s, c, a in x.H[0]["symbols"] if at <= a < at + run] for v, run, at in runs(x.lengths) if v == 0 and run == r]
        return want in got
    return pred


def _repeat_text():
    """three byte values at 1/8 each, six at 1/16, seven at 1/32 and a rest: code lengths 3, 4 and 5 in runs of 3, 6, 7"""
    parts = []
    for first, k, count in ((10, 3, 400), (20, 6, 200), (30, 7, 100)):
        parts += [np.full(count, first + i, dtype=np.uint8) for i in range(k)]
    parts.append(np.repeat(np.arange(200, 210, dtype=np.uint8), 5))
    return np.random.default_rng(8).permutation(np.concatenate(parts)).tobytes()  # (the first seed whose matches leave the runs whole)


def _repeat_runs(x):
    if not x.dynamic:
        return False
    by_at = {at: (v, run) for v, run, at in runs(x.lengths)}
    if not (by_at.get(10, (0, 0))[1] == 3 and by_at.get(20, (0, 0))[1] == 6 and by_at.get(30, (0, 0))[1] == 7):
        return False
    sym = {a: (s, c) for s, c, a in x.H[0]["symbols"]}
    v3 = (by_at[10][0], None)
    return (sym.get(10) == sym.get(11) == sym.get(12) == v3     # 3: the length three times, 1 + 2 makes no 16
            and sym.get(21) == (16, 5) and 22 not in sym        # 6: the length, 16 x 5
            and sym.get(31) == (16, 6) and 32 not in sym)       # 7: the length, 16 x 6


def _border_text():
    """25 rounds of ten fresh letters: a^29, (bc)^15, (def)^10 + d, (ghij)^8: one match of 28 each at distances 1 .. 4.
    One length symbol with more than a quarter of the tokens and four distance symbols of equal counts: 2 bits each"""
    out = bytearray()
    for r in range(25):
        a = [bytes([r * 10 + i]) for i in range(10)]
        out += a[0] * 29 + (a[1] + a[2]) * 15 + (a[3] + a[4] + a[5]) * 10 + a[3] + (a[6] + a[7] + a[8] + a[9]) * 8
    return bytes(out)


def _border_run(x):
    if not x.dynamic:
        return False
    h = x.H[0]
    # one 16 stands for the first distance length: what it repeats is a literal/length symbol's length
    return any(s == 16 and a <= h["hlit"] < a + c for s, c, a in h["symbols"]) and x.lengths[h["hlit"] - 1] == x.lengths[h["hlit"]]


def _deep_cl_text(seed):
    """byte values with probabilities 2^-L, few of the short lengths and many of length 10, values shuffled: the header's
    code-length symbols 2 .. 10 come in Fibonacci-like counts"""
    rng = np.random.default_rng(seed)
    n_of = {2: 1, 3: 1, 4: 2, 5: 3, 6: 5, 7: 8, 8: 13, 9: 21, 10: 178}
    values = rng.permutation(256)[:sum(n_of.values())]
    parts, i = [], 0
    for L, k in n_of.items():
        for _ in range(k):
            parts.append(np.full(8192 >> L, values[i], dtype=np.uint8))
            i += 1
    return rng.permutation(np.concatenate(parts)).tobytes()


def _deep_cl(x):
    if not x.dynamic:
        return False
    hist = collections.Counter(s for s, _, _ in x.H[0]["symbols"])
    return DC._huffman_depth(hist.values()) > 7 and max(x.H[0]["cl_lengths"]) == 7


def _no_distance_code(x):
    return DC._all_literals_no_distance_code(x.A) and len(x.data) > 4 and not any(x.rec_len)


def _single_distance(x):
    return DC._one_distance_symbol(x.A) and all(d == 2 for _, _, d in x.matches)


class Case:
    def __init__(self, name, data, pred, why):
        self.name, self.data, self.pred, self.why = name, data, pred, why
        self.tries = None

    def __repr__(self):
        return self.name


def _plain_cases():
    out = []
    for n in (1, 3, 4, 5, 255, 256, 257, 511, 512, 513, CH - 1, CH):
        out.append(Case("len_%d" % n, DC.text(n, "l2text%d" % n), lambda x: len(x.A) == 1, "random text over 21 letters"))
    for d in (1, 2, 3, 4, 255):
        out.append(Case("in_block_%d" % d, _in_block(d), _in_block_pred(d), "a source in the match's own sub-block at distance %d" % d))
    out.append(Case("run_across_sub_blocks", _plant(600, "runx", [(200, b"G" * 300)]), _run_across, "a distance-1 run over the boundary at 256"))
    out.append(Case("source_last_position", _plant(700, "srclast", [(255, b"abcdefgh"), (300, b"abcdefgh")]), _source_last_position,
                    "the source is position 255 of the previous sub-block"))
    for at in (255, 511):
        out.append(Case("lazy_taken_%d" % at, _lazy_text(at, True), _lazy_taken_at(at), "4 at the sub-block's last position gives way to 9 behind it"))
        out.append(Case("lazy_refused_%d" % at, _lazy_text(at, False), _lazy_refused_at(at), "10 at the sub-block's last position stands against 9"))
    out.append(Case("lazy_taken_at_end", _lazy_end_text(True), _lazy_end(True), "a lazy step into the chunk's last five positions"))
    out.append(Case("lazy_none_at_end", _lazy_end_text(False), _lazy_end(False), "a match of 4 ends the chunk: nothing behind it to wait for"))
    out.append(Case("lazy_then_258", _lazy_258_text(), _lazy_258, "a lazy literal, then a match of 258"))
    out.append(Case("period_4", b"abcd" * 256, _period4, "64 positions of one hash in every sub-block"))
    out.append(Case("hash_spread", _spread_text(K + 3, "spread"), _more_than_k_spread, "more than K positions of one hash, one a sub-block"))
    out.append(Case("oldest_kept", _spread_text(K - 1, "kept"), _spread(K - 1, True), "the best candidate is the oldest of the K kept"))
    out.append(Case("just_evicted", _spread_text(K, "evicted"), _spread(K, False), "the best candidate was the one just evicted"))
    out.append(Case("hash_collision", _collision_text(), _collision, "equal hashes, different four bytes"))
    a = [1, 4, 8, 19, 31, 170]  # gaps of 2, 3, 10, 11 and 138 unused literals between them
    out.append(Case("zeros_2", _gaps_text(a, "gaps_a"), _zero_run(2, [(0, None), (0, None)]), "two zeros: no run symbol"))
    out.append(Case("zeros_3", _gaps_text(a, "gaps_a"), _zero_run(3, [(17, 3)]), "three zeros: 17"))
    out.append(Case("zeros_10", _gaps_text(a, "gaps_a"), _zero_run(10, [(17, 10)]), "ten zeros: still 17"))
    out.append(Case("zeros_11", _gaps_text(a, "gaps_a"), _zero_run(11, [(18, 11)]), "eleven zeros: 18"))
    out.append(Case("zeros_138", _gaps_text(a, "gaps_a"), _zero_run(138, [(18, 138)]), "138 zeros: one 18"))
    out.append(Case("zeros_139", _gaps_text([5, 145], "gaps_b"), _zero_run(139, [(18, 138), (0, None)]), "139 zeros: 18 and a plain zero"))
    out.append(Case("repeats_3_6_7", _repeat_text(), _repeat_runs, "runs of 3, 6 and 7 of a non-zero length"))
    out.append(Case("run_over_border", _border_text(), _border_run, "one 16 repeats the last literal/length length into the distance lengths"))
    out.append(Case("deep_code_length_code", _deep_cl_text(DEEP_CL_SEED), _deep_cl, "the code-length code is limited to 7 bits"))
    out.append(Case("no_distance_code", bytes(b"ACGT"[i] for i in _de_bruijn(4, 4)) + b"AAA", _no_distance_code, "every 4-gram once: literals only"))
    out.append(Case("single_distance_code", b"ab" * 258, _single_distance, "distance 2 only: one 1-bit distance code"))
    out.append(Case("random_stored", DC._rng("l2random").integers(0, 256, CH, dtype=np.uint8).tobytes(), lambda x: DC._stored(x.A),
                    "random bytes of a whole chunk: stored"))
    return out


DEEP_CL_SEED = 4  # the first seed whose matches leave the code-length symbols' counts that steep


# ---- the stored / dynamic boundary at level 2 ----
class _Level2:
    """what deflate_cases' boundary search asks of an encoder"""
    def __init__(self, enc):
        self.raw = lambda data, fresh=False: enc.raw(data, 2, fresh)
        self.last_dynamic_bytes = enc.last_dynamic_bytes


def _boundary_cases(enc):
    out = []
    for tag, want, dynamic, why in (("a", 4, True, "dynamic bytes n + 4: the first text one byte smaller than stored"),
                                    ("b", 5, False, "dynamic bytes n + 5: stored")):
        name = "l2_boundary_" + tag
        data, tries = DC._search_small(_Level2(enc), want, name)
        c = Case(name, data, (lambda x: x.dynamic) if dynamic else (lambda x: DC._stored(x.A)), why)
        c.tries, c.dynamic_bytes = tries, want + len(data)
        out.append(c)
    return out


CASES = _plain_cases() + _boundary_cases(host_encoder())
assert len({c.name for c in CASES}) == len(CASES)


# ---- ratio ----
def fastq_varied(records, seed=20):
    """the text of test_host_encoder_beats_huffman_only_on_fastq"""
    rng = np.random.default_rng(seed)
    qsym = np.frombuffer(b"F:,#FFFF::0123456789-", dtype=np.uint8)[:16]
    p = np.array([40, 15, 8, 2, 6, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1], dtype=np.float64)
    out = []
    for _ in range(records):
        x, y = rng.integers(1000, 32000, 2)
        out.append(b"@A00123:45:HXXXXXXX:1:1101:%d:%d 1:N:0:ACGT\n" % (x, y))
        out.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150).tobytes() + b"\n+\n")
        out.append(rng.choice(qsym, 150, p=p / p.sum()).tobytes() + b"\n")
    return b"".join(out)


def fastq_constant(records, seed=21):
    """@read%09d, random bases, constant quality"""
    bases = np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), (records, 150))
    return b"".join(b"@read%09d\n" % i + bases[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(records))


def zlib_per_chunk(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """bytes of `text` when every chunk is a raw deflate stream of its own plus 28 bytes of framing"""
    total = 0
    for o in range(0, len(text), CH):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        total += len(z.compress(text[o:o + CH]) + z.flush()) + 28
    return total


ABLATION = (("level 1", None),
            ("in-block alone", ("-DDFL2_K=1", "-DDFL2_INBLOCK=1", "-DDFL2_LAZY=0", "-DDFL2_RLE=0")),
            ("buckets of 8 alone", ("-DDFL2_K=8", "-DDFL2_INBLOCK=0", "-DDFL2_LAZY=0", "-DDFL2_RLE=0")),
            ("lazy alone", ("-DDFL2_K=1", "-DDFL2_INBLOCK=0", "-DDFL2_LAZY=1", "-DDFL2_RLE=0")),
            ("header runs alone", ("-DDFL2_K=1", "-DDFL2_INBLOCK=0", "-DDFL2_LAZY=0", "-DDFL2_RLE=1")),
            ("none of the four (one 14-bit hash slot)", ("-DDFL2_K=1", "-DDFL2_INBLOCK=0", "-DDFL2_LAZY=0", "-DDFL2_RLE=0")),
            ("all four, buckets of 2", ("-DDFL2_K=2",)),
            ("all four, buckets of 4", ("-DDFL2_K=4",)),
            ("all four, buckets of 8: level 2", ()))


def ratio_report(records=300000):
    """the lines of profiles/r07_deflate_level2_ratio_host_build.txt: host build, per-chunk zlib levels, the ablation"""
    lines = ["# compression ratio of the device DEFLATE encoder's two levels built as plain C++ (tests/deflate2_core_host.cpp) against zlib run",
             "# chunk by chunk (32 KiB, raw deflate, memLevel 9, + 28 bytes of framing a chunk); %d records a text; every output gunzipped" % records,
             "# back to its input.  Ablation: csrc/bdx_deflate2_core.h built with its DFL2_* switches (a bucket table always takes 32 KiB:",
             "# 16 384 / K hashes)."]
    with tempfile.TemporaryDirectory(prefix="dfl2_ratio_") as d:
        encs = [(name, build_host_encoder(d, flags) if flags is not None else None) for name, flags in ABLATION]
        for tname, text in (("varied_quality", fastq_varied(records)), ("constant_quality", fastq_constant(records))):
            lines.append("%s: %d B" % (tname, len(text)))
            for name, enc in encs:
                comp = encs[-1][1].raw(text, 1) if enc is None else enc.raw(text, 2)
                assert gzip.decompress(comp) == text
                lines.append("  %-42s %10d B = %.3fx" % (name, len(comp), len(text) / len(comp)))
            lines.append("  %-42s %10d B = %.3fx" % ("zlib Huffman-only", zlib_per_chunk(text, 6, zlib.Z_HUFFMAN_ONLY),
                                                     len(text) / zlib_per_chunk(text, 6, zlib.Z_HUFFMAN_ONLY)))
            for level in range(1, 10):
                z = zlib_per_chunk(text, level)
                lines.append("  %-42s %10d B = %.3fx" % ("zlib level %d" % level, z, len(text) / z))
    return lines


def coverage_lines(enc=None):
    """one line per case (host build: needs no GPU)"""
    enc = enc or host_encoder()
    lines = []
    for c in CASES:
        comp = enc(c.data, fresh=True)
        x = View(enc, c.data, comp)
        m = x.matches
        lines.append("%-24s n %6d  %-7s bytes %6d  tokens %6d  max distance %6d  max length %4d  header symbols %3d  HCLEN %2d%s" % (
            c.name, len(c.data), "dynamic" if x.dynamic else "stored", len(comp), len(x.A[0]["tokens"]), max([d for _, _, d in m], default=0),
            max([l for _, l, _ in m], default=0), len(x.H[0].get("symbols", [])), x.H[0].get("hclen", 0),
            "  search: %d host encodes" % c.tries if c.tries else ""))
    return lines


if __name__ == "__main__":
    import sys

    print("\n".join(ratio_report(int(sys.argv[2])) if len(sys.argv) > 2 and sys.argv[1] == "ratio" else coverage_lines()))
