"""Cases for the device FASTQ pipeline (csrc/bdx_fastq.hip: index, pack, stable radix partition, gather), shared by its CPU
and GPU tests.  The kernels' geometry is parsed from the source, so a retune moves the cases with it; the references are
plain Python / numpy written from the contract in include/biodemux_hip.h; every named text and every gather case carries
a predicate (`ok`), computed from the constants and the case itself, that proves it reaches the edge it is named for.
tests/test_device_io_cases_cpu.py asserts the predicates and holds the references to the host library;
tests/test_device_fastq_edges_gpu.py holds the device to the references."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(ROOT, "biodemux.jl_amd", "csrc", "bdx_fastq.hip")
COVERAGE = os.path.join(ROOT, "profiles", "fastq_case_coverage.txt")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NL, CR = 10, 13


# ---- geometry, from the text of the kernels ----
def parse_constants(path=SOURCE):
    """every `constexpr <type> FQ_X = <expression of integers and earlier FQ_ names>;` of the source, evaluated"""
    vals = {}
    for name, expr in re.findall(r"constexpr\s+\w+\s+(FQ_\w+)\s*=\s*([^;]+);", open(path).read()):
        e = re.sub(r"\(\s*\w+_t\s*\)", "", expr).replace("/", "//")
        assert re.fullmatch(r"[\w\s*+\-/()]+", e), (name, expr)
        vals[name] = int(eval(e, {"__builtins__": {}}, dict(vals)))  # noqa: S307 - digits, FQ_ names and arithmetic only
    return vals


_C = parse_constants()
_NEEDED = ("FQ_THREADS", "FQ_LANE_BYTES", "FQ_STEPS", "FQ_TILE", "FQ_SCAN_BLOCK")
assert all(k in _C for k in _NEEDED), "constants of bdx_fastq.hip not found: %s" % [k for k in _NEEDED if k not in _C]
FQ_THREADS, FQ_LANE_BYTES, FQ_STEPS, FQ_TILE, FQ_SCAN_BLOCK = (_C[k] for k in _NEEDED)
FQ_WAVE_BYTES = 64 * FQ_LANE_BYTES           # text one wavefront looks at per step
FQ_STEP_BYTES = FQ_THREADS * FQ_LANE_BYTES   # text one workgroup looks at per step
EDGES = (FQ_LANE_BYTES, FQ_WAVE_BYTES, FQ_STEP_BYTES, FQ_TILE)  # lane, wave, step, tile
NEAR_MISSES = (0x0B, 0x09, 0x8A, 0x1A, 0x2A, 0x00, 0xFF)        # one bit, or the top bit, away from '\n' (0x0A), and the extremes


def tiles(text_len):
    return -(-text_len // FQ_TILE)


def scan_partials(items):
    """workgroup partials of the generic scan over `items` items; above FQ_SCAN_BLOCK of them the one-workgroup scan of
    the partials loops with a carry"""
    return -(-items // FQ_SCAN_BLOCK)


def hist_items(n):
    """items of the digit histogram scan of a partition of n records: 256 digits x tiles of FQ_THREADS records"""
    return 256 * -(-n // FQ_THREADS)


def radix_passes(n_classes):
    """8-bit passes of the partition: the bytes of n_classes - 1 that can be non-zero"""
    p, v = 0, n_classes - 1
    while v:
        p, v = p + 1, v >> 8
    return p


# ---- references (include/biodemux_hip.h: bdx_fq_index_device, bdx_fq_pack_device, bdx_fq_gather_device) ----
def _u8(text):
    return text if isinstance(text, np.ndarray) else np.frombuffer(text, dtype=np.uint8)


def ref_index(text, final, max_reads):
    """-> (n_records, next, off int64[4 * n_records], len int32[4 * n_records])"""
    t = _u8(text)
    size, want = len(t), 4 * max_reads
    if size == 0 or max_reads <= 0:
        return 0, 0, np.zeros(0, np.int64), np.zeros(0, np.int32)
    nl = np.flatnonzero(t == NL)
    k = min(len(nl), want)
    if not final:
        k -= k % 4  # more text follows: complete records only
    ends = nl[:k].astype(np.int64)
    starts = np.concatenate([np.zeros(1, np.int64), ends[:-1] + 1])[:k]
    lens = ends - starts
    lens -= (lens > 0) & (t[np.maximum(ends - 1, 0)] == CR)  # a "\r" before the "\n" is no part of the line
    nxt = int(ends[-1]) + 1 if k else 0
    more_off, more_len = [], []
    if final and k < want and nxt < size:  # an unterminated last line counts
        more_off.append(nxt)
        more_len.append(size - nxt - (1 if t[size - 1] == CR else 0))
        nxt = size
    nrec = (k + len(more_off) + 3) // 4
    while k + len(more_off) < 4 * nrec:  # a truncated last record: empty lines at the end of the text
        more_off.append(size)
        more_len.append(0)
    off = np.concatenate([starts, np.array(more_off, dtype=np.int64)])
    return nrec, nxt, off, np.concatenate([lens, np.array(more_len, dtype=np.int64)]).astype(np.int32)


def _segments(t, starts, lens):
    """the bytes t[starts[k], +lens[k]) of every k, one after the other"""
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.uint8)
    before = np.cumsum(lens) - lens
    return t[np.repeat(starts - before, lens) + np.arange(total, dtype=np.int64)]


def ref_pack(text, off, ln, n):
    """-> (seq uint8[sum of the sequence lengths], seq_off int64[n + 1])"""
    t = _u8(text)
    sl = np.asarray(ln[1:4 * n:4], dtype=np.int64)
    seq_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(sl)]).astype(np.int64)
    return _segments(t, np.asarray(off[1:4 * n:4]), sl), seq_off


def ref_classes(bc1, bc2, stride, n_classes):
    """class of every record: 0 unknown (bc1 == 0), 1 ambiguous (bc1 < 0), else 2 + (bc1 - 1) * stride + (max(bc2, 1) - 1);
    ValueError when one lies outside [0, n_classes).  Python ints; beyond 2^16 records int64, in which the product of two
    int32 values (below 2^62) and the two small terms are exact as well."""
    n = len(bc1)
    if n <= 1 << 16:
        cls = [0 if a == 0 else 1 if a < 0 else 2 + (a - 1) * int(stride) + (max(b, 1) - 1)
               for a, b in zip(np.asarray(bc1).tolist(), np.asarray(bc2).tolist())]
        bad = [i for i, c in enumerate(cls) if not 0 <= c < n_classes]
        if bad:
            raise ValueError("record %d: class %d outside [0, %d)" % (bad[0], cls[bad[0]], n_classes))
        return np.array(cls, dtype=np.int64)
    a, b = np.asarray(bc1, dtype=np.int64), np.asarray(bc2, dtype=np.int64)
    cls = np.where(a == 0, 0, np.where(a < 0, 1, 2 + (a - 1) * int(stride) + (np.maximum(b, 1) - 1)))
    if ((cls < 0) | (cls >= n_classes)).any():
        raise ValueError("a class outside [0, %d)" % n_classes)
    return cls


def ref_slices(ln, n, keep_start, keep_end, trim):
    """per record: first kept base a (1-based), bytes of the sequence and of the quality line that are written"""
    sl = np.asarray(ln[1:4 * n:4], dtype=np.int64)
    ql = np.asarray(ln[3:4 * n:4], dtype=np.int64)
    a = np.ones(n, np.int64)
    if trim and keep_start is not None:
        ks, ke = np.asarray(keep_start, dtype=np.int64)[:n], np.asarray(keep_end, dtype=np.int64)[:n]
        cut = ks != -1
        ca = np.maximum(ks, 1)
        cb = np.minimum(ke, sl)            # last kept base, 1-based inclusive
        cq = np.minimum(cb, ql)            # the quality line: the same range, clamped to its own length
        a = np.where(cut, ca, a)
        sl = np.where(cut, np.where(ca > cb, 0, cb - ca + 1), sl)
        ql = np.where(cut, np.where((ca > cb) | (ca > cq), 0, cq - ca + 1), ql)
    return a, sl, ql


def ref_gather(text, off, ln, bc1, bc2, stride, n_classes, keep_start, keep_end, trim):
    """-> (the blocks of all classes back to back in class order, as uint8; class_bytes int64[n_classes]).  Inside a class
    the records keep their input order: a stable sort by class."""
    t = np.concatenate([_u8(text), np.array([NL], np.uint8)])  # (the extra byte: the "\n" every written line ends with)
    nlp = len(t) - 1
    n = len(bc1)
    off, ln = np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64)
    cls = ref_classes(bc1, bc2, stride, n_classes)
    a, sl, ql = ref_slices(ln, n, keep_start, keep_end, trim)
    hl, pl = ln[0:4 * n:4], ln[2:4 * n:4]
    one, nls = np.ones(n, np.int64), np.full(n, nlp, np.int64)
    order = np.argsort(cls, kind="stable")
    starts = np.stack([off[0:4 * n:4], nls, off[1:4 * n:4] + a - 1, nls, off[2:4 * n:4], nls, off[3:4 * n:4] + a - 1, nls], axis=1)
    lens = np.stack([hl, one, sl, one, pl, one, ql, one], axis=1)
    out = _segments(t, starts[order].ravel(), lens[order].ravel())
    class_bytes = np.bincount(cls, weights=hl + sl + pl + ql + 4, minlength=n_classes).astype(np.int64)  # (exact below 2^53)
    return out, class_bytes


def ref_record(text, off, ln, i, keep_start, keep_end, trim):
    """record i as it is written, by plain slicing (1-based inclusive): the check of the vectorised reference above"""
    line = [bytes(text[int(off[4 * i + k]):int(off[4 * i + k]) + int(ln[4 * i + k])]) for k in range(4)]
    if trim and keep_start is not None and int(keep_start[i]) != -1:
        a, b = max(int(keep_start[i]), 1), min(int(keep_end[i]), len(line[1]))
        line[1], line[3] = (line[1][a - 1:b], line[3][a - 1:b]) if a <= b else (b"", b"")
    return b"\n".join(line) + b"\n"


# ---- named index texts ----
IndexText = namedtuple("IndexText", "name text edge ok")
_RECORD = b"@r\nACGTA\n+\nIIIII\n"  # 17 bytes: its newlines drift against every power of two


def filler(n, start=0):
    reps = (start + n) // len(_RECORD) + 1
    return (_RECORD * reps)[start:start + n]


def _nl_set(text):
    return set(np.flatnonzero(_u8(text) == NL).tolist())


def _with_newlines_at(n, positions, base=None):
    t = bytearray(base if base is not None else (b"ACGT" * (n // 4 + 1))[:n])
    for p in positions:
        t[p] = NL
    return bytes(t)


def fixed_records(n, width=64):
    """n records of exactly `width` bytes: "@" + 8 digits, sequence and quality of (width - 14) / 2 bytes"""
    s = (width - 14) // 2
    assert 14 + 2 * s == width
    rng = np.random.default_rng(width)
    return b"".join(b"@%08d\n" % i + rng.choice(np.frombuffer(b"ACGT", np.uint8), s).tobytes() + b"\n+\n" + b"F" * s + b"\n"
                    for i in range(n))


@functools.lru_cache(maxsize=None)
def index_texts():
    out = []

    def add(name, text, edge, ok):
        out.append(IndexText(name, text, edge, bool(ok)))

    for B in EDGES:
        pos = [k * B - 1 for k in (1, 2, 3)] + [k * B for k in (1, 2, 3)]
        text = _with_newlines_at(3 * B + 5, pos + [7, 3 * B + 3])
        add("newlines_around_%d" % B, text, "newlines at k*%d-1 and k*%d, k = 1..3" % (B, B),
            set(pos) <= _nl_set(text) and len(text) > 3 * B and all(text[p + 1] != NL for p in pos if p % B == 0))
    L = FQ_LANE_BYTES
    text = b"ACGT" * L + b"\n" * L + b"ACGT\n+\nIIII\n"
    add("lane_of_newlines", text, "one lane's %d bytes all newlines" % L,
        (4 * L) % L == 0 and text[4 * L:5 * L] == b"\n" * L and text[4 * L - 1] != NL and text[5 * L] != NL)
    text = (b"ACGT" * FQ_TILE)[:3 * FQ_TILE - 7]
    add("no_newline_3_tiles", text, "no newline in a text of 3 tiles", NL not in text and tiles(len(text)) == 3)
    lengths = [1, 15, 16, 17] + [B + d for B in EDGES for d in (-1, 0, 1)] + [2 * FQ_TILE]
    for n in sorted(set(lengths)):
        text = filler(n)
        text = text[:-1] + b"A" if text[-1] == NL else text
        add("length_%d" % n, text, "text of %d bytes, last line open" % n, len(text) == n and text[-1] != NL)
        text = filler(n - 1) + b"\n"
        add("length_%d_closed" % n, text, "text of %d bytes that ends in a newline" % n, len(text) == n and text[-1] == NL)
    for m in NEAR_MISSES:
        t = bytearray(b"A" * 128)
        ps = [16 * (j + 1) + j for j in range(4)]  # byte lane j of a 32-bit word
        for p in ps:
            t[p - 1], t[p], t[p + 1] = m, NL, m
        t[96:100] = bytes([m]) * 4   # a word of near misses only
        t[100:104] = bytes([m, NL, NL, m])
        text = bytes(t)
        add("near_miss_%02x" % m, text, "0x%02X before and after a newline in all four byte lanes of a word" % m,
            [p % 4 for p in ps] == [0, 1, 2, 3] and all(text[p - 1] == m == text[p + 1] and text[p] == NL for p in ps)
            and len(_nl_set(text)) == 6 and m != NL and len(text) >= 2 * FQ_LANE_BYTES)
    text = b"\r\n" + filler(200)
    add("crlf_first_line", text, "\"\\r\\n\" as the first line", text[:2] == b"\r\n")
    text = b"@a\r\n\nACGT\r\n\n@b\nAC\r\n\n+\n\n" + filler(100)
    add("cr_then_empty_line", text, "a \"\\r\" ends the previous line, an empty line follows", b"\r\n\n" in text)
    text = filler(17 * 6) + b"@x\nAC\n+\n\r"
    add("last_line_single_cr", text, "the last line is one \"\\r\" without a newline", text.endswith(b"\n\r"))
    per = FQ_TILE // 64
    text = fixed_records(4 * per + 10)
    caps = caps_for(text)
    add("cap_tiles", text, "64-byte records over 5 tiles: caps 1, inside tile 0, at the end of a tile, inside tile 2, beyond",
        FQ_TILE % 64 == 0 and tiles(len(text)) == 5 and text[FQ_TILE - 1] == NL
        and set(caps) == {"one", "inside_tile0", "tile_end", "inside_tile2", "beyond"} and 4 * caps["tile_end"] == 4 * per)
    assert len({t.name for t in out}) == len(out)
    return tuple(out)


def caps_for(text):
    """max_reads values for a text, by what they reach: {label: cap}.  A label is left out where the text has no such cap."""
    nl = np.flatnonzero(_u8(text) == NL)
    nt = tiles(len(text))
    cum = [int(np.searchsorted(nl, (k + 1) * FQ_TILE)) for k in range(nt)]  # newlines up to the end of tile k
    caps = {"one": 1, "beyond": len(nl) // 4 + 7}
    if nt and cum[0] >= 8:
        caps["inside_tile0"] = cum[0] // 8
    for k in range(nt - 1):  # the cap's last line ends tile k and later tiles hold more: they have nothing to scatter
        if cum[k] and cum[k] % 4 == 0 and (cum[k] > (cum[k - 1] if k else 0)) and cum[k] < len(nl):
            caps["tile_end"] = cum[k] // 4
            break
    if nt >= 3 and cum[2] - cum[1] >= 8:
        caps["inside_tile2"] = (cum[1] + (cum[2] - cum[1]) // 2) // 4 + 1
        assert cum[1] < 4 * caps["inside_tile2"] < cum[2]
    return caps


# ---- gather cases ----
GatherCase = namedtuple("GatherCase", "name text off len n bc1 bc2 keep_start keep_end stride n_classes trim edge ok")
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
PATTERNS = ("one_class", "two_alternating", "own_class", "descending", "middle_byte", "top_byte")
CLASS_COUNTS = {2: (1, 1), 256: (2, 1), 257: (5, 2), 65536: (2, 2), 65537: (255, 3), 90002: (300, 3)}  # n_classes: (stride, passes)


def table_of(records, crlf=False, tail=b""):
    """FASTQ text of (header, sequence, plus, quality) lines and its line table"""
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(h + nl + s + nl + p + nl + q + nl for h, s, p, q in records) + tail
    n, nxt, off, ln = ref_index(text, 1, len(records) + 1)
    assert n == len(records) + (1 if tail else 0) and nxt == len(text)
    return text, n, off, ln


def plain_records(n, seed):
    rng = np.random.default_rng(seed)
    acgt, q = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"#,:FI", np.uint8)
    out = []
    for i in range(n):
        k = int(rng.integers(0, 13))
        out.append((b"@%d" % i, rng.choice(acgt, k).tobytes(), b"+", rng.choice(q, k).tobytes()))
    return out


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _keeps(n, seed):
    rng = np.random.default_rng(seed)
    ks = rng.integers(-1, 6, n)
    ke = rng.integers(-1, 14, n)
    ke[ks == -1] = -1
    return _i32(ks), _i32(ke)


def pattern(name, n):
    """-> (bc1, bc2, stride, n_classes, edge, predicate over the classes)"""
    i = np.arange(n)
    z = np.zeros(n, np.int64)
    many = n > 1
    if name == "one_class":
        return z + 3, z, 1, 7, "all records in class 4", lambda c: len(set(c)) == 1
    if name == "two_alternating":
        return z + 2, 1 + 2 * (i % 2), 3, 14, "classes 5 and 7 alternating", lambda c: set(c) == ({5, 7} if many else {5}) and all(c[1:] != c[:-1])
    if name == "own_class":
        return i + 1, z, 1, n + 2, "every record in a class of its own, ascending", lambda c: len(set(c)) == n and all(np.diff(c) > 0)
    if name == "descending":
        return n - i, z, 1, n + 2, "classes strictly descending", lambda c: all(np.diff(c) < 0)
    if name == "middle_byte":
        return 256 * ((i * 5) % 7) + 4, z, 1, 2048, "classes differ in the middle byte only", \
            lambda c: len(set(c & 0xFF)) == 1 and not (c >> 16).any() and len(set(c >> 8)) == min(n, 7) and radix_passes(2048) == 2
    if name == "top_byte":
        return 9 + 65536 * (((i * 7) // 3) % 2), z, 1, 65548, "classes c and c + 65536", \
            lambda c: len(set(c & 0xFFFF)) == 1 and set(c >> 16) == ({0, 1} if many else {0}) and radix_passes(65548) == 3
    raise KeyError(name)


def _case(name, text, n, off, ln, bc1, bc2, ks, ke, stride, n_classes, trim, edge, ok):
    return GatherCase(name, text, off, ln, n, _i32(bc1), _i32(bc2), None if ks is None else _i32(ks), None if ke is None else _i32(ke),
                      int(stride), int(n_classes), int(trim), edge, bool(ok))


def _bc_of_class(c, stride, i):
    """a (bc1, bc2) pair of class c; bc2 of an unmatched record is noise, a first second barcode is 0 or 1 in turn"""
    if c == 0:
        return 0, 5
    if c == 1:
        return -1 - (i % 3), -2
    b1, b2 = divmod(c - 2, stride)
    return b1 + 1, (b2 + 1 if b2 or i % 2 else 0)


@functools.lru_cache(maxsize=None)
def gather_cases():
    out = []
    # record counts x class patterns: unique headers, so a record out of place is visible
    for n in COUNTS:
        text, _, off, ln = table_of(plain_records(n, 100 + n))
        ks, ke = _keeps(n, n)
        for p in PATTERNS:
            bc1, bc2, stride, ncl, edge, pred = pattern(p, n)
            cls = ref_classes(bc1, bc2, stride, ncl)
            out.append(_case("n%d_%s" % (n, p), text, n, off, ln, bc1, bc2, ks, ke, stride, ncl, 1, edge, pred(cls) and len(cls) == n))
    # class counts: 1, 1, 2, 2, 3 and 3 passes of the partition
    n = 300
    text, _, off, ln = table_of(plain_records(n, 7))
    ks, ke = _keeps(n, 8)
    for ncl, (stride, passes) in CLASS_COUNTS.items():
        rng = np.random.default_rng(ncl)
        cls = rng.integers(0, ncl, n)
        cls[:3] = (0, 1, ncl - 1)
        bc = [_bc_of_class(int(c), stride, i) for i, c in enumerate(cls)]
        bc1, bc2 = [b[0] for b in bc], [b[1] for b in bc]
        ok = radix_passes(ncl) == passes and (ncl - 2) % stride == 0 and np.array_equal(ref_classes(_i32(bc1), _i32(bc2), stride, ncl), cls)
        out.append(_case("classes_%d" % ncl, text, n, off, ln, bc1, bc2, ks, ke, stride, ncl, 1,
                         "%d classes: %d pass%s, first and last class used" % (ncl, passes, "es" * (passes > 1)), ok))
    # barcode values
    stride, nb1 = 4, 5
    vals = [(a, b) for a in (0, -1, -7, INT32_MIN, 1, nb1) for b in (-3, 0, 1, stride)]
    text, n, off, ln = table_of(plain_records(len(vals), 9))
    ks, ke = _keeps(n, 10)
    cls = ref_classes(_i32([v[0] for v in vals]), _i32([v[1] for v in vals]), stride, 2 + nb1 * stride)
    out.append(_case("barcode_values", text, n, off, ln, [v[0] for v in vals], [v[1] for v in vals], ks, ke, stride, 2 + nb1 * stride, 1,
                     "bc1 in {0, -1, -7, INT32_MIN, 1, largest}, bc2 in {negative, 0, 1, stride}",
                     cls.max() == 2 + nb1 * stride - 1 and sorted(set(cls)) == [0, 1, 2, 5, 18, 21]))
    # line lengths, on each of the four lines; one record of four empty lines
    lens = (0, 1, 63, 64, 65, 128, 129, 1000)
    recs = []
    for k in range(4):
        for L in lens:
            r = [bytes(65 + (len(recs) * 7 + j * (m + 1)) % 26 for j in range(5)) for m in range(4)]
            r[k] = bytes(97 + (len(recs) + j) % 26 for j in range(L))
            recs.append(tuple(r))
    recs.insert(11, (b"", b"", b"", b""))
    text, n, off, ln = table_of(recs)
    cyc = [(-1, -1), (1, 0), (2, 70), (64, 65), (65, 128), (1, INT32_MAX), (129, 2000), (1, 64), (0, 63), (66, 129), (1000, 1000)]
    ks, ke = [cyc[i % len(cyc)][0] for i in range(n)], [cyc[i % len(cyc)][1] for i in range(n)]
    bc1 = [(i * 3) % 5 - 1 for i in range(n)]
    seen = {(k, int(ln[4 * i + k])) for i in range(n) for k in range(4)}
    ok = all((k, L) in seen for k in range(4) for L in lens) and any(not ln[4 * i:4 * i + 4].any() for i in range(n))
    for trim in (1, 0):
        out.append(_case("line_lengths_trim%d" % trim, text, n, off, ln, bc1, [0] * n, ks, ke, 1, 5, trim,
                         "every line at 0, 1, 63, 64, 65, 128, 129 and 1000 bytes; a record of four empty lines", ok))
    # the trim grid; the quality line is shorter than, as long as and longer than the sequence
    recs, ks, ke = [], [], []
    for L in (10, 70):
        for s in (-1, 0, 1, 2, L, L + 1):
            a = max(s, 1)
            for e in (-1, 0, s - 1, s, L, L + 1, INT32_MAX):
                for Q in (0, a - 1, a, L - 1, L, L + 5):
                    i = len(recs)
                    recs.append((b"@t%d" % i, bytes(65 + (i + j) % 26 for j in range(L)), b"+", bytes(97 + (i + 3 * j) % 26 for j in range(Q))))
                    ks.append(s)
                    ke.append(e)
    recs.append((b"@end", b"ACGTACGT", b"+", b"IIIIIIII"))  # (no short quality line is the last of the text)
    ks.append(-1)
    ke.append(-1)
    text, n, off, ln = table_of(recs)
    bc1 = [(i * 5) % 4 - 1 for i in range(n)]
    ok = n == 2 * 6 * 7 * 6 + 1 and int(ln[4 * n - 1]) == 8 and {s for s in ks} == {-1, 0, 1, 2, 10, 11, 70, 71}
    for name, trim, kks, kke in (("trim_grid", 1, ks, ke), ("trim_grid_trim0", 0, ks, ke), ("trim_grid_trim0_null_keeps", 0, None, None)):
        out.append(_case(name, text, n, off, ln, bc1, [0] * n, kks, kke, 1, 4, trim,
                         "keep_start x keep_end x quality length, sequences of 10 and 70 bases", ok))
    # line tables of a CRLF text and of a text whose last record is cut
    n = 65
    text, _, off, ln = table_of(plain_records(n, 21), crlf=True)
    ks, ke = _keeps(n, 22)
    out.append(_case("crlf_table", text, n, off, ln, np.arange(n) % 4 - 1, [0] * n, ks, ke, 1, 4, 1, "lines of a CRLF text: no \"\\r\" is written",
                     all(text[int(o) + int(l)] == CR for o, l in zip(off, ln)) and text.count(b"\r") == 4 * n))
    text, n, off, ln = table_of(plain_records(64, 23), tail=b"@last\nACG")
    ks, ke = _keeps(n, 24)
    out.append(_case("truncated_table", text, n, off, ln, np.arange(n) % 4 - 1, [0] * n, ks, ke, 1, 4, 1,
                     "the last record is cut: two padded lines at off = text_len, len = 0",
                     n == 65 and list(off[-2:]) == [len(text)] * 2 and list(ln[-3:]) == [3, 0, 0]))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def gather_case(name):
    return next(c for c in gather_cases() if c.name == name)


# ---- the large case: every scan of the pipeline takes the carry loop of its one-workgroup stage ----
LARGE_N = 1_050_000


@functools.lru_cache(maxsize=1)
def large_case():
    """LARGE_N records of 13 to 25 bytes: "@" + 7 digits, sequence and quality of 0 to 6 bytes, 5 classes; its line table is
    written down from the layout (the tests hold it to the host index)"""
    n = LARGE_N
    rng = np.random.default_rng(20261018)
    s = rng.integers(0, 7, n)
    rl = 13 + 2 * s
    start = np.cumsum(rl) - rl
    t = rng.choice(np.frombuffer(b"ACGTNacgt#,:FI", np.uint8), int(rl.sum()))
    ids = np.arange(n)
    t[start] = ord("@")
    for k in range(7):
        t[start + 1 + k] = 48 + ids // 10 ** (6 - k) % 10
    t[start + 8] = NL
    t[start + 9 + s] = NL
    t[start + 10 + s] = ord("+")
    t[start + 11 + s] = NL
    t[start + 12 + 2 * s] = NL
    off = np.stack([start, start + 9, start + 10 + s, start + 12 + s], axis=1).ravel().astype(np.int64)
    ln = np.stack([np.full(n, 8), s, np.ones(n, np.int64), s], axis=1).ravel().astype(np.int32)
    bc1 = np.array([0, -1, 1, 2, 3])[rng.integers(0, 5, n)]
    ks = ids % 5 - 1
    ke = np.where(ks == -1, -1, (ids // 5) % 8)
    ok = (len(t) > 16 << 20 and tiles(len(t)) > FQ_SCAN_BLOCK and scan_partials(n) > FQ_SCAN_BLOCK
          and scan_partials(hist_items(n)) > FQ_SCAN_BLOCK)
    return _case("large", t, n, off, ln, bc1, np.zeros(n, np.int64), ks, ke, 1, 5, 1,
                 "index, pack scan, byte scan and histogram scan all carry across %d partials" % FQ_SCAN_BLOCK, ok)


# ---- the host library (csrc/bdx_io.cpp), the partner every device step has ----
def host_index(path, text, max_reads):
    """FastqFile.next_batch over a file of `text` -> (n_records, cursor, off, len)"""
    from biodemux_jl_amd import nativeio

    with open(path, "wb") as fh:
        fh.write(bytes(text))
    f = nativeio.FastqFile(str(path))
    try:
        n, off, ln = f.next_batch(max_reads, 4)
        return n, f.cursor, off[:4 * n].copy(), ln[:4 * n].copy()
    finally:
        f.close()


def host_open(path, text):
    from biodemux_jl_amd import nativeio

    with open(path, "wb") as fh:
        fh.write(bytes(text))
    return nativeio.FastqFile(str(path))


def host_gather(out_dir, f, c):
    """bdx_fq_demux_write of the case into plain files under out_dir (which it makes) -> (their bytes in class order, bytes
    per class).  Only the classes that hold records get a path."""
    import ctypes as C

    os.mkdir(out_dir)
    cls = np.ascontiguousarray(ref_classes(c.bc1, c.bc2, c.stride, c.n_classes), dtype=np.int32)
    used = np.unique(cls)
    name = lambda k: os.path.join(str(out_dir), "c%06d.fastq" % k)  # noqa: E731
    paths = (C.c_char_p * c.n_classes)()
    for k in used:
        paths[int(k)] = name(k).encode()
    off, ln = np.ascontiguousarray(c.off, dtype=np.int64), np.ascontiguousarray(c.len, dtype=np.int32)
    ks = None if c.keep_start is None else c.keep_start.ctypes.data
    ke = None if c.keep_end is None else c.keep_end.ctypes.data
    rc = f.L.bdx_fq_demux_write(f.h, off.ctypes.data, ln.ctypes.data, c.n, cls.ctypes.data, c.n_classes, paths, ks, ke, c.trim, 0, 4)
    assert rc == 0, f.L.bdx_io_last_error()
    class_bytes = np.zeros(c.n_classes, np.int64)
    blocks = []
    for k in used:
        if os.path.exists(name(k)):
            with open(name(k), "rb") as fh:
                blocks.append(fh.read())
            class_bytes[int(k)] = len(blocks[-1])
    assert sorted(os.listdir(out_dir)) == sorted("c%06d.fastq" % k for k in used if class_bytes[int(k)])
    return b"".join(blocks), class_bytes


# ---- profiles/fastq_case_coverage.txt ----
def coverage_lines():
    lines = ["# tests/fastq_cases.py: one line per case and the edge it reaches (python tests/fastq_cases.py > profiles/fastq_case_coverage.txt)",
             "# geometry: %d threads, %d bytes per lane, %d steps, tile %d bytes, scan block %d items" % (
                 FQ_THREADS, FQ_LANE_BYTES, FQ_STEPS, FQ_TILE, FQ_SCAN_BLOCK)]
    for t in index_texts():
        lines.append("index  %-28s bytes %8d  tiles %5d  newlines %6d  caps %-46s %s" % (
            t.name, len(t.text), tiles(len(t.text)), len(_nl_set(t.text)), ",".join(sorted(caps_for(t.text))), t.edge))
    for c in gather_cases() + (large_case(),):
        lines.append("gather %-28s n %8d  tiles %5d  classes %6d  passes %d  partials pack/bytes %5d  hist %5d  trim %d  %s" % (
            c.name, c.n, tiles(len(c.text)), c.n_classes, radix_passes(c.n_classes), scan_partials(c.n), scan_partials(hist_items(c.n)),
            c.trim, c.edge))
    return lines


if __name__ == "__main__":
    print("\n".join(coverage_lines()))
