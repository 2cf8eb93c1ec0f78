"""Cases for the opt-in FASTQ checks (csrc/bdx_fastq.hip: bdx_fq_check_device, bdx_fq_check_pair_device; csrc/bdx_io.cpp:
bdx_fq_check, bdx_fq_check_pair), shared by their CPU and GPU tests.  `ref_check` and `ref_check_pair` restate the
contract of include/biodemux_hip.h in numpy / plain Python; the kernels' geometry is parsed from the source; every named
case carries a predicate (`ok`) that proves it reaches the edge it is named for.

An entry reports only the LOWEST failing record.  `walk` therefore calls it again on the rest of the table behind every
failure it reports, until none is left: the list it returns is held to the restatement's verdict on every record."""
import functools
from collections import namedtuple

import numpy as np

import fastq_cases as FC

HEADER, PLUS, LENGTH = 1, 2, 4
MASKS = tuple(range(1, 8))

_C = FC.parse_constants()
_NEEDED = ("FQ_THREADS", "FQ_CHECK_GRID", "FQ_NAME_LANES", "FQ_NAME_GROUPS")
assert all(k in _C for k in _NEEDED), "constants of bdx_fastq.hip not found: %s" % [k for k in _NEEDED if k not in _C]
FQ_THREADS, FQ_CHECK_GRID, FQ_NAME_LANES, FQ_NAME_GROUPS = (_C[k] for k in _NEEDED)
WAVE = 64
SWEEP = FQ_CHECK_GRID * FQ_THREADS            # records one trip of the record check's grid takes
PAIR_SWEEP = FQ_CHECK_GRID * FQ_NAME_GROUPS   # ... of the pair check's
PAIRS_PER_WAVE = WAVE // FQ_NAME_LANES


# ---- the restatement (include/biodemux_hip.h) ----
def ref_masks(text, off, ln, n):
    """the rules each of the n records breaks, as a mask: int64[n]"""
    t = np.concatenate([FC._u8(text), np.zeros(1, np.uint8)])  # (the extra byte: where an empty line at the text's end points)
    off, ln = np.asarray(off, dtype=np.int64)[:4 * n], np.asarray(ln, dtype=np.int64)[:4 * n]
    h, p = t[off[0::4]], t[off[2::4]]
    m = np.where((ln[0::4] == 0) | (h != ord("@")), HEADER, 0)
    m |= np.where((ln[2::4] == 0) | (p != ord("+")), PLUS, 0)
    m |= np.where(ln[1::4] != ln[3::4], LENGTH, 0)
    return m.astype(np.int64)


def ref_check(text, off, ln, n, rules):
    """-> (first_bad, broken): the lowest record that breaks a rule of `rules` and the selected rules it breaks, or (-1, 0)"""
    m = ref_masks(text, off, ln, n) & rules
    bad = np.flatnonzero(m)
    return (int(bad[0]), int(m[bad[0]])) if len(bad) else (-1, 0)


def ref_name(header: bytes) -> bytes:
    """bytes after the first one, up to the first ' ' or '\\t' or the line's end, one trailing "/1" or "/2" dropped"""
    token = bytes(header[1:])
    ends = [k for k in (token.find(b" "), token.find(b"\t")) if k >= 0]
    if ends:
        token = token[:min(ends)]
    return token[:-2] if token.endswith((b"/1", b"/2")) else token


def _header(text, off, ln, i):
    return bytes(text[int(off[4 * i]):int(off[4 * i]) + int(ln[4 * i])])


def ref_pair_flags(text1, off1, ln1, text2, off2, ln2, n):
    """per record: the names of the two header lines differ"""
    return np.array([ref_name(_header(text1, off1, ln1, i)) != ref_name(_header(text2, off2, ln2, i)) for i in range(n)], dtype=bool)


def ref_check_pair(text1, off1, ln1, text2, off2, ln2, n):
    bad = np.flatnonzero(ref_pair_flags(text1, off1, ln1, text2, off2, ln2, n))
    return int(bad[0]) if len(bad) else -1


def walk(check, n, limit=64):
    """check(start, count) -> (first_bad, broken) relative to `start`; -> every failure in [0, n) as [(index, broken)]"""
    out, start = [], 0
    while start <= n and len(out) <= limit:
        bad, broken = check(start, n - start)
        if bad < 0:
            assert broken == 0
            return out
        assert 0 <= bad < n - start
        out.append((start + bad, broken))
        start += bad + 1
    raise AssertionError("more than %d failures" % limit)


def expected_walk(masks, rules):
    return [(int(i), int(masks[i] & rules)) for i in np.flatnonzero(masks & rules)]


# ---- record-check cases ----
CheckCase = namedtuple("CheckCase", "name text off len n edge ok")
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1024, 1025)
BIG_N = SWEEP + FQ_THREADS + 1  # the grid-stride loop's second trip, and one record of a third workgroup in it


def good_records(n):
    return [(b"@r%d" % i, b"ACGT", b"+", b"IIII") for i in range(n)]


@functools.lru_cache(maxsize=None)
def _clean(n):
    text, k, off, ln = FC.table_of(good_records(n))
    assert k == n
    return np.frombuffer(text, np.uint8), off, ln


def broken_copy(n, breaks):
    """the clean text of n records with record i breaking the rules breaks[i] (a mask), the bytes changed in place: the
    header's '@' becomes 'A', the '+' becomes '-', "ACGT\\n+\\nIIII" becomes "ACG\\n+\\nIIIII" (the table follows)"""
    t, off, ln = _clean(n)
    t, off, ln = t.copy(), off.copy(), ln.copy()
    for i, m in breaks.items():
        if m & HEADER:
            t[off[4 * i]] = ord("A")
        if m & LENGTH:
            s = int(off[4 * i + 1])
            t[s:s + 11] = np.frombuffer(b"ACG\n+\nIIIII", np.uint8)
            off[4 * i + 2] -= 1
            off[4 * i + 3] -= 1
            ln[4 * i + 1], ln[4 * i + 3] = 3, 5
        if m & PLUS:
            t[off[4 * i + 2]] = ord("-")
    return t, off, ln


def _broken_case(name, n, breaks, edge, more=True):
    t, off, ln = broken_copy(n, breaks)
    masks = ref_masks(t, off, ln, n)
    ok = more and {int(i): int(masks[i]) for i in np.flatnonzero(masks)} == {k: v for k, v in breaks.items() if v}
    # ... and the table is the text's own: the index restatement gives it back
    if n <= 2048:
        rn, _, roff, rln = FC.ref_index(t, 1, n + 1)
        ok = ok and rn == n and np.array_equal(roff, off) and np.array_equal(rln, ln)
    return CheckCase(name, t, off, ln, n, edge, bool(ok))


def _text_case(name, records, edge, expect, crlf=False, tail=b""):
    """a hand-written text; `expect`: {record: mask} of the records that break a rule"""
    text, n, off, ln = FC.table_of(records, crlf=crlf, tail=tail)
    masks = ref_masks(text, off, ln, n)
    return CheckCase(name, np.frombuffer(text, np.uint8), off, ln, n, edge,
                     {int(i): int(masks[i]) for i in np.flatnonzero(masks)} == expect)


@functools.lru_cache(maxsize=None)
def check_cases():
    out = []
    for n in COUNTS:
        out.append(_broken_case("n%d_clean" % n, n, {}, "%d records, none broken" % n))
        out.append(_broken_case("n%d_first" % n, n, {0: LENGTH}, "%d records, record 0 broken" % n))
        out.append(_broken_case("n%d_last" % n, n, {n - 1: PLUS}, "%d records, the last one broken" % n))
    # either side of every edge of the kernel's geometry: lane, wave, workgroup
    n = 4 * FQ_THREADS + 1
    for e, what in ((1, "lane"), (WAVE, "wave"), (FQ_THREADS, "workgroup"), (2 * FQ_THREADS, "second workgroup")):
        for k in (e - 1, e):
            out.append(_broken_case("edge_%s_%d" % (what.replace(" ", "_"), k), n, {k: HEADER}, "the single broken record at %d, %s edge %d" % (k, what, e),
                                    k in (e - 1, e) and e < n))
    # two broken records: the lower one wins, whichever rule each breaks; the unselected rule must not report
    for a, b in ((HEADER, PLUS), (PLUS, HEADER), (HEADER, LENGTH), (LENGTH, HEADER), (PLUS, LENGTH), (LENGTH, PLUS)):
        out.append(_broken_case("two_%d_then_%d" % (a, b), 300, {70: a, 200: b}, "record 70 breaks rule %d, record 200 rule %d: other waves" % (a, b), a != b))
        out.append(_broken_case("two_%d_then_%d_one_wave" % (a, b), 300, {5: a, 6: b}, "records 5 and 6 of one wave break rules %d and %d" % (a, b), 6 < WAVE))
    # each rule alone, every pair, all three on one record
    for m in MASKS:
        out.append(_broken_case("breaks_%d" % m, 9, {4: m}, "record 4 breaks exactly the rules %d" % m))
    h, s, p, q = b"@x", b"ACGT", b"+", b"IIII"
    out.append(_text_case("empty_lines", [(b"", s, p, q), (h, b"", p, q), (h, s, b"", q), (h, s, p, b""), (b"", b"", b"", b""), (h, b"", p, b""), (h, s, p, q)],
                          "an empty line in every position, four empty lines, empty sequence and quality",
                          {0: HEADER, 1: LENGTH, 2: PLUS, 3: LENGTH, 4: HEADER | PLUS}))
    out.append(_text_case("crlf", [(h, s, p, q), (b"x", s, p, q), (h, s, p, b"III"), (h, s, p, q)], "a CRLF text: lengths without the \"\\r\"",
                          {1: HEADER, 2: LENGTH}, crlf=True))
    out.append(CheckCase(*_mixed_line_ends()))
    good = [(h, s, p, q)] * 3
    for tail, expect, what in ((b"@last\n", PLUS, "after line 1"), (b"@last\nAC", PLUS | LENGTH, "inside line 2"),
                               (b"@last\nACGT\n", PLUS | LENGTH, "after line 2"), (b"@last\nACGT\n+\n", LENGTH, "after line 3"),
                               (b"@last\nACGT\n+\nII", LENGTH, "inside line 4"), (b"@last\n\n+\n", 0, "after line 3 of a record with an empty sequence"),
                               (b"@last\n\n", PLUS, "after an empty line 2")):
        c = _text_case("cut_%s" % what.replace(" ", "_"), good, "the last record is cut %s" % what, {3: expect} if expect else {}, tail=tail)
        out.append(c._replace(ok=c.ok and c.n == 4 and int(c.off[-1]) + int(c.len[-1]) == len(c.text)))
    firsts = [(bytes([0x40 + d]) + b"x", s, bytes([0x2B + e]), q) for d in (-1, 0, 1) for e in (-1, 0, 1)]
    out.append(_text_case("first_bytes", firsts, "first bytes 0x40 +- 1 of line 1 and 0x2B +- 1 of line 3",
                          {i: (HEADER if d else 0) | (PLUS if e else 0) for i, (d, e) in enumerate((d, e) for d in (-1, 0, 1) for e in (-1, 0, 1)) if d or e}))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def _mixed_line_ends():
    text = b"@a\r\nACGT\r\n+\nIIII\n@b\nAC\r\n+\r\nII\n"
    n, _, off, ln = FC.ref_index(text, 1, 3)
    return ("mixed_line_ends", np.frombuffer(text, np.uint8), off, ln, n, "\"\\r\\n\" and \"\\n\" mixed inside a record: the lengths agree",
            n == 2 and not ref_masks(text, off, ln, n).any() and list(ln) == [2, 4, 1, 4, 2, 2, 1, 2])


@functools.lru_cache(maxsize=None)
def big_check_cases():
    """BIG_N records: more than one trip of the grid-stride loop"""
    n = BIG_N
    out = [_broken_case("big_clean", n, {}, "%d records, none broken" % n, n > SWEEP),
           _broken_case("big_last", n, {n - 1: HEADER | LENGTH}, "the last of %d records" % n),
           _broken_case("big_second_trip", n, {SWEEP + 5: PLUS}, "record %d: the second trip of lane 5" % (SWEEP + 5), SWEEP + 5 < n),
           _broken_case("big_both_trips_of_a_lane", n, {5: LENGTH, SWEEP + 5: HEADER}, "records 5 and %d: both trips of one lane" % (SWEEP + 5)),
           _broken_case("big_trip_edge", n, {SWEEP - 1: PLUS, SWEEP: HEADER}, "records %d and %d: the end of the first trip" % (SWEEP - 1, SWEEP))]
    return tuple(out)


# ---- name cases ----
NameCase = namedtuple("NameCase", "name text1 off1 len1 text2 off2 len2 n edge ok")
TOKEN_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def _name_case(name, heads1, heads2, edge, expect, more=True, vary=False, tail1=b"", tail2=b""):
    """records whose header lines are heads1[i] / heads2[i]; `expect`: the records whose names differ; `vary`: sequence
    lengths 0 .. 15 in turn (the pair rule reads header lines only), so that the headers start at every offset modulo 16"""
    def table(heads, tail, salt):
        recs = [(h, b"A" * ((i + salt) % 16 if vary else 4), b"+", b"IIII") for i, h in enumerate(heads)]
        return FC.table_of(recs, tail=tail)

    text1, n1, off1, ln1 = table(heads1, tail1, 0)
    text2, n2, off2, ln2 = table(heads2, tail2, 5)
    flags = ref_pair_flags(text1, off1, ln1, text2, off2, ln2, n1)
    ok = more and n1 == n2 and sorted(expect) == np.flatnonzero(flags).tolist()
    return NameCase(name, np.frombuffer(text1, np.uint8), off1, ln1, np.frombuffer(text2, np.uint8), off2, ln2, n1, edge, bool(ok))


def _token(L, salt=0):
    return bytes(97 + (k * 7 + salt) % 26 for k in range(L))


@functools.lru_cache(maxsize=None)
def name_cases():
    out = []
    h1, h2, expect = [], [], []
    for L in TOKEN_LENGTHS:
        t = _token(L, L)
        rows = [(b"@" + t, b"@" + t + b" 1:N:0"), (b"@" + t + b"x", b"@" + t)]  # equal; one a prefix of the other
        diff = [False, True]
        if L:
            rows += [(b"@" + t, b"@" + b"#" + t[1:]), (b"@" + t + b"\tz", b"@" + t[:-1] + b"#")]  # the first / the last byte differs
            diff += [True, True]
        for (a, b), d in zip(rows, diff):
            if d:
                expect.append(len(h1))
            h1.append(a)
            h2.append(b)
    out.append(_name_case("token_lengths", h1, h2, "tokens of %s bytes: equal, a prefix, first byte, last byte" % (TOKEN_LENGTHS,), expect,
                          {len(ref_name(h)) for h in h1} >= set(TOKEN_LENGTHS)))
    out.append(_name_case("terminators", [b"@abc x", b"@abc", b"@abc", b"@ab c", b"@abc\t", b"@abc  x", b"@a\tb c"],
                          [b"@abc\ty", b"@abc z", b"@abcd", b"@ab\tc", b"@abc", b"@abc\t\tx", b"@a b\tc"],
                          "space against tab, no terminator, a terminator at once behind the name", [2]))
    pairs = [(b"@r/1", b"@r/2", 0), (b"@r/3", b"@r/3", 0), (b"@r/3", b"@r", 1), (b"@a/1b", b"@a/2b", 1), (b"@a/1b", b"@a/1b", 0),
             (b"@r/1 comment", b"@r/2 other", 0), (b"@/1", b"@/2", 0), (b"@/1", b"@", 0), (b"@/1", b"@x", 1), (b"@r/1/1", b"@r/1", 1),
             (b"@r/1/2", b"@r/1/1", 0), (b">abc", b"@abc", 0), (b"", b"@", 0), (b"", b"", 0), (b"", b"@a", 1), (b"@r/1", b"@r", 0),
             (b"@r/", b"@r/1", 1), (b"@1", b"@2", 1), (b"@r /1", b"@r", 0), (b"@r/0", b"@r/1", 1)]
    out.append(_name_case("suffixes", [p[0] for p in pairs], [p[1] for p in pairs],
                          "\"/1\" against \"/2\", \"/3\", \"/1\" inside the token and in front of a comment, a name that is only \"/1\", empty lines",
                          [i for i, p in enumerate(pairs) if p[2]], ref_name(b"@/1") == b"" and ref_name(b"@a/1b") == b"a/1b" and ref_name(b"@r/3") == b"r/3"))
    # headers at every offset modulo 16 in both texts: names of 20 bytes cross every 4-, 8- and 16-byte boundary
    h1, h2, expect = [], [], []
    for i in range(64):
        t = _token(20, i)
        h1.append(b"@" + t + b"/1")
        h2.append(b"@" + (t if i % 3 else t[:-1] + b"#") + b"/2 c")
        if i % 3 == 0:
            expect.append(i)
    c = _name_case("alignments", h1, h2, "names of 20 bytes that start at every offset modulo 16 in both texts", expect, vary=True)
    starts = {(int(c.off1[4 * i]) % 16, int(c.off2[4 * i]) % 16) for i in range(c.n)}
    out.append(c._replace(ok=c.ok and {a for a, _ in starts} == set(range(16)) and {b for _, b in starts} == set(range(16))))
    for name, t1, t2, expect in (("last_byte_equal", b"@last", b"@last", []), ("last_byte_differs", b"@last", b"@lasu", [3]),
                                 ("last_byte_suffix", b"@last/1", b"@last/2", []), ("last_byte_longer", b"@last", b"@lastx", [3])):
        c = _name_case(name, [b"@a", b"@b", b"@c"], [b"@a", b"@b", b"@c"], "the last header line ends on the text's last byte", expect,
                       tail1=t1, tail2=t2)
        out.append(c._replace(ok=c.ok and c.n == 4 and int(c.off1[12]) + int(c.len1[12]) == len(c.text1)
                              and int(c.off2[12]) + int(c.len2[12]) == len(c.text2)))
    # geometry: FQ_NAME_LANES lanes a pair, PAIRS_PER_WAVE pairs a wave, FQ_NAME_GROUPS a workgroup, PAIR_SWEEP a trip
    n = PAIR_SWEEP + FQ_NAME_GROUPS + 1
    edges = sorted({0, 1, PAIRS_PER_WAVE - 1, PAIRS_PER_WAVE, FQ_NAME_GROUPS - 1, FQ_NAME_GROUPS, PAIR_SWEEP - 1, PAIR_SWEEP, PAIR_SWEEP + 1, n - 1})
    h1 = [b"@read%d/1" % i for i in range(n)]
    h2 = [b"@read%d/2 x" % (i + (n if i in edges else 0)) for i in range(n)]
    out.append(_name_case("geometry", h1, h2, "%d pairs; the names differ at %s" % (n, edges), edges, n > PAIR_SWEEP))
    for k in (1, PAIRS_PER_WAVE - 1, PAIRS_PER_WAVE + 1, FQ_NAME_GROUPS + 1):
        out.append(_name_case("n%d_last_differs" % k, [b"@q%d" % i for i in range(k)], [b"@q%d" % (i + (i == k - 1)) for i in range(k)],
                              "%d pairs, the last one differs" % k, [k - 1]))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


if __name__ == "__main__":
    for c in check_cases() + big_check_cases():
        print("check %-32s n %8d  %s" % (c.name, c.n, c.edge))
    for c in name_cases():
        print("name  %-32s n %8d  %s" % (c.name, c.n, c.edge))
