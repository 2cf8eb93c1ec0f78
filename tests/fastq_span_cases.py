"""Cases for the index by byte spans (bdx_fq_count_lines_device, bdx_fq_index_span_device; _io="device-deal"), shared by
tests/test_device_deal_cpu.py and tests/test_device_deal_gpu.py: a numpy restatement of the contract in
include/biodemux_hip.h and the texts that reach its edges, each with a predicate (`ok`) computed from its bytes at the
span size it is built for.  The CPU test asserts the predicates and holds the restatement to the host library's index."""
import functools
from collections import namedtuple

import numpy as np

NL, CR = 10, 13
SPANS = (16, 17, 100, 4096)  # span sizes every case text is run at
TAIL0 = 16                   # the first tail the walkers offer; doubled while a span is not complete


def _u8(text):
    return text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)


# ---- the restatement ----
def ref_window_index(window, span_len, phase, starts_line, final):
    """bdx_fq_index_span_device over window = d_text[0, text_len) -> (n_records, complete, off int64[4n], len int32[4n]);
    off and len are None when complete == 0"""
    w = _u8(window)
    n = len(w)
    assert 0 <= span_len <= n and 0 <= phase <= 3
    nl = np.flatnonzero(w == NL).astype(np.int64)
    total = len(nl)
    # line i of the window has i newlines in front of its first byte: its global number is phase + i
    first = np.concatenate([np.zeros(1, np.int64), nl + 1])   # where line i starts (line `total`: the unterminated rest)
    end = np.concatenate([nl, np.full(1, n, np.int64)])       # where it ends
    begins = first < span_len                                 # the line starts inside the span ...
    begins[0] &= bool(starts_line)                            # ... offset 0 only when it is a line start at all
    rec = np.flatnonzero(begins & ((phase + np.arange(total + 1)) % 4 == 0))
    nrec = len(rec)
    if nrec == 0:
        return 0, 1, np.zeros(0, np.int64), np.zeros(0, np.int32)
    lines = (rec[:, None] + np.arange(4)[None, :]).ravel()
    if lines[-1] >= total and not final:
        return nrec, 0, None, None  # the last record's fourth line is not terminated inside the window
    real = lines <= total           # (behind the unterminated rest: padding of a truncated record)
    li = np.minimum(lines, total)
    off = np.where(real, first[li], n)
    e = np.where(real, end[li], n)
    ln = e - off
    ln -= (ln > 0) & (w[np.maximum(e - 1, 0)] == CR)
    return nrec, 1, off.astype(np.int64), ln.astype(np.int32)


def span_args(text, S, k, tail):
    """what the host knows of span k: -> (window, span_len, phase, starts_line, final)"""
    t = _u8(text)
    start = k * S
    assert 0 <= start < len(t)
    stop = min(len(t), start + S + tail)
    phase = int(np.count_nonzero(t[:start] == NL)) % 4
    starts_line = int(start == 0 or t[start - 1] == NL)
    return t[start:stop], min(S, stop - start), phase, starts_line, int(stop == len(t))


def ref_span_index(text, S, k, tail):
    """span k of `text` cut into spans of S bytes, offered with `tail` bytes behind it -> ref_window_index's result"""
    return ref_window_index(*span_args(text, S, k, tail))


def n_spans(text, S):
    return -(-len(text) // S)


def walk_spans(text, S, index=ref_span_index, tail0=TAIL0):
    """every span with a growing tail -> (off, len) of all spans, shifted by kS and concatenated in span order, and the
    records per span"""
    offs, lens, per_span = [np.zeros(0, np.int64)], [np.zeros(0, np.int32)], []
    for k in range(n_spans(text, S)):
        tail = tail0
        while True:
            n, complete, off, ln = index(text, S, k, tail)
            if complete:
                break
            assert k * S + S + tail < len(text), "not complete although the window reaches the end of the text"
            tail *= 2
        assert len(off) == 4 * n == len(ln)
        offs.append(off + k * S)
        lens.append(ln)
        per_span.append(n)
    return np.concatenate(offs), np.concatenate(lens), per_span


# ---- the case texts ----
SpanText = namedtuple("SpanText", "name text S edge ok")
_RECORD = b"@r\nACGTA\n+\nIIIII\n"  # 17 bytes: its newlines drift against every power of two


def _records(n, seq=5, head=b"@r", nl=b"\n"):
    return b"".join(head + nl + (b"ACGT" * seq)[:seq] + nl + b"+" + nl + b"I" * seq + nl for _ in range(n))


def _line_starts(t):
    """offsets at which a line of the text starts, and their global numbers"""
    t = _u8(t)
    s = np.concatenate([np.zeros(1, np.int64), np.flatnonzero(t == NL) + 1])
    s = s[s < len(t)]
    return s, np.arange(len(s))


def _pairs(text, S):
    return {tuple(span_args(text, S, k, 0)[2:4]) for k in range(n_spans(text, S))}


def _spans_without_record_start(text, S):
    """spans that hold line starts, none of them a record's"""
    s, num = _line_starts(text)
    out = []
    for k in range(n_spans(text, S)):
        m = (s >= k * S) & (s < (k + 1) * S)
        if m.any() and not (num[m] % 4 == 0).any():
            out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def span_texts():
    out = []

    def add(name, text, S, edge, ok):
        out.append(SpanText(name, bytes(text), S, edge, bool(ok)))

    t = b"@a\n" + b"ACGTACGTACGT" + b"\n+\n" + b"I" * 12 + b"\n" + _records(6)
    add("newline_on_last_byte", t, 16, "a newline on byte S - 1", t[15] == NL and t[16] != NL)
    t = b"@ab\n" + b"ACGTACGTACGT" + b"\n+\n" + b"I" * 12 + b"\n" + _records(6)
    add("newline_on_first_byte", t, 16, "a newline on byte S", t[16] == NL and t[15] != NL)
    t = b"@a\r\n" + b"ACGTACGTACG" + b"\r\n+\r\n" + b"I" * 11 + b"\r\n" + _records(6, nl=b"\r\n")
    add("cr_lf_across_boundary", t, 16, "\"\\r\" on byte S - 1, \"\\n\" on byte S", t[15] == CR and t[16] == NL)
    t = _records(2) + b"@long\n" + b"ACGT" * 15 + b"\n+\n" + b"I" * 60 + b"\n" + _records(3)
    s, _ = _line_starts(t)
    gaps = [k for k in range(n_spans(t, 16) - 1) if not ((s >= k * 16) & (s < (k + 2) * 16)).any()]
    add("line_longer_than_two_spans", t, 16, "two spans in a row without a line start", gaps)
    t = _records(9, seq=20)
    add("line_starts_no_record_start", t, 16, "spans whose line starts are no record starts", _spans_without_record_start(t, 16))
    t = _RECORD * 40
    add("all_phase_pairs", t, 16, "every (phase, starts_line) pair on some span",
        _pairs(t, 16) == {(p, s) for p in range(4) for s in (0, 1)})
    t = b"@r\nACGT\n+\nIIII\n" + _records(6)
    s, num = _line_starts(t)
    add("header_on_last_byte", t, 16, "a record starts on byte S - 1", t[15:16] == b"@" and 15 in s[num % 4 == 0].tolist())
    t = _records(5) + b"@x\nACGT\n+\nIIII"
    add("unterminated_last_line", t, 16, "the text does not end in a newline", t[-1] != NL and t.count(b"\n") % 4 == 3)
    for k, tail in ((1, b"@last\n"), (2, b"@last\nACG\n"), (3, b"@last\nACG\n+")):
        t = _records(5) + tail
        s, _ = _line_starts(t)
        add("last_record_%d_lines" % k, t, 16, "the last record has %d lines" % k, len(s) % 4 == k)
    t = _records(5) + b"\n\n\n\n\n\n"
    add("trailing_blank_lines", t, 16, "six empty lines behind the last record", t.endswith(b"\n" * 7) and len(_line_starts(t)[0]) % 4 == 2)
    add("empty_text", b"", 16, "no byte at all", True)
    t = b"@r\nAC\n+\nII\n"
    add("shorter_than_one_span", t, 16, "a text of %d bytes" % len(t), 0 < len(t) < 16)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def big_text():
    """8 MiB of records of four bytes (four empty lines): one span; a tail of long lines behind it, so that the window
    takes more than 1024 tiles of 16 KiB"""
    span = 8 << 20
    tail = (b"@t\n" + b"ACGT" * 4000 + b"\n+\n" + b"I" * 16000 + b"\n") * 300
    return np.concatenate([np.full(span, NL, np.uint8), _u8(tail)]), span
