"""GPU checks of the wave kernel's sweep columns in its LEAN forms (csrc/bdx_sweep_col.h, sweep_block of csrc/bdx_wave_kernel.h):
a column's peq address comes from a byte field of the group's expanded code words, and the doublings of the untracked columns
are adds; the score of a tracked column is the carry-out of its doublings.

The harness is test_wave_sweep_window_gpu.py's (imported, not copied): barcodes over A, C and G in reads of T, so the seed
hits, the records and their windows [diagonal - kb, diagonal + m + kb) are known; every case runs at BDX_CU_COUNT=1 with
545 .. 1 100 reads, compares every output and the counter vector bit for bit with the oracle, and asserts through the launch
log that the wave kernel took the whole batch in the form the case is about.  What a case is meant to exercise — the phase of
a window's first base in its image dword, the position of a non-base byte, the column at which a sweep's score first reaches
its minimum — is computed from the offsets and with a bit-parallel edit distance on the CPU and asserted before anything runs
on the device.
"""
from __future__ import annotations

import numpy as np
import pytest

import helpers as H
from test_wave_sweep_window_gpu import KNOWN, KNOWN_GEN, TRIM5, _bcs, _check, _cfg, _dist, _edit, _fill, _pack, _place, _plan, _synth_case

pytestmark = pytest.mark.gpu

SHIFT = 8  # the batch's first byte lies 8 bytes past a 16-byte boundary: the flat index of a base is its byte offset + 8 (mod 16)
N = 150


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import os

    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


def _track_from(m, kb):
    """First tracked column of a sweep's first block (bdx_plan.cpp track_from, seeded_tfq's cells for q = 8)."""
    t = m - kb - 1
    return 20 if t >= 20 else 12 if t >= 12 else 0


def _scores(b, r):
    """Score (edit distance of `b` to the best substring ending there) after every column of `r` (Myers' recurrence)."""
    m = len(b)
    mask, top = (1 << m) - 1, 1 << (m - 1)
    peq = {}
    for i, c in enumerate(b):
        peq[c] = peq.get(c, 0) | (1 << i)
    pv, mv, score, out = mask, 0, m, []
    for c in r:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = (mv | ~(xh | pv)) & mask
        mh = pv & xh
        score += (1 if ph & top else 0) - (1 if mh & top else 0)
        ph = (ph << 1) & mask
        mh = (mh << 1) & mask
        pv = (mh | ~(xv | ph)) & mask
        mv = ph & xv
        out.append(score)
    return out


def _window(read, b, piece):
    """[lo, hi) of the record that the intact piece at barcode offset `piece` opens: the piece's first occurrence gives the diagonal."""
    m = len(b)
    kb = _plan(m)[0]
    diag = read.index(b[piece:piece + 8]) - piece
    return max(diag - kb, 0), min(diag + m + kb, len(read))


def _subs(m, e):
    """e substitutions, one in the seed of each of the last e pieces (the first piece stays intact)."""
    kb, L, offs = _plan(m)
    return [("s", offs[kb - t] + 3) for t in range(e)]


# ---- window start at every nibble phase ----
def test_window_start_at_every_nibble_phase(monkeypatch):
    """Copies with 0 .. kb substitutions in the interior of reads of 140 .. 150 bases, at the read's first two columns (the
    window is clamped at the first base) and flush with its end: the flat index of the window's first base takes every value
    mod 8 for every edit count, and so does that of the windows clamped at either end of their read."""
    m = 24
    bcs = _bcs(m)
    kb = _plan(m)[0]
    reads, want, phases, clamped = [], [], {e: set() for e in range(kb + 1)}, {"head": set(), "tail": set()}
    for i in range(384):
        e = i % (kb + 1)
        where = ("mid", "mid", "head", "tail")[(i // 3) % 4]
        bi = i % len(bcs)
        b = bcs[bi]
        col = 1 if where == "head" and i % 2 else 2 + (i // 12) % 60
        n = N - (5 * i) % 11
        read, c = _place(_edit(b, _subs(m, e)), "mid" if where == "head" and i % 2 else where, n, col)
        lo, hi = _window(read, b, 0)
        assert _dist(b, read[lo:hi]) == e == _dist(b, read), (i, e)
        phase = (SHIFT + sum(len(r) for r in reads) + lo) % 8
        phases[e].add(phase)
        if lo == 0 and c < kb:
            clamped["head"].add(phase)
        if hi == n and c + m + kb > n:
            clamped["tail"].add(phase)
        reads.append(read)
        want.append(bi + 1)
    assert all(p == set(range(8)) for p in phases.values()), phases
    assert clamped["head"] == clamped["tail"] == set(range(8)), clamped
    n_p = len(reads)
    reads += _fill(m, 1003 - n_p, seed=4)
    seq, off = _pack(reads)
    exp = _check("col-phase", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, shift=SHIFT)
    assert (exp["bc1"][:n_p] == np.array(want)).all()


# ---- non-base bytes at every field ----
def test_non_base_bytes_at_every_field_of_an_image_dword(monkeypatch):
    """N, a lower-case letter and a zero byte: inside a copy at a flat index of every value mod 8 (each of the eight fields of
    the two expanded words), at the window's first and at its last column, and as the first byte behind a window that the
    read's end clamps (the first byte of the next read: the junk columns' nibbles are OR-ed over it)."""
    m = 24
    bcs = _bcs(m)
    kb, L, offs = _plan(m)
    reads, want, seen = [], [], set()
    for bad in ("N", "a", "\x00"):
        for rep in range(24):  # inside the copy: one piece is broken by the byte, the others seed the record
            bi = (rep + len(reads)) % len(bcs)
            b = bcs[bi]
            j = offs[rep % (kb + 1)] + (rep // 3) % L
            body = b[:j] + (b[j].lower() if bad == "a" else bad) + b[j + 1:]
            read, c = _place(body, "mid", N, 12 + 4 * rep)
            lo, hi = _window(read, b, offs[(rep + 1) % (kb + 1)])
            assert lo <= c + j < hi and _dist(b, read[lo:hi]) == 1
            seen.add((bad, "in", (SHIFT + sum(len(r) for r in reads) + c + j) % 8))
            reads.append(read)
            want.append(bi + 1)
        for rep in range(16):  # the window's first / last column
            bi = (rep + len(reads)) % len(bcs)
            b = bcs[bi]
            read, c = _place(b, "mid", N, 10 + 3 * rep)
            lo, hi = _window(read, b, 0)
            at = lo if rep % 2 == 0 else hi - 1
            assert read[at] == "T" and 0 < lo and hi < N
            read = read[:at] + ("t" if bad == "a" else bad) + read[at + 1:]
            assert _dist(b, read[lo:hi]) == 0
            seen.add((bad, "first" if rep % 2 == 0 else "last", (SHIFT + sum(len(r) for r in reads) + at) % 8))
            reads.append(read)
            want.append(bi + 1)
        for rep in range(16):  # behind a window clamped by the read's end: the next read begins with the byte
            bi = (rep + len(reads)) % len(bcs)
            b = bcs[bi]
            read, c = _place(b, "tail", N - rep % 3, 0)  # (reads of 150, 149, 148 bases: the byte's field moves)
            lo, hi = _window(read, b, 0)
            assert hi == len(read) and c + m + kb > hi
            seen.add((bad, "behind", (SHIFT + sum(len(r) for r in reads) + hi) % 8))
            reads.append(read)
            want.append(bi + 1)
            nxt = bcs[(bi + 1) % len(bcs)]
            reads.append(("t" if bad == "a" else bad) + _place(nxt, "mid", N - 1, 40 + rep)[0])
            want.append((bi + 1) % len(bcs) + 1)
    for bad in ("N", "a", "\x00"):
        assert {p for (x, k, p) in seen if x == bad and k == "in"} == set(range(8)), seen
        for k in ("first", "last", "behind"):
            assert len({p for (x, kk, p) in seen if x == bad and kk == k}) >= 4, (bad, k, seen)
    n_p = len(reads)
    reads += _fill(m, 1003 - n_p, seed=6)
    seq, off = _pack(reads)
    exp = _check("col-nonbase", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, shift=SHIFT)
    assert (exp["bc1"][:n_p] == np.array(want)).all(), np.flatnonzero(exp["bc1"][:n_p] != np.array(want))


# ---- score trajectories in the tracked columns ----
def _trajectory_plants(m):
    """-> (reads, wanted verdicts, columns at which a plant's window first attains its minimum, kinds seen)."""
    bcs = _bcs(m)
    kb, L, offs = _plan(m)
    tf, last = _track_from(m, kb), m + 2 * kb - 1
    reads, want, first_min, kinds = [], [], set(), set()

    def add(kind, bi, read, piece=0):
        b = bcs[bi]
        lo, hi = _window(read, b, piece)
        s = _scores(b, read[lo:hi])
        best = min(s)
        d = _dist(b, read)
        if kind == "two-dips":  # the score falls, rises and falls again inside the tracked columns
            t = [x for x in np.sign(np.diff(s[tf:])) if x != 0]
            if not any(t[i] < 0 < t[i + 1] and any(x < 0 for x in t[i + 2:]) for i in range(len(t) - 1)):
                return False
        assert d == best or d > kb, (kind, d, best)  # (the window holds the read's best alignment whenever it is within the budget)
        first_min.add(s.index(best))
        kinds.add((kind, d <= kb))
        reads.append(read)
        want.append(bi + 1 if d <= kb else 0)
        return True

    r = 0
    for rep in range(3):
        # a prefix of the barcode flush with the read's end: the window ends with the read, the score falls by one per
        # column to the last one — the minimum is first attained at column p + kb - 1, for every tracked column up to m + kb - 1
        for p in range(max(tf + 1 - kb, 8), m + 1):
            bi = r % len(bcs)
            assert add("prefix", bi, "T" * (N - p) + bcs[bi][:p])
            r += 1
        for e in range(0, kb + 2):  # copies with e inserted read bases / e deleted barcode bases behind the first piece
            for kind in ("i", "d"):
                bi = r % len(bcs)
                ops = [(kind, offs[1] + 2 + 2 * t) for t in range(e)]
                assert add("ins" if kind == "i" else "del", bi, _place(_edit(bcs[bi], ops), "mid", N, 20 + r % 70)[0])
                r += 1
    # two overlapping copies in one window: a copy cut short of its last base(s) and the barcode's tail once more
    found = 0
    for bi in range(len(bcs)):
        b = bcs[bi]
        for cut, tail in ((1, 3), (1, 2), (2, 4), (1, 4), (2, 3)):
            if m - cut + tail <= m + kb and add("two-dips", bi, _place(b[:m - cut] + b[m - tail:], "mid", N, 15 + 2 * bi)[0]):
                found += 1
                break
    assert found >= 4, found
    assert first_min >= set(range(tf, last + 1)), (sorted(first_min), tf, last)
    assert {("ins", True), ("ins", False), ("del", True), ("del", False), ("prefix", False)} <= kinds, kinds
    return reads, want


@pytest.mark.parametrize("m", [16, 24, 32], ids=["m16-tf12", "m24-tf20", "m32-tf20-two-blocks"])
def test_score_trajectories_in_the_tracked_columns(m, monkeypatch):
    """Plants whose window first attains its minimum at every tracked column, from the first one to the window's last: barcode
    prefixes cut by the read's end, copies with 0 .. kb + 1 insertions / deletions (kb + 1: nothing matches), and two
    overlapping copies, whose score falls, rises and falls again (m = 32: the tracked columns reach into the second block)."""
    reads, want = _trajectory_plants(m)
    n_p = len(reads)
    reads += _fill(m, 1003 - n_p, seed=8)
    seq, off = _pack(reads)
    exp = _check(("col-traj", m), _cfg(_bcs(m)), seq, off, monkeypatch, {KNOWN})
    assert (exp["bc1"][:n_p] == np.array(want)).all(), np.flatnonzero(exp["bc1"][:n_p] != np.array(want))


# ---- a second block ----
def test_second_block_next_to_28_column_windows(monkeypatch):
    """Barcodes of 20 .. 32 bases in one config: windows of 33 .. 44 columns share every 32-read tile with windows of at most 32
    columns, so the second block runs for some lanes of a wave only."""
    rng = np.random.Generator(np.random.PCG64(77))
    bcs = []
    while len(bcs) < 40:
        m = 20 + len(bcs) % 13
        b = "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=m))
        if all(sum(x != y for x, y in zip(b, o)) >= 8 for o in bcs):
            bcs.append(b)
    reads, widths = [], []
    for i in range(1003):
        b = bcs[(7 * i) % len(bcs)]
        kb, L, offs = _plan(len(b))
        ops = [[], [("i", offs[1] + 2)], [("d", offs[1] + 2), ("i", offs[kb] + 1)], [("i", offs[1] + 1)] * kb, [("s", offs[kb] + 2)]][i % 5]
        reads.append(_place(_edit(b, ops), ("mid", "tail", "mid", "head")[i % 4], N, 5 + i % 90)[0])
        widths.append(len(b) + 2 * kb)
    w = np.array(widths)
    assert {28} <= set(widths) and set(range(33, 45)) & set(widths) and max(widths) <= 44
    for t0 in range(0, 1003, 32):
        assert (w[t0:t0 + 32] <= 32).any() and (w[t0:t0 + 32] > 32).any(), t0
    seq, off = _pack(reads)
    exp = _check("col-mixed-m", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, listed="tier1")
    assert (exp["bc1"] > 0).mean() > 0.9


# ---- the other LEAN forms ----
def test_known_trim_form_trim_side_5(monkeypatch):
    """trim_side = 5: the known-trim class reads the score and the minimum before the column per column (which column lowered it)."""
    _synth_case("col-t5", monkeypatch, {TRIM5}, 0, trim_side=5)


def test_general_known_score_form_dual(monkeypatch):
    """Dual 24 x 16 barcodes at rate 0.1: the general known-score form."""
    _synth_case("col-dual", monkeypatch, {KNOWN_GEN}, 0, dual=True, max_error_rate=0.1)


def test_headline_shape_at_rate_02_tier_1(monkeypatch):
    """The headline shape at rate 0.2: tier 1 of capped budgets, the reads handed on bounded by may_list."""
    _synth_case("col-c2d", monkeypatch, {KNOWN}, "tier1", max_error_rate=0.2)
