"""GPU checks of the wave kernel's sweep windows (csrc/bdx_wave.hip): the known-score forms sweep a record over exactly
[dmin - kb, dmax + m + kb), every block of a sweep stops at the last column some lane of the wave needs, and the 2-bit
image is packed by a dot product.

The plants follow test_wave_seed_bitmap_gpu.py: barcodes over A, C and G, reads of T apart from what is planted, so the
seed hits of a read — and with them the records, their diagonals and their windows — are known.  A plant is a copy of a
barcode with exactly kb (or kb + 1) unit edits whose optimal alignment touches the first or the last column of its
record's window; that it does is asserted on the CPU, with a bit-parallel edit distance over the read cut one column
short, before anything runs on the GPU, and the oracle's verdicts are asserted to be what the plant is meant to produce.
Every case runs at BDX_CU_COUNT=1 with 545 .. 1 100 reads (16 waves: 32-read tiles, some or all waves walk a second
tile, the last tile is ragged), compares every output and the counter vector bit for bit with the oracle, and asserts
through the launch log that the wave kernel took the whole batch, in the form the case is about.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import fuzz
import helpers as H
from kernel_lattice import wave_span

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
KNOBS = ("BDX_CU_COUNT", "BDX_WAVE_RW", "BDX_WAVE_WAVES", "BDX_GRID", "BDX_NO_WAVE")
OUTPUTS = ("bc1", "bc2", "keep_start", "keep_end")
KNOWN = "false, 0, 0, false, 0, false, false"      # known-score form, single pass over whole reads (the headline's)
KNOWN_GEN = "false, 0, 0, false, 0, true, false"   # known-score form, dual configs / column windows
KNOWN_WIN = "false, 0, 0, false, 0, true, true"    # known-score form, window mode
TRIM5 = "false, 0, 0, false, 1, true, false"       # known-trim class
SPLIT = "true, 0, 0, false, 0, false, false"       # split mode


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


# ---- construction ----
def _acg_barcodes(n, m, min_hamming, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < n:
        b = "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=m))
        if all(sum(x != y for x, y in zip(b, o)) >= min_hamming for o in out):
            out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def _bcs(m):
    return tuple(_acg_barcodes({16: 32, 24: 48, 32: 48}[m], m, {16: 6, 24: 8, 32: 10}[m], seed=100 + m))


def _plan(m, rate=0.1):
    """(kb, piece length, piece offsets) of an m-base barcode at `rate`: kb + 1 pieces of floor(m / (kb + 1)) bases, seeds
    of the first min(8, piece length) bases of each (build_wave_tables)."""
    kb = int(rate * m)
    L = m // (kb + 1)
    return kb, L, [t * L for t in range(kb + 1)]


def _dist(b, r):
    """Smallest unit edit distance between barcode `b` and any substring of `r` (Myers' bit-vector recurrence)."""
    m = len(b)
    mask, top = (1 << m) - 1, 1 << (m - 1)
    peq = {}
    for i, c in enumerate(b):
        peq[c] = peq.get(c, 0) | (1 << i)
    pv, mv, score, best = mask, 0, m, m
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
        best = min(best, score)
    return best


def _edit(b, ops):
    """`b` with the unit edits `ops` applied, each given at its offset in the barcode: ("s", i) substitutes base i by T,
    ("i", i) inserts a T in front of base i, ("d", i) deletes base i."""
    out = []
    at = {}
    for kind, i in ops:
        at.setdefault(i, []).append(kind)
    for i, c in enumerate(b):
        kinds = at.get(i, [])
        out.append("T" * kinds.count("i"))
        if "d" in kinds:
            continue
        out.append("T" if "s" in kinds else c)
    return "".join(out)


def _front_ops(m, kind, extra):
    """Edits that break every piece but the last one (one edit in the seed of each), `extra`: one more edit in front of the
    last piece.  kind: "ins" (extra read bases), "del" (deleted barcode bases), "mix" (a substitution and indels)."""
    kb, L, offs = _plan(m)
    ops = []
    for t in range(kb):
        k = {"ins": "i", "del": "d", "mix": "s" if t == 0 else "i"}[kind]
        ops.append((k, offs[t] + 3))
    if extra:
        ops.append(({"ins": "i", "del": "d", "mix": "i"}[kind], offs[kb - 1] + L - 2))
    return ops


def _back_ops(m, kind, extra):
    """The mirror: only the first piece stays intact, the edits lie behind it."""
    kb, L, offs = _plan(m)
    ops = []
    for t in range(1, kb + 1):
        k = {"ins": "i", "del": "d", "mix": "s" if t == kb else "i"}[kind]
        ops.append((k, offs[t] + 3))
    if extra:
        ops.append(({"ins": "i", "del": "d", "mix": "i"}[kind], offs[1] + 6))
    return ops


def _place(body, where, n, col):
    """`body` in a read of n T's: at column `col` ("mid"), at the read's first base ("head") or flush with its end ("tail")."""
    c = {"mid": col, "head": 0, "tail": n - len(body)}[where]
    assert 0 <= c and c + len(body) <= n
    return "T" * c + body + "T" * (n - c - len(body)), c


def edge_plants(m, n=150, copies=2):
    """-> (reads, meta): the window-edge plants of every kind, side and place, with kb and kb + 1 edits.  meta rows:
    (barcode, kind, side, place, edits, touches) — touches: the plant's only alignment within the budget uses the window's
    first / last column (asserted here)."""
    bcs = _bcs(m)
    kb, L, offs = _plan(m)
    q = min(8, L)
    reads, meta = [], []
    r = 0
    for rep in range(copies):
        for kind in ("ins", "del", "mix"):
            for side in ("front", "back"):
                for place in ("mid", "head", "tail"):
                    for extra in (0, 1):
                        ops = (_front_ops if side == "front" else _back_ops)(m, kind, extra)
                        for bi in [(r + k) % len(bcs) for k in range(len(bcs))]:  # (the first barcode the plant works out for)
                            b = bcs[bi]
                            body = _edit(b, ops)
                            read, c = _place(body, place, n, 30 + (5 * r) % 23)
                            # the one intact piece, its seed hit and the record's diagonal
                            piece = offs[kb] if side == "front" else 0
                            pos = read.index(b[piece:piece + q])
                            diag = pos - piece
                            lo, hi = max(diag - kb, 0), min(diag + m + kb, n)
                            d = _dist(b, read[lo:hi])
                            # one column less on the plant's side of the window and a copy with kb edits is out of the budget
                            cut = read[lo + 1:hi] if side == "front" else read[lo:hi - 1]
                            touches = not extra and _dist(b, cut) > kb
                            # (a copy with kb + 1 edits may leave the window: its distance is asked of the whole read)
                            if _dist(b, read) == kb + extra and (extra or (d == kb and (touches or kind != "ins"))):
                                break
                        else:
                            raise AssertionError((kind, side, place, extra))
                        if kind == "ins" and not extra:  # (extra read bases push the alignment to the window's very edge)
                            assert (c == lo) if side == "front" else (c + len(body) == hi), (kind, side, place)
                        reads.append(read)
                        meta.append((bi, kind, side, place, kb + extra, touches))
                        r += 1
    return reads, meta


def _fill(m, count, n=150, seed=0):
    """Ordinary reads: a whole barcode somewhere in T's (the tiles around the plants)."""
    bcs = _bcs(m)
    return [_place(bcs[(seed + i) % len(bcs)], "mid", n, (7 * i + seed) % (n - m))[0] for i in range(count)]


def _cfg(bcs, **kw):
    base = dict(bc_seqs=list(bcs), bc_lengths_no_N=[len(b) for b in bcs], ids=[f"bc{i + 1}" for i in range(len(bcs))],
                max_error_rate=0.1)
    base.update(kw)
    return H.bdx.DemuxConfig(**base)


# ---- the run ----
def _form(name):
    a = [x.strip() for x in name[name.index("<") + 1:name.rindex(">")].split(",")]
    return int(a[0]), ", ".join(a[4:])


@functools.lru_cache(maxsize=None)
def _oracle_of(key):
    cfg, seq, off = _CASES[key]
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=True)  # (per-pass scores: may_list)
    return oc.classify(seq, off), oc.counts


def may_list(cfg, off, exp, first, tier1):
    """Upper bound, from the oracle's outputs alone, on the reads the first launch may hand on (bdx_last_list_reads) for a
    single-pass :semiglobal config with unit costs and min_delta = 0; None for any other config.  A sweep that misses an
    alignment leaves its read undecided: the tier behind repairs the verdict, and only this count shows it.
    Not tier 1 (full budgets): every read is answered but the empty ones (the replay wants n >= 1).
    Tier 1: budgets kb1(b) = min(kb(b), m_b / q - 1), q the launch's seed length; a barcode the tier does not
    see scores >= slo = min_b (kb1(b) + 1) / norm_b.  With min_delta = 0 a read is settled iff it has a winner, the winner's
    distance is within its capped budget and its score is < slo strictly: the oracle's winner at the full budget is the
    smallest score of all, so if tier 1 sees it, it is tier 1's winner too, and if tier 1 does not see it, it scores
    >= slo and so does everything tier 1 sees.  Every other read is handed on."""
    if cfg.is_dual or cfg.min_delta != 0 or (cfg.mismatch, cfg.indel, cfg.nindel) != (1, 1, None) or cfg.matching_algorithm != "semiglobal":
        return None
    lens = off[1:] - off[:-1]
    if not tier1:
        return int((lens == 0).sum())
    q = int(first["kernel"].split("<")[1].split(",")[3])
    norm = np.array(cfg.bc_lengths_no_N, dtype=np.float64)
    m = np.array([len(b) for b in cfg.bc_seqs])
    kb = np.floor(cfg.max_error_rate * norm).astype(np.int64)
    kb1 = np.minimum(kb, m // q - 1)
    slo = float(np.min((kb1 + 1) / norm))
    w = exp["pass_bc"][:, 0].astype(np.int64)
    score = exp["pass_score"][:, 0]
    has = w > 0
    wi = np.where(has, w - 1, 0)
    d = np.rint(np.where(has, score, 0.0) * norm[wi]).astype(np.int64)
    settled = has & (d <= kb1[wi]) & (score < slo) & (lens > 0)
    return int(len(lens) - settled.sum())


_CASES = {}


def _check(key, cfg, seq, off, monkeypatch, forms, listed=0, hint=None, shift=0, rw=32):
    """Oracle == device on every output and the counters; the first launch is a bdx_wave_kernel of one of `forms` over the
    whole batch with `rw`-read tiles, more tiles than waves and a ragged last tile; `listed`: the reads it hands on — a
    number (exactly that many), "tier1" (at most may_list: the launch is tier 1 of capped budgets) or a callable of the
    oracle's outputs that returns the upper bound.  hint / shift: through classify_device with that read-length hint and
    with the bytes `shift` bytes into their allocation."""
    import torch

    n = len(off) - 1
    assert 545 <= n <= 1100, n
    _CASES[key] = (cfg, seq, off)
    exp, counts = _oracle_of(key)
    full = exp
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BDX_CU_COUNT", "1")
    with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
        if hint is None and shift == 0:
            got = hc.classify(seq, off)
        else:
            dev = torch.device("cuda:0")
            buf = torch.zeros(len(seq) + 64, dtype=torch.uint8, device=dev)
            base = (-buf.data_ptr()) % 16 + shift  # (the batch's first byte: `shift` bytes past a 16-byte boundary)
            buf[base:base + len(seq)] = torch.from_numpy(seq).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            if hint is not None:
                hc.set_read_length_hint(hint)
            d_out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in OUTPUTS}
            hc.classify_device(buf.data_ptr() + base, d_off.data_ptr(), n, **{k: v.data_ptr() for k, v in d_out.items()})
            hc.sync()
            got = {k: v.cpu().numpy() for k, v in d_out.items()}
            exp = {k: exp[k] for k in OUTPUTS}
        launches = hc.last_launches
        what = f"{key} [{hc.kernel_path}] {launches}"
        fuzz.assert_same(got, exp, what)
        assert np.array_equal(hc.counts, counts), what
        assert "wave" in hc.kernel_path and hc.wave_launches > 0, what
        first = launches[0]
        assert first["kernel"].startswith("bdx_wave_kernel<") and first["reads"] == n and not first["list"], what
        got_rw, form = _form(first["kernel"])
        assert form in forms and got_rw == first["tile"] == rw, what
        assert -(-n // rw) > first["units"] and n % rw != 0, what
        if listed == "tier1":
            assert hc.kernel_path.startswith("tier1:"), what
            bound = may_list(cfg, off, full, first, True)
            assert bound is not None and hc.last_list_reads <= bound < n, f"{what}: {hc.last_list_reads} reads listed on, bound {bound}"
        elif callable(listed):
            bound = listed(full)
            assert hc.last_list_reads <= bound < n, f"{what}: {hc.last_list_reads} reads listed on, bound {bound}"
        else:
            assert hc.last_list_reads == listed, what
    monkeypatch.delenv("BDX_CU_COUNT", raising=False)
    return exp


def _pack(reads):
    return H.bdx.pack_reads(reads)


# ---- window edges ----
@pytest.mark.parametrize("m", [24, 16, 32], ids=["m24-kb2", "m16-kb1", "m32-kb3"])
def test_alignments_that_touch_the_windows_edge(m, monkeypatch):
    """Copies with exactly kb edits whose only alignment within the budget starts in the window's first column (the last
    piece intact, the edits in front of it) or ends in its last one (the mirror), by extra read bases, deleted barcode
    bases and a substitution plus indels; in the read's interior, at its first base (lo clamped) and flush with its end (hi
    clamped); and the same plants with kb + 1 edits, which match nothing.  m = 16: one error, two pieces; m = 32: three
    errors, a spread of diagonals that fills the 32 columns of a block.  Not every plant touches the edge: extra read bases
    always push the alignment into the window's first / last column, deleted barcode bases pull it away from it, so the
    deletion and mixed plants reach an edge only where the clamp to the read makes one (20 of the 72 plants per m touch;
    edge_plants checks each with the window cut one column short and the test wants at least twelve)."""
    reads, meta = edge_plants(m)
    assert sum(t for *_, t in meta) >= 12
    reads += _fill(m, 1000 - len(reads))
    seq, off = _pack(reads)
    kb = _plan(m)[0]
    exp = _check(("edges", m), _cfg(_bcs(m)), seq, off, monkeypatch, {KNOWN})
    for i, (bi, kind, side, place, edits, _) in enumerate(meta):
        assert exp["bc1"][i] == (bi + 1 if edits <= kb else 0), (i, kind, side, place, edits, int(exp["bc1"][i]))
    assert (exp["bc1"][len(meta):] > 0).all()


# ---- records ----
def test_indel_between_two_intact_pieces(monkeypatch):
    """Extra read bases / deleted barcode bases between intact pieces: the pieces' diagonals lie 1 .. 2 kb apart — up to kb
    they are one alignment within the budget, beyond it the record (diagonals within kb of its first hit) or two records
    still sweep windows that hold both pieces, and nothing matches."""
    m = 24
    bcs = _bcs(m)
    kb = _plan(m)[0]
    reads, want = [], []
    for rep in range(6):
        for s in range(1, 2 * kb + 1):
            for kind in ("ins", "del"):
                b = bcs[len(reads) % len(bcs)]
                body = b[:8] + "T" * s + b[8:] if kind == "ins" else b[:8] + b[8 + s:]
                read, _ = _place(body, ("mid", "head", "tail")[rep % 3], 150, 20 + 9 * rep + s)
                d = _dist(b, read)
                # (deleted bases: the first piece and the intact third one are s apart, the second piece is broken)
                assert d == (s if s <= kb else d) and (d <= kb) == (s <= kb), (kind, s, d)
                reads.append(read)
                want.append(bcs.index(b) + 1 if s <= kb else 0)
    n_p = len(reads)
    reads += _fill(m, 900 - n_p, seed=3)
    seq, off = _pack(reads)
    exp = _check("indel-spread", _cfg(bcs), seq, off, monkeypatch, {KNOWN})
    assert (exp["bc1"][:n_p] == np.array(want)).all(), (exp["bc1"][:n_p], want)


def test_two_copies_of_one_barcode_and_a_chance_seed_next_to_a_copy(monkeypatch):
    """Two copies of a barcode 1 .. 2 kb + 2 positions apart with different edit counts (two records whose windows reach
    into each other's copy: the barcode's distance is the better copy's); a chance 8-mer of barcode A directly in front of
    / behind a true copy of barcode B (A's record sweeps over B's copy and finds nothing; only B matches)."""
    m = 24
    bcs = _bcs(m)
    kb = _plan(m)[0]
    reads, want = [], []
    for gap in range(1, 2 * kb + 3):
        for e1, e2 in ((2, 1), (1, 2), (0, 2), (3, 1), (2, 3), (3, 3)):
            bi = len(reads) % len(bcs)
            b = bcs[bi]
            c1 = _edit(b, [("s", 8 * t + 3) for t in range(3)][:e1])
            c2 = _edit(b, [("s", 8 * t + 5) for t in range(3)][:e2])
            read, _ = _place(c1 + "T" * gap + c2, "mid", 150, 11 + 7 * gap + e1)
            d = _dist(b, read)
            assert d == min(e1, e2), (gap, e1, e2, d)
            reads.append(read)
            want.append(bi + 1 if d <= kb else 0)
    for i in range(96):
        a, bi = bcs[i % len(bcs)], (i + 7) % len(bcs)
        b = _edit(bcs[bi], [("s", 8 * (i % 3) + 2)][: i % 2])
        piece = a[8 * (i % 3):8 * (i % 3) + 8]
        read, _ = _place(piece + b if i % 4 < 2 else b + piece, "mid", 150, 13 + i)
        assert _dist(a, read) > kb
        reads.append(read)
        want.append(bi + 1)
    n_p = len(reads)
    reads += _fill(m, 1000 - n_p, seed=5)
    seq, off = _pack(reads)
    exp = _check("two-copies", _cfg(bcs), seq, off, monkeypatch, {KNOWN})
    assert (exp["bc1"][:n_p] == np.array(want)).all(), (exp["bc1"][:n_p], want)


# ---- reads ----
def test_short_reads_and_ragged_reads_with_a_wrong_length_hint(monkeypatch):
    """Reads of 0, m - 1, m and m + kb bases (an empty window, a window clamped on both sides), and reads of 20 .. 260
    bases, classified with a read-length hint of 150: the tiles are laid out from the offsets alone."""
    m = 24
    bcs = _bcs(m)
    kb = _plan(m)[0]
    rng = np.random.Generator(np.random.PCG64(11))
    reads = []
    for i in range(80):
        b = bcs[i % len(bcs)]
        reads += ["", b[:m - 1], b, b + "T" * kb, "T" * kb + b[1:]]
    n_short = len(reads)
    while len(reads) < 1003:
        n = int(rng.integers(20, 261))
        b = bcs[len(reads) % len(bcs)]
        body = b if n >= m else b[:n]
        reads.append(_place(body, ("mid", "head", "tail")[len(reads) % 3], n, int(rng.integers(0, n - len(body) + 1)))[0])
    seq, off = _pack(reads)
    # planted to overflow: the plan sizes a tile's span for 32 reads of the hinted length (size_wave); a tile of longer reads
    # does not fit and is handed on whole (geometry(): head + bases + 16 <= span); so is an empty read (the replay wants n >= 1)
    span = wave_span(32, 150)
    over = 0
    for r0 in range(0, len(reads), 32):
        r1 = min(r0 + 32, len(reads))
        whole = int(off[r1] - off[r0]) + int(off[r0]) % 16 + 16 > span
        over += r1 - r0 if whole else sum(len(r) == 0 for r in reads[r0:r1])
    assert 80 < over < len(reads) // 3, over
    exp = _check("ragged", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, listed=over, hint=150)
    bc = exp["bc1"][:n_short].reshape(-1, 5)
    assert (bc[:, 0] == 0).all() and (bc[:, 1:] > 0).all(), bc[:4]


def test_n_and_lower_case_bytes_inside_a_window(monkeypatch):
    """N and lower-case letters inside a copy: the 4-bit image says "other" for them (a mismatch in every row) while the
    2-bit image, which the seed probe reads, aliases them to a base — the vector takes the exact pack."""
    m = 24
    bcs = _bcs(m)
    reads = []
    for i in range(240):
        b = list(bcs[i % len(bcs)])
        for t in range(i % 4):  # 0 .. 3 bytes that are no base, one per piece
            j = 8 * t + (i // 4) % 8
            b[j] = "N" if (i + t) % 2 else b[j].lower()
        reads.append(_place("".join(b), "mid", 150, 10 + i % 100)[0])
    reads += _fill(m, 1001 - len(reads), seed=9)
    seq, off = _pack(reads)
    _check("n-lower", _cfg(bcs), seq, off, monkeypatch, {KNOWN})


def test_exact_copy_at_every_byte_lane(monkeypatch):
    """An exact copy at every start offset 0 .. 15 modulo 16 of the flat image: every byte lane of the 2-bit pack carries
    the first base of a seed."""
    m = 24
    bcs = _bcs(m)
    reads, seen = [], set()
    for r in range(160):
        col = 10 + r % 16
        reads.append(_place(bcs[r % len(bcs)], "mid", 150, col)[0])
        seen.add((150 * r + col) & 15)
    assert seen == set(range(16))
    reads += _fill(m, 999 - len(reads), seed=1)
    seq, off = _pack(reads)
    exp = _check("lanes", _cfg(bcs), seq, off, monkeypatch, {KNOWN})
    assert (exp["bc1"] > 0).all()


@pytest.mark.parametrize("shift", list(range(1, 16)))
def test_batch_whose_bytes_start_off_a_vector_boundary(shift, monkeypatch):
    """The batch's first byte lies 1 .. 15 bytes past a 16-byte boundary: the tile's vectors are fetched aligned, so the
    same reads meet the pack in other byte lanes."""
    m = 24
    bcs = _bcs(m)
    reads, _ = edge_plants(m, copies=1)
    reads += _fill(m, 587 - len(reads), seed=2)
    seq, off = _pack(reads)
    _check("shifted", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, shift=shift)


# ---- other cells ----
def test_mixed_barcode_lengths(monkeypatch):
    """Barcodes of 20 .. 32 bases in one config (budgets 2 and 3, windows of 28 .. 44 columns in one wave: the second block
    runs for some lanes only, and stops at their last column)."""
    rng = np.random.Generator(np.random.PCG64(21))
    bcs = []
    while len(bcs) < 40:
        m = int(rng.integers(20, 33))
        b = "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=m))
        if all(sum(x != y for x, y in zip(b, o)) >= 8 for o in bcs):
            bcs.append(b)
    reads = []
    for i in range(1003):
        b = bcs[i % len(bcs)]
        kb, L, offs = _plan(len(b))
        ops = [[], [("i", offs[1] + 2)], [("d", offs[1] + 2), ("i", offs[kb] + 1)], [("i", offs[1] + 1)] * kb][i % 4]
        reads.append(_place(_edit(b, ops), ("mid", "head", "tail")[i % 3], 150, 5 + i % 90)[0])
    seq, off = _pack(reads)
    exp = _check("mixed-m", _cfg(bcs), seq, off, monkeypatch, {KNOWN}, listed="tier1")  # (budgets 2 and 3: the planner makes it tier 1 of capped budgets)
    assert (exp["bc1"] > 0).mean() > 0.9


def _synth_case(key, monkeypatch, forms, listed, n=1003, dual=False, **kw):
    from biodemux_jl_amd import synth

    if dual:
        b1 = synth.make_barcodes(24, 24, seed=synth.SEED + 1)
        b2 = synth.make_barcodes(16, 24, seed=synth.SEED + 2)
        seq, off, _ = synth.make_reads(b1, n, 150, seed=synth.SEED, plant_lo=0, plant_hi=40, second=(b2, 100, 126))
        cfg = H.bdx.DemuxConfig(bc_seqs=b1, bc_lengths_no_N=[24] * 24, ids=[f"x{i + 1}" for i in range(24)], is_dual=True,
                                bc_seqs2=b2, bc_lengths_no_N2=[24] * 16, ids2=[f"y{i + 1}" for i in range(16)], **kw)
    else:
        bcs = synth.make_barcodes(96, 24, seed=synth.SEED)
        seq, off, _ = synth.make_reads(bcs, n, 150, seed=synth.SEED)
        cfg = _cfg(bcs, **kw)
    return _check(key, cfg, seq, off, monkeypatch, forms, listed=listed)


def test_headline_shape_at_rate_02_tier_1(monkeypatch):
    """96 barcodes of 24 nt at rate 0.2: the wave kernel is tier 1 with capped budgets and hands the undecided reads on —
    those without a barcode within two edits, and no more."""
    _synth_case("c2d", monkeypatch, {KNOWN}, "tier1", max_error_rate=0.2)


def test_dual_config(monkeypatch):
    """Dual 24 x 16 barcodes at rate 0.1: the general known-score form, two passes per read."""
    _synth_case("dual", monkeypatch, {KNOWN_GEN}, 0, dual=True, max_error_rate=0.1)


def test_column_window(monkeypatch):
    """ref_search_range = 1:60 of 150 bases: the windows are clamped to the pass's column window."""
    _synth_case("r60", monkeypatch, {KNOWN_GEN, KNOWN_WIN}, 0, ref_search_range=H.bdx.parse_dynamic_range("1:60"))


def test_trim_side_5_keeps_its_windows(monkeypatch):
    """trim_side = 5: the known-trim class reports columns and keeps its window with one slack column on either side."""
    _synth_case("t5", monkeypatch, {TRIM5}, 0, trim_side=5)


def test_split_mode_keeps_its_windows(monkeypatch):
    """indel = 2: split mode hands first / last columns over to the exact kernel; its windows are untouched.  It hands on
    every read with a candidate and answers the others itself; a candidate is a barcode within kb = floor(floor(rate m) /
    cmin) = 2 unit edits of the read, so the reads with one are exactly those the same batch matches at unit costs."""
    from biodemux_jl_amd import synth

    bcs = synth.make_barcodes(96, 24, seed=synth.SEED)
    seq, off, _ = synth.make_reads(bcs, 1003, 150, seed=synth.SEED)
    unit = H.orc.OracleClassifier(_cfg(bcs), nthreads=NTHREADS, want_pass=False).classify(seq, off)
    with_candidate = int((unit["bc1"] > 0).sum())
    assert 0 < with_candidate < 1003
    _synth_case("split", monkeypatch, {SPLIT}, lambda exp: with_candidate, indel=2)


# ---- fuzz ----
# (seeds whose config the planner gives to the wave kernel at one CU, alone or as tier 1)
FUZZ = [("random_case_many_barcodes", s) for s in range(41000, 41008)] + [("random_case_tiers", s) for s in (42001, 42010, 42014)] + \
       [("random_case_band", s) for s in range(43000, 43006)] + [("random_case_wide", s) for s in (44000, 44003, 44004)]


@functools.lru_cache(maxsize=None)
def _fuzz_case(family, seed):
    cfg, seq, off = getattr(fuzz, family)(seed, n_reads=1003 + 38 * (seed % 3))  # (1003, 1041, 1079: ragged last tiles of 16 and of 32 reads)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=True)
    return cfg, seq, off, oc.classify(seq, off), oc.counts


@pytest.mark.parametrize("family,seed", FUZZ)
def test_fuzz(family, seed, monkeypatch):
    """The fuzz generators whose configs reach the wave kernel (test_geometry_fuzz_gpu.py EXPECTED_SHAPES), new seeds, one CU:
    whatever form the planner picks, every output and the counters equal the oracle's; the first launch is a wave kernel
    over the whole batch with more tiles than waves, it hands on fewer reads than it was given, and where may_list knows
    the config (single pass, unit costs, no min_delta, not split mode) no more than the oracle's outputs allow."""
    cfg, seq, off, exp, counts = _fuzz_case(family, seed)
    n = len(off) - 1
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BDX_CU_COUNT", "1")
    with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
        got = hc.classify(seq, off)
        launches = hc.last_launches
        what = f"{family} seed {seed} [{hc.kernel_path}] {launches}"
        fuzz.assert_same(got, exp, what)
        assert np.array_equal(hc.counts, counts), what
        assert "wave" in hc.kernel_path and hc.wave_launches > 0, what
        first = launches[0]
        assert first["kernel"].startswith("bdx_wave_kernel<") and first["reads"] == n and not first["list"], what
        rw, form = _form(first["kernel"])
        assert rw == first["tile"] and rw in (16, 32) and -(-n // rw) > first["units"] and n % rw != 0, what
        listed = hc.last_list_reads
        assert listed < n, what
        bound = None if form.startswith("true") else may_list(cfg, off, exp, first, hc.kernel_path.startswith("tier1:"))
        if bound is not None:
            assert listed <= bound, f"{what}: {listed} reads listed on, bound {bound}"
    monkeypatch.delenv("BDX_CU_COUNT", raising=False)
