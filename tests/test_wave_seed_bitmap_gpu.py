"""GPU checks of the wave kernel's seed scan (csrc/bdx_wave.hip): the probe of the seed bitmap at every position of a
group of sixteen, and the append of a lane's hits once per round of trips.

The construction is that of test_wave_append_gpu.py: the barcodes use only A, C and G and the reads are T apart from what
is planted in them, so a seed hit is exactly a q-base window of a read that equals a piece of some barcode, and every
hit of a batch is known (over three letters a window of a barcode is now and then a piece of another one: a chance hit,
known as well).  A planted barcode carries a T in all of its pieces but one wherever a case is about ONE probe: the read
then matches (within the budget) through that piece's seed hit alone, and a probe that misses it shows as a verdict that
differs from the oracle's.  Every case is compared bit for bit with the oracle and with the general kernel alone
(BDX_NO_WAVE), and asserts through the launch log that the wave kernel answered, in the form the case is about.
"""
from __future__ import annotations

import numpy as np
import pytest

import fuzz
import helpers as H

pytestmark = pytest.mark.gpu

RW = 32
HQ = RW * 6  # size_wave: hq_cap = rw * max(6, 4 + 2.5 chance), chance < 0.8 for every config below
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}  # the kernel's 2-bit base code ((byte >> 1) & 3); base i of a window: key bits 2 i, 2 i + 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _acg_barcodes(n, m, min_hamming, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < n:
        b = "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=m))
        if all(sum(x != y for x, y in zip(b, o)) >= min_hamming for o in out):
            out.append(b)
    return out


def _pieces(m, rate=0.1):
    """(q, piece offsets) of an m-base barcode: kb = floor(rate m) errors, kb + 1 pieces of floor(m / (kb + 1)) bases, seeds of
    the first q = min(8, piece length) bases of each (build_wave_tables)."""
    kb = int(rate * m)
    L = m // (kb + 1)
    return min(8, L), [t * L for t in range(kb + 1)]


def _keys(bcs):
    q, offs = _pieces(len(bcs[0]))
    return {b[o:o + q] for b in bcs for o in offs}


def _hits(read, keys, q):
    return [i for i in range(len(read) - q + 1) if read[i:i + q] in keys]


def _one_piece(b, keep):
    """Barcode `b` with a T in the middle of the seed of every piece but piece `keep`: kb substitutions, one seed hit."""
    q, offs = _pieces(len(b))
    s = list(b)
    for j, o in enumerate(offs):
        if j != keep:
            s[o + q // 2] = "T"
    return "".join(s)


def _read(col, body, n=150):
    s = "T" * col + body
    assert len(s) <= n
    return s + "T" * (n - len(s))


def _cfg(bcs, **kw):
    base = dict(bc_seqs=bcs, bc_lengths_no_N=[len(b) for b in bcs], ids=[f"bc{i + 1}" for i in range(len(bcs))],
                max_error_rate=0.1)
    base.update(kw)
    return H.bdx.DemuxConfig(**base)


def _template_args(name):
    return [x.strip() for x in name[name.index("<") + 1:name.rindex(">")].split(",")]


def _check(cfg, reads, monkeypatch, q, winm=False):
    """Oracle == wave kernel == general kernel; the wave run's launch log names a bdx_wave_kernel with seed length `q`
    (window mode or not) over the whole batch.  Returns (the oracle's outputs, reads the wave kernel handed on)."""
    seq, off = H.bdx.pack_reads(reads)
    oc = H.orc.OracleClassifier(cfg, nthreads=16, want_pass=False)
    exp = oc.classify(seq, off)
    listed = None
    for wave in (True, False):
        monkeypatch.setenv("BDX_WAVE_RW", str(RW))
        if wave:
            monkeypatch.delenv("BDX_NO_WAVE", raising=False)
        else:
            monkeypatch.setenv("BDX_NO_WAVE", "1")
        with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
            monkeypatch.delenv("BDX_NO_WAVE", raising=False)
            monkeypatch.delenv("BDX_WAVE_RW", raising=False)
            got = hc.classify(seq, off)
            launches = hc.last_launches
            fuzz.assert_same(got, exp, f"wave {wave} [{hc.kernel_path}] {launches}")
            assert np.array_equal(hc.counts, oc.counts), (wave, hc.kernel_path)
            if wave:
                assert hc.wave_launches > 0 and "wave" in hc.kernel_path, hc.kernel_path
                first = launches[0]
                assert first["kernel"].startswith("bdx_wave_kernel<") and first["reads"] == len(reads) and not first["list"], launches
                ta = _template_args(first["kernel"])
                assert int(ta[0]) == RW and int(ta[3]) == q and int(ta[5]) == 0 and ta[10] == ("true" if winm else "false"), first
                listed = hc.last_list_reads
            else:
                assert hc.wave_launches == 0 and "wave" not in hc.kernel_path, hc.kernel_path
    return exp, listed


BCS24 = None


def _bcs24():
    global BCS24
    if BCS24 is None:
        BCS24 = _acg_barcodes(48, 24, 8, seed=3)
    return BCS24


def test_one_seed_hit_at_every_offset(monkeypatch):
    """One intact piece per read (the other two carry a T), its window at every offset 0 .. 15 of a group of sixteen
    positions: offsets 0 .. 8 are probed from the group's first word, 9 .. 15 from the word that straddles into the next
    one, and the windows at offsets 9 .. 15 reach into the next group.  Every read matches through that one hit."""
    bcs = _bcs24()
    keys = _keys(bcs)
    reads, seen = [], set()
    for r, (col, keep) in enumerate((c, k) for c in range(10, 42) for k in range(3)):
        reads.append(_read(col, _one_piece(bcs[r % 48], keep)))
        assert col + 8 * keep in _hits(reads[-1], keys, 8)
        seen.add(((150 * r + col + 8 * keep) & 15, keep))  # (the first tile's image starts at the batch's first base)
    assert len(seen) == 48
    reads += [_read(10 + i % 40, bcs[i % 48]) for i in range(RW * 20)]  # (ordinary tiles: more than one tile per wave)
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=8)
    assert (exp["bc1"][:96] > 0).all() and listed == 0, listed


def test_windows_one_key_bit_from_a_piece(monkeypatch):
    """Windows that differ from a piece only in key bit 4 (base 2: A <-> C, G <-> T), and windows that share only a piece's
    low four key bits (its first two bases): neither is a seed, and the reads that carry them instead of an intact piece
    do not match (three errors against a budget of two).  Among them reads whose piece IS intact."""
    bcs = _bcs24()
    keys = _keys(bcs)
    rng = np.random.Generator(np.random.PCG64(5))
    flip = {"A": "C", "C": "A", "G": "T", "T": "G"}
    assert all(CODE[x] ^ CODE[y] == 1 for x, y in flip.items())
    reads, want = [], []
    for r in range(RW * 6):
        b = bcs[r % 48]
        keep = r % 3
        s = list(_one_piece(b, keep))
        kind = r % 4
        if kind == 1:  # key bit 4 of the intact piece's window
            s[8 * keep + 2] = flip[s[8 * keep + 2]]
        elif kind == 2:  # the piece's first two bases, then six others
            while True:
                w = b[8 * keep:8 * keep + 2] + "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=6))
                if w not in keys and sum(x != y for x, y in zip(w, b[8 * keep:8 * keep + 8])) >= 2:
                    break
            s[8 * keep:8 * keep + 8] = list(w)
        col = 10 + int(rng.integers(0, 48))
        read = _read(col, "".join(s))
        assert (col + 8 * keep in _hits(read, keys, 8)) == (kind not in (1, 2))
        reads.append(read)
        want.append(kind not in (1, 2))
    reads += [_read(10 + i % 40, bcs[i % 48]) for i in range(RW * 20)]
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=8)
    assert ((exp["bc1"][:len(want)] > 0) == np.array(want)).all() and listed == 0, listed


@pytest.mark.parametrize("ragged_tile", [False, True], ids=["whole-tiles", "ragged-last-tile"])
def test_hit_in_the_last_window_of_a_read_and_of_a_tile(ragged_tile, monkeypatch):
    """The barcode ends at the read's last base and only its last piece is intact: the one seed hit is the last window of
    the read that can hold a seed — in every read, so also in the last read of each tile and of the batch (the last window
    of a tile's image, with nothing but the image's padding behind it)."""
    bcs = _bcs24()
    n = RW * 24 + (5 if ragged_tile else 0)
    reads = [_read(150 - 24, _one_piece(bcs[r % 48], 2)) for r in range(n)]
    assert all(_hits(r, _keys(bcs), 8)[-1] == 150 - 8 for r in reads[:48])
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=8)
    assert (exp["bc1"] > 0).all() and listed == 0, listed


@pytest.mark.parametrize("m,n_bc,hd", [(14, 32, 6), (12, 8, 5)], ids=["q7", "q6"])
def test_shorter_seeds(m, n_bc, hd, monkeypatch):
    """Seeds of 7 and 6 bases (14- and 12-nt barcodes at rate 0.1: one error, two pieces): one intact piece per read, at
    every offset of a group."""
    q, offs = _pieces(m)
    assert (q, len(offs)) == ({14: 7, 12: 6}[m], 2)
    bcs = _acg_barcodes(n_bc, m, hd, seed=20 + m)
    keys = _keys(bcs)
    reads = []
    for r, (col, keep) in enumerate((c, k) for c in range(10, 42) for k in range(2)):
        reads.append(_read(col, _one_piece(bcs[r % n_bc], keep)))
        assert col + offs[keep] in _hits(reads[-1], keys, q)
    reads += [_read(10 + i % 40, bcs[i % n_bc]) for i in range(RW * 20)]
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=q)
    assert (exp["bc1"][:64] > 0).mean() > 0.9, exp["bc1"][:64]  # (a short barcode with an error may tie with another one)


@pytest.mark.parametrize("rng_str,winm", [("1:80", False), ("1:60", True)], ids=["ranged-scan", "window-mode"])
def test_ranged_configs(rng_str, winm, monkeypatch):
    """ref_search_range = 1:80 of 150 bases: the ranged scan (six groups per read instead of the flat image); 1:60: window
    mode (a window of at most half the read: scattered tiles).  One intact piece per read at every offset of a group inside
    the window, and barcodes outside the window, which do not count."""
    bcs = _bcs24()
    last = int(rng_str.split(":")[1])
    reads = [_read(col, _one_piece(bcs[r % 48], keep)) for r, (col, keep) in
             enumerate((c, k) for c in range(0, last - 24 + 1, 1) for k in range(3))]
    n_in = len(reads)
    reads += [_read(100 + i % 20, bcs[i % 48]) for i in range(RW * 3)]  # outside the window
    reads += [_read(i % (last - 24), bcs[i % 48]) for i in range(RW * 20)]
    cfg = _cfg(bcs, ref_search_range=H.bdx.parse_dynamic_range(rng_str))
    exp, listed = _check(cfg, reads, monkeypatch, q=8, winm=winm)
    assert (exp["bc1"][:n_in] > 0).all() and (exp["bc1"][n_in:n_in + RW * 3] == 0).all()


def test_lane_with_hits_in_several_trips(monkeypatch):
    """A lane scans the groups 64 apart (1024 positions), one per trip, and appends the hits of all its trips at once.  The
    first tile plants whole barcodes (three hits each) so that lane 3 .. 5 collect hits in four of the tile's five trips,
    beside lanes with the hits of a single trip; the tile stays within the hit queue."""
    bcs = _bcs24()
    keys = _keys(bcs)
    cols = {t: (60 - 150 * t) % 1024 for t in range(RW)}
    tile = [_read(cols[t] if cols[t] <= 126 else 20 + t, bcs[t]) for t in range(RW)]
    flat = "".join(tile)  # (tile 0 of the batch: the image starts at the first base)
    trips = {}
    for p in _hits(flat, keys, 8):
        trips.setdefault((p >> 4) & 63, set()).add(p >> 10)
    assert max(len(v) for v in trips.values()) >= 4 and any(len(v) == 1 for v in trips.values()), trips
    assert len(_hits(flat, keys, 8)) <= HQ
    reads = tile + [_read(10 + i % 40, bcs[i % 48]) for i in range(RW * 20)]
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=8)
    assert (exp["bc1"][:RW] > 0).all() and listed == 0, listed


def test_tile_just_below_and_just_above_the_hit_queue(monkeypatch):
    """Tiles with HQ - 1, HQ and HQ + 1 seed hits: only the last goes to the list, whole."""
    import test_wave_append_gpu as WA

    assert (WA.RW, WA.HQ) == (RW, HQ)
    bcs = WA._acg_barcodes(48)
    reads = WA._build(bcs, [HQ - 1, HQ, HQ + 1], np.full(RW * 3, 150), seed=8)
    keys = _keys(bcs)
    assert [sum(len(_hits(r, keys, 8)) for r in reads[k:k + RW]) for k in (0, RW, 2 * RW)] == [HQ - 1, HQ, HQ + 1]
    reads += [_read(10 + i % 40, bcs[i % 48]) for i in range(RW * 20)]
    exp, listed = _check(_cfg(bcs), reads, monkeypatch, q=8)
    assert listed == RW, listed
