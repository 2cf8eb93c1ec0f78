"""GPU checks of the wave kernel's seed-hit append (csrc/bdx_wave.hip, seed scan): every lane appends its own hits behind
the hits of the lanes below it, and a tile whose hits overflow the hit queue (nhq > HQ) goes to the list whole.

The batches are built so that the hits of every tile are known exactly: the barcodes use only A, C and G, the reads are
T apart from what is planted in them, so a seed hit is exactly an 8-base window of the read that equals a piece of some
barcode (pieces: 24-nt barcodes at rate 0.1 have kb = 2 and three 8-base pieces at offsets 0, 8 and 16), and no window
that touches a T (or a neighbouring read, or the bytes past a tile) can hit.  With 32-read tiles (BDX_WAVE_RW=32) and
48 barcodes the hit queue holds HQ = 32 * 6 = 192 entries (size_wave: chance = 150 * 144 / 4^8 < 0.8).
Every case is compared with the oracle and with the general kernel alone (BDX_NO_WAVE).
"""
from __future__ import annotations

import numpy as np
import pytest

import fuzz
import helpers as H

pytestmark = pytest.mark.gpu

RW = 32
HQ = RW * 6
Q = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _acg_barcodes(n, m=24, seed=3, extra=()):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = list(extra)
    while len(out) < n:
        b = "".join("ACG"[int(c)] for c in rng.integers(0, 3, size=m))
        if all(sum(x != y for x, y in zip(b, o)) >= 8 for o in out):
            out.append(b)
    return out


def _keys(bcs):
    return {b[o:o + Q] for b in bcs for o in (0, 8, 16)}


def _hits(read, keys):
    return sum(1 for i in range(len(read) - Q + 1) if read[i:i + Q] in keys)


def _cfg(bcs, **kw):
    base = dict(bc_seqs=bcs, bc_lengths_no_N=[len(b) for b in bcs], ids=[f"bc{i + 1}" for i in range(len(bcs))],
                max_error_rate=0.1)
    base.update(kw)
    return H.bdx.DemuxConfig(**base)


def _tile_reads(rng, bcs, keys, target, lengths):
    """RW reads of the given lengths whose windows hit `target` times in all: a planted barcode (with a substitution now and
    then) in every other read, and lone pieces between T's (one hit each), the tile's remaining hits spread evenly."""
    pieces = sorted(keys)
    reads = []
    left = target
    for t in range(RW):
        n = int(lengths[t])
        body = []
        if t % 2 == 0:
            b = list(bcs[int(rng.integers(0, len(bcs)))])
            if rng.random() < 0.5:
                j = int(rng.integers(0, len(b)))
                b[j] = "ACG"[("ACG".index(b[j]) + 1) % 3]
            body.append("".join(b))
        share = left if t == RW - 1 else -(-left // (RW - t))
        while _hits("T".join(body), keys) < share:
            body.append(pieces[int(rng.integers(0, len(pieces)))])
        s = "T" * 10 + "T".join(body)
        assert len(s) + 10 <= n, "read too short for its hits"
        s = s + "T" * (n - len(s))
        reads.append(s)
        left -= _hits(s, keys)
    assert left == 0, left
    return reads


def _build(bcs, targets, lengths, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = _keys(bcs)
    reads = []
    for k, target in enumerate(targets):
        reads += _tile_reads(rng, bcs, keys, target, lengths[k * RW:(k + 1) * RW])
    return reads


def _both(cfg, seq, off, monkeypatch, want_pass):
    oc = H.orc.OracleClassifier(cfg, nthreads=16, want_pass=want_pass)
    exp = oc.classify(seq, off)
    lists = {}
    for wave in (True, False):
        monkeypatch.setenv("BDX_WAVE_RW", str(RW))
        if wave:
            monkeypatch.delenv("BDX_NO_WAVE", raising=False)
        else:
            monkeypatch.setenv("BDX_NO_WAVE", "1")
        with H.bdx.HipClassifier(cfg, want_pass=want_pass) as hc:
            monkeypatch.delenv("BDX_NO_WAVE", raising=False)
            monkeypatch.delenv("BDX_WAVE_RW", raising=False)
            got = hc.classify(seq, off)
            fuzz.assert_same(got, exp, f"wave {wave} [{hc.kernel_path}]")
            assert np.array_equal(hc.counts, oc.counts), (wave, hc.kernel_path)
            if wave:
                assert hc.wave_launches > 0 and "wave" in hc.kernel_path, hc.kernel_path
                lists[wave] = hc.last_list_reads
            else:
                assert hc.wave_launches == 0 and "wave" not in hc.kernel_path, hc.kernel_path
    return exp, lists[True]


@pytest.mark.parametrize("ragged", [False, True], ids=["150nt", "ragged"])
@pytest.mark.parametrize("want_pass", [False, True], ids=["verdicts", "per-pass"])
def test_hit_queue_exactly_full_and_one_over(ragged, want_pass, monkeypatch):
    """Tiles with HQ - 1, HQ, HQ + 1 and HQ hits: only the tile with HQ + 1 hits goes to the list (all of its RW reads)."""
    bcs = _acg_barcodes(48)
    targets = [HQ - 1, HQ, HQ + 1, HQ]
    rng = np.random.Generator(np.random.PCG64(7))
    lengths = rng.integers(110, 200, size=RW * len(targets)) if ragged else np.full(RW * len(targets), 150)
    reads = _build(bcs, targets, lengths, seed=8 + ragged)
    # the rest of the batch: ordinary tiles (so that the waves have more than one tile each)
    reads += [("T" * int(10 + i % 40) + bcs[i % len(bcs)] + "T" * 150)[:150] for i in range(RW * 60)]
    seq, off = H.bdx.pack_reads(reads)
    exp, listed = _both(_cfg(bcs), seq, off, monkeypatch, want_pass)
    assert listed == RW, listed
    assert (exp["bc1"] > 0).mean() > 0.3


@pytest.mark.parametrize("ragged", [False, True], ids=["150nt", "ragged"])
def test_lane_with_sixteen_hits(ragged, monkeypatch):
    """A run of A's that matches a piece at every position: lanes whose sixteen positions all hit (a poly-A barcode), beside
    lanes with one or two hits, in tiles that stay within the hit queue."""
    bcs = _acg_barcodes(48, extra=["A" * 24])
    keys = _keys(bcs)
    rng = np.random.Generator(np.random.PCG64(11))
    reads = []
    for t in range(RW * 40):
        n = int(rng.integers(90, 220)) if ragged else 150
        if t % 16 == 3:  # 40 .. 44 A's, 33 .. 37 hits in a row: at least one 16-position group of the flat image lies inside
            run = "A" * int(rng.integers(Q + 32, Q + 37))
            s = "T" * int(rng.integers(10, 26)) + run
        else:
            b = bcs[1 + int(rng.integers(0, len(bcs) - 1))]
            s = "T" * int(rng.integers(10, 60)) + b
        reads.append((s + "T" * n)[:n])
    for k in range(0, len(reads), RW):
        assert sum(_hits(r, keys) for r in reads[k:k + RW]) <= HQ
    seq, off = H.bdx.pack_reads(reads)
    exp, listed = _both(_cfg(bcs), seq, off, monkeypatch, want_pass=False)
    assert listed == 0, listed
    assert (exp["bc1"] > 0).mean() > 0.3
