"""GPU checks of the wave kernel's LEAN forms where the trims of its transcode and of its sweep set-up can go wrong
(csrc/bdx_wave_kernel.h: pack16_lean, the one-word junk mask and the start value of Pv in sweep_lane, the tile deal).

Every case is a few thousand reads at most, built here read by read, must run a LEAN form of the wave kernel as its first
launch over the whole batch (asserted from the launch log, with the number of reads handed on), and is compared bit for bit — every output and the
counter vector — with the CPU oracle and with the general kernel alone (BDX_NO_WAVE), once as the batch comes and once
through classify_device with a WRONG read-length hint (one base more than the longest read: the resolve works out its own
multiplier); one batch mixes the read lengths (the resolve's mixed-length branch).

* windows cut by the read's edges: a 24-nt barcode with 0 .. 2 edits at read positions 0, 1, 2, n - 24, n - 25, n - 26 of reads of
  150, and batches of reads of 8, 23, 24, 25, 26, 28, 31, 32, 33 and 40 bases: sweeps of 1 .. 32 columns, blocks in which every
  lane ends in the last word and blocks in which some lane does not;
* a window longer than 32 columns: 32-nt barcodes at rate 0.15 with copies that carry two insertions (a second block whose
  first word is partly junk);
* barcodes of 8, 16, 24, 31 and 32 bases (the start value of Pv);
* bytes outside ACGTN in one lane of a vector: at the first byte of a tile, at the last byte of a tile's last full vector and in
  the partial last vector (whose stale lanes neither store nor call for the exact pack), the last tile holding one read and five;
* hits at the queue's edges: an intact copy at read offsets 4 and 12, a tile of reads that are one 8-mer over and over (eighteen
  hits a read, 576 in the tile: the queue runs over and the tile's 32 reads are listed, no other read is), batches of
  33, 64 and 65 reads.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import fuzz
import helpers as H
import test_wave_tile_deal_gpu as TD

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def config(bcs, rate=0.1):
    return H.bdx.DemuxConfig(bc_seqs=list(bcs), bc_lengths_no_N=[len(b) for b in bcs], ids=[f"bc{i + 1}" for i in range(len(bcs))], max_error_rate=rate)


@functools.lru_cache(maxsize=None)
def barcodes(n, m):
    from biodemux_jl_amd import synth

    return tuple(synth.make_barcodes(n, m, seed=synth.SEED + m, min_hamming=min(8, max(3, m // 3))))


def pack(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.frombuffer(bytes(r), dtype=np.uint8) for r in reads]).copy(), off


def background(rng, n, length):
    return [bytearray(ACGT[rng.integers(0, 4, length)].tobytes()) for _ in range(n)]


def plant(read, copy, pos):
    """`copy` written over the read from `pos` on, cut at the read's end (pos < 0: counted from the end)."""
    n = len(read)
    pos = max(0, n + pos) if pos < 0 else pos
    end = min(n, pos + len(copy))
    read[pos:end] = copy[:end - pos]


def check(key, cfg, reads, monkeypatch, listed=0):
    """oracle == wave run == wave run with a wrong length hint == the general kernel alone, the wave runs' first launch a LEAN form
    of the wave kernel (NV = 5, no split / pairs / window mode) over the whole batch, `listed` reads handed on; -> oracle outputs."""
    seq, off = pack(reads)
    n = len(reads)
    env = {"BDX_WAVE_RW": 32}
    exp, counts = TD.oracle(cfg, seq, off)
    ref, ref_counts, _, _, ref_path = TD.run_device(cfg, seq, off, monkeypatch, dict(env, BDX_NO_WAVE=1))
    assert "wave" not in ref_path, ref_path
    fuzz.assert_same(ref, exp, f"{key} [{ref_path}]")
    for hint in (None, max(len(r) for r in reads) + 1):
        got, got_counts, launches_h, handed, path = TD.run_device(cfg, seq, off, monkeypatch, env, hint=hint)
        what = f"{key} hint {hint} [{path}] {launches_h}"
        fuzz.assert_same(got, exp, what)
        assert np.array_equal(got_counts, counts) and int(got_counts[0]) == n, what
        assert np.array_equal(got_counts, ref_counts), what
        first = launches_h[0]
        assert first["kernel"].startswith("bdx_wave_kernel<32, ") and first["reads"] == n and not first["list"], what
        args = [x.strip() for x in first["kernel"].split("<")[1].rstrip(">").split(",")]
        assert args[2] == "5" and args[4:7] == ["false", "0", "0"] and args[8] in ("0", "1", "2") and args[10] == "false", what  # a LEAN form
        assert handed == listed, f"{what}: {handed} reads handed on"
    return exp


LENGTHS = (150, 8, 23, 24, 25, 26, 28, 31, 32, 33, 40)


@pytest.mark.parametrize("length", LENGTHS + (0,), ids=[str(x) for x in LENGTHS] + ["mixed"])
def test_windows_cut_by_the_reads_edges(length, monkeypatch):
    from biodemux_jl_amd import synth

    bcs = TD.c2_barcodes()
    rng = np.random.default_rng(1300 + length)
    n = 32 * 40 + 11
    reads = background(rng, n, length) if length else [background(rng, 1, LENGTHS[(i * 5) % len(LENGTHS)])[0] for i in range(n)]
    spots = (0, 1, 2, -24, -25, -26)
    for i, r in enumerate(reads):
        if i % 8 == 7:
            continue  # (a read without a copy)
        copy = synth.mutate_copy(rng, bcs[(i * 7) % 96], (i // 6) % 3)
        plant(r, copy, spots[i % 6])
    exp = check(("edges", length), config(bcs), reads, monkeypatch)
    if length == 0 or length >= 26:
        assert (exp["bc1"] > 0).mean() > 0.3


def test_window_longer_than_32_columns(monkeypatch):
    bcs = barcodes(24, 32)
    rng = np.random.default_rng(1332)
    n = 32 * 30 + 3
    reads = background(rng, n, 150)
    for i, r in enumerate(reads):
        b = bytearray(bcs[i % 24].encode())
        if i % 3 != 2:  # two insertions, eight intact bases in front of, between and behind them
            p0, p1 = 9 + i % 3, 20 + i % 4
            b = b[:p0] + bytes([ACGT[rng.integers(0, 4)]]) + b[p0:p1] + bytes([ACGT[rng.integers(0, 4)]]) + b[p1:]
        plant(r, b, (3, 40, 150 - len(b), 150 - len(b) - 3)[i % 4])
    exp = check("long window", config(bcs, rate=0.15), reads, monkeypatch)  # (tier 1 of a tiered config: the headline form at the capped budget)
    assert (exp["bc1"] > 0).mean() > 0.5


@pytest.mark.parametrize("m", [8, 16, 24, 31, 32])
def test_barcode_lengths(m, monkeypatch):
    from biodemux_jl_amd import synth

    bcs = barcodes(8 if m == 8 else 24, m)
    rng = np.random.default_rng(1400 + m)
    n = 32 * 24 + 9
    reads = background(rng, n, 150)
    for i, r in enumerate(reads):
        copy = synth.mutate_copy(rng, bcs[i % len(bcs)], (i // 5) % (1 + m // 10))
        plant(r, copy, (0, 17, 60, -m, -m - 2)[i % 5])
    exp = check(("m", m), config(bcs), reads, monkeypatch)
    assert (exp["bc1"] > 0).mean() > 0.3


# a lower-case letter, an IUPAC code, NUL, the neighbour of each letter under the 3-bit index (byte >> 1) & 7 and bytes of the
# indices no letter has
ODD_BYTES = (ord("a"), ord("R"), 0x00, ord("A") ^ 1, ord("C") ^ 1, ord("T") ^ 1, ord("G") ^ 1, ord("N") ^ 1, ord("A") | 0x20, 0x48, 0x4A, 0x4C, 0xFF, 0x80)


@pytest.mark.parametrize("last", [1, 5])
def test_bytes_outside_acgtn_in_one_lane(last, monkeypatch):
    from biodemux_jl_amd import synth

    bcs = TD.c2_barcodes()
    rng = np.random.default_rng(1500 + last)
    tiles = 3 * len(ODD_BYTES)
    reads = background(rng, 32 * tiles + last, 150)
    for i, r in enumerate(reads):
        plant(r, synth.mutate_copy(rng, bcs[i % 96], i % 3), (0, 20, -24, -30)[i % 4])
    seq, off = pack(reads)
    for t in range(tiles):  # one odd byte per tile (32 reads of 150: 300 whole vectors)
        s0, s1 = int(off[32 * t]), int(off[32 * t + 32])
        seq[(s0, s1 - 1, s0 + 16 * 17 + 5)[t % 3]] = ODD_BYTES[t // 3]
    s0, s1 = int(off[32 * tiles]), int(off[-1])  # the last tile: whole vectors and a partial one
    seq[s0 + 16 * ((s1 - s0) // 16) - 1] = ord("a")
    seq[s1 - 1] = ODD_BYTES[3]
    reads = [bytearray(seq[off[i]:off[i + 1]].tobytes()) for i in range(len(reads))]
    exp = check(("bytes", last), config(bcs), reads, monkeypatch)
    assert (exp["bc1"] > 0).mean() > 0.5


@pytest.mark.parametrize("n", [33, 64, 65, 32 * 20 + 7])
def test_hits_at_the_queues_edges(n, monkeypatch):
    bcs = TD.c2_barcodes()
    rng = np.random.default_rng(1600 + n)
    reads = background(rng, n, 150)
    for i, r in enumerate(reads):
        plant(r, bcs[(5 * i) % 96].encode(), (4, 12)[i % 2] + 16 * (i % 7))  # three intact pieces across two groups of sixteen
    if n > 65:  # one tile whose reads are an 8-mer of a barcode over and over: eighteen hits a read, 576 in the tile's queue
        for i in range(64, 96):
            reads[i] = bytearray((bcs[i % 96][:8] * 19).encode()[:150])
    exp = check(("queue", n), config(bcs), reads, monkeypatch, listed=32 if n > 65 else 0)  # (the tile whose queue runs over is listed whole)
    assert (exp["bc1"] > 0).mean() > 0.8
